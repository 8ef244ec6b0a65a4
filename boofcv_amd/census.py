"""Census transform and census block-matching stereo (I:factory/transform/census, I:abst/transform/census, I:alg/transform/census,
F:factory/feature/disparity, F:abst/feature/disparity/WrapDisparityBlockMatchCensus.java).
  FactoryCensusTransform.variant / blockDense -> FilterImageInterface     I:factory/transform/census/FactoryCensusTransform.java:46-93
  CensusTransform.dense3x3 / dense5x5 / sample_S64, the sample lists      I:alg/transform/census/CensusTransform.java:53-225
  FactoryStereoDisparity.blockMatch, errorType = CENSUS                   F:factory/feature/disparity/FactoryStereoDisparity.java:62-102

A module beside the api package (like binary.py): it takes the image types and the view marshaller from boofcv_amd.api and adds no name there;
api.FactoryStereoDisparity.blockMatch keeps refusing errorType = CENSUS, FactoryStereoDisparityCensus.blockMatch is the census form.
Implemented on the GPU: GrayU8 inputs, the REFLECT border of the factory, sample offsets within -7 .. 7.  Rules, the `int bit` of the GrayS64
words and the deviations: bhip_census_u8_u8 and bhip_disparity_bm_census_u8_u8 in include/boofhip.h."""
import ctypes as C
import enum

import numpy as np

from . import _lib
from .api.core import IllegalArgumentException, _check, _ctx
from .api.disparity import ConfigDisparityBM, DisparityError, StereoDisparity
from .api.image import BorderType, GrayF32, GrayS16, GrayS32, GrayU8, _Gray

__all__ = ["CensusTransform", "CensusVariants", "ConfigDisparityError", "FactoryCensusTransform", "FactoryStereoDisparityCensus", "FilterCensusTransform",
           "GrayS64", "StereoDisparityCensus"]


class GrayS64(_Gray):
    """T:struct/image/GrayS64.java"""
    dtype, _ptr = np.int64, _lib._llp


class CensusVariants(enum.IntEnum):
    """I:factory/transform/census/CensusVariants.java (ordinals = BHIP_CENSUS_*)"""
    BLOCK_3_3 = _lib.BHIP_CENSUS_BLOCK_3_3
    BLOCK_5_5 = _lib.BHIP_CENSUS_BLOCK_5_5
    BLOCK_7_7 = _lib.BHIP_CENSUS_BLOCK_7_7
    BLOCK_9_7 = _lib.BHIP_CENSUS_BLOCK_9_7
    BLOCK_13_5 = _lib.BHIP_CENSUS_BLOCK_13_5
    CIRCLE_9 = _lib.BHIP_CENSUS_CIRCLE_9


def _variant_samples(variant):
    """the reference's sample list of a variant, [(x, y)]: it exists once, in the library"""
    n = C.c_int(0)
    xy = np.zeros(2 * 64, np.int32)
    if _lib.load().bhip_census_variant_samples(int(variant), xy.ctypes.data_as(_lib._ip), 64, C.byref(n)) != 0:
        raise IllegalArgumentException("Unknown type %s" % (variant,))
    return [(int(xy[2 * i]), int(xy[2 * i + 1])) for i in range(n.value)]


def _samples_arg(samples):
    xy = np.ascontiguousarray([c for p in samples for c in p], np.int32).reshape(-1)
    return xy, xy.ctypes.data_as(_lib._ip), len(samples)


def _reflect_only(border):
    if border != BorderType.REFLECT:
        raise RuntimeError("the census transform on the GPU has the REFLECT border of FactoryCensusTransform only (use the Java path)")


class CensusTransform:
    """I:alg/transform/census/CensusTransform.java.  border: BorderType.REFLECT, the factory's CENSUS_BORDER (the only one on the GPU)."""

    @staticmethod
    def createBlockSamples(radiusX, radiusY=None):
        """createBlockSamples(radius) / createBlockSamples(radiusX, radiusY) -> [(x, y)], row-major, without the centre"""
        radiusY = radiusX if radiusY is None else radiusY
        return [(x, y) for y in range(-radiusY, radiusY + 1) for x in range(-radiusX, radiusX + 1) if x != 0 or y != 0]

    @staticmethod
    def createCircleSamples():
        return _variant_samples(CensusVariants.CIRCLE_9)

    @staticmethod
    def _run(fn, pre, input, output, outType, ctx):
        if not isinstance(input, GrayU8):
            raise RuntimeError("only GrayU8 images are implemented on the GPU (use the Java path)")
        if not isinstance(output, outType):
            raise IllegalArgumentException("the output must be a %s" % outType.__name__)
        if output.width != input.width or output.height != input.height:
            output.reshape(input.width, input.height)          # InputSanityCheck.checkReshape / output.reshape
        ctx = _ctx(ctx)
        _check(ctx, fn(ctx._h, *pre, *input._in(), *output._out()))

    @staticmethod
    def dense3x3(input, output, border=BorderType.REFLECT, ctx=None):
        _reflect_only(border)
        CensusTransform._run(_lib.load().bhip_census_u8_u8, (), input, output, GrayU8, ctx)

    @staticmethod
    def dense5x5(input, output, border=BorderType.REFLECT, ctx=None):
        _reflect_only(border)
        CensusTransform._run(_lib.load().bhip_census_u8_s32, (), input, output, GrayS32, ctx)

    @staticmethod
    def sample_S64(input, sample, output, border=BorderType.REFLECT, workSpace=None, ctx=None):
        _reflect_only(border)
        xy, p, n = _samples_arg(sample)
        CensusTransform._run(_lib.load().bhip_census_sample_u8_s64, (p, n), input, output, GrayS64, ctx)


class FilterCensusTransform:
    """FilterCensusTransformD33U8 / D55S32 / SampleS64 (I:abst/transform/census/): FilterImageInterface<GrayU8, GrayU8 | GrayS32 | GrayS64>"""

    def __init__(self, outputType, samples, ctx=None):
        if len(samples) > 64:                                   # FilterCensusTransformSampleS64's constructor
            raise IllegalArgumentException("At most 64 sample points for now. size = %d" % len(samples))
        self.outputType, self.samples = outputType, list(samples)
        self.ctx = ctx                                          # None: the default context, created by the first process()

    def process(self, input, output):
        self.ctx = _ctx(self.ctx)
        if self.outputType is GrayU8:
            CensusTransform.dense3x3(input, output, ctx=self.ctx)
        elif self.outputType is GrayS32:
            CensusTransform.dense5x5(input, output, ctx=self.ctx)
        else:
            CensusTransform.sample_S64(input, self.samples, output, ctx=self.ctx)

    def getHorizontalBorder(self): return 0
    def getVerticalBorder(self): return 0
    def getInputType(self): return GrayU8
    def getOutputType(self): return self.outputType


def _gray_u8_only(imageType):
    if imageType is not GrayU8:
        raise RuntimeError("only GrayU8 images are implemented on the GPU (use the Java path)")


class FactoryCensusTransform:
    """I:factory/transform/census/FactoryCensusTransform.java:46-93"""
    CENSUS_BORDER = BorderType.REFLECT

    @staticmethod
    def variant(type, imageType=GrayU8, ctx=None):
        try:
            type = CensusVariants(type)
        except ValueError:
            raise IllegalArgumentException("Unknown type %s" % (type,))
        _gray_u8_only(imageType)
        outputType = GrayU8 if type is CensusVariants.BLOCK_3_3 else GrayS32 if type is CensusVariants.BLOCK_5_5 else GrayS64
        return FilterCensusTransform(outputType, _variant_samples(type), ctx)

    @staticmethod
    def blockDense(*args, ctx=None):
        """blockDense(radius, imageType) / blockDense(radiusX, radiusY, imageType); imageType may be left out (GrayU8)"""
        radii = [a for a in args if isinstance(a, (int, np.integer))]
        types = [a for a in args if not isinstance(a, (int, np.integer))]
        if len(radii) not in (1, 2) or len(types) > 1:
            raise TypeError("blockDense(radius[, imageType]) or blockDense(radiusX, radiusY[, imageType])")
        imageType = types[0] if types else GrayU8
        if len(radii) == 1:
            if radii[0] not in (1, 2, 3):
                raise IllegalArgumentException("Currently only radius 1 to 3 is supported")
            _gray_u8_only(imageType)
            return FilterCensusTransform((GrayU8, GrayS32, GrayS64)[radii[0] - 1], CensusTransform.createBlockSamples(radii[0]), ctx)
        filt = FilterCensusTransform(GrayS64, CensusTransform.createBlockSamples(radii[0], radii[1]), ctx)   # more than 64 samples: thrown here
        _gray_u8_only(imageType)
        return filt


class ConfigDisparityError:
    """F:factory/feature/disparity/ConfigDisparityError.java:30-42"""

    class Census:
        def __init__(self, variant=CensusVariants.BLOCK_5_5):
            self.variant = variant

        def checkValidity(self):
            pass


class StereoDisparityCensus(StereoDisparity):
    """WrapDisparityBlockMatchCensus<GrayU8, GrayU8 | GrayS32 | GrayS64, GrayU8 | GrayF32> (F:abst/feature/disparity/WrapDisparityBlockMatchCensus.java:32-80)
    as FactoryStereoDisparity.blockMatch builds it for errorType = CENSUS.  Rules, limits and deviations: bhip_disparity_bm_census_u8_u8 in
    include/boofhip.h.  The census images of the pair stay on the device; getCLeft / getCRight compute them on demand, with the filter, from
    the images the last process() was given (as they are then: keep them unchanged until asked)."""

    def __init__(self, config, dispType, censusTran, variant, ctx=None):
        self.config, self.dispType, self.disparity = config, dispType, None
        self.ctx = ctx                                          # None: the default context, created by the first process()
        self.censusTran, self.variant = censusTran, variant
        self._pair = None
        self._census = [None, None]

    def process(self, imageLeft, imageRight):
        if not isinstance(imageLeft, GrayU8) or not isinstance(imageRight, GrayU8):
            raise IllegalArgumentException("this algorithm takes GrayU8 images")
        if imageLeft.width != imageRight.width or imageLeft.height != imageRight.height:
            raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape
        w, h, c = imageLeft.width, imageLeft.height, self.config
        if c.minDisparity + c.rangeDisparity > w - 2 * c.regionRadiusX:   # DisparityBlockMatchRowFormat.process :100-102
            raise RuntimeError("The maximum disparity is too large for this image size: max size %d" % (w - 2 * c.regionRadiusX))
        if self.disparity is None or self.disparity.width != w or self.disparity.height != h:
            self.disparity = self.dispType(w, h)
        d = self.disparity
        self.ctx = self.censusTran.ctx = _ctx(self.ctx)
        L = _lib.load()
        fn = L.bhip_disparity_bm_census_u8_f32 if self.dispType is GrayF32 else L.bhip_disparity_bm_census_u8_u8
        _check(self.ctx, fn(self.ctx._h, C.byref(c._c()), int(self.variant), *imageLeft._out(), *imageRight._out(), w, h, *d._out()))
        self._pair = (imageLeft, imageRight)
        self._census = [None, None]

    def _c_image(self, k):
        if self._census[k] is None:
            out = self.censusTran.getOutputType()(1, 1)       # the constructor's createImage(1, 1)
            if self._pair is not None:
                self.censusTran.process(self._pair[k], out)
            self._census[k] = out
        return self._census[k]

    def getCLeft(self): return self._c_image(0)
    def getCRight(self): return self._c_image(1)
    def getCensusTran(self): return self.censusTran
    def getInputType(self): return self.censusTran.getInputType()


class FactoryStereoDisparityCensus:
    """FactoryStereoDisparity.blockMatch for errorType = CENSUS (F:factory/feature/disparity/FactoryStereoDisparity.java:62-102, 116-144, 230-240)"""

    @staticmethod
    def blockMatch(config, imageType=GrayU8, dispType=GrayF32, configCensus=None, ctx=None):
        """config: an api.ConfigDisparityBM with errorType = CENSUS; configCensus: its configCensus field, a ConfigDisparityError.Census (None: the
        default, BLOCK_5_5).  IllegalArgumentException where the factory and the constructors it calls throw it; inputs other than GrayU8 raise
        RuntimeError: use the Java path."""
        if config is None:
            config = ConfigDisparityBM()
        if configCensus is None:
            configCensus = ConfigDisparityError.Census()
        if config.subpixel:
            if dispType is not GrayF32:
                raise IllegalArgumentException("With subpixel on, disparity image must be GrayF32")
        elif dispType is not GrayU8:
            raise IllegalArgumentException("With subpixel on, disparity image must be GrayU8")
        if config.errorType != DisparityError.CENSUS:
            raise IllegalArgumentException("Unsupported error type %s: this factory builds the CENSUS form" % config.errorType)
        if imageType not in (GrayU8, GrayS16, GrayF32):       # createDisparitySelect (GrayU16 has no mirror here)
            raise IllegalArgumentException("Unknown image type")
        try:
            variant = CensusVariants(configCensus.variant)     # FactoryCensusTransform.variant
        except ValueError:
            raise IllegalArgumentException("Unknown type %s" % (configCensus.variant,))
        # DisparityBlockMatchRowFormat constructor :72-75
        maxDisparity = config.minDisparity + config.rangeDisparity
        if maxDisparity <= 0:
            raise IllegalArgumentException("Max disparity must be greater than zero. max=%d" % maxDisparity)
        if config.minDisparity < 0 or config.minDisparity >= maxDisparity:
            raise IllegalArgumentException("Min disparity must be >= 0 and < maxDisparity. min=%d max=%d" % (config.minDisparity, maxDisparity))
        _gray_u8_only(imageType)
        return StereoDisparityCensus(config, dispType, FactoryCensusTransform.variant(variant, imageType, ctx), variant, ctx)
