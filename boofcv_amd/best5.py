"""Five-region block-matching stereo (F:factory/feature/disparity, F:alg/feature/disparity/block/score/DisparityScoreBMBestFive_S32.java).
  ConfigDisparityBMBest5                                   F:factory/feature/disparity/ConfigDisparityBMBest5.java (no field of its own)
  FactoryStereoDisparity.blockMatchBest5                   F:factory/feature/disparity/FactoryStereoDisparity.java:146-201
  DisparityBlockMatchBestFive.getBorderX / getBorderY      F:alg/feature/disparity/DisparityBlockMatchBestFive.java:60-67

A module beside the api package (like census.py and binary.py): it adds no name there; api.FactoryStereoDisparity.blockMatchBest5 keeps refusing,
FactoryStereoDisparityBest5.blockMatchBest5 is the GPU form, for errorType = SAD and CENSUS on GrayU8 pairs.  Rules, limits and deviations:
bhip_disparity_bm5_u8_u8 in include/boofhip.h."""
import ctypes as C
from dataclasses import dataclass, field

from . import _lib
from .api.core import IllegalArgumentException, _check, _ctx
from .api.disparity import ConfigDisparityBM, DisparityError, StereoDisparity
from .api.image import GrayF32, GrayS16, GrayU8
from .census import CensusVariants, ConfigDisparityError, FactoryCensusTransform, StereoDisparityCensus

__all__ = ["ConfigDisparityBMBest5", "FactoryStereoDisparityBest5", "StereoDisparityBest5", "StereoDisparityBest5Census"]


@dataclass
class ConfigDisparityBMBest5(ConfigDisparityBM):
    """F:factory/feature/disparity/ConfigDisparityBMBest5.java: ConfigDisparityBM under another name.  configCensus: the reference's field of
    that name (a ConfigDisparityError.Census; None: the default, BLOCK_5_5), read when errorType = CENSUS."""
    configCensus: object = field(default=None)


def _process(self, fn, pre, imageLeft, imageRight):
    """the argument checks of WrapBaseBlockMatch.process / DisparityBlockMatchRowFormat.process (:95-107: radiusX, not 2*radiusX), then the call"""
    if not isinstance(imageLeft, GrayU8) or not isinstance(imageRight, GrayU8):
        raise IllegalArgumentException("this algorithm takes GrayU8 images")
    if imageLeft.width != imageRight.width or imageLeft.height != imageRight.height:
        raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape
    w, h, c = imageLeft.width, imageLeft.height, self.config
    if c.minDisparity + c.rangeDisparity > w - 2 * c.regionRadiusX:
        raise RuntimeError("The maximum disparity is too large for this image size: max size %d" % (w - 2 * c.regionRadiusX))
    if self.disparity is None or self.disparity.width != w or self.disparity.height != h:
        self.disparity = self.dispType(w, h)
    _check(self.ctx, fn(self.ctx._h, C.byref(c._c()), *pre, *imageLeft._out(), *imageRight._out(), w, h, *self.disparity._out()))


class StereoDisparityBest5(StereoDisparity):
    """WrapDisparityBlockMatchRowFormat over DisparityScoreBMBestFive_S32, as blockMatchBest5 builds it for errorType = SAD"""

    def __init__(self, config, dispType, ctx=None):
        self.config, self.dispType, self.disparity = config, dispType, None
        self.ctx = ctx                                          # None: the default context, created by the first process()

    def process(self, imageLeft, imageRight):
        self.ctx = _ctx(self.ctx)
        L = _lib.load()
        _process(self, L.bhip_disparity_bm5_u8_f32 if self.dispType is GrayF32 else L.bhip_disparity_bm5_u8_u8, (), imageLeft, imageRight)

    def getBorderX(self): return 2 * self.config.regionRadiusX
    def getBorderY(self): return 2 * self.config.regionRadiusY


class StereoDisparityBest5Census(StereoDisparityCensus):
    """WrapDisparityBlockMatchCensus over DisparityScoreBMBestFive_S32, as blockMatchBest5 builds it for errorType = CENSUS"""

    def process(self, imageLeft, imageRight):
        self.ctx = self.censusTran.ctx = _ctx(self.ctx)
        L = _lib.load()
        _process(self, L.bhip_disparity_bm5_census_u8_f32 if self.dispType is GrayF32 else L.bhip_disparity_bm5_census_u8_u8, (int(self.variant),),
                 imageLeft, imageRight)
        self._pair = (imageLeft, imageRight)
        self._census = [None, None]

    def getBorderX(self): return 2 * self.config.regionRadiusX
    def getBorderY(self): return 2 * self.config.regionRadiusY


class FactoryStereoDisparityBest5:
    """FactoryStereoDisparity.blockMatchBest5 (F:factory/feature/disparity/FactoryStereoDisparity.java:146-201, 116-144, 242-255)"""

    @staticmethod
    def blockMatchBest5(config=None, imageType=GrayU8, dispType=GrayF32, ctx=None):
        """IllegalArgumentException where the factory and the constructors it calls throw it; the branches the GPU does not have (NCC, inputs
        other than GrayU8) raise RuntimeError: use the Java path."""
        if config is None:
            config = ConfigDisparityBMBest5()
        if config.subpixel:
            if dispType is not GrayF32:
                raise IllegalArgumentException("With subpixel on, disparity image must be GrayF32")
        elif dispType is not GrayU8:
            raise IllegalArgumentException("With subpixel on, disparity image must be GrayU8")
        if config.errorType not in (DisparityError.SAD, DisparityError.CENSUS, DisparityError.NCC):
            raise IllegalArgumentException("Unsupported error type %s" % config.errorType)
        if config.errorType == DisparityError.NCC:
            raise RuntimeError("errorType = NCC is not implemented on the GPU (use the Java path)")
        if imageType not in (GrayU8, GrayS16, GrayF32):       # createDisparitySelect / createScoreRowSad (GrayU16 has no mirror here)
            if config.errorType == DisparityError.SAD:
                raise IllegalArgumentException("Unsupported image type %s" % getattr(imageType, "__name__", imageType))
            raise IllegalArgumentException("Unknown image type")
        variant = None
        if config.errorType == DisparityError.CENSUS:
            configCensus = getattr(config, "configCensus", None) or ConfigDisparityError.Census()
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
        if imageType is not GrayU8:
            raise RuntimeError("only GrayU8 images are implemented on the GPU (use the Java path)")
        if variant is None:
            return StereoDisparityBest5(config, dispType, ctx)
        return StereoDisparityBest5Census(config, dispType, FactoryCensusTransform.variant(variant, imageType, ctx), variant, ctx)
