"""Filters: kernels, convolution, down-convolution, the discrete pyramid, blur, gradients and the BRIEF sampler (T:struct/convolve,
I:alg/filter/{convolve,blur,derivative}, I:factory/filter/kernel, I:alg/transform/pyramid, F:alg/feature/describe/DescribePointBrief.java).
  BOverride* hooks (static op classes)           I:alg/filter/convolve/BOverrideConvolveImage.java:37-83 etc."""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .core import IllegalArgumentException, _check, _ctx
from .image import BorderType, GrayF32, GrayS16, GrayU8

__all__ = ["BlurImageOps", "ConvolveImageDownNormalized", "ConvolveImageNoBorder", "ConvolveImageNormalized", "DescribePointBrief",
           "FactoryKernelGaussian", "FactoryPyramid", "GradientSobel", "GradientThree", "Kernel1D_F32", "Kernel2D_F32", "PyramidDiscreteSampleBlur"]


@dataclass
class Kernel1D_F32:
    """T:struct/convolve/Kernel1D_F32.java: data, width, offset (origin index; width/2 by default)"""
    data: np.ndarray
    width: int = 0
    offset: int = -1

    def __post_init__(self):
        self.data = np.ascontiguousarray(self.data, dtype=np.float32)
        self.width = len(self.data)
        if self.offset < 0:
            self.offset = self.width // 2


def _conv(fn, kernel, src, dst, ctx):
    ctx = _ctx(ctx)
    s, d = src._in(), dst._out()
    if dst.width != src.width or dst.height != src.height:
        raise IllegalArgumentException("Image shapes do not match")  # InputSanityCheck.checkSameShape
    _check(ctx, fn(ctx._h, kernel.data.ctypes.data_as(_lib._fp), kernel.width, kernel.offset, *s, *d))


class ConvolveImageNoBorder:
    """BOverrideConvolveImage.horizontal/vertical/convolve targets (I:alg/filter/convolve/ConvolveImageNoBorder.java:53-90)"""

    @staticmethod
    def convolve(kernel, input, output, ctx=None):
        ctx = _ctx(ctx)
        if output.width != input.width or output.height != input.height:
            raise IllegalArgumentException("Image shapes do not match")
        _check(ctx, _lib.load().bhip_conv2d_f32(ctx._h, kernel.data.ctypes.data_as(_lib._fp), kernel.width, kernel.offset, *input._in(), *output._out()))

    @staticmethod
    def horizontal(kernel, input, output, ctx=None):
        _conv(_lib.load().bhip_conv_h_f32, kernel, input, output, ctx)

    @staticmethod
    def vertical(kernel, input, output, ctx=None):
        _conv(_lib.load().bhip_conv_v_f32, kernel, input, output, ctx)


class ConvolveImageNormalized:
    """BOverrideConvolveImageNormalized targets (I:alg/filter/convolve/ConvolveImageNormalized.java:48-93)"""

    @staticmethod
    def horizontal(kernel, src, dst, ctx=None):
        _conv(_lib.load().bhip_conv_norm_h_f32, kernel, src, dst, ctx)

    @staticmethod
    def vertical(kernel, src, dst, ctx=None):
        _conv(_lib.load().bhip_conv_norm_v_f32, kernel, src, dst, ctx)


class FactoryKernelGaussian:
    @staticmethod
    def gaussian1D_F32(sigma, radius):
        """FactoryKernelGaussian.gaussian(Kernel1D_F32.class, sigma, radius) (I:factory/filter/kernel/FactoryKernelGaussian.java:120-153)"""
        if sigma <= 0 and radius <= 0:
            raise IllegalArgumentException("Sigma must be > 0")
        L = _lib.load()
        w = -L.bhip_gaussian_kernel1d_f32(float(sigma), int(radius), None, 0)
        out = np.zeros(w, dtype=np.float32)
        L.bhip_gaussian_kernel1d_f32(float(sigma), int(radius), out.ctypes.data_as(_lib._fp), w)
        return Kernel1D_F32(out)

    @staticmethod
    def gaussian1D_S32(radius):
        """FactoryKernelGaussian.gaussian(Kernel1D_S32.class, -1, radius) (I:factory/filter/kernel/FactoryKernelGaussian.java:120-160): int32 taps"""
        if radius <= 0:
            raise IllegalArgumentException("Radius must be > 0")
        L = _lib.load()
        w = -L.bhip_gaussian_kernel1d_s32(int(radius), None, 0)
        out = np.zeros(w, dtype=np.int32)
        L.bhip_gaussian_kernel1d_s32(int(radius), out.ctypes.data_as(_lib._i32p), w)
        return out


def _s32_taps(kernel):
    """Kernel1D_S32 taps: the int32 array FactoryKernelGaussian.gaussian1D_S32 returns, or anything with such a .data"""
    return np.ascontiguousarray(getattr(kernel, "data", kernel), dtype=np.int32)


class ConvolveImageDownNormalized:
    """I:alg/filter/convolve/ConvolveImageDownNormalized.java:53-86 (Kernel1D_F32, GrayF32), :109-137 (Kernel1D_S32, GrayU8 -> GrayI8): the
    NORMALIZED ConvolveDown of the discrete pyramid"""

    @staticmethod
    def _run(axis, kernel, image, dest, skip, ctx):
        ctx = _ctx(ctx)
        L = _lib.load()
        if isinstance(image, GrayU8):
            if not isinstance(dest, GrayU8):
                raise IllegalArgumentException("a GrayU8 image is down-convolved into a GrayU8 (GrayI8) image")
            taps = _s32_taps(kernel)
            fn, kp, kw = getattr(L, "bhip_conv_down_norm_%s_u8" % axis), taps.ctypes.data_as(_lib._i32p), len(taps)
        elif isinstance(image, GrayF32):
            fn, kp, kw = getattr(L, "bhip_conv_down_norm_%s_f32" % axis), kernel.data.ctypes.data_as(_lib._fp), kernel.width
        else:
            raise RuntimeError("only GrayF32 and GrayU8 images are implemented on the GPU (use the Java path)")
        _check(ctx, fn(ctx._h, kp, kw, *image._in(), *dest._in(), int(skip)))

    @staticmethod
    def horizontal(kernel, image, dest, skip, ctx=None):
        ConvolveImageDownNormalized._run("h", kernel, image, dest, skip, ctx)

    @staticmethod
    def vertical(kernel, image, dest, skip, ctx=None):
        ConvolveImageDownNormalized._run("v", kernel, image, dest, skip, ctx)


class PyramidDiscreteSampleBlur:
    """I:alg/transform/pyramid/PyramidDiscreteSampleBlur.java:48-126: layer i = layer i-1 blurred with the (border-normalised) kernel and
    sub-sampled by scale[i]/scale[i-1]; layer 0 = the input when scale[0] == 1."""

    def __init__(self, kernel, sigma, saveOriginalReference, scaleFactors, ctx=None, imageType=None):
        self.ctx = _ctx(ctx)
        self.kernel = kernel
        self.imageType = GrayF32 if imageType is None else imageType   # GrayF32 (Kernel1D_F32) or GrayU8 (Kernel1D_S32)
        self.saveOriginalReference = bool(saveOriginalReference)
        self.scale = [int(s) for s in scaleFactors]
        # ImagePyramidBase.checkScales (T:struct/pyramid/ImagePyramidBase.java:100-112)
        if self.scale[0] < 0:
            raise IllegalArgumentException("The first layer must be more than zero.")
        for a, b in zip(self.scale, self.scale[1:]):
            if b < a:
                raise IllegalArgumentException("Higher layers must be the same size or larger than previous layers.")
        self.sigmas = [0.0] * len(self.scale)
        for i in range(1, len(self.scale)):
            prev, applied = self.sigmas[i - 1], sigma * self.scale[i - 1]
            self.sigmas[i] = math.sqrt(prev * prev + applied * applied)
        self.layers = None

    def getNumLayers(self):
        return len(self.scale)

    def getScale(self, layer):
        return float(self.scale[layer])

    def getSigma(self, layer):
        return self.sigmas[layer]

    def getSampleOffset(self, layer):
        return 0.0

    def process(self, input):
        L = _lib.load()
        n = len(self.scale)
        sc = np.asarray(self.scale, dtype=np.int32)
        dims = np.zeros(2 * n, dtype=np.int32)
        offs = np.zeros(n, dtype=np.int64)
        total = C.c_longlong(0)
        if L.bhip_pyramid_layout(input.width, input.height, sc.ctypes.data_as(_lib._ip), n, dims.ctypes.data_as(_lib._ip),
                                 offs.ctypes.data_as(_lib._llp), C.byref(total)) != 0:
            raise IllegalArgumentException("bad pyramid scales")
        if not isinstance(input, self.imageType):
            raise IllegalArgumentException("this pyramid was built for %s images" % self.imageType.__name__)
        if self.imageType is GrayU8:
            taps = _s32_taps(self.kernel)
            packed = np.zeros(total.value, dtype=np.uint8)
            rc = L.bhip_pyramid_u8(self.ctx._h, taps.ctypes.data_as(_lib._i32p), len(taps), sc.ctypes.data_as(_lib._ip), n, *input._in(),
                                   packed.ctypes.data_as(_lib._u8p))
        else:
            packed = np.zeros(total.value, dtype=np.float32)
            rc = L.bhip_pyramid_f32(self.ctx._h, self.kernel.data.ctypes.data_as(_lib._fp), self.kernel.width, sc.ctypes.data_as(_lib._ip), n, *input._in(),
                                    packed.ctypes.data_as(_lib._fp))
        _check(self.ctx, rc)
        self.layers = []
        for i in range(n):
            w, h = int(dims[2 * i]), int(dims[2 * i + 1])
            if i == 0 and self.scale[0] == 1 and self.saveOriginalReference:
                self.layers.append(input)  # setFirstLayer(input)
            else:
                self.layers.append(self.imageType(w, h, packed[offs[i]:offs[i] + w * h]))
        return self

    def getLayer(self, i):
        return self.layers[i]

    def getWidth(self, i):
        return self.layers[i].width

    def getHeight(self, i):
        return self.layers[i].height


class FactoryPyramid:
    @staticmethod
    def discreteGaussian(scaleFactors, sigma, radius, saveOriginalReference=False, ctx=None, imageType=None):
        """I:factory/transform/pyramid/FactoryPyramid.java:53-61: FactoryKernelGaussian.gaussian(FactoryKernel.getKernelType(imageType, 1), sigma,
        radius) -- Kernel1D_F32 for GrayF32 (the default), Kernel1D_S32 for GrayU8"""
        imageType = GrayF32 if imageType is None else imageType
        if imageType is GrayU8:
            if sigma > 0:
                raise RuntimeError("the integer Gaussian kernel is built from its radius only on the GPU (sigma = -1)")
            kernel = FactoryKernelGaussian.gaussian1D_S32(radius)
        elif imageType is GrayF32:
            kernel = FactoryKernelGaussian.gaussian1D_F32(sigma, radius)
        else:
            raise RuntimeError("only GrayF32 and GrayU8 pyramids are implemented on the GPU (use the Java path)")
        return PyramidDiscreteSampleBlur(kernel, sigma, saveOriginalReference, scaleFactors, ctx, imageType)


@dataclass
class Kernel2D_F32:
    """T:struct/convolve/Kernel2D_F32.java: width x width values row-major, offset = origin index along both axes"""
    data: np.ndarray
    width: int = 0
    offset: int = -1

    def __post_init__(self):
        self.data = np.ascontiguousarray(self.data, dtype=np.float32)
        self.width = self.data.shape[0]
        if self.data.ndim != 2 or self.data.shape[1] != self.width:
            raise IllegalArgumentException("square kernel expected")
        if self.offset < 0:
            self.offset = self.width // 2


class BlurImageOps:
    """GrayF32, and for mean / gaussian GrayU8 as well (the blurs of the local thresholds)"""

    @staticmethod
    def mean(input, output, radiusX, radiusY=None, storage=None, ctx=None):
        """BOverrideBlurImageOps.mean target (I:alg/filter/blur/BlurImageOps.java:343-376; GrayU8 :75-92)"""
        ctx = _ctx(ctx)
        radiusY = radiusX if radiusY is None else radiusY
        if radiusX <= 0 or radiusY <= 0:
            raise IllegalArgumentException("Radius must be > 0")
        u8 = isinstance(input, GrayU8)
        if output is None:
            output = type(input)(input.width, input.height) if u8 else GrayF32(input.width, input.height)
        fn = _lib.load().bhip_mean_u8 if u8 else _lib.load().bhip_mean_f32
        _check(ctx, fn(ctx._h, *input._in(), int(radiusX), int(radiusY), *output._out()))
        return output

    @staticmethod
    def median(input, output, radius, ctx=None):
        """BOverrideBlurImageOps.median target (I:alg/filter/blur/BlurImageOps.java:752-765)"""
        ctx = _ctx(ctx)
        if radius <= 0:
            raise IllegalArgumentException("Radius must be > 0")
        if output is None:
            output = GrayF32(input.width, input.height)
        _check(ctx, _lib.load().bhip_median_f32(ctx._h, *input._in(), int(radius), *output._out()))
        return output

    @staticmethod
    def gaussian(input, output, sigma, radius, storage=None, ctx=None):
        """BOverrideBlurImageOps.gaussian target (I:alg/filter/blur/BlurImageOps.java:406-425; GrayU8 :122-141 with sigma <= 0: the kernel of the radius)"""
        ctx = _ctx(ctx)
        if isinstance(input, GrayU8):
            if sigma > 0:
                raise IllegalArgumentException("the GrayU8 Gaussian blur on the GPU takes its kernel from the radius (sigma <= 0)")
            if radius <= 0:
                raise IllegalArgumentException("Sigma must be > 0")
            if output is None:
                output = GrayU8(input.width, input.height)
            _check(ctx, _lib.load().bhip_gaussian_u8(ctx._h, *input._in(), int(radius), *output._out()))
            return output
        if output is None:
            output = GrayF32(input.width, input.height)
        _check(ctx, _lib.load().bhip_gaussian_f32(ctx._h, *input._in(), float(sigma), int(radius), *output._out()))
        return output


class _Gradient:
    fn = None
    fn_u8 = None

    @classmethod
    def process(cls, orig, derivX, derivY, border=None, ctx=None):
        """border: None = null (frame untouched), 0 = ImageBorderValue(0), BorderType.EXTENDED (GradientSobel only: what
        FactoryDerivative.sobel uses).  GrayF32 -> GrayF32, or GrayU8 -> GrayS16."""
        ctx = _ctx(ctx)
        extended = border is BorderType.EXTENDED
        if not extended and border not in (None, 0):
            raise RuntimeError("border policy not implemented on the GPU")
        if isinstance(orig, GrayU8):
            if not isinstance(derivX, GrayS16) or not isinstance(derivY, GrayS16):
                raise IllegalArgumentException("a GrayU8 image has GrayS16 derivatives")
            fn = cls.fn_u8
        elif isinstance(orig, GrayF32):
            fn = cls.fn
        else:
            raise RuntimeError("only GrayF32 and GrayU8 images are implemented on the GPU (use the Java path)")
        (px, *geom), (py, *_) = derivX._out(), derivY._out()   # both derivatives are written with derivX's startIndex and stride
        _check(ctx, getattr(_lib.load(), fn)(ctx._h, *orig._in(), px, py, *geom, 2 if extended else 0 if border is None else 1))


class GradientSobel(_Gradient):
    """I:alg/filter/derivative/GradientSobel.java:110-124 (GrayU8), 158-173 (GrayF32)"""
    fn = "bhip_sobel_f32"
    fn_u8 = "bhip_sobel_u8_s16"


class GradientThree(_Gradient):
    """I:alg/filter/derivative/GradientThree.java -> impl/GradientThree_Standard.java:40-62 (GrayF32), 67-88 (GrayU8)"""
    fn = "bhip_three_f32"
    fn_u8 = "bhip_three_u8_s16"


class DescribePointBrief:
    """DescribePointBrief.process for a list of points (F:alg/feature/describe/DescribePointBrief.java:73-89).  As in this fork of the
    reference, the fixed BRIEF variant samples the UNblurred image (SURVEY finding 6)."""

    def __init__(self, radius, samplePoints, compare, ctx=None):
        self.ctx = _ctx(ctx)
        self.radius = int(radius)
        self.samplePoints = np.ascontiguousarray(samplePoints, dtype=np.int32)
        self.compare = np.ascontiguousarray(compare, dtype=np.int32)
        self.image = None

    def setImage(self, image):
        self.image = image

    def processAll(self, xy):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        n, npts = len(xy), len(self.compare)
        out = np.zeros((n, (npts + 31) // 32), dtype=np.int32)
        im = self.image
        if isinstance(im, GrayU8):   # ImplDescribeBinaryCompare_U8
            _check(self.ctx, _lib.load().bhip_brief_u8(self.ctx._h, *im._in(), self.radius, npts,
                                                      self.samplePoints.ctypes.data_as(_lib._i32p), self.compare.ctypes.data_as(_lib._i32p),
                                                      xy.ctypes.data_as(_lib._dp), n, out.ctypes.data_as(_lib._i32p)))
            return out
        _check(self.ctx, _lib.load().bhip_brief_f32(self.ctx._h, *im._in(), self.radius, npts,
                                                   self.samplePoints.ctypes.data_as(_lib._i32p), self.compare.ctypes.data_as(_lib._i32p),
                                                   xy.ctypes.data_as(_lib._dp), n, out.ctypes.data_as(_lib._i32p)))
        return out

    def process(self, c_x, c_y, feature):
        feature.data[:] = self.processAll([[c_x, c_y]])[0]
