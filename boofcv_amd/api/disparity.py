"""Dense stereo disparity by block matching (F:abst/feature/disparity, F:factory/feature/disparity)."""
import ctypes as C
from dataclasses import dataclass

from .. import _lib
from .core import IllegalArgumentException, _check, _ctx
from .image import GrayF32, GrayS16, GrayU8

__all__ = ["ConfigDisparityBM", "DisparityError", "FactoryStereoDisparity", "StereoDisparity"]


class DisparityError:
    """F:factory/feature/disparity/DisparityError.java:26-55"""
    SAD, CENSUS, NCC = "SAD", "CENSUS", "NCC"

    @staticmethod
    def isCorrelation(errorType):
        return errorType not in (DisparityError.SAD, DisparityError.CENSUS)


@dataclass
class ConfigDisparityBM:
    """F:factory/feature/disparity/ConfigDisparityBM.java:31-87"""
    minDisparity: int = 0
    rangeDisparity: int = 100
    regionRadiusX: int = 3
    regionRadiusY: int = 3
    maxPerPixelError: float = 0
    validateRtoL: int = 1
    texture: float = 0.15
    subpixel: bool = True
    errorType: str = DisparityError.SAD

    def checkValidity(self):
        if self.minDisparity < 0:
            raise IllegalArgumentException("miDisparity < 0")
        if self.rangeDisparity < 1:
            raise IllegalArgumentException("rangeDisparity < 1")

    def _c(self):
        return _lib.DisparityBmCfg(int(self.minDisparity), int(self.rangeDisparity), int(self.regionRadiusX), int(self.regionRadiusY),
                                   float(self.maxPerPixelError), int(self.validateRtoL), float(self.texture))


class StereoDisparity:
    """StereoDisparity<GrayU8, GrayU8 | GrayF32> as FactoryStereoDisparity.blockMatch builds it for errorType = SAD:
    WrapDisparityBlockMatchRowFormat / WrapBaseBlockMatch (F:abst/feature/disparity/WrapBaseBlockMatch.java:42-95) over DisparityScoreBM_S32.
    Rules, limits and deviations: bhip_disparity_bm_u8_u8 in include/boofhip.h.  The disparity image is written as a whole by every process()."""

    def __init__(self, config, dispType, ctx=None):
        self.config, self.dispType = config, dispType
        self.ctx = _ctx(ctx)
        self.disparity = None

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
        fn = _lib.load().bhip_disparity_bm_u8_f32 if self.dispType is GrayF32 else _lib.load().bhip_disparity_bm_u8_u8
        _check(self.ctx, fn(self.ctx._h, C.byref(c._c()), *imageLeft._out(), *imageRight._out(), w, h, *d._out()))

    def getDisparity(self): return self.disparity
    def getBorderX(self): return self.config.regionRadiusX
    def getBorderY(self): return self.config.regionRadiusY
    def getMinDisparity(self): return self.config.minDisparity
    def getRangeDisparity(self): return self.config.rangeDisparity
    def getInvalidValue(self): return self.config.rangeDisparity
    def getInputType(self): return GrayU8
    def getDisparityType(self): return self.dispType


class FactoryStereoDisparity:
    """F:factory/feature/disparity/FactoryStereoDisparity.java"""

    @staticmethod
    def blockMatch(config=None, imageType=GrayU8, dispType=GrayF32, ctx=None):
        """blockMatch(config, imageType, dispType) (:62-144, 203-240).  IllegalArgumentException where the factory and the constructors it calls
        throw it; the branches the GPU does not have (CENSUS, NCC, inputs other than GrayU8) raise RuntimeError: use the Java path."""
        if config is None:
            config = ConfigDisparityBM()
        if config.subpixel:
            if dispType is not GrayF32:
                raise IllegalArgumentException("With subpixel on, disparity image must be GrayF32")
        elif dispType is not GrayU8:
            raise IllegalArgumentException("With subpixel on, disparity image must be GrayU8")
        if config.errorType not in (DisparityError.SAD, DisparityError.CENSUS, DisparityError.NCC):
            raise IllegalArgumentException("Unsupported error type %s" % config.errorType)
        if config.errorType != DisparityError.SAD:
            raise RuntimeError("only errorType = SAD is implemented on the GPU (use the Java path)")
        if imageType not in (GrayU8, GrayS16, GrayF32):   # createDisparitySelect / createScoreRowSad (GrayU16 has no mirror here)
            raise IllegalArgumentException("Unsupported image type %s" % getattr(imageType, "__name__", imageType))
        # DisparityBlockMatchRowFormat constructor :72-75
        maxDisparity = config.minDisparity + config.rangeDisparity
        if maxDisparity <= 0:
            raise IllegalArgumentException("Max disparity must be greater than zero. max=%d" % maxDisparity)
        if config.minDisparity < 0 or config.minDisparity >= maxDisparity:
            raise IllegalArgumentException("Min disparity must be >= 0 and < maxDisparity. min=%d max=%d" % (config.minDisparity, maxDisparity))
        if imageType is not GrayU8:
            raise RuntimeError("only GrayU8 images are implemented on the GPU (use the Java path)")
        return StereoDisparity(config, dispType, ctx)

    @staticmethod
    def blockMatchBest5(config=None, imageType=GrayU8, dispType=GrayF32, ctx=None):
        raise RuntimeError("blockMatchBest5 is not implemented on the GPU (use the Java path)")

    @staticmethod
    def sgm(config=None, imageType=GrayU8, dispType=GrayF32, ctx=None):
        raise RuntimeError("semi-global matching is not implemented on the GPU (use the Java path)")

    @staticmethod
    def regionSparseWta(*args, **kwargs):
        raise RuntimeError("regionSparseWta is not implemented on the GPU (use the Java path)")
