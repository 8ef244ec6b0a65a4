"""Thresholding: gray image -> binary image (I:factory/filter/binary, I:abst/filter/binary, I:alg/filter/binary, T:struct/ConfigLength.java).
  FactoryThresholdBinary.threshold(ConfigThreshold, type) -> InputToBinary     I:factory/filter/binary/FactoryThresholdBinary.java:318-372
  BOverrideFactoryThresholdBinary hooks (the provider seam)                    I:factory/filter/binary/BOverrideFactoryThresholdBinary.java

A module beside the api package (like device.py and sharded.py): it takes the image types and the view marshaller from boofcv_amd.api and adds
no name there.  Implemented on the GPU: FIXED, LOCAL_MEAN, LOCAL_GAUSSIAN, BLOCK_MIN_MAX and BLOCK_MEAN on GrayU8 and GrayF32, GLOBAL_OTSU
(pixel range 0..255) and BLOCK_OTSU on GrayU8.  Everything else is refused with IllegalArgumentException when the filter is created."""
import enum

import numpy as np

from . import _lib
from .api.core import IllegalArgumentException, _check, _ctx
from .api.image import GrayF32, GrayU8

__all__ = ["ConfigLength", "ConfigThreshold", "ConfigThresholdBlockMinMax", "ConfigThresholdLocalOtsu", "FactoryThresholdBinary", "GThresholdImageOps",
           "InputToBinary", "ThresholdImageOps", "ThresholdType"]


class ThresholdType(enum.IntEnum):
    """I:factory/filter/binary/ThresholdType.java:28-109 (ordinals = BHIP_THRESHOLD_*)"""
    FIXED = _lib.BHIP_THRESHOLD_FIXED
    GLOBAL_ENTROPY = _lib.BHIP_THRESHOLD_GLOBAL_ENTROPY
    GLOBAL_OTSU = _lib.BHIP_THRESHOLD_GLOBAL_OTSU
    GLOBAL_LI = _lib.BHIP_THRESHOLD_GLOBAL_LI
    GLOBAL_HUANG = _lib.BHIP_THRESHOLD_GLOBAL_HUANG
    LOCAL_GAUSSIAN = _lib.BHIP_THRESHOLD_LOCAL_GAUSSIAN
    LOCAL_MEAN = _lib.BHIP_THRESHOLD_LOCAL_MEAN
    LOCAL_OTSU = _lib.BHIP_THRESHOLD_LOCAL_OTSU
    BLOCK_MIN_MAX = _lib.BHIP_THRESHOLD_BLOCK_MIN_MAX
    BLOCK_MEAN = _lib.BHIP_THRESHOLD_BLOCK_MEAN
    BLOCK_OTSU = _lib.BHIP_THRESHOLD_BLOCK_OTSU
    LOCAL_SAVOLA = _lib.BHIP_THRESHOLD_LOCAL_SAVOLA
    LOCAL_NICK = _lib.BHIP_THRESHOLD_LOCAL_NICK

    def isAdaptive(self):
        return self is not ThresholdType.FIXED

    def isGlobal(self):
        return self <= ThresholdType.GLOBAL_HUANG


_BOTH = (ThresholdType.FIXED, ThresholdType.LOCAL_MEAN, ThresholdType.LOCAL_GAUSSIAN, ThresholdType.BLOCK_MIN_MAX, ThresholdType.BLOCK_MEAN)
_U8_ONLY = (ThresholdType.GLOBAL_OTSU, ThresholdType.BLOCK_OTSU)


class ConfigLength:
    """T:struct/ConfigLength.java: a length in pixels, fixed or relative to a total with a minimum"""

    def __init__(self, length=-1.0, fraction=-1.0):
        self.length, self.fraction = float(length), float(fraction)

    @staticmethod
    def fixed(pixels):
        return ConfigLength(pixels, -1)

    @staticmethod
    def relative(fraction, minimum):
        return ConfigLength(minimum, fraction)

    def compute(self, totalLength):
        return max(self.fraction * totalLength, self.length) if self.fraction >= 0 else self.length

    def computeI(self, totalLength):
        size = self.compute(totalLength)
        return int(size + 0.5) if size >= 0 else -1

    def isRelative(self):
        return self.fraction >= 0

    def isFixed(self):
        return self.fraction < 0

    def getLengthI(self):
        return int(self.length + 0.5)

    def checkValidity(self):
        if self.length < 0 and self.fraction < 0:
            raise IllegalArgumentException("length and/or fraction must be >= 0")

    def copy(self):
        return ConfigLength(self.length, self.fraction)


def _length(width):
    return width if isinstance(width, ConfigLength) else ConfigLength.fixed(width)


class ConfigThreshold:
    """I:factory/filter/binary/ConfigThreshold.java:30-133"""

    def __init__(self):
        self.type = None
        self.fixedThreshold = 0.0
        self.scale = 1.0
        self.down = True
        self.width = ConfigLength.fixed(11)
        self.savolaK = 0.3
        self.nickK = -0.2
        self.minPixelValue = 0
        self.maxPixelValue = 255
        self.thresholdFromLocalBlocks = True

    @staticmethod
    def fixed(value):
        config = ConfigThreshold()
        config.type = ThresholdType.FIXED
        config.fixedThreshold = float(value)
        return config

    @staticmethod
    def global_(type):
        type = ThresholdType(type)
        if not type.isAdaptive():
            raise IllegalArgumentException("Type must be adaptive")
        if not type.isGlobal():
            raise IllegalArgumentException("Type must be global")
        config = ConfigThreshold()
        config.type = type
        return config

    @staticmethod
    def local(type, width):
        type = ThresholdType(type)
        if not type.isAdaptive():
            raise IllegalArgumentException("Type must be adaptive")
        if type.isGlobal():
            raise IllegalArgumentException("Type must be local")
        if type == ThresholdType.BLOCK_MIN_MAX:
            config = ConfigThresholdBlockMinMax(_length(width), 10, True)
        elif type == ThresholdType.BLOCK_OTSU:
            config = ConfigThresholdLocalOtsu()
        else:
            config = ConfigThreshold()
        config.scale = 0.95
        config.type = type
        config.width = _length(width)
        return config

    def checkValidity(self):
        pass

    def _c(self):
        """the bhip_threshold_cfg of this configuration"""
        if self.type is None:
            raise IllegalArgumentException("Unknown type None")
        return _lib.ThresholdCfg(int(self.type), float(self.fixedThreshold), float(self.scale), int(bool(self.down)), float(self.width.length),
                                 float(self.width.fraction), int(self.minPixelValue), int(self.maxPixelValue), int(bool(self.thresholdFromLocalBlocks)),
                                 float(getattr(self, "minimumSpread", 10.0)), int(bool(getattr(self, "useOtsu2", True))), float(getattr(self, "tuning", 0.0)))


class ConfigThresholdBlockMinMax(ConfigThreshold):
    """I:factory/filter/binary/ConfigThresholdBlockMinMax.java"""

    def __init__(self, width=None, minimumSpread=10.0, down=None):
        super().__init__()
        self.scale = 0.85
        self.minimumSpread = float(minimumSpread)
        if width is not None:
            self.type = ThresholdType.BLOCK_MIN_MAX
            self.width = _length(width)
            self.down = bool(down)


class ConfigThresholdLocalOtsu(ConfigThreshold):
    """I:factory/filter/binary/ConfigThresholdLocalOtsu.java"""

    def __init__(self, regionWidth=None, tuning=0.0):
        super().__init__()
        self.type = ThresholdType.BLOCK_OTSU
        self.tuning = float(tuning)
        self.useOtsu2 = True
        if regionWidth is not None:
            self.width = _length(regionWidth)


def _refuse(type, imageType):
    type = ThresholdType(type)
    if imageType not in (GrayU8, GrayF32):
        raise IllegalArgumentException("only GrayU8 and GrayF32 are implemented on the GPU")
    if type not in _BOTH and not (type in _U8_ONLY and imageType is GrayU8):
        raise IllegalArgumentException("%s on %s is not implemented on the GPU" % (type.name, imageType.__name__))


class InputToBinary:
    """I:abst/filter/binary/InputToBinary.java: process(input, output) writes the GrayU8 0/1 image"""

    def __init__(self, config, imageType, ctx=None):
        _refuse(config.type, imageType)
        if config.type == ThresholdType.GLOBAL_OTSU and (config.minPixelValue, config.maxPixelValue) != (0, 255):
            raise IllegalArgumentException("GLOBAL_OTSU is implemented on the GPU for the pixel range 0..255")
        self.config, self.imageType, self.ctx = config, imageType, ctx

    def getInputType(self):
        return self.imageType

    def process(self, input, output):
        if not isinstance(input, self.imageType) or not isinstance(output, GrayU8):
            raise IllegalArgumentException("expected a %s input and a GrayU8 output" % self.imageType.__name__)
        if (output.width, output.height) != (input.width, input.height):
            if not ThresholdType.BLOCK_MIN_MAX <= self.config.type <= ThresholdType.BLOCK_OTSU:
                raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape
            output.reshape(input.width, input.height)   # ThresholdBlock.process
        ctx = _ctx(self.ctx)
        s, d = input._in(), output._out()
        fn = _lib.load().bhip_threshold_u8 if self.imageType is GrayU8 else _lib.load().bhip_threshold_f32
        _check(ctx, fn(ctx._h, self.config._c(), *s, *d))
        return output


def _cfg(type, width=None, scale=1.0, down=True, **more):
    c = ConfigThresholdBlockMinMax() if type == ThresholdType.BLOCK_MIN_MAX else ConfigThresholdLocalOtsu() if type == ThresholdType.BLOCK_OTSU else ConfigThreshold()
    c.type, c.scale, c.down = ThresholdType(type), float(scale), bool(down)
    if width is not None:
        c.width = _length(width)
    for k, v in more.items():
        setattr(c, k, v)
    return c


class FactoryThresholdBinary:
    """I:factory/filter/binary/FactoryThresholdBinary.java"""

    @staticmethod
    def threshold(config, inputType, ctx=None):
        if config.type is None or int(config.type) not in [int(t) for t in ThresholdType]:
            raise IllegalArgumentException("Unknown type %s" % config.type)
        return InputToBinary(config, inputType, ctx)

    @staticmethod
    def globalFixed(threshold, down, inputType, ctx=None):
        return InputToBinary(_cfg(ThresholdType.FIXED, down=down, fixedThreshold=float(threshold)), inputType, ctx)

    @staticmethod
    def globalOtsu(minValue, maxValue, scale, down, inputType, ctx=None):
        return InputToBinary(_cfg(ThresholdType.GLOBAL_OTSU, scale=scale, down=down, minPixelValue=minValue, maxPixelValue=maxValue), inputType, ctx)

    @staticmethod
    def localMean(width, scale, down, inputType, ctx=None):
        return InputToBinary(_cfg(ThresholdType.LOCAL_MEAN, width, scale, down), inputType, ctx)

    @staticmethod
    def localGaussian(regionWidth, scale, down, inputType, ctx=None):
        return InputToBinary(_cfg(ThresholdType.LOCAL_GAUSSIAN, regionWidth, scale, down), inputType, ctx)

    @staticmethod
    def blockMinMax(regionWidth, scale, down, thresholdFromLocalBlocks, minimumSpread, inputType, ctx=None):
        return InputToBinary(_cfg(ThresholdType.BLOCK_MIN_MAX, regionWidth, scale, down, thresholdFromLocalBlocks=thresholdFromLocalBlocks,
                                  minimumSpread=float(minimumSpread)), inputType, ctx)

    @staticmethod
    def blockMean(regionWidth, scale, down, thresholdFromLocalBlocks, inputType, ctx=None):
        return InputToBinary(_cfg(ThresholdType.BLOCK_MEAN, regionWidth, scale, down, thresholdFromLocalBlocks=thresholdFromLocalBlocks), inputType, ctx)

    @staticmethod
    def blockOtsu(regionWidth, scale, down, thresholdFromLocalBlocks, otsu2, tuning, inputType, ctx=None):
        return InputToBinary(_cfg(ThresholdType.BLOCK_OTSU, regionWidth, scale, down, thresholdFromLocalBlocks=thresholdFromLocalBlocks, useOtsu2=bool(otsu2),
                                  tuning=float(tuning)), inputType, ctx)

    # the factory methods of the types that stay on the Java path
    @staticmethod
    def localSauvola(width, down, k, inputType, ctx=None):
        _refuse(ThresholdType.LOCAL_SAVOLA, inputType)

    @staticmethod
    def localNick(width, down, k, inputType, ctx=None):
        _refuse(ThresholdType.LOCAL_NICK, inputType)

    @staticmethod
    def localOtsu(regionWidth, scale, down, otsu2, tuning, inputType, ctx=None):
        _refuse(ThresholdType.LOCAL_OTSU, inputType)

    @staticmethod
    def globalEntropy(minValue, maxValue, scale, down, inputType, ctx=None):
        _refuse(ThresholdType.GLOBAL_ENTROPY, inputType)

    @staticmethod
    def globalLi(minValue, maxValue, scale, down, inputType, ctx=None):
        _refuse(ThresholdType.GLOBAL_LI, inputType)

    @staticmethod
    def globalHuang(minValue, maxValue, scale, down, inputType, ctx=None):
        _refuse(ThresholdType.GLOBAL_HUANG, inputType)


class GThresholdImageOps:
    """I:alg/filter/binary/GThresholdImageOps.java (ThresholdImageOps.java has the typed forms of the same functions)"""

    @staticmethod
    def _run(config, input, output, ctx):
        if output is None:
            output = GrayU8(input.width, input.height)
        return InputToBinary(config, type(input), ctx).process(input, output)

    @staticmethod
    def threshold(input, output, threshold, down, ctx=None):
        return GThresholdImageOps._run(_cfg(ThresholdType.FIXED, down=down, fixedThreshold=float(threshold)), input, output, ctx)

    @staticmethod
    def localMean(input, output, width, scale, down, storage1=None, storage2=None, storage3=None, ctx=None):
        return GThresholdImageOps._run(_cfg(ThresholdType.LOCAL_MEAN, width, scale, down), input, output, ctx)

    @staticmethod
    def localGaussian(input, output, width, scale, down, storage1=None, storage2=None, ctx=None):
        return GThresholdImageOps._run(_cfg(ThresholdType.LOCAL_GAUSSIAN, width, scale, down), input, output, ctx)

    @staticmethod
    def computeOtsu(histogram, length=None, totalPixels=None):
        """computeOtsu(int[] histogram, int length, int totalPixels) (:105-142), or computeOtsu(GrayU8 input, minValue, maxValue) (:56-67) with the
        histogram of the host image.  A few hundred scalar operations on the host, as in the reference; the filters compute it on the device."""
        if isinstance(histogram, GrayU8):
            image, minValue, maxValue = histogram, int(length), int(totalPixels)
            image._in()
            counts = np.bincount(image.array().reshape(-1).astype(np.int64) - minValue, minlength=1 + maxValue - minValue)
            return GThresholdImageOps.computeOtsu(counts, len(counts), image.width * image.height) + minValue
        dlength = float(length)
        total = 0.0
        for i in range(length):
            total += (i / dlength) * int(histogram[i])
        sumB, wB, varMax, threshold = 0.0, 0, 0.0, 0
        for i in range(length):
            wB += int(histogram[i])
            if wB == 0:
                continue
            wF = totalPixels - wB
            if wF == 0:
                break
            sumB += (i / dlength) * int(histogram[i])
            mB = sumB / wB
            mF = (total - sumB) / wF
            varBetween = float(wB) * float(wF) * (mB - mF) * (mB - mF)
            if varBetween > varMax:
                varMax, threshold = varBetween, i
        return threshold


ThresholdImageOps = GThresholdImageOps
