"""Stationary background models (F:alg/background/stationary/*.java, F:factory/background/*.java)."""
import ctypes as C

import numpy as np

from .. import _lib
from .core import Context, IllegalArgumentException, _check, _NativeObject
from .image import GrayF32, GrayU8, InterleavedType, Planar, PlanarType
from .distort import InterpolationType

__all__ = ["BackgroundModelStationary", "BackgroundStationaryBasic", "BackgroundStationaryGaussian", "BackgroundStationaryGmm", "ConfigBackground",
           "ConfigBackgroundBasic", "ConfigBackgroundGaussian", "ConfigBackgroundGmm", "FactoryBackgroundModel", "Float_MIN_VALUE"]


Float_MIN_VALUE = np.float32(1.401298464324817e-45)


class ConfigBackground:
    """F:factory/background/ConfigBackground.java"""
    unknownValue = 0


class ConfigBackgroundBasic(ConfigBackground):
    """F:factory/background/ConfigBackgroundBasic.java"""

    def __init__(self, threshold, learnRate=0.05):
        self.threshold, self.learnRate = threshold, learnRate
        self.interpolation = InterpolationType.BILINEAR
        self.unknownValue = 0

    def checkValidity(self):
        if self.learnRate < 0 or self.learnRate > 1:
            raise IllegalArgumentException("Learn rate must be 0 <= rate <= 1")
        if self.threshold <= 0:
            raise IllegalArgumentException("threshold must be > 0")


class ConfigBackgroundGaussian(ConfigBackground):
    """F:factory/background/ConfigBackgroundGaussian.java"""

    def __init__(self, threshold, learnRate=0.05):
        self.threshold, self.learnRate = threshold, learnRate
        self.initialVariance = Float_MIN_VALUE
        self.minimumDifference = 0
        self.interpolation = InterpolationType.BILINEAR
        self.unknownValue = 0

    def checkValidity(self):
        if self.learnRate < 0 or self.learnRate > 1:
            raise IllegalArgumentException("Learn rate must be 0 <= rate <= 1")
        if self.threshold <= 0:
            raise IllegalArgumentException("threshold must be > 0")
        if self.initialVariance == 0:
            raise IllegalArgumentException("Don't set initialVariance to zero, set it to Float.MIN_VALUE instead")
        if self.initialVariance < 0:
            raise IllegalArgumentException("Variance must be set to a value larger than zero")
        if self.minimumDifference < 0:
            raise IllegalArgumentException("minimumDifference must be >= 0")


class ConfigBackgroundGmm(ConfigBackground):
    """F:factory/background/ConfigBackgroundGmm.java"""

    def __init__(self):
        self.learningPeriod = 1000.0
        self.initialVariance = 400
        self.decayCoefient = 0.005
        self.maxDistance = 3
        self.numberOfGaussian = 5
        self.significantWeight = 0.01
        self.unknownValue = 0

    def checkValidity(self):
        if self.learningPeriod <= 0:
            raise IllegalArgumentException("Learning period must be more than zero")
        if self.decayCoefient < 0:
            raise IllegalArgumentException("Decay coeffient must be more than or equal to zero")
        if self.initialVariance == 0:
            raise IllegalArgumentException("Don't set initialVariance to zero, set it to Float.MIN_VALUE instead")
        if self.initialVariance < 0:
            raise IllegalArgumentException("Variance must be set to a value larger than zero")


def _bg_image_kind(imageType):
    """-> (bhip_image_family, bhip_pixel_type, bands) of GrayU8 / GrayF32 / PlanarType(n, GrayU8 / GrayF32); everything else is the Java path"""
    if isinstance(imageType, InterleavedType):
        raise RuntimeError("interleaved images are not implemented on the GPU (use the Java path)")
    family, band, bands = (_lib.BHIP_IMAGE_PLANAR, imageType.bandType, imageType.numBands) if isinstance(imageType, PlanarType) else (_lib.BHIP_IMAGE_GRAY, imageType, 0)
    if band not in (GrayU8, GrayF32):
        raise RuntimeError("only GrayU8 and GrayF32 bands are implemented on the GPU (use the Java path)")
    if family == _lib.BHIP_IMAGE_PLANAR and bands < 1:
        raise IllegalArgumentException("a Planar image has at least one band")
    if bands > 4:
        raise RuntimeError("at most 4 bands are implemented on the GPU (use the Java path)")
    return family, (_lib.BHIP_PIXEL_U8 if band is GrayU8 else _lib.BHIP_PIXEL_F32), bands


class BackgroundModelStationary(_NativeObject):
    """BackgroundModel + BackgroundModelStationary (F:alg/background/BackgroundModel.java, BackgroundModelStationary.java) over one bhip_bg with
    one stream.  The native handle has a fixed frame size: this class creates it at the first frame and replaces it when the reference
    re-initialises for another size; the InputSanityCheck errors are raised here."""
    _alg = None
    _destroy = "bhip_bg_destroy"

    def __init__(self, imageType, ctx=None):
        self.imageType = imageType
        self._family, self._pixel, self._bands = _bg_image_kind(imageType)
        self.ctx = ctx              # None: Context.default(), looked up when the handle is created
        self._size = None           # (width, height) the handle was created for
        self.unknownValue = 0
        self._mw = self._mh = 0     # the reference model's width / height ("not initialised" is a test on them)

    # ---- BackgroundModel ----
    def getUnknownValue(self):
        return self.unknownValue & 0xFF

    def setUnknownValue(self, unknownValue):
        if unknownValue < 0 or unknownValue > 255:
            raise IllegalArgumentException("out of range. 0 to 255")
        self.unknownValue = int(unknownValue)
        if self._h:
            _check(self.ctx, _lib.load().bhip_bg_set_unknown_value(self._h, self.unknownValue))

    def getImageType(self):
        return self.imageType

    def _closed(self):
        self._size = None

    # ---- the native side ----
    def _set(self, name, value):
        if self._h:
            _check(self.ctx, getattr(_lib.load(), "bhip_bg_set_" + name)(self._h, value))

    def _handle(self, width, height):
        """the handle for width x height frames, created (and the old one dropped) when the size differs"""
        if self._h and self._size == (width, height):
            return
        self.close()
        if self.ctx is None:
            self.ctx = Context.default()
        h = C.c_void_p()
        _check(self.ctx, self._create(_lib.load(), width, height, h))
        self._adopt(h)
        self._size = (width, height)
        self._push()
        self._set("unknown_value", self.unknownValue)

    def _frame(self, frame):
        """-> (pointer, start, bandStride, stride, width, height, keep-alive)"""
        if self._family == _lib.BHIP_IMAGE_GRAY:
            if not isinstance(frame, self.imageType):
                raise IllegalArgumentException("this model takes %s frames" % self.imageType.__name__)
            ptr, start, stride, w, h = frame._in()
            return ptr, start, 0, stride, w, h, frame
        if not isinstance(frame, Planar) or frame.getNumBands() != self._bands or any(not isinstance(b, self.imageType.bandType) for b in frame.bands):
            raise IllegalArgumentException("this model takes Planar<%s> frames of %d bands" % (self.imageType.bandType.__name__, self._bands))
        a = np.ascontiguousarray(np.stack([b.array() for b in frame.bands]))
        ptr = a.ctypes.data_as(_lib._u8p if a.dtype == np.uint8 else _lib._fp)
        return ptr, 0, frame.width * frame.height, frame.width, frame.width, frame.height, a

    def _call(self, segment, frame, mask):
        L = _lib.load()
        u8 = self._pixel == _lib.BHIP_PIXEL_U8
        ptr, start, bandStride, stride, w, h, keep = self._frame(frame)
        mp, ms, mst = mask._out() if mask is not None else (None, 0, 0)
        if segment:
            fn = L.bhip_bg_segment_u8 if u8 else L.bhip_bg_segment_f32
            _check(self.ctx, fn(self._h, ptr, start, 0, bandStride, stride, mp, ms, 0, mst))
        else:
            fn = L.bhip_bg_update_u8 if u8 else L.bhip_bg_update_f32
            _check(self.ctx, fn(self._h, ptr, start, 0, 0, bandStride, stride, 1, mp, ms, 0, 0, mst))
        del keep

    def _fetch(self):
        L = _lib.load()
        n = C.c_longlong()
        _check(self.ctx, L.bhip_bg_model_floats(self._h, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        _check(self.ctx, L.bhip_bg_fetch_model(self._h, 0, out.ctypes.data_as(_lib._fp)))
        return out

    @staticmethod
    def _same_shape(*imgs):
        for im in imgs[1:]:
            if im.width != imgs[0].width or im.height != imgs[0].height:
                raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape

    @staticmethod
    def _fill(segmented, value):
        segmented.array()[...] = value   # ImageMiscOps.fill

    def reset(self):
        self._mw = self._mh = self._reset_size
        if self._h:
            _check(self.ctx, _lib.load().bhip_bg_reset(self._h, -1))


class BackgroundStationaryBasic(BackgroundModelStationary):
    """BackgroundStationaryBasic_SB / _PL (F:alg/background/stationary/BackgroundStationaryBasic.java, _SB.java:58-123, _PL.java:66-142)"""
    _reset_size = 0

    def __init__(self, learnRate, threshold, imageType, ctx=None):
        super().__init__(imageType, ctx)
        if learnRate < 0 or learnRate > 1:
            raise IllegalArgumentException("LearnRate must be 0 <= rate <= 1.0f")
        self.learnRate, self.threshold = float(learnRate), float(threshold)

    def _create(self, L, width, height, h):
        cfg = _lib.BgBasicCfg()
        L.bhip_bg_basic_cfg_default(C.byref(cfg))
        cfg.threshold = 1
        return L.bhip_bg_create_basic(self.ctx._h, C.byref(cfg), self._family, self._pixel, self._bands, width, height, 1, C.byref(h))

    def _push(self):
        self._set("learn_rate", self.learnRate)
        self._set("threshold", self.threshold)

    def getLearnRate(self):
        return self.learnRate

    def setLearnRate(self, learnRate):
        self.learnRate = float(learnRate)
        self._set("learn_rate", self.learnRate)

    def getThreshold(self):
        return self.threshold

    def setThreshold(self, threshold):
        self.threshold = float(threshold)
        self._set("threshold", self.threshold)

    def _uninitialised(self, frame):
        return self._mw != frame.width

    def updateBackground(self, frame, mask=None):
        """updateBackground(frame) or updateBackground(frame, segment): update, then segment"""
        if self._uninitialised(frame):
            self._handle(frame.width, frame.height)
            _check(self.ctx, _lib.load().bhip_bg_reset(self._h, -1))
            self._mw, self._mh = frame.width, frame.height
        elif (self._mw, self._mh) != (frame.width, frame.height):
            raise IllegalArgumentException("Image shapes do not match")
        self._call(False, frame, None)
        if mask is not None:
            self.segment(frame, mask)

    def segment(self, frame, segmented):
        if self._uninitialised(frame):
            self._fill(segmented, self.unknownValue)
            return
        if (self._mw, self._mh) != (frame.width, frame.height):
            raise IllegalArgumentException("Image shapes do not match")
        self._same_shape(frame, segmented)
        self._call(True, frame, segmented)

    def getBackground(self):
        nb = max(self._bands, 1)
        if self._mw == 0 or not self._h:
            bands = [GrayF32(0, 0) for _ in range(nb)]
        else:
            a = self._fetch().reshape(nb, self._mh, self._mw)
            bands = [GrayF32.wrap(a[b]) for b in range(nb)]
        return bands[0] if self._family == _lib.BHIP_IMAGE_GRAY else Planar.wrap(bands)


class BackgroundStationaryGaussian(BackgroundStationaryBasic):
    """BackgroundStationaryGaussian_SB / _PL (F:alg/background/stationary/BackgroundStationaryGaussian.java, _SB.java:58-142, _PL.java:72-180).
    "Not initialised" is `background.width == 1`, so a model of width 1 never initialises (the native library reproduces that for width 1)."""
    _reset_size = 1

    def __init__(self, learnRate, threshold, imageType, ctx=None):
        BackgroundModelStationary.__init__(self, imageType, ctx)
        if threshold < 0:
            raise IllegalArgumentException("Threshold must be more than 0")
        self.learnRate, self.threshold = float(learnRate), float(threshold)
        self.initialVariance = Float_MIN_VALUE
        self.minimumDifference = 0.0
        self._mw = self._mh = 1

    def _create(self, L, width, height, h):
        cfg = _lib.BgGaussianCfg()
        L.bhip_bg_gaussian_cfg_default(C.byref(cfg))
        cfg.threshold = 1
        return L.bhip_bg_create_gaussian(self.ctx._h, C.byref(cfg), self._family, self._pixel, self._bands, width, height, 1, C.byref(h))

    def _push(self):
        BackgroundStationaryBasic._push(self)
        self._set("initial_variance", self.initialVariance)
        self._set("minimum_difference", self.minimumDifference)

    def getInitialVariance(self):
        return self.initialVariance

    def setInitialVariance(self, initialVariance):
        self.initialVariance = float(initialVariance)
        self._set("initial_variance", self.initialVariance)

    def getMinimumDifference(self):
        return self.minimumDifference

    def setMinimumDifference(self, minimumDifference):
        self.minimumDifference = float(minimumDifference)
        self._set("minimum_difference", self.minimumDifference)

    def _uninitialised(self, frame):
        return self._mw == 1

    def getBackground(self):
        raise AttributeError("BackgroundStationaryGaussian has no getBackground()")


class BackgroundStationaryGmm(BackgroundModelStationary):
    """BackgroundStationaryGmm_SB / _MB (F:alg/background/stationary/BackgroundStationaryGmm.java:48-78, _SB.java:50-100, _MB.java:54-105) with
    BackgroundGmmCommon's constructor defaults: maxDistance 3*3, significantWeight min(0.2f, 100*learningRate), initialVariance 100."""
    _reset_size = 0

    def __init__(self, learningPeriod, decayCoef, maxGaussians, imageType, ctx=None):
        super().__init__(imageType, ctx)
        if learningPeriod <= 0:
            raise IllegalArgumentException("Must be greater than zero")
        if maxGaussians >= 256 or maxGaussians <= 0:
            raise IllegalArgumentException("Maximum number of gaussians per pixel is 255")
        if maxGaussians > 8:
            raise RuntimeError("more than 8 Gaussians per pixel are not implemented on the GPU (use the Java path)")
        self.learningRate = np.float32(1.0) / np.float32(learningPeriod)
        self._period = float(learningPeriod)
        self.decay = float(decayCoef)
        self.maxGaussians = int(maxGaussians)
        self.maxDistance = 9.0
        self.significantWeight = float(min(np.float32(0.2), np.float32(100) * self.learningRate))
        self.initialVariance = 100.0
        self._commonUnknown = 0     # BackgroundGmmCommon.unknownValue: refreshed only by segment() on an initialised model

    def _create(self, L, width, height, h):
        cfg = _lib.BgGmmCfg()
        L.bhip_bg_gmm_cfg_default(C.byref(cfg))
        cfg.numberOfGaussian = self.maxGaussians
        cfg.decayCoefient = self.decay
        return L.bhip_bg_create_gmm(self.ctx._h, C.byref(cfg), self._family, self._pixel, self._bands, width, height, 1, C.byref(h))

    def _push(self):
        self._set("learning_period", self._period)
        self._set("initial_variance", self.initialVariance)
        self._set("max_distance", self.maxDistance)
        self._set("significant_weight", self.significantWeight)
        self._set("common_unknown_value", self._commonUnknown)

    def getInitialVariance(self):
        return self.initialVariance

    def setInitialVariance(self, initialVariance):
        self.initialVariance = float(initialVariance)
        self._set("initial_variance", self.initialVariance)

    def getLearningPeriod(self):
        return float(np.float32(1.0) / self.learningRate)

    def setLearningPeriod(self, period):
        self._period = float(period)
        with np.errstate(divide="ignore"):
            self.learningRate = np.float32(1.0) / np.float32(period)
        self._set("learning_period", self._period)

    def getSignificantWeight(self):
        return self.significantWeight

    def setSignificantWeight(self, value):
        self.significantWeight = float(value)
        self._set("significant_weight", self.significantWeight)

    def getMaxDistance(self):
        return self.maxDistance

    def setMaxDistance(self, maxDistance):
        self.maxDistance = float(maxDistance)
        self._set("max_distance", self.maxDistance)

    def updateBackground(self, frame, mask=None):
        if (self._mw, self._mh) != (frame.width, frame.height):
            self._handle(frame.width, frame.height)
            _check(self.ctx, _lib.load().bhip_bg_reset(self._h, -1))
            self._mw, self._mh = frame.width, frame.height
        if mask is not None:
            mask.reshape(frame.width, frame.height)
        self._call(False, frame, mask)

    def segment(self, frame, segmented):
        if (self._mw, self._mh) != (frame.width, frame.height):
            segmented.reshape(frame.width, frame.height)
            self._fill(segmented, self.unknownValue)
            return
        self._commonUnknown = self.unknownValue
        self._same_shape(frame, segmented)
        self._call(True, frame, segmented)


class FactoryBackgroundModel:
    """F:factory/background/FactoryBackgroundModel.java:47-64,112-141,193-225.  The moving* models warp the model through a homography before
    every update; they are not implemented on the GPU."""

    @staticmethod
    def stationaryBasic(config, imageType, ctx=None):
        config.checkValidity()
        return BackgroundStationaryBasic(config.learnRate, config.threshold, imageType, ctx)   # config.unknownValue is not forwarded (:47-64)

    @staticmethod
    def stationaryGaussian(config, imageType, ctx=None):
        config.checkValidity()
        ret = BackgroundStationaryGaussian(config.learnRate, config.threshold, imageType, ctx)
        ret.setInitialVariance(config.initialVariance)
        ret.setMinimumDifference(config.minimumDifference)
        ret.setUnknownValue(config.unknownValue)
        return ret

    @staticmethod
    def stationaryGmm(config, imageType, ctx=None):
        if config is None:
            config = ConfigBackgroundGmm()
        else:
            config.checkValidity()
        ret = BackgroundStationaryGmm(config.learningPeriod, config.decayCoefient, config.numberOfGaussian, imageType, ctx)
        ret.setInitialVariance(config.initialVariance)
        ret.setMaxDistance(config.maxDistance)
        ret.setSignificantWeight(config.significantWeight)
        ret.setUnknownValue(config.unknownValue)
        return ret

    @staticmethod
    def movingBasic(config, transform, imageType, ctx=None):
        raise RuntimeError("BackgroundMovingBasic is not implemented on the GPU (use the Java path)")

    @staticmethod
    def movingGaussian(config, transform, imageType, ctx=None):
        raise RuntimeError("BackgroundMovingGaussian is not implemented on the GPU (use the Java path)")

    @staticmethod
    def movingGmm(config, transform, imageType, ctx=None):
        raise RuntimeError("BackgroundMovingGmm is not implemented on the GPU (use the Java path)")
