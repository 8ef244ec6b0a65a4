"""Point detection: integral image, Fast-Hessian, non-maximum suppression, N-best, corner and FAST intensities, the general detector
(I:alg/transform/ii, F:alg/feature/detect/{intensity,extract,interest}, F:abst/feature/detect, F:factory/feature/detect).  The static op
classes are what the BOverride* hooks replace."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .core import Float_MAX_VALUE, IllegalArgumentException, _check, _ctx
from .image import GrayF32, GrayS16, GrayS32, GrayU8, Point2D_I16

__all__ = ["ConfigExtract", "ConfigFastCorner", "ConfigFastHessian", "ConfigGeneralDetector", "FactoryDetectPoint", "FactoryFeatureExtractor",
           "FactoryIntensityPointAlg", "FastCornerDetector", "FastHessianFeatureDetector", "GeneralFeatureDetector", "GradientCornerIntensity",
           "IntegralImageFeatureIntensity", "IntegralImageOps", "NonMaxSuppression", "SelectNBestFeatures", "WrapFastToPointDetector",
           "WrapperFastCornerIntensity"]


@dataclass
class ConfigFastHessian:
    """F:abst/feature/detect/interest/ConfigFastHessian.java:33-70"""
    detectThreshold: float = 1.0
    extractRadius: int = 2
    maxFeaturesPerScale: int = -1
    initialSampleSize: int = 1
    initialSize: int = 9
    numberScalesPerOctave: int = 4
    numberOfOctaves: int = 4
    scaleStepSize: int = 6

    def _c(self):
        return _lib.FhCfg(self.detectThreshold, self.extractRadius, self.maxFeaturesPerScale, self.initialSampleSize, self.initialSize,
                          self.numberScalesPerOctave, self.numberOfOctaves, self.scaleStepSize)


@dataclass
class ConfigExtract:
    """F:abst/feature/detect/extract/ConfigExtract.java:32-56"""
    radius: int = 1
    threshold: float = 0.0
    ignoreBorder: int = 0
    useStrictRule: bool = True
    detectMinimums: bool = False
    detectMaximums: bool = True

    def checkValidity(self):
        if self.radius <= 0:
            raise IllegalArgumentException("Search radius must be >= 1")
        if self.ignoreBorder < 0:
            raise IllegalArgumentException("Ignore border must be >= 0 ")


@dataclass
class ConfigGeneralDetector(ConfigExtract):
    """F:abst/feature/detect/interest/ConfigGeneralDetector.java:34-70"""
    maxFeatures: int = -1


class IntegralImageOps:
    @staticmethod
    def transform(input, transformed=None, ctx=None):
        """GIntegralImageOps.transform (I:alg/transform/ii/GIntegralImageOps.java:55-70)"""
        ctx = _ctx(ctx)
        if isinstance(input, GrayU8):
            # transform(GrayU8, GrayS32) (I:alg/transform/ii/impl/ImplIntegralImageOps.java:94-118)
            if transformed is None:
                transformed = GrayS32(input.width, input.height)
            elif not isinstance(transformed, GrayS32):
                raise IllegalArgumentException("GrayU8 is transformed into GrayS32")
            elif transformed.width != input.width or transformed.height != input.height:
                transformed.reshape(input.width, input.height)
            _check(ctx, _lib.load().bhip_integral_u8_s32(ctx._h, *input._in(), *transformed._out()))
            return transformed
        if transformed is None:
            transformed = GrayF32(input.width, input.height)
        elif transformed.width != input.width or transformed.height != input.height:
            transformed.reshape(input.width, input.height)
        _check(ctx, _lib.load().bhip_integral_f32(ctx._h, *input._in(), *transformed._out()))
        return transformed


class IntegralImageFeatureIntensity:
    @staticmethod
    def hessian(integral, skip, size, intensity, ctx=None):
        """F:alg/feature/detect/intensity/IntegralImageFeatureIntensity.java:43-56; intensity must be (width/skip) x (height/skip)."""
        ctx = _ctx(ctx)
        if isinstance(integral, GrayS32):
            _check(ctx, _lib.load().bhip_hessian_s32(ctx._h, *integral._in(), skip, size, *intensity._out()))
            return
        _check(ctx, _lib.load().bhip_hessian_f32(ctx._h, *integral._in(), skip, size, *intensity._out()))


def _points(xy):
    return [Point2D_I16(int(x), int(y)) for x, y in xy]


class NonMaxSuppression:
    """FactoryFeatureExtractor.nonmax(config) -> WrapperNonMaximumBlock(NonMaxBlock(NonMaxBlockSearchStrict.Max / .Min / .MinMax))
    (F:factory/feature/detect/extract/FactoryFeatureExtractor.java:63-102): thresholdMax = config.threshold, thresholdMin = -config.threshold;
    a config that detects no maximums gets the Min search.  Only the strict rule runs on the GPU; the relaxed rule raises RuntimeError,
    which is the BOverride convention for "use the Java code"."""

    def __init__(self, config, ctx=None):
        config = config or ConfigExtract()
        config.checkValidity()
        if not config.useStrictRule:
            raise RuntimeError("only the strict extractors are implemented on the GPU")
        self.ctx = _ctx(ctx)
        self.radius, self.threshold, self.border = config.radius, config.threshold, config.ignoreBorder
        self.thresholdMin = -config.threshold
        self.detectMax = bool(config.detectMaximums)
        self.detectMin = bool(config.detectMinimums) or not self.detectMax
        self.foundMinXY = self.foundMaxXY = np.zeros((0, 2), np.int16)   # the lists of the last process() as int16 [n, 2] arrays

    def process(self, intensity, candidateMin=None, candidateMax=None, foundMin=None, foundMax=None):
        """-> the maximums (the minimums for a minima-only extractor); foundMin / foundMax, when given, are refilled as in the reference"""
        cap = max(1, ((intensity.width + self.radius) // (self.radius + 1)) * ((intensity.height + self.radius) // (self.radius + 1)))
        L = _lib.load()
        xyMax = np.zeros((cap, 2), dtype=np.int16)
        nMax, nMin = C.c_int(0), C.c_int(0)
        if self.detectMin:
            xyMin = np.zeros((cap, 2), dtype=np.int16)
            _check(self.ctx, L.bhip_nonmax_block_minmax_f32(self.ctx._h, *intensity._in(), self.radius, self.thresholdMin, self.threshold, self.border, 1,
                                                           1 if self.detectMax else 0, xyMin.ctypes.data_as(_lib._i16p), C.byref(nMin),
                                                           xyMax.ctypes.data_as(_lib._i16p), C.byref(nMax), cap))
            self.foundMinXY = xyMin[:nMin.value]
        else:
            _check(self.ctx, L.bhip_nonmax_block_f32(self.ctx._h, *intensity._in(), self.radius, self.threshold, self.border,
                                                    xyMax.ctypes.data_as(_lib._i16p), cap, C.byref(nMax)))
            self.foundMinXY = xyMax[:0]
        self.foundMaxXY = xyMax[:nMax.value]
        outMin, outMax = _points(self.foundMinXY), _points(self.foundMaxXY)
        for lst, out in ((foundMin, outMin), (foundMax, outMax)):   # NonMaxBlock.process resets both lists it is given
            if lst is not None:
                del lst[:]
                lst.extend(out)
        return outMax if self.detectMax else outMin

    def getSearchRadius(self): return self.radius
    def setSearchRadius(self, r): self.radius = r
    def getIgnoreBorder(self): return self.border
    def setIgnoreBorder(self, b): self.border = b
    def getThresholdMaximum(self): return self.threshold
    def setThresholdMaximum(self, t): self.threshold = t
    def getThresholdMinimum(self): return self.thresholdMin
    def setThresholdMinimum(self, t): self.thresholdMin = t
    def getUsesCandidates(self): return False
    def canDetectMaximums(self): return self.detectMax
    def canDetectMinimums(self): return self.detectMin


class FactoryFeatureExtractor:
    @staticmethod
    def nonmax(config=None, ctx=None):
        return NonMaxSuppression(config, ctx)


class SelectNBestFeatures:
    """F:alg/feature/detect/extract/SelectNBestFeatures.java:31-97: keep the N most intense corners.  The order of the kept corners is
    the order ddogleg's QuickSelect leaves them in; the GPU runs the restated routine (see include/boofhip.h: order unpinned vs the jar)."""

    def __init__(self, N, ctx=None):
        self.ctx = _ctx(ctx)
        self.target = N
        self.bestCorners = []

    def setN(self, N):
        self.target = N

    def process(self, intensityImage, origCorners, positive):
        xy = np.array([[p.x, p.y] for p in origCorners], dtype=np.int16).reshape(-1, 2)
        out = np.zeros((max(len(xy), 1), 2), dtype=np.int16)
        n = C.c_int(0)
        _check(self.ctx, _lib.load().bhip_select_nbest_f32(self.ctx._h, *intensityImage._in(), xy.ctypes.data_as(_lib._i16p), len(xy), int(self.target),
                                                          1 if positive else 0, out.ctypes.data_as(_lib._i16p), C.byref(n)))
        self.bestCorners = [Point2D_I16(int(x), int(y)) for x, y in out[:n.value]]

    def getBestCorners(self):
        return self.bestCorners


class GradientCornerIntensity:
    """FactoryIntensityPointAlg.shiTomasi / harris (F:factory/feature/detect/intensity/FactoryIntensityPointAlg.java:91-160):
      unweighted, GrayF32   ImplSsdCorner_F32 with ShiTomasiCorner_F32 / HarrisCorner_F32 (F:alg/feature/detect/intensity/impl/ImplSsdCorner_F32.java:62-196),
                            the single-threaded summation order
      unweighted, GrayS16   ImplSsdCorner_S16 with ShiTomasiCorner_S32 / HarrisCorner_S32 (.../impl/ImplSsdCorner_S16.java:63-198)
      weighted, GrayF32     ImplSsdCornerWeighted_F32 (.../impl/ImplSsdCornerWeighted_F32.java:46-104)
      weighted, GrayS16     ImplSsdCornerWeighted_S16 (.../impl/ImplSsdCornerWeighted_S16.java:50-108)"""

    def __init__(self, kind, windowRadius, kappa=0.0, ctx=None, weighted=False, derivType=None):
        self.kind, self.radius, self.kappa = kind, int(windowRadius), float(kappa)
        self.weighted = bool(weighted)
        self.derivType = GrayF32 if derivType is None else derivType
        self.ctx = _ctx(ctx)

    def getRadius(self):
        return self.radius

    def getIgnoreBorder(self):
        return 0 if self.weighted else self.radius   # ImplSsdCornerWeighted_*.getIgnoreBorder / ImplSsdCornerBox

    def getInputType(self):
        return self.derivType

    def process(self, derivX, derivY, intensity):
        for d in (derivX, derivY):
            if isinstance(d, GrayS16) != (self.derivType is GrayS16) or isinstance(d, (GrayU8, GrayS32)):
                raise IllegalArgumentException("derivatives must be %s" % self.derivType.__name__)
        if derivX.width != derivY.width or derivX.height != derivY.height:
            raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape
        (px, *geom), (py, *geomY) = derivX._in(), derivY._in()
        if geom != geomY:
            raise IllegalArgumentException("derivX and derivY must share startIndex and stride")
        intensity.reshape(derivX.width, derivX.height)
        L = _lib.load()
        args = (px, py, *geom, *intensity._out())
        if self.derivType is GrayS16:
            _check(self.ctx, L.bhip_corner_intensity_s16(self.ctx._h, self.kind, self.radius, self.kappa, 1 if self.weighted else 0, *args))
        elif self.weighted:
            _check(self.ctx, L.bhip_corner_intensity_weighted_f32(self.ctx._h, self.kind, self.radius, self.kappa, *args))
        else:
            _check(self.ctx, L.bhip_corner_intensity_f32(self.ctx._h, self.kind, self.radius, self.kappa, *args))


def _corner_intensity(kind, windowRadius, kappa, weighted, derivType, ctx):
    derivType = GrayF32 if derivType is None else derivType
    if derivType is not GrayF32 and derivType is not GrayS16:
        raise RuntimeError("only GrayF32 and GrayS16 derivatives are implemented on the GPU (use the Java path)")
    if weighted and int(windowRadius) <= 0:
        raise IllegalArgumentException("Radius must be > 0")   # FactoryKernelGaussian.sigmaForRadius, from the ImplSsdCornerWeighted_* constructor
    return GradientCornerIntensity(kind, windowRadius, kappa, ctx, weighted, derivType)


class FactoryIntensityPointAlg:
    @staticmethod
    def shiTomasi(windowRadius, weighted=False, derivType=None, ctx=None):
        """F:factory/feature/detect/intensity/FactoryIntensityPointAlg.java:132-160"""
        return _corner_intensity(0, windowRadius, 0.0, weighted, derivType, ctx)

    @staticmethod
    def harris(windowRadius, kappa, weighted=False, derivType=None, ctx=None):
        """F:factory/feature/detect/intensity/FactoryIntensityPointAlg.java:91-118"""
        return _corner_intensity(1, windowRadius, kappa, weighted, derivType, ctx)

    @staticmethod
    def fast(pixelTol, minContinuous, imageType=None, ctx=None):
        """F:factory/feature/detect/intensity/FactoryIntensityPointAlg.java:48-86 (defined with FastCornerDetector, below)"""
        return FastCornerDetector(pixelTol, minContinuous, GrayU8 if imageType is None else imageType, ctx)


@dataclass
class ConfigFastCorner:
    """F:abst/feature/detect/interest/ConfigFastCorner.java:31-64"""
    pixelTol: float = 20
    minContinuous: int = 9
    maxFeatures: float = 0.1

    def checkValidity(self):
        if self.maxFeatures < 0 or self.maxFeatures > 1:
            raise IllegalArgumentException("maxfeatures must be from 0 to 1, inclusive")
        if self.minContinuous < 9 or self.minContinuous > 12:
            raise IllegalArgumentException("minContinuous must be from 9 to 12, inclusive")


class FastCornerDetector:
    """FactoryIntensityPointAlg.fast(pixelTol, minContinuous, imageType) -> FastCornerDetector with ImplFastCorner{9..12}_U8 / _F32
    (F:alg/feature/detect/intensity/FastCornerDetector.java:67-200; rules and deviations: bhip_fast_u8 in include/boofhip.h).  The GrayF32
    helper takes a float tolerance.  The corner lists of the last process() are also kept as int16 [n, 2] arrays: lowXY, highXY."""

    def __init__(self, pixelTol, minContinuous, imageType=GrayU8, ctx=None):
        if imageType is not GrayU8 and imageType is not GrayF32:
            raise IllegalArgumentException("Unknown image type")
        if minContinuous not in (9, 10, 11, 12):
            raise IllegalArgumentException("Specified minCont is not supported")
        self.imageType, self.minContinuous = imageType, int(minContinuous)
        self.pixelTol = float(pixelTol) if imageType is GrayF32 else int(pixelTol)
        self.maxFeaturesFraction = 1.0
        self.ctx = _ctx(ctx)
        self.lowXY = self.highXY = np.zeros((0, 2), np.int16)

    def getRadius(self): return 3
    def getIgnoreBorder(self): return 3
    def getMaxFeaturesFraction(self): return self.maxFeaturesFraction

    def setMaxFeaturesFraction(self, maxFeaturesFraction):
        if maxFeaturesFraction <= 0 or maxFeaturesFraction > 1:
            raise IllegalArgumentException("0 to 1")
        self.maxFeaturesFraction = maxFeaturesFraction

    def process(self, image, intensity=None):
        """process(image, intensity) with a GrayF32 of the image's size, or process(image): the lists only"""
        if not isinstance(image, self.imageType):
            raise IllegalArgumentException("this detector takes %s images" % self.imageType.__name__)
        if intensity is not None and (intensity.width != image.width or intensity.height != image.height):
            raise IllegalArgumentException("the intensity image must have the image's size")
        w, h = image.width, image.height
        # the detector stops after the row that reaches the limit, so a list is never longer than the limit plus that row
        cap = max(1, min(max(w - 6, 0) * max(h - 6, 0), int(self.maxFeaturesFraction * w * h) + w))
        low, high = np.zeros((cap, 2), np.int16), np.zeros((cap, 2), np.int16)
        nLow, nHigh = C.c_int(0), C.c_int(0)
        fn = _lib.load().bhip_fast_f32 if self.imageType is GrayF32 else _lib.load().bhip_fast_u8
        _check(self.ctx, fn(self.ctx._h, *image._in(), self.pixelTol, self.minContinuous, self.maxFeaturesFraction,
                            *(intensity._out() if intensity is not None else (None, 0, 0)), low.ctypes.data_as(_lib._i16p), C.byref(nLow),
                            high.ctypes.data_as(_lib._i16p), C.byref(nHigh), cap))
        self.lowXY, self.highXY = low[:nLow.value], high[:nHigh.value]

    def getCornersLow(self):
        return _points(self.lowXY)

    def getCornersHigh(self):
        return _points(self.highXY)


class WrapperFastCornerIntensity:
    """GeneralFeatureIntensity over FastCornerDetector (F:abst/feature/detect/intensity/WrapperFastCornerIntensity.java:30-84)"""

    def __init__(self, alg):
        self.alg = alg
        self.ctx = alg.ctx
        self.intensity = GrayF32(1, 1)

    def process(self, input, derivX=None, derivY=None, derivXX=None, derivYY=None, derivXY=None):
        self.intensity.reshape(input.width, input.height)   # BaseGeneralFeatureIntensity.init
        self.alg.process(input, self.intensity)

    def getIntensity(self): return self.intensity
    def getCandidatesMin(self): return self.alg.getCornersLow()
    def getCandidatesMax(self): return self.alg.getCornersHigh()
    def getRequiresGradient(self): return False
    def getRequiresHessian(self): return False
    def hasCandidates(self): return True
    def getIgnoreBorder(self): return self.alg.getIgnoreBorder()
    def localMinimums(self): return True
    def localMaximums(self): return True


class WrapFastToPointDetector:
    """PointDetector over FastCornerDetector.process(image) (F:abst/feature/detect/interest/WrapFastToPointDetector.java:28-62)"""

    def __init__(self, detector):
        self.detector = detector

    def process(self, image):
        self.detector.process(image)

    def totalSets(self):
        return 2

    def getPointSet(self, which):
        if which == 0:
            return self.detector.getCornersLow()
        if which == 1:
            return self.detector.getCornersHigh()
        raise IllegalArgumentException("Invalid set request")

    def getDetector(self):
        return self.detector


class GeneralFeatureDetector:
    """F:alg/feature/detect/interest/GeneralFeatureDetector.java:67-160: intensity.process -> extractor.process -> selectBest (maxFeatures > 0:
    SelectNBestFeatures, :143-160) for minimums and maximums, with the exclusion lists the KLT tracker passes (:113-136).  `intensity` is a
    gradient corner intensity (maximums only, as WrapperGradientCornerIntensity) or a GeneralFeatureIntensity that takes the image
    (WrapperFastCornerIntensity: minimums and maximums)."""

    def __init__(self, intensity, extractor):
        self.intensity, self.extractor = intensity, extractor
        self.takesImage = hasattr(intensity, "localMinimums")
        self.localMin = self.takesImage and intensity.localMinimums()
        self.localMax = intensity.localMaximums() if self.takesImage else True
        if extractor.canDetectMinimums() and not self.localMin:
            raise IllegalArgumentException("Extracting local minimums, but intensity has minimums set to false")
        if extractor.canDetectMaximums() and not self.localMax:
            raise IllegalArgumentException("Extracting local maximums, but intensity has maximums set to false")
        if intensity.getIgnoreBorder() > extractor.getIgnoreBorder():
            extractor.setIgnoreBorder(intensity.getIgnoreBorder())
        self.maxFeatures = 0
        self.intensityImage = GrayF32(1, 1)
        self.foundMinimum = []
        self.foundMaximum = []
        self.selectBest = SelectNBestFeatures(10, intensity.ctx)
        self.excludeMinimum = None
        self.excludeMaximum = None

    def setExcludeMinimum(self, exclude):
        """list of Point2D_I16 (or None): pixels that must not be returned as minimums"""
        self.excludeMinimum = exclude

    def setExcludeMaximum(self, exclude):
        """list of Point2D_I16 (or None): pixels that must not be returned as maxima"""
        self.excludeMaximum = exclude

    def setMaxFeatures(self, n):
        self.maxFeatures = n

    def getRequiresGradient(self):
        return self.intensity.getRequiresGradient() if self.takesImage else True

    def getRequiresHessian(self):
        return False

    def setThreshold(self, threshold):
        self.extractor.setThresholdMaximum(threshold)

    def getThreshold(self):
        return self.extractor.getThresholdMaximum()

    def process(self, image, derivX=None, derivY=None, derivXX=None, derivYY=None, derivXY=None):
        if self.takesImage:
            self.intensity.process(image, derivX, derivY, derivXX, derivYY, derivXY)
            self.intensityImage = self.intensity.getIntensity()
        else:
            self.intensity.process(derivX, derivY, self.intensityImage)
        numSelectMin = numSelectMax = -1
        if self.maxFeatures > 0:
            if self.localMin:
                numSelectMin = self.maxFeatures if self.excludeMinimum is None else self.maxFeatures - len(self.excludeMinimum)
            if self.localMax:
                numSelectMax = self.maxFeatures if self.excludeMaximum is None else self.maxFeatures - len(self.excludeMaximum)
            if numSelectMin <= 0 and numSelectMax <= 0:   # :119-121 no room to detect any more features
                self.foundMinimum, self.foundMaximum = [], []
                return
        for exclude, mark in ((self.excludeMinimum, -Float_MAX_VALUE), (self.excludeMaximum, Float_MAX_VALUE)):
            if exclude is not None:
                for p in exclude:
                    self.intensityImage.set(p.x, p.y, mark)
        self.foundMinimum, self.foundMaximum = [], []
        self.extractor.process(self.intensityImage, None, None, self.foundMinimum, self.foundMaximum)
        # :146-160 selectBest: only a side with room is pruned (numSelect = maxFeatures without an exclusion list)
        for attr, numSelect, positive in (("foundMinimum", numSelectMin, False), ("foundMaximum", numSelectMax, True)):
            if numSelect > 0:
                self.selectBest.setN(numSelect)
                self.selectBest.process(self.intensityImage, getattr(self, attr), positive)
                setattr(self, attr, list(self.selectBest.getBestCorners()))

    def getIntensity(self):
        return self.intensityImage

    def getMinimums(self):
        return self.foundMinimum

    def getMaximums(self):
        return self.foundMaximum


class FastHessianFeatureDetector:
    """FactoryInterestPointAlgs.fastHessian(config).detect(integral) (F:alg/feature/detect/interest/FastHessianFeatureDetector.java:156-188)"""

    def __init__(self, config=None, ctx=None):
        self.config = config or ConfigFastHessian()
        self.ctx = _ctx(ctx)
        self.foundPoints = np.zeros((0, 3))

    def detect(self, integral):
        cfg = self.config._c()
        cap = 1 << 15
        while True:
            out = np.zeros((cap, 3))
            n = C.c_int(0)
            fn = _lib.load().bhip_fh_detect_s32 if isinstance(integral, GrayS32) else _lib.load().bhip_fh_detect_f32
            _check(self.ctx, fn(self.ctx._h, C.byref(cfg), *integral._in(), out.ctypes.data_as(_lib._dp), cap, C.byref(n)))
            if n.value <= cap:
                self.foundPoints = out[:n.value].copy()
                return
            cap = n.value

    def getFoundPoints(self):
        return self.foundPoints


class FactoryDetectPoint:
    """F:factory/feature/detect/interest/FactoryDetectPoint.java"""

    @staticmethod
    def createGeneral(intensity, config, ctx=None):
        """:235-251 -- a copy of the config with ignoreBorder += radius and the sides the intensity does not have switched off"""
        cfg = ConfigGeneralDetector(config.radius, config.threshold, config.ignoreBorder + config.radius, config.useStrictRule, config.detectMinimums,
                                    config.detectMaximums, config.maxFeatures)
        takesImage = hasattr(intensity, "localMinimums")
        if takesImage and not intensity.localMaximums():
            cfg.detectMaximums = False
        if not takesImage or not intensity.localMinimums():
            cfg.detectMinimums = False
        det = GeneralFeatureDetector(intensity, FactoryFeatureExtractor.nonmax(cfg, ctx or intensity.ctx))
        det.setMaxFeatures(cfg.maxFeatures)
        return det

    @staticmethod
    def createFast(configFast=None, configDetector=None, imageType=None, ctx=None):
        """createFast(configFast, configDetector, imageType) -> GeneralFeatureDetector (:130-141), or, without a detector config,
        createFast(configFast, imageType) -> WrapFastToPointDetector (:151-160): set 0 = dark corners, set 1 = bright corners"""
        if configDetector is not None and not isinstance(configDetector, ConfigExtract):   # the two-argument form
            configDetector, imageType = None, configDetector
        configFast = configFast or ConfigFastCorner()
        configFast.checkValidity()
        alg = FactoryIntensityPointAlg.fast(configFast.pixelTol, configFast.minContinuous, imageType, ctx)
        alg.setMaxFeaturesFraction(configFast.maxFeatures)
        if configDetector is None:
            return WrapFastToPointDetector(alg)
        return FactoryDetectPoint.createGeneral(WrapperFastCornerIntensity(alg), configDetector, ctx)
