"""The SIFT detector: FactoryInterestPoint.sift (F:factory/feature/detect/interest/FactoryInterestPoint.java:133-148), WrapSiftDetector
(F:abst/feature/detect/interest/WrapSiftDetector.java:38-88) over SiftDetector (F:alg/feature/detect/interest/SiftDetector.java:119-331),
SiftScaleSpace (F:alg/feature/detect/interest/SiftScaleSpace.java:102-270) and NonMaxLimiter (F:abst/feature/detect/extract/NonMaxLimiter.java),
ConfigSiftScaleSpace (F:abst/feature/describe/ConfigSiftScaleSpace.java) and ConfigSiftDetector (F:abst/feature/detect/interest/ConfigSiftDetector.java).

A module beside the api package (like census.py, best5.py, enhance.py and hornschunck.py): it takes the image types, ConfigExtract and the
view marshaller from boofcv_amd.api and adds no name there.

Detect + describe: FactoryDetectDescribe.sift (F:factory/feature/detdesc/FactoryDetectDescribe.java:72-96), DetectDescribe_CompleteSift
(F:abst/feature/detdesc/DetectDescribe_CompleteSift.java) over CompleteSift (F:alg/feature/detdesc/CompleteSift.java), with
OrientationHistogramSift, DescribePointSift, ConfigSiftOrientation, ConfigSiftDescribe and ConfigCompleteSift.  The number of angles of every
detection -- hence the count and the order of features -- and x, y, scale, white equal the Java result exactly; angles and descriptor
elements differ from it by the last ulp of atan2 / sin / cos alone (bhip_csift_cfg in include/boofhip.h).

Scale images, DoG images and detections equal the single-threaded Java result bit for bit.  Rules, refusals and limits: bhip_sift_cfg in
include/boofhip.h.  Math.pow is the host's pow (unpinned against Java's); with maxFeaturesPerScale > 0 the order QuickSelect leaves is the
restated routine's (unpinned against the ddogleg jar), the kept set is pinned whenever no two |value| around the cut are equal."""
import ctypes as C
import math

import numpy as np

from . import _lib
from .api.core import IllegalArgumentException, _check, _ctx
from .api.detect import ConfigExtract
from .api.image import BrightFeature, GrayF32, GrayU8, Point2D_F64

__all__ = ["ConfigSiftScaleSpace", "ConfigSiftDetector", "SiftScaleSpace", "SiftDetector", "ScalePoint", "NonMaxLimiter", "InterestPointDetectorSift",
           "FactoryInterestPointSift", "ConfigSiftOrientation", "ConfigSiftDescribe", "ConfigCompleteSift", "OrientationHistogramSift", "DescribePointSift",
           "CompleteSift", "DetectDescribeCompleteSift", "FactoryDetectDescribeSift"]


class ConfigSiftScaleSpace:
    """sigma0 is a float field in the reference: the value SiftScaleSpace gets is its widening"""

    def __init__(self, firstOctave=0, lastOctave=5, numScales=3, sigma0=2.75):
        self.firstOctave, self.lastOctave, self.numScales = int(firstOctave), int(lastOctave), int(numScales)
        self.sigma0 = float(np.float32(sigma0))

    def checkValidity(self):
        pass

    @staticmethod
    def createPaper():
        c = ConfigSiftScaleSpace()
        c.sigma0, c.numScales, c.firstOctave, c.lastOctave = float(np.float32(1.6)), 3, -1, 5
        return c


class ConfigSiftDetector:
    """extract = ConfigExtract(2, 0, 1, true, true, true); maxFeaturesPerScale <= 0: no limit; edgeR"""

    def __init__(self, extract=None, maxFeaturesPerScale=0, edgeR=10.0):
        self.extract = extract if extract is not None else ConfigExtract(2, 0.0, 1, True, True, True)
        self.maxFeaturesPerScale, self.edgeR = int(maxFeaturesPerScale), float(edgeR)

    def checkValidity(self):
        pass

    @staticmethod
    def createPaper():
        return ConfigSiftDetector(ConfigExtract(1, 0.0, 1, True, True, True), 0, 10.0)


def _cfg(configSS, configDet):
    """-> bhip_sift_cfg from the two configs (None: the reference's defaults); configSS may also be a SiftScaleSpace"""
    c = _lib.SiftCfg()
    _lib.load().bhip_sift_cfg_default(C.byref(c))
    if configSS is not None:
        c.firstOctave, c.lastOctave, c.numScales, c.sigma0 = configSS.firstOctave, configSS.lastOctave, configSS.numScales, configSS.sigma0
    if configDet is not None:
        e = configDet.extract
        c.extractRadius, c.extractThreshold, c.extractIgnoreBorder = int(e.radius), float(e.threshold), int(e.ignoreBorder)
        c.extractUseStrictRule, c.extractDetectMin, c.extractDetectMax = int(bool(e.useStrictRule)), int(bool(e.detectMinimums)), int(bool(e.detectMaximums))
        c.maxFeaturesPerScale, c.edgeR = max(int(configDet.maxFeaturesPerScale), 0), float(configDet.edgeR)
    return c


class ScalePoint(Point2D_F64):
    """F:struct/feature/ScalePoint.java: x, y, scale, white"""

    def __init__(self, x=0.0, y=0.0, scale=0.0, white=False):
        super().__init__(x, y)
        self.scale, self.white = scale, white


class SiftScaleSpace:
    """initialize(input) computes every octave on the GPU at once; computeNextOctave steps through them as the reference's does"""

    def __init__(self, firstOctave, lastOctave, numScales, sigma0, ctx=None):
        if lastOctave <= firstOctave:
            raise IllegalArgumentException("Last octave must be more than the first octave")
        if numScales < 1:
            raise IllegalArgumentException("Number of scales must be >= 1")
        self.firstOctave, self.lastOctave, self.numScales, self.sigma0 = int(firstOctave), int(lastOctave), int(numScales), float(sigma0)
        self.ctx = _ctx(ctx)
        self.currentOctave = self.firstOctave
        self._octaves = []

    def computeSigmaScale(self, *a):
        """computeSigmaScale(scale) in the current octave, or computeSigmaScale(octave, scale)"""
        octave, scale = (self.currentOctave, a[0]) if len(a) == 1 else a
        return self.sigma0 * math.pow(2, octave + scale / float(self.numScales))

    def initialize(self, input):
        if not isinstance(input, (GrayF32, GrayU8)):
            raise IllegalArgumentException("GrayF32 (or GrayU8, converted as WrapSiftDetector does) expected")
        L = _lib.load()
        c = _cfg(self, None)
        dims = (C.c_int * 128)()
        sf, df = C.c_longlong(0), C.c_longlong(0)
        src = input._in()   # validated before anything reaches C
        n = L.bhip_sift_layout(C.byref(c), input.width, input.height, dims, 64, C.byref(sf), C.byref(df))
        if n < 0:
            raise (RuntimeError if n == _lib.BHIP_ERR_UNSUPPORTED else IllegalArgumentException)("no SIFT scale space for a %d x %d image" % (input.width, input.height))
        scale, dog = np.zeros(sf.value, np.float32), np.zeros(df.value, np.float32)
        fn = L.bhip_sift_scale_space_u8 if isinstance(input, GrayU8) else L.bhip_sift_scale_space_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(c), *src, scale.ctypes.data_as(_lib._fp), dog.ctypes.data_as(_lib._fp)))
        self._octaves = []
        oS = oD = 0
        for i in range(n):
            w, h = dims[2 * i], dims[2 * i + 1]
            plane = (w * h + 3) & ~3
            self._octaves.append(([GrayF32(w, h, scale[oS + k * plane:oS + k * plane + w * h]) for k in range(self.numScales + 3)],
                                  [GrayF32(w, h, dog[oD + k * plane:oD + k * plane + w * h]) for k in range(self.numScales + 2)]))
            oS += (self.numScales + 3) * plane
            oD += (self.numScales + 2) * plane
        self.currentOctave = self.firstOctave

    def computeNextOctave(self):
        self.currentOctave += 1
        if self.currentOctave > self.lastOctave:
            return False
        top = self._octaves[self.currentOctave - 1 - self.firstOctave][0][self.numScales]
        if top.width <= 5 or top.height <= 5:
            return False
        return True

    def getImageScale(self, scaleIndex):
        return self._octaves[self.currentOctave - self.firstOctave][0][scaleIndex]

    def getDifferenceOfGaussian(self, dogIndex):
        return self._octaves[self.currentOctave - self.firstOctave][1][dogIndex]

    def getNumScales(self):
        return self.numScales

    def getNumScaleImages(self):
        return self.numScales + 3

    def getCurrentOctave(self):
        return self.currentOctave

    def getTotalOctaves(self):
        return self.lastOctave - self.firstOctave + 1

    def pixelScaleCurrentToInput(self):
        return math.pow(2.0, self.currentOctave)


class NonMaxLimiter:
    """NonMaxLimiter(FactoryFeatureExtractor.nonmax(config), maxTotalFeatures) as the detector's constructor reads it"""

    def __init__(self, extract, maxTotalFeatures):
        self.extract, self.maxTotalFeatures = extract, int(maxTotalFeatures)


class SiftDetector:
    """process(input) -> getDetections(): the list of ScalePoint in the reference's order; where [n, 4] int16 records octave, DoG index and the
    pixel of every detection (what the orientation and description stages start from)"""

    def __init__(self, scaleSpace, edgeR, extractor, ctx=None):
        e = extractor.extract
        if not e.detectMaximums or not e.detectMinimums:
            raise IllegalArgumentException("The extractor must be able to detect maximums and minimums")
        if edgeR < 1:
            raise IllegalArgumentException("R must be >= 1")
        if e.ignoreBorder != 1:
            raise RuntimeError("Non-max should have an ignore border of 1")
        e.checkValidity()
        if not e.useStrictRule:
            raise RuntimeError("the SIFT detector runs on the GPU with the strict extractor only (use the Java path)")
        self.scaleSpace, self.edgeR, self.extractor = scaleSpace, float(edgeR), extractor
        self.ctx = _ctx(ctx) if ctx is not None else scaleSpace.ctx
        self._cap = 4096
        self._set(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, np.uint8), np.zeros((0, 4), np.int16))

    def _set(self, x, y, scale, white, where):
        self.x, self.y, self.scale, self.white, self.where = x, y, scale, white, where

    def process(self, input):
        if not isinstance(input, (GrayF32, GrayU8)):
            raise IllegalArgumentException("GrayF32 (or GrayU8, converted as WrapSiftDetector does) expected")
        L = _lib.load()
        c = _cfg(self.scaleSpace, ConfigSiftDetector(self.extractor.extract, self.extractor.maxTotalFeatures, self.edgeR))
        src = input._in()
        fn = L.bhip_sift_detect_u8 if isinstance(input, GrayU8) else L.bhip_sift_detect_f32
        while True:
            cap = self._cap
            x, y, scale = (np.empty(cap, np.float64) for _ in range(3))
            white, where, n = np.empty(cap, np.uint8), np.empty((cap, 4), np.int16), C.c_int(0)
            _check(self.ctx, fn(self.ctx._h, C.byref(c), *src, x.ctypes.data_as(_lib._dp), y.ctypes.data_as(_lib._dp), scale.ctypes.data_as(_lib._dp),
                                white.ctypes.data_as(_lib._u8p), where.ctypes.data_as(_lib._i16p), C.byref(n), cap))
            if n.value <= cap:
                break
            self._cap = n.value   # the list did not fit: once more with room for all of it
        k = n.value
        self._set(x[:k], y[:k], scale[:k], white[:k], where[:k])

    def getDetections(self):
        return [ScalePoint(float(self.x[i]), float(self.y[i]), float(self.scale[i]), bool(self.white[i])) for i in range(len(self.x))]


class InterestPointDetectorSift:
    """WrapSiftDetector: InterestPointDetector<GrayF32 | GrayU8>"""

    def __init__(self, detector, inputType):
        self.detector, self.inputType = detector, inputType

    def detect(self, image):
        if not isinstance(image, self.inputType):
            raise IllegalArgumentException("this detector takes %s images" % self.inputType.__name__)
        self.detector.process(image)

    def getNumberOfFeatures(self):
        return len(self.detector.x)

    def getLocation(self, featureIndex):
        return Point2D_F64(float(self.detector.x[featureIndex]), float(self.detector.y[featureIndex]))

    def getRadius(self, featureIndex):
        return float(self.detector.scale[featureIndex])

    def getOrientation(self, featureIndex):
        return 0.0

    def hasScale(self):
        return True

    def hasOrientation(self):
        return False

    def getInputType(self):
        return self.inputType


class FactoryInterestPointSift:
    """FactoryInterestPoint.sift on the GPU"""

    @staticmethod
    def sift(configSS, configDet, imageType, ctx=None):
        """sift(configSS, configDet, imageType) (:133-148): None = new ConfigSiftScaleSpace() / new ConfigSiftDetector().  Image types the GPU does
        not have (Planar, interleaved, other pixel types) raise RuntimeError: use the Java path."""
        if configSS is None:
            configSS = ConfigSiftScaleSpace()
        if configDet is None:
            configDet = ConfigSiftDetector()
        if imageType is not GrayF32 and imageType is not GrayU8:
            raise RuntimeError("the SIFT detector runs on the GPU for GrayF32 and GrayU8 images only (use the Java path)")
        scaleSpace = SiftScaleSpace(configSS.firstOctave, configSS.lastOctave, configSS.numScales, configSS.sigma0, ctx)
        configDet.extract.checkValidity()   # FactoryFeatureExtractor.nonmax
        limiter = NonMaxLimiter(configDet.extract, configDet.maxFeaturesPerScale)
        return InterestPointDetectorSift(SiftDetector(scaleSpace, configDet.edgeR, limiter), imageType)


class ConfigSiftOrientation:
    """F:abst/feature/orientation/ConfigSiftOrientation.java: histogramSize 36, sigmaEnlarge 2.0 (createPaper: 36, 1.5)"""

    def __init__(self, histogramSize=36, sigmaEnlarge=2.0):
        self.histogramSize, self.sigmaEnlarge = int(histogramSize), float(sigmaEnlarge)

    @staticmethod
    def createPaper():
        return ConfigSiftOrientation(36, 1.5)

    def checkValidity(self):
        pass


class ConfigSiftDescribe:
    """F:abst/feature/describe/ConfigSiftDescribe.java: 4, 4, 8, 1.0, 0.5, 0.2"""

    def __init__(self, widthSubregion=4, widthGrid=4, numHistogramBins=8, sigmaToPixels=1.0, weightingSigmaFraction=0.5, maxDescriptorElementValue=0.2):
        self.widthSubregion, self.widthGrid, self.numHistogramBins = int(widthSubregion), int(widthGrid), int(numHistogramBins)
        self.sigmaToPixels, self.weightingSigmaFraction = float(sigmaToPixels), float(weightingSigmaFraction)
        self.maxDescriptorElementValue = float(maxDescriptorElementValue)

    def checkValidity(self):
        pass


class ConfigCompleteSift:
    """F:abst/feature/detdesc/ConfigCompleteSift.java: ConfigCompleteSift() or ConfigCompleteSift(firstOctave, lastOctave, maxFeaturesPerScale)"""

    def __init__(self, *a):
        self.scaleSpace, self.detector = ConfigSiftScaleSpace(), ConfigSiftDetector()
        self.orientation, self.describe = ConfigSiftOrientation(), ConfigSiftDescribe()
        if len(a) == 3:
            self.scaleSpace.firstOctave, self.scaleSpace.lastOctave, self.detector.maxFeaturesPerScale = int(a[0]), int(a[1]), int(a[2])
        elif a:
            raise TypeError("ConfigCompleteSift() or ConfigCompleteSift(firstOctave, lastOctave, maxFeaturesPerScale)")

    @staticmethod
    def createPaper():
        c = ConfigCompleteSift()
        c.scaleSpace, c.detector, c.orientation = ConfigSiftScaleSpace.createPaper(), ConfigSiftDetector.createPaper(), ConfigSiftOrientation.createPaper()
        return c

    def checkValidity(self):
        for c in (self.scaleSpace, self.detector, self.orientation, self.describe):
            c.checkValidity()


class OrientationHistogramSift:
    """the constructor arguments of OrientationHistogramSift(histogramSize, sigmaEnlarge, derivType); the histograms are the GPU's"""

    def __init__(self, histogramSize, sigmaEnlarge, derivType=GrayF32):
        self.histogramSize, self.sigmaEnlarge = int(histogramSize), float(sigmaEnlarge)


class DescribePointSift:
    """the constructor arguments of DescribePointSift(widthSubregion, widthGrid, numHistogramBins, sigmaToPixels, weightingSigmaFraction,
    maxDescriptorElementValue, derivType)"""

    def __init__(self, widthSubregion, widthGrid, numHistogramBins, sigmaToPixels, weightingSigmaFraction, maxDescriptorElementValue, derivType=GrayF32):
        self.widthSubregion, self.widthGrid, self.numHistogramBins = int(widthSubregion), int(widthGrid), int(numHistogramBins)
        self.sigmaToPixels, self.weightingSigmaFraction = float(sigmaToPixels), float(weightingSigmaFraction)
        self.maxDescriptorElementValue = float(maxDescriptorElementValue)

    def getDescriptorLength(self):
        return self.widthGrid * self.widthGrid * self.numHistogramBins

    def getCanonicalRadius(self):
        return self.widthGrid * self.widthSubregion // 2


def _desc_cfg(orientation=None, describe=None):
    """-> bhip_csift_cfg from a ConfigSiftOrientation / OrientationHistogramSift and a ConfigSiftDescribe / DescribePointSift (None: the defaults)"""
    c = _lib.CompleteSiftCfg()
    _lib.load().bhip_csift_cfg_default(C.byref(c))
    if orientation is not None:
        c.histogramSize, c.sigmaEnlarge = int(orientation.histogramSize), float(orientation.sigmaEnlarge)
    if describe is not None:
        c.widthSubregion, c.widthGrid, c.numHistogramBins = int(describe.widthSubregion), int(describe.widthGrid), int(describe.numHistogramBins)
        c.sigmaToPixels, c.weightingSigmaFraction = float(describe.sigmaToPixels), float(describe.weightingSigmaFraction)
        c.maxDescriptorElementValue = float(describe.maxDescriptorElementValue)
    return c


class CompleteSift(SiftDetector):
    """process(input) -> getLocations() (one ScalePoint per feature: a detection appears once per angle), getDescriptions() (BrightFeature),
    getOrientations(); the arrays x, y, scale, orientation, white, descriptors [n, dof] hold the same"""

    def __init__(self, scaleSpace, edgeR, extractor, orientation, describe, ctx=None):
        super().__init__(scaleSpace, edgeR, extractor, ctx)
        self.orientationAlg, self.describeAlg = orientation, describe
        dof = _lib.load().bhip_csift_dof(C.byref(_desc_cfg(orientation, describe)))
        if dof < 0:
            raise (RuntimeError if dof == _lib.BHIP_ERR_UNSUPPORTED else IllegalArgumentException)("no SIFT descriptor for this orientation / describe config")
        self._dof = dof
        self.orientation, self.descriptors = np.zeros(0), np.zeros((0, dof))

    def process(self, input):
        if not isinstance(input, (GrayF32, GrayU8)):
            raise IllegalArgumentException("GrayF32 (or GrayU8, converted as DetectDescribe_CompleteSift does) expected")
        L = _lib.load()
        c = _cfg(self.scaleSpace, ConfigSiftDetector(self.extractor.extract, self.extractor.maxTotalFeatures, self.edgeR))
        dc = _desc_cfg(self.orientationAlg, self.describeAlg)
        src = input._in()
        fn = L.bhip_csift_u8 if isinstance(input, GrayU8) else L.bhip_csift_f32
        while True:
            cap = self._cap
            x, y, scale, ori = (np.empty(cap, np.float64) for _ in range(4))
            white, desc, n = np.empty(cap, np.uint8), np.empty((cap, self._dof), np.float64), C.c_int(0)
            _check(self.ctx, fn(self.ctx._h, C.byref(c), C.byref(dc), *src, x.ctypes.data_as(_lib._dp), y.ctypes.data_as(_lib._dp), scale.ctypes.data_as(_lib._dp),
                                ori.ctypes.data_as(_lib._dp), white.ctypes.data_as(_lib._u8p), desc.ctypes.data_as(_lib._dp), C.byref(n), cap))
            if n.value <= cap:
                break
            self._cap = n.value   # the list did not fit: once more with room for all of it
        k = n.value
        self._set(x[:k], y[:k], scale[:k], white[:k], np.zeros((0, 4), np.int16))
        self.orientation, self.descriptors = ori[:k], desc[:k]

    def getLocations(self):
        return self.getDetections()

    def getDescriptions(self):
        return [BrightFeature(self._dof, self.descriptors[i], bool(self.white[i])) for i in range(len(self.x))]

    def getOrientations(self):
        return [float(a) for a in self.orientation]

    def getDescriptorLength(self):
        return self._dof


class DetectDescribeCompleteSift:
    """DetectDescribe_CompleteSift: DetectDescribePoint<GrayF32 | GrayU8, BrightFeature>"""

    def __init__(self, alg, inputType):
        self.alg, self.inputType = alg, inputType

    def createDescription(self):
        return BrightFeature(self.alg.getDescriptorLength())

    def getDescription(self, index):
        return BrightFeature(self.alg.getDescriptorLength(), self.alg.descriptors[index], bool(self.alg.white[index]))

    def getDescriptionType(self):
        return BrightFeature

    def detect(self, input):
        if not isinstance(input, self.inputType):
            raise IllegalArgumentException("this detector takes %s images" % self.inputType.__name__)
        self.alg.process(input)

    def getNumberOfFeatures(self):
        return len(self.alg.x)

    def getLocation(self, featureIndex):
        return ScalePoint(float(self.alg.x[featureIndex]), float(self.alg.y[featureIndex]), float(self.alg.scale[featureIndex]), bool(self.alg.white[featureIndex]))

    def getRadius(self, featureIndex):
        return float(self.alg.scale[featureIndex])

    def getOrientation(self, featureIndex):
        return float(self.alg.orientation[featureIndex])

    def hasScale(self):
        return True

    def hasOrientation(self):
        return True

    def getInputType(self):
        return self.inputType


class FactoryDetectDescribeSift:
    """FactoryDetectDescribe.sift on the GPU"""

    @staticmethod
    def sift(config=None, imageType=GrayF32, ctx=None):
        """sift(config) (:72-96): None = new ConfigCompleteSift().  The reference's method is generic in the image type; here the type is an
        argument, and the types the GPU does not have (Planar, interleaved, other pixel types) raise RuntimeError: use the Java path."""
        if config is None:
            config = ConfigCompleteSift()
        if imageType is not GrayF32 and imageType is not GrayU8:
            raise RuntimeError("SIFT detect + describe runs on the GPU for GrayF32 and GrayU8 images only (use the Java path)")
        ss, det, ori, de = config.scaleSpace, config.detector, config.orientation, config.describe
        scaleSpace = SiftScaleSpace(ss.firstOctave, ss.lastOctave, ss.numScales, ss.sigma0, ctx)
        orientation = OrientationHistogramSift(ori.histogramSize, ori.sigmaEnlarge, GrayF32)
        describe = DescribePointSift(de.widthSubregion, de.widthGrid, de.numHistogramBins, de.sigmaToPixels, de.weightingSigmaFraction,
                                     de.maxDescriptorElementValue, GrayF32)
        det.extract.checkValidity()   # FactoryFeatureExtractor.nonmax
        limiter = NonMaxLimiter(det.extract, det.maxFeaturesPerScale)
        return DetectDescribeCompleteSift(CompleteSift(scaleSpace, det.edgeR, limiter, orientation, describe), imageType)
