"""Detect + describe: SURF on gray and planar frames, the BRIEF definition and the Fast-Hessian + BRIEF fusion (F:abst/feature/detdesc,
F:abst/feature/describe, F:abst/feature/orientation, F:alg/feature/describe/brief, F:factory/feature/{detdesc,describe}).
  FactoryDetectDescribe.surfStable / surfFast   F:factory/feature/detdesc/FactoryDetectDescribe.java:118-135,209-226
  DetectDescribePoint                            F:abst/feature/detdesc/DetectDescribePoint.java:32-46"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .core import Context, Double_MAX_VALUE, IllegalArgumentException, _check, _NativeObject, _PinnedPool
from .image import BrightFeature, GrayF32, GrayU8, PlanarType, Point2D_F64, TupleDesc_B, _check_extent
from .detect import ConfigFastHessian
from .filter import DescribePointBrief

__all__ = ["BinaryCompareDefinition_I32", "ConfigAverageIntegral", "ConfigBrief", "ConfigSlidingIntegral", "ConfigSurfDescribe",
           "DetectDescribeFusion", "DetectDescribePoint", "FactoryBriefDefinition", "FactoryDescribeRegionPoint", "FactoryDetectDescribe",
           "FactoryInterestPoint", "Random", "SurfPlanar_to_DetectDescribePoint", "WrapDescribeBrief", "WrapFHtoInterestPoint"]


class ConfigSurfDescribe:
    """F:abst/feature/describe/ConfigSurfDescribe.java:34-78"""

    @dataclass
    class Speed:
        widthLargeGrid: int = 4
        widthSubRegion: int = 5
        widthSample: int = 3
        useHaar: bool = False
        weightSigma: float = 4.5

    @dataclass
    class Stability:
        widthLargeGrid: int = 4
        widthSubRegion: int = 5
        widthSample: int = 3
        useHaar: bool = False
        overLap: int = 2
        sigmaLargeGrid: float = 2.5
        sigmaSubRegion: float = 2.5


@dataclass
class ConfigSlidingIntegral:
    """F:abst/feature/orientation/ConfigSlidingIntegral.java:34-54"""
    objectRadiusToScale: float = 0.5
    samplePeriod: float = 0.65
    windowSize: float = math.pi / 3.0
    radius: int = 8
    weightSigma: float = -1.0
    sampleWidth: int = 6


@dataclass
class ConfigAverageIntegral:
    """F:abst/feature/orientation/ConfigAverageIntegral.java:34-51"""
    objectRadiusToScale: float = 0.5
    radius: int = 6
    samplePeriod: float = 1.0
    sampleWidth: int = 6
    weightSigma: float = -1.0


class DetectDescribePoint(_NativeObject):
    """DetectDescribePoint<GrayF32,BrightFeature> backed by bhip_surf (WrapDetectDescribeSurf.java:47-159).

    Results are recycled on the next detect(), instances are not thread safe -- both as in the reference.
    detectBatch() is the batched extension (one launch sequence for many frames)."""
    _destroy = "bhip_surf_destroy"

    def __init__(self, stable, configDetector, configDescribe, configOrientation, ctx=None):
        self.ctx = ctx or Context.default()
        L = _lib.load()
        fh = (configDetector or ConfigFastHessian())._c()
        if stable:
            d = configDescribe or ConfigSurfDescribe.Stability()
            sd = _lib.SurfCfg(d.widthLargeGrid, d.widthSubRegion, d.widthSample, 4.5, d.overLap, d.sigmaLargeGrid, d.sigmaSubRegion)
            o = configOrientation or ConfigSlidingIntegral()
            oc = _lib.OriCfg(o.objectRadiusToScale, o.samplePeriod, o.windowSize, o.radius, o.weightSigma, o.sampleWidth)
        else:
            d = configDescribe or ConfigSurfDescribe.Speed()
            sd = _lib.SurfCfg(d.widthLargeGrid, d.widthSubRegion, d.widthSample, d.weightSigma, 2, 2.5, 2.5)
            o = configOrientation or ConfigAverageIntegral()
            oc = _lib.OriCfg(o.objectRadiusToScale, o.samplePeriod, 0.0, o.radius, o.weightSigma, o.sampleWidth)
        if d.useHaar:
            raise RuntimeError("useHaar=true is not implemented on the GPU (use the Java path)")
        h = C.c_void_p()
        _check(self.ctx, L.bhip_surf_create(self.ctx._h, C.byref(fh), C.byref(sd), C.byref(oc), 1 if stable else 0, C.byref(h)))
        self._adopt(h)
        self._dof = L.bhip_surf_dof(h)
        self._batch = 0
        self._image = 0
        self._cache = {}

    # --- DescriptorInfo
    def createDescription(self):
        return BrightFeature(self._dof)

    def getDescriptionType(self):
        return BrightFeature

    # --- detection
    def detect(self, input):
        self.detectBatch([input])

    def detectBatch(self, images):
        if not images:
            raise IllegalArgumentException("empty batch")
        w, h = images[0].width, images[0].height
        for im in images:
            if im.width != w or im.height != h:
                raise IllegalArgumentException("all images of a batch must have the same shape")
        views = [im._in() for im in images]
        n = len(images)
        u8 = isinstance(images[0], GrayU8)
        if any(isinstance(im, GrayU8) != u8 for im in images):
            raise IllegalArgumentException("all images of a batch must have the same type")
        ptrs = (C.POINTER(C.c_uint8 if u8 else C.c_float) * n)(*[v[0] for v in views])
        starts = (C.c_int * n)(*[v[1] for v in views])
        strides = (C.c_int * n)(*[v[2] for v in views])
        self._cache = {}
        self._batch = 0
        fn = _lib.load().bhip_surf_detect_u8 if u8 else _lib.load().bhip_surf_detect_f32
        _check(self.ctx, fn(self._h, ptrs, starts, strides, w, h, n))
        self._batch = n
        self._image = 0
        self._shape = (w, h)

    def detectDevice(self, dev_ptr, imageStride, stride, width, height, batch):
        """Batch already resident in HBM (bench path): dev_ptr is a device address of float32 pixels."""
        self._cache = {}
        self._batch = 0
        _check(self.ctx, _lib.load().bhip_surf_detect_dev_f32(self._h, C.c_void_p(dev_ptr), imageStride, stride, width, height, batch))
        self._batch = batch
        self._image = 0
        self._shape = (width, height)

    def selectImage(self, image):
        """Which image of the last batch the index-based getters refer to (0 for the single-image reference call)."""
        if not (0 <= image < self._batch):
            raise IllegalArgumentException("image index out of range")
        self._image = image

    def _results(self, image=None):
        image = self._image if image is None else image
        if image not in self._cache:
            L = _lib.load()
            n = C.c_int(0)
            _check(self.ctx, L.bhip_surf_count(self._h, image, C.byref(n)))
            n = n.value
            # page-locked result arrays (the copies are DMA transfers; a descriptor list handed on to associate() uploads the same way)
            xys, ang, white, desc = _PinnedPool.arrays(self.ctx, [((n, 3), np.float64), ((n,), np.float64), ((n,), np.uint8), ((n, self._dof), np.float64)])
            if n:
                _check(self.ctx, L.bhip_surf_fetch(self._h, image, xys.ctypes.data_as(_lib._dp), ang.ctypes.data_as(_lib._dp),
                                                   white.ctypes.data_as(_lib._u8p), desc.ctypes.data_as(_lib._dp)))
            self._cache[image] = (xys, ang, white, desc)
        return self._cache[image]

    def fetchAll(self, out=None):
        """The whole batch of the last detect in one set of copies (bhip_surf_fetch_all): (xy_scale [total,3], angle [total],
        white [total], desc [total,dof], starts [batch+1]); image i owns rows starts[i]:starts[i+1].
        out = (xy_scale, angle, white, desc) receives the copies when given: C-contiguous float64 / uint8 arrays with at least `total` rows
        (e.g. views of page-locked memory a caller keeps across batches -- the copies then run at PCIe speed); views of the first `total`
        rows are returned."""
        L = _lib.load()
        counts = self.counts()
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        total = int(starts[-1])
        if out is None:
            xys = np.empty((total, 3)); ang = np.empty(total); white = np.empty(total, dtype=np.uint8); desc = np.empty((total, self._dof))
        else:
            xys, ang, white, desc = out
            want = ((xys, np.float64, (3,)), (ang, np.float64, ()), (white, np.uint8, ()), (desc, np.float64, (self._dof,)))
            for a, dt, tail in want:
                if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.shape[1:] == tail and a.shape[0] >= total):
                    raise IllegalArgumentException("fetchAll: output arrays must be C-contiguous, of the right type and at least %d rows long" % total)
            xys, ang, white, desc = xys[:total], ang[:total], white[:total], desc[:total]
        if total:
            _check(self.ctx, L.bhip_surf_fetch_all(self._h, xys.ctypes.data_as(_lib._dp), ang.ctypes.data_as(_lib._dp), white.ctypes.data_as(_lib._u8p),
                                                   desc.ctypes.data_as(_lib._dp)))
        return xys, ang, white, desc, starts

    def associateImages(self, srcImages, dstImages, maxError=Double_MAX_VALUE, backwardsValidation=True):
        """Greedy Euclidean-squared association of image srcImages[p] with image dstImages[p] of the last detect, on the descriptors still
        resident on the device (bhip_assoc_l2_surf).  -> (pairs, fitQuality) over the batch's compact key-point index space (see fetchAll)."""
        L = _lib.load()
        a = np.ascontiguousarray(srcImages, dtype=np.int32)
        b = np.ascontiguousarray(dstImages, dtype=np.int32)
        if a.shape != b.shape:
            raise IllegalArgumentException("source and destination image lists differ in length")
        total = max(self.totalFeatures(), 1)
        pairs = np.full(total, -1, dtype=np.int32)
        fit = np.zeros(total)
        _check(self.ctx, L.bhip_assoc_l2_surf(self._h, len(a), a.ctypes.data_as(_lib._ip), b.ctypes.data_as(_lib._ip), float(maxError),
                                              1 if backwardsValidation else 0, pairs.ctypes.data_as(_lib._ip), fit.ctypes.data_as(_lib._dp)))
        return pairs, fit

    def counts(self):
        """getNumberOfFeatures() of every image of the last batch (one native call) -> int32 array"""
        out = np.zeros(max(self._batch, 1), dtype=np.int32)
        if self._batch:
            _check(self.ctx, _lib.load().bhip_surf_counts(self._h, out.ctypes.data_as(_lib._ip), len(out)))
        return out[:self._batch]

    def totalFeatures(self):
        n = C.c_longlong(0)
        _check(self.ctx, _lib.load().bhip_surf_total(self._h, C.byref(n)))
        return n.value

    def deviceView(self, image):
        """(dev_desc_ptr, dev_keypoint_ptr, dev_white_ptr, n) of image `image` -- valid until the next detect."""
        d, k, w, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        _check(self.ctx, _lib.load().bhip_surf_dev_view(self._h, image, C.byref(d), C.byref(k), C.byref(w), C.byref(n)))
        return d.value, k.value, w.value, n.value

    def describePoints(self, xy_scale, image=0):
        """computeDescriptors() for a caller-supplied point list on the integral image of the last detect."""
        pts = np.ascontiguousarray(xy_scale, dtype=np.float64).reshape(-1, 3)
        n = len(pts)
        ang = np.zeros(n); white = np.zeros(n, dtype=np.uint8); desc = np.zeros((n, self._dof))
        _check(self.ctx, _lib.load().bhip_surf_describe_points(self._h, image, pts.ctypes.data_as(_lib._dp), n, ang.ctypes.data_as(_lib._dp),
                                                              white.ctypes.data_as(_lib._u8p), desc.ctypes.data_as(_lib._dp)))
        return ang, white, desc

    def fetchIntegral(self, image, width=None, height=None):
        """Integral image of image `image` of the last detect.  The buffer is sized from the detector's own shape (the C side copies
        W*H words of the last detect); width / height, when given, must agree with it."""
        w, h = self._shape
        if (width is not None and width != w) or (height is not None and height != h):
            raise IllegalArgumentException("the last detect ran on %d x %d images, not %s x %s" % (w, h, width, height))
        out = np.zeros((h, w), dtype=np.float32)
        _check(self.ctx, _lib.load().bhip_surf_fetch_integral(self._h, image, out.ctypes.data_as(_lib._fp)))
        return out

    # --- InterestPointDetector / FoundPointSO
    def getNumberOfFeatures(self):
        return len(self._results()[0])

    def getLocation(self, featureIndex):
        x = self._results()[0][featureIndex]
        return Point2D_F64(float(x[0]), float(x[1]))

    def getRadius(self, featureIndex):
        return float(self._results()[0][featureIndex][2]) * 2.0  # BoofDefaults.SURF_SCALE_TO_RADIUS

    def getOrientation(self, featureIndex):
        return float(self._results()[1][featureIndex])

    def getDescription(self, index):
        r = self._results()
        return BrightFeature(self._dof, r[3][index], bool(r[2][index]))

    def hasScale(self):
        return True

    def hasOrientation(self):
        return True


class SurfPlanar_to_DetectDescribePoint(DetectDescribePoint):
    """DetectDescribePoint<Planar<GrayF32>,BrightFeature> (F:abst/feature/detdesc/SurfPlanar_to_DetectDescribePoint.java:40-132 over
    F:alg/feature/detdesc/DetectDescribeSurfPlanar.java and F:alg/feature/describe/DescribePointSurfPlanar.java): key points from the band
    average, orientation with object radius = scale, one descriptor per band concatenated and normalised as a whole."""

    def __init__(self, stable, configDetector, configDescribe, configOrientation, numBands, ctx=None):
        super().__init__(stable, configDetector, configDescribe, configOrientation, ctx)
        self.numBands = int(numBands)
        self._dof = self._dof * self.numBands

    def detect(self, input):
        if input.getNumBands() != self.numBands:
            raise IllegalArgumentException("Unexpected number of bands. Expected %d found %d" % (self.numBands, input.getNumBands()))
        views = [b._in() for b in input.bands]
        start, stride = views[0][1:3]
        for v in views:
            if v[1:3] != (start, stride):
                raise IllegalArgumentException("bands must share startIndex and stride")   # Planar images do (ImageMultiBand layout)
        ptrs = (C.POINTER(C.c_float) * self.numBands)(*[v[0] for v in views])
        self._cache = {}
        self._batch = 0
        for b in input.bands:   # the call passes the Planar image's own size
            _check_extent(input.width, input.height, start, stride, b.data.size)
        _check(self.ctx, _lib.load().bhip_surf_detect_planar_f32(self._h, ptrs, self.numBands, start, stride, input.width, input.height))
        self._batch = 1
        self._image = 0
        self._shape = (input.width, input.height)

    def detectBatch(self, images):
        raise RuntimeError("colour SURF processes one planar frame per call")

    def getRadius(self, featureIndex):
        return float(self._results()[0][featureIndex][2])   # DetectDescribeSurfPlanar.getRadius: the scale itself


class Random:
    """java.util.Random (the JDK's documented linear congruential generator; host-side, needed only to build the BRIEF definition the way
    FactoryBriefDefinition does).  nextGaussian uses math.log / math.sqrt where Java uses StrictMath: the table is *parity unpinned* in the
    last ulp of log -- a Java caller passes the definition its own JVM generated."""

    def __init__(self, seed):
        self.seed = (int(seed) ^ 0x5DEECE66D) & ((1 << 48) - 1)
        self._next_gaussian = None

    def next(self, bits):
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        v = self.seed >> (48 - bits)
        return v - (1 << 32) if v >= (1 << 31) and bits == 32 else v

    def nextInt(self, bound=None):
        if bound is None:
            return self.next(32)
        if bound <= 0:
            raise IllegalArgumentException("bound must be positive")
        if (bound & -bound) == bound:
            return (bound * self.next(31)) >> 31
        while True:
            bits = self.next(31)
            val = bits % bound
            if bits - val + (bound - 1) < (1 << 31):
                return val

    def nextDouble(self):
        return ((self.next(26) << 27) + self.next(27)) * (1.0 / (1 << 53))

    def nextGaussian(self):
        if self._next_gaussian is not None:
            g, self._next_gaussian = self._next_gaussian, None
            return g
        while True:
            v1 = 2 * self.nextDouble() - 1
            v2 = 2 * self.nextDouble() - 1
            s = v1 * v1 + v2 * v2
            if 0 < s < 1:
                break
        m = math.sqrt(-2 * math.log(s) / s)
        self._next_gaussian = v2 * m
        return v1 * m


class BinaryCompareDefinition_I32:
    """F:alg/feature/describe/brief/BinaryCompareDefinition_I32.java: sample points (x,y) and the index pairs that are compared."""

    def __init__(self, radius, samplePoints, compare):
        self.radius = int(radius)
        self.samplePoints = np.ascontiguousarray(samplePoints, dtype=np.int32).reshape(-1, 2)
        self.compare = np.ascontiguousarray(compare, dtype=np.int32).reshape(-1, 2)

    def getLength(self):
        return len(self.compare)


class FactoryBriefDefinition:
    @staticmethod
    def gaussian2(rand, radius, numPairs):
        """F:alg/feature/describe/brief/FactoryBriefDefinition.java:57-85: sample i = (int)(gaussian * sigma) per axis, redrawn until it lies
        inside the circle; compare[i] = (i, rand.nextInt(numPairs)); the RNG calls interleave exactly as in the reference."""
        sigma = (2.0 * radius + 1.0) / 5.0
        pts = np.zeros((numPairs, 2), dtype=np.int32)
        cmp_ = np.zeros((numPairs, 2), dtype=np.int32)
        for i in range(numPairs):
            while True:
                x = int(rand.nextGaussian() * sigma)
                y = int(rand.nextGaussian() * sigma)
                if math.sqrt(x * x + y * y) < radius:
                    break
            pts[i] = (x, y)
            cmp_[i] = (i, rand.nextInt(numPairs))
        return BinaryCompareDefinition_I32(radius, pts, cmp_)


@dataclass
class ConfigBrief:
    """F:abst/feature/describe/ConfigBrief.java:33-52"""
    radius: int = 16
    numPoints: int = 512
    blurSigma: float = -1
    blurRadius: int = 4
    fixed: bool = True

    def checkValidity(self):
        pass


class WrapDescribeBrief:
    """DescribeRegionPoint<T,TupleDesc_B> (F:abst/feature/describe/WrapDescribeBrief.java:30-86) over DescribePointBrief: process() ignores
    orientation and radius and always succeeds."""

    def __init__(self, definition, imageType, ctx=None):
        self.definition = definition
        self.imageType = imageType
        self.length = definition.getLength()
        self.alg = DescribePointBrief(definition.radius, definition.samplePoints, definition.compare, ctx=ctx)

    def createDescription(self):
        return TupleDesc_B(self.length)

    def setImage(self, image):
        self.alg.setImage(image)

    def process(self, x, y, orientation, radius, storage):
        self.alg.process(x, y, storage)
        return True

    def requiresRadius(self): return False
    def requiresOrientation(self): return False
    def getImageType(self): return self.imageType
    def getDescriptionType(self): return TupleDesc_B
    def getCanonicalWidth(self): return self.definition.radius * 2 + 1


class FactoryDescribeRegionPoint:
    @staticmethod
    def brief(config=None, imageType=GrayF32, definition=None, ctx=None):
        """F:factory/feature/describe/FactoryDescribeRegionPoint.java:187-202.  `definition` lets a caller hand in the table its JVM made
        (FactoryBriefDefinition.gaussian2(new Random(123), radius, numPoints)); otherwise it is generated here the same way."""
        config = config or ConfigBrief()
        config.checkValidity()
        if not config.fixed:
            raise RuntimeError("the scale / orientation aware BRIEF (WrapDescribeBriefSo) is not implemented on the GPU (use the Java path)")
        if imageType is not GrayF32 and imageType is not GrayU8:
            raise RuntimeError("only GrayF32 and GrayU8 are implemented on the GPU (use the Java path)")
        if definition is None:
            definition = FactoryBriefDefinition.gaussian2(Random(123), config.radius, config.numPoints)
        return WrapDescribeBrief(definition, imageType, ctx=ctx)


class WrapFHtoInterestPoint:
    """InterestPointDetector over the Fast-Hessian detector (F:abst/feature/detect/interest/WrapFHtoInterestPoint.java:36-90).  On the GPU it
    only runs fused with a describer (FactoryDetectDescribe.fuseTogether); stand-alone detection is FastHessianFeatureDetector."""

    def __init__(self, config=None):
        self.config = config or ConfigFastHessian()


class FactoryInterestPoint:
    @staticmethod
    def fastHessian(config=None):
        """F:factory/feature/detect/interest/FactoryInterestPoint.java:127-130"""
        return WrapFHtoInterestPoint(config)


class DetectDescribeFusion(DetectDescribePoint):
    """DetectDescribePoint<T,TupleDesc_B> = DetectDescribeFusion(fastHessian, null, brief) (F:abst/feature/detdesc/DetectDescribeFusion.java:
    45-165): Fast-Hessian points in detector order, every one described (WrapDescribeBrief.process always returns true), orientation 0
    (WrapFHtoInterestPoint.getOrientation), radius = scale * 2.  Detection, BRIEF and -- through associateImages -- Hamming association run
    on the device without the points or words leaving it (bhip_surf_create_brief)."""

    def __init__(self, detector, describe, ctx=None):
        self.ctx = ctx or Context.default()
        L = _lib.load()
        fh = detector.config._c()
        d = describe.definition
        self.describe = describe
        self._words = (describe.length + 31) // 32
        h = C.c_void_p()
        _check(self.ctx, L.bhip_surf_create_brief(self.ctx._h, C.byref(fh), d.radius, describe.length, d.samplePoints.ctypes.data_as(_lib._i32p),
                                                  d.compare.ctypes.data_as(_lib._i32p), C.byref(h)))
        self._adopt(h)
        self._dof = 0
        self._batch = 0
        self._image = 0
        self._cache = {}

    def createDescription(self):
        return TupleDesc_B(self.describe.length)

    def getDescriptionType(self):
        return TupleDesc_B

    def _results(self, image=None):
        image = self._image if image is None else image
        if image not in self._cache:
            L = _lib.load()
            n = C.c_int(0)
            _check(self.ctx, L.bhip_surf_count(self._h, image, C.byref(n)))
            n = n.value
            xys = np.zeros((n, 3)); ang = np.zeros(n); white = np.zeros(n, dtype=np.uint8); words = np.zeros((n, self._words), dtype=np.int32)
            if n:
                _check(self.ctx, L.bhip_surf_fetch(self._h, image, xys.ctypes.data_as(_lib._dp), ang.ctypes.data_as(_lib._dp),
                                                   white.ctypes.data_as(_lib._u8p), None))
                _check(self.ctx, L.bhip_surf_fetch_brief(self._h, image, words.ctypes.data_as(_lib._i32p)))
            self._cache[image] = (xys, ang, white, words)
        return self._cache[image]

    def fetchAll(self, out=None):
        """(xy_scale [total,3], words [total, ceil(numPoints/32)] int32, starts [batch+1]) of the whole last batch."""
        L = _lib.load()
        counts = self.counts()
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        total = int(starts[-1])
        xys = np.empty((total, 3)); words = np.empty((total, self._words), dtype=np.int32)
        if total:
            _check(self.ctx, L.bhip_surf_fetch_all(self._h, xys.ctypes.data_as(_lib._dp), None, None, None))
            _check(self.ctx, L.bhip_surf_fetch_brief(self._h, -1, words.ctypes.data_as(_lib._i32p)))
        return xys, words, starts

    def associateImages(self, srcImages, dstImages, maxError=Double_MAX_VALUE, backwardsValidation=True):
        """Greedy Hamming association (ScoreAssociateHamming_B) of image srcImages[p] with image dstImages[p] of the last detect, on the
        words still resident on the device (bhip_assoc_hamming_surf)."""
        L = _lib.load()
        a = np.ascontiguousarray(srcImages, dtype=np.int32)
        b = np.ascontiguousarray(dstImages, dtype=np.int32)
        if a.shape != b.shape:
            raise IllegalArgumentException("source and destination image lists differ in length")
        total = max(self.totalFeatures(), 1)
        pairs = np.full(total, -1, dtype=np.int32)
        fit = np.zeros(total)
        _check(self.ctx, L.bhip_assoc_hamming_surf(self._h, len(a), a.ctypes.data_as(_lib._ip), b.ctypes.data_as(_lib._ip), float(maxError),
                                                   1 if backwardsValidation else 0, pairs.ctypes.data_as(_lib._ip), fit.ctypes.data_as(_lib._dp)))
        return pairs, fit

    def deviceViewBrief(self, image):
        """(dev_words_ptr, ints_per_feature, n) of image `image` -- valid until the next detect."""
        d, w, n = C.c_void_p(), C.c_int(0), C.c_int(0)
        _check(self.ctx, _lib.load().bhip_surf_dev_view_brief(self._h, image, C.byref(d), C.byref(w), C.byref(n)))
        return d.value, w.value, n.value

    def describePoints(self, xy_scale, image=0):
        raise RuntimeError("a fused BRIEF object describes the points it detects; use DescribePointBrief for a caller's point list")

    def getOrientation(self, featureIndex):
        return 0.0

    def getDescription(self, index):
        return TupleDesc_B(self.describe.length, self._results()[3][index])

    def hasOrientation(self):
        return False   # orientation == null -> detector.hasOrientation() (DetectDescribeFusion.java:150-155)


class FactoryDetectDescribe:
    @staticmethod
    def fuseTogether(detector, orientation, describe, ctx=None):
        """F:factory/feature/detdesc/FactoryDetectDescribe.java:279-284.  On the GPU: Fast-Hessian + (no orientation) + fixed BRIEF."""
        if not isinstance(detector, WrapFHtoInterestPoint) or orientation is not None or not isinstance(describe, WrapDescribeBrief):
            raise RuntimeError("only fuseTogether(fastHessian, null, brief) is implemented on the GPU (use the Java path)")
        return DetectDescribeFusion(detector, describe, ctx=ctx)

    @staticmethod
    def surfColorFast(configDetector=None, configDesc=None, configOrientation=None, imageType=None, ctx=None):
        """F:factory/feature/detdesc/FactoryDetectDescribe.java:154-176"""
        if not isinstance(imageType, PlanarType):
            raise IllegalArgumentException("Image type not supported")
        return SurfPlanar_to_DetectDescribePoint(False, configDetector, configDesc, configOrientation, imageType.numBands, ctx)

    @staticmethod
    def surfColorStable(configDetector=None, configDescribe=None, configOrientation=None, imageType=None, ctx=None):
        """F:factory/feature/detdesc/FactoryDetectDescribe.java:246-268"""
        if not isinstance(imageType, PlanarType):
            raise IllegalArgumentException("Image type not supported")
        return SurfPlanar_to_DetectDescribePoint(True, configDetector, configDescribe, configOrientation, imageType.numBands, ctx)

    @staticmethod
    def surfFast(configDetector=None, configDesc=None, configOrientation=None, imageType=GrayF32, ctx=None):
        if imageType is not GrayF32 and imageType is not GrayU8:
            raise RuntimeError("only GrayF32 and GrayU8 are implemented on the GPU (use the Java path)")
        return DetectDescribePoint(False, configDetector, configDesc, configOrientation, ctx)

    @staticmethod
    def surfStable(configDetector=None, configDescribe=None, configOrientation=None, imageType=GrayF32, ctx=None):
        if imageType is not GrayF32 and imageType is not GrayU8:
            raise RuntimeError("only GrayF32 and GrayU8 are implemented on the GPU (use the Java path)")
        return DetectDescribePoint(True, configDetector, configDescribe, configOrientation, ctx)
