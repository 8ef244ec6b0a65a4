"""Pyramid KLT point tracker (F:alg/tracker/klt, G:abst/feature/tracker, G:factory/feature/tracker).
    G: = main/boofcv-geo/src/main/java/boofcv/"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .core import IllegalArgumentException, _check, _ctx, _NativeObject
from .image import GrayF32, GrayS16, GrayU8, Point2D_I16
from .detect import ConfigExtract, ConfigGeneralDetector, FactoryFeatureExtractor, FactoryIntensityPointAlg, GeneralFeatureDetector

__all__ = ["FactoryPointTracker", "KltConfig", "KltFeature", "KltTrackFault", "KltTracker", "PkltConfig", "PointTrack", "PointTrackerKltPyramid",
           "PyramidKltFeature", "PyramidKltTracker"]


@dataclass
class KltConfig:
    """F:alg/tracker/klt/KltConfig.java:32-49"""
    forbiddenBorder: int = 0
    maxPerPixelError: float = 25.0
    maxIterations: int = 15
    minDeterminant: float = 0.001
    minPositionDelta: float = 0.01

    def _c(self):
        return _lib.KltCfg(int(self.forbiddenBorder), float(self.maxPerPixelError), int(self.maxIterations), float(self.minDeterminant),
                           float(self.minPositionDelta))


class PkltConfig:
    """F:alg/tracker/klt/PkltConfig.java:28-34"""

    def __init__(self, templateRadius=2, pyramidScaling=(1, 2, 4)):
        self.config = KltConfig()
        self.templateRadius = int(templateRadius)
        self.pyramidScaling = [int(s) for s in pyramidScaling]


class KltTrackFault:
    """F:alg/tracker/klt/KltTrackFault.java:28-44 (ordinals)"""
    SUCCESS, DRIFTED, OUT_OF_BOUNDS, FAILED, LARGE_ERROR = range(5)
    NAMES = ("SUCCESS", "DRIFTED", "OUT_OF_BOUNDS", "FAILED", "LARGE_ERROR")


class PointTrack:
    """G:abst/feature/tracker/PointTrack.java: a Point2D_F64 with featureId, cookie and description"""

    def __init__(self, x=0.0, y=0.0, featureId=0):
        self.x, self.y, self.featureId = float(x), float(y), int(featureId)
        self.cookie = None
        self.description = None
        self.fault = KltTrackFault.SUCCESS   # result of the last track() (what made a dropped track drop)

    def set(self, x, y):
        self.x, self.y = float(x), float(y)

    def getDescription(self):
        return self.description

    def setDescription(self, d):
        self.description = d

    def __repr__(self):
        return "PointTrack(%r, %r, id=%d)" % (self.x, self.y, self.featureId)


class KltFeature:
    """F:alg/tracker/klt/KltFeature.java: position, radius, the three (2r+1)^2 templates and Gxx, Gyy, Gxy"""

    def __init__(self, radius):
        self.radius = int(radius)
        w = 2 * self.radius + 1
        self.x = self.y = 0.0
        self.desc, self.derivX, self.derivY = GrayF32(w, w), GrayF32(w, w), GrayF32(w, w)
        self.Gxx = self.Gyy = self.Gxy = 0.0

    def setPosition(self, x, y):
        self.x, self.y = float(np.float32(x)), float(np.float32(y))


class KltTracker:
    """F:alg/tracker/klt/KltTracker.java:147-495 with BilinearRectangle_F32 for the image and the derivatives, on the stage-level entry points
    bhip_klt_set_description_f32 / bhip_klt_track_f32 -- or, for a GrayU8 image with GrayS16 derivatives, BilinearRectangle_U8 / _S16 on
    bhip_klt_set_description_u8 / bhip_klt_track_u8.  Where the reference throws "Region is outside of the image" this raises
    IllegalArgumentException."""

    def __init__(self, config=None, ctx=None):
        self.config = config or KltConfig()
        self.ctx = _ctx(ctx)
        self.image = self.derivX = self.derivY = None
        self.error = 0.0

    def setImage(self, image, derivX=None, derivY=None):
        for d in (derivX, derivY):
            if d is not None and (d.width != image.width or d.height != image.height):
                raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape
        derivType = GrayS16 if isinstance(image, GrayU8) else GrayF32
        if not isinstance(image, (GrayF32, GrayU8)) or any(d is not None and not isinstance(d, derivType) for d in (derivX, derivY)):
            raise RuntimeError("only GrayF32 images with GrayF32 derivatives and GrayU8 images with GrayS16 derivatives are tracked on the GPU "
                               "(use the Java path)")
        self.image, self.derivX, self.derivY = image, derivX, derivY

    unsafe_setImage = setImage

    def getConfig(self):
        return self.config

    def getError(self):
        return self.error

    def setDescriptionAll(self, xy, radius):
        """-> (desc, derivX, derivY [n][(2r+1)^2], G [n][3] = Gxx, Gyy, Gxy, ok [n] uint8) for n positions"""
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        n, ln = len(xy), (2 * radius + 1) ** 2
        if self.derivX is None or self.derivY is None:
            raise IllegalArgumentException("setDescription needs the derivative images")
        (px, *geom), (py, *geomY) = self.derivX._out(), self.derivY._out()
        if geom != geomY:
            raise IllegalArgumentException("derivX and derivY must share startIndex and stride")
        d, dx, dy = (np.zeros((n, ln), np.float32) for _ in range(3))
        G = np.zeros((n, 3), np.float32)
        ok = np.zeros(n, np.uint8)
        cfg = self.config._c()
        im = self.image
        L = _lib.load()
        fn = L.bhip_klt_set_description_u8 if isinstance(im, GrayU8) else L.bhip_klt_set_description_f32
        p, start, stride, w, h = im._in()
        _check(self.ctx, fn(self.ctx._h, C.byref(cfg), int(radius), p, start, stride, px, py, *geom, w, h,
                            xy.ctypes.data_as(_lib._fp), n, d.ctypes.data_as(_lib._fp), dx.ctypes.data_as(_lib._fp),
                            dy.ctypes.data_as(_lib._fp), G.ctypes.data_as(_lib._fp), ok.ctypes.data_as(_lib._u8p)))
        return d, dx, dy, G, ok

    def trackAll(self, xy, radius, desc, derivX, derivY, G):
        """-> (xy [n][2] after track(), fault [n], error [n]) for n features given by their templates"""
        xy = np.array(xy, dtype=np.float32).reshape(-1, 2)
        n = len(xy)
        desc, derivX, derivY, G = (np.ascontiguousarray(a, dtype=np.float32) for a in (desc, derivX, derivY, G))
        fault = np.zeros(n, np.int32)
        err = np.zeros(n, np.float32)
        cfg = self.config._c()
        im = self.image
        L = _lib.load()
        fn = L.bhip_klt_track_u8 if isinstance(im, GrayU8) else L.bhip_klt_track_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(cfg), int(radius), *im._in(),
                            desc.ctypes.data_as(_lib._fp), derivX.ctypes.data_as(_lib._fp), derivY.ctypes.data_as(_lib._fp),
                            G.ctypes.data_as(_lib._fp), xy.ctypes.data_as(_lib._fp), n, fault.ctypes.data_as(_lib._ip),
                            err.ctypes.data_as(_lib._fp)))
        return xy, fault, err

    def setDescription(self, feature):
        d, dx, dy, G, ok = self.setDescriptionAll([[feature.x, feature.y]], feature.radius)
        if ok[0] == 2:
            raise IllegalArgumentException("Region is outside of the image")
        w = 2 * feature.radius + 1
        if ok[0] or not self._fullyOutside(feature):   # a feature fully outside the image is left untouched
            feature.desc.array()[:, :] = d[0].reshape(w, w)
            feature.derivX.array()[:, :] = dx[0].reshape(w, w)
            feature.derivY.array()[:, :] = dy[0].reshape(w, w)
            feature.Gxx, feature.Gyy, feature.Gxy = float(G[0, 0]), float(G[0, 1]), float(G[0, 2])
        return bool(ok[0])

    def _fullyOutside(self, f):
        r, W, H = f.radius, self.image.width, self.image.height
        return f.x < -r or f.x > W + r - 1 or f.y < -r or f.y > H + r - 1

    def track(self, feature):
        G = [[feature.Gxx, feature.Gyy, feature.Gxy]]
        xy, fault, err = self.trackAll([[feature.x, feature.y]], feature.radius, feature.desc.array().reshape(1, -1), feature.derivX.array().reshape(1, -1),
                                       feature.derivY.array().reshape(1, -1), G)
        if fault[0] == _lib.BHIP_KLT_REFERENCE_THROWS:
            raise IllegalArgumentException("Region is outside of the image")
        feature.x, feature.y = float(xy[0, 0]), float(xy[0, 1])
        if fault[0] in (KltTrackFault.SUCCESS, KltTrackFault.LARGE_ERROR):
            self.error = float(err[0])
        return int(fault[0])


class PyramidKltFeature:
    """F:alg/tracker/klt/PyramidKltFeature.java: one KltFeature per layer and the position in the input image"""

    def __init__(self, numLayers, radius):
        self.radius = int(radius)
        self.desc = [KltFeature(radius) for _ in range(numLayers)]
        self.x = self.y = 0.0
        self.cookie = None

    def setPosition(self, x, y):
        self.x, self.y = float(np.float32(x)), float(np.float32(y))

    def getCookie(self):
        return self.cookie


class PyramidKltTracker:
    """F:alg/tracker/klt/PyramidKltTracker.java:58-151 over a KltTracker; the per-layer float arithmetic (x / scale, x * scale) is fp32"""

    def __init__(self, tracker):
        self.tracker = tracker
        self.image = self.derivX = self.derivY = None

    def setImage(self, image, derivX=None, derivY=None):
        if derivX is not None and (image.getNumLayers() != len(derivX) or image.getNumLayers() != len(derivY)):
            raise IllegalArgumentException("Number of layers does not match.")
        self.image, self.derivX, self.derivY = image, derivX, derivY

    def setDescription(self, feature):
        for layer in range(self.image.getNumLayers()):
            scale = np.float32(self.image.getScale(layer))
            x, y = np.float32(feature.x) / scale, np.float32(feature.y) / scale
            if self.derivX is not None:
                self.tracker.unsafe_setImage(self.image.getLayer(layer), self.derivX[layer], self.derivY[layer])
            else:
                self.tracker.unsafe_setImage(self.image.getLayer(layer), None, None)
            feature.desc[layer].setPosition(x, y)
            if not self.tracker.setDescription(feature.desc[layer]):
                return False
        return True

    def track(self, feature):
        x, y = np.float32(feature.x), np.float32(feature.y)
        for layer in range(self.image.getNumLayers() - 1, -1, -1):
            scale = np.float32(self.image.getScale(layer))
            x, y = x / scale, y / scale
            self.tracker.unsafe_setImage(self.image.getLayer(layer), None, None)
            f = feature.desc[layer]
            f.setPosition(x, y)
            ret = self.tracker.track(f)
            if ret != KltTrackFault.SUCCESS:
                return ret
            x, y = np.float32(f.x) * scale, np.float32(f.y) * scale
        feature.setPosition(x, y)
        return KltTrackFault.SUCCESS

    def getError(self):
        return self.tracker.getError()


class PointTrackerKltPyramid(_NativeObject):
    """G:abst/feature/tracker/PointTrackerKltPyramid.java:139-348 as FactoryPointTracker.klt builds it (Shi-Tomasi radius 1 unweighted, Sobel with
    BorderType.EXTENDED, discreteGaussian(scaling, -1, 2), bilinear interpolation; imageType GrayF32 with GrayF32 derivatives, or GrayU8 with
    GrayS16 derivatives on bhip_klt_create_u8 / bhip_klt_process_u8) over one bhip_klt with batch = 1: pyramid, gradient, tracking,
    re-description, corner detection and the track lists all stay on the device.  Differences from the Java object: the lists are returned as
    fresh PointTrack objects (positions are the float PyramidKltFeature.x,y; cookie / description are not kept between calls), dropTrack finds
    its track by featureId, addTrack gives featureId -1, and a track at a position where the reference throws is dropped (fault 5)."""
    _destroy = "bhip_klt_destroy"

    def __init__(self, config, templateRadius, scaling, configExtract, ctx=None, detectBorder=None, imageType=None):
        self.ctx = _ctx(ctx)
        self.imageType = GrayF32 if imageType is None else imageType   # GrayF32 (GrayF32 derivatives) or GrayU8 (GrayS16 derivatives)
        self.config = config or KltConfig()
        self.templateRadius = int(templateRadius)
        self.scaling = [int(s) for s in scaling]
        self.configExtract = configExtract or ConfigGeneralDetector()
        self.configExtract.checkValidity()
        if not self.configExtract.useStrictRule or self.configExtract.detectMinimums or not self.configExtract.detectMaximums:
            raise RuntimeError("only the strict maxima extractor is implemented on the GPU")
        # FactoryDetectPoint.createGeneral: ignoreBorder += radius; GeneralFeatureDetector: at least the intensity's own border (Shi-Tomasi radius 1)
        self.detectBorder = max(self.configExtract.ignoreBorder + self.configExtract.radius, 1) if detectBorder is None else int(detectBorder)
        self._shape = None

    def _create(self, width, height):
        self.close()
        L = _lib.load()
        h = C.c_void_p()
        cfg = self.config._c()
        sc = (C.c_int * len(self.scaling))(*self.scaling)
        create = L.bhip_klt_create_u8 if self.imageType is GrayU8 else L.bhip_klt_create
        _check(self.ctx, create(self.ctx._h, C.byref(cfg), self.templateRadius, sc, len(self.scaling), int(self.configExtract.radius),
                                float(self.configExtract.threshold), int(self.detectBorder), width, height, 1, C.byref(h)))
        self._adopt(h)
        self._shape = (width, height)

    def _need(self):
        if not self._h:
            raise IllegalArgumentException("process() has not been called")

    def process(self, image):
        if not isinstance(image, (GrayF32, GrayU8)):
            raise RuntimeError("only GrayF32 and GrayU8 sequences are tracked on the GPU (use the Java path)")
        if not isinstance(image, self.imageType):
            raise IllegalArgumentException("this tracker was built for %s images, not %s" % (self.imageType.__name__, type(image).__name__))
        p, start, stride, w, h = image._in()
        if self._shape != (w, h) or not self._h:
            self._create(w, h)
        L = _lib.load()
        start, stride = (C.c_int * 1)(start), (C.c_int * 1)(stride)
        if self.imageType is GrayU8:
            _check(self.ctx, L.bhip_klt_process_u8(self._h, (_lib._u8p * 1)(p), start, stride))
        else:
            _check(self.ctx, L.bhip_klt_process_f32(self._h, (C.POINTER(C.c_float) * 1)(p), start, stride))

    def getLayer(self, layer, which=0):
        """layer of the image pyramid (which = 0) or of derivX / derivY (1 / 2) of the last process()"""
        self._need()
        sc = np.asarray(self.scaling, dtype=np.int32)
        dims = np.zeros(2 * len(sc), dtype=np.int32)
        _lib.load().bhip_pyramid_layout(self._shape[0], self._shape[1], sc.ctypes.data_as(_lib._ip), len(sc), dims.ctypes.data_as(_lib._ip), None, None)
        w, h = int(dims[2 * layer]), int(dims[2 * layer + 1])
        if self.imageType is GrayU8:   # the GrayU8 pyramid, GrayS16 derivatives
            if which == 0:
                out = GrayU8(w, h)
                _check(self.ctx, _lib.load().bhip_klt_fetch_layer_u8(self._h, 0, int(layer), out._p()))
            else:
                out = GrayS16(w, h)
                _check(self.ctx, _lib.load().bhip_klt_fetch_layer_s16(self._h, 0, int(layer), int(which), out._p()))
            return out
        out = GrayF32(w, h)
        _check(self.ctx, _lib.load().bhip_klt_fetch_layer(self._h, 0, int(layer), int(which), out._p()))
        return out

    def spawnTracks(self):
        self._need()
        L = _lib.load()
        maxFeatures = self.configExtract.maxFeatures
        if maxFeatures <= 0:
            _check(self.ctx, L.bhip_klt_spawn(self._h, -1))
            return
        # maxFeatures > 0: GeneralFeatureDetector with SelectNBestFeatures (a host call), composed from the existing pieces
        scale0 = np.float32(self.scaling[0])
        exclude = [Point2D_I16(int(np.float32(t.x) / scale0), int(np.float32(t.y) / scale0)) for t in self.getActiveTracks()]
        cfg = ConfigExtract(self.configExtract.radius, self.configExtract.threshold, self.detectBorder)
        derivType = GrayS16 if self.imageType is GrayU8 else GrayF32
        det = GeneralFeatureDetector(FactoryIntensityPointAlg.shiTomasi(1, False, derivType, ctx=self.ctx), FactoryFeatureExtractor.nonmax(cfg, self.ctx))
        det.setMaxFeatures(maxFeatures)
        det.setExcludeMaximum(exclude)
        det.process(self.getLayer(0, 0), self.getLayer(0, 1), self.getLayer(0, 2))
        found = det.getMaximums()
        xy = np.array([[p.x, p.y] for p in found], dtype=np.int16).reshape(-1, 2)
        _check(self.ctx, L.bhip_klt_spawn_points(self._h, xy.ctypes.data_as(_lib._i16p), (C.c_int * 1)(len(xy)), len(xy)))

    def addTrack(self, x, y):
        self._need()
        ok = np.zeros(1, np.uint8)
        _check(self.ctx, _lib.load().bhip_klt_add_tracks(self._h, (C.c_int * 1)(0), (C.c_double * 2)(float(x), float(y)), 1, ok.ctypes.data_as(_lib._u8p)))
        return PointTrack(x, y, -1) if ok[0] else None

    def dropTrack(self, track):
        self._need()
        ok = np.zeros(1, np.uint8)
        _check(self.ctx, _lib.load().bhip_klt_drop_tracks(self._h, (C.c_int * 1)(0), (C.c_longlong * 1)(track.featureId), 1, ok.ctypes.data_as(_lib._u8p)))
        return bool(ok[0])

    def dropAllTracks(self):
        if self._h:
            _check(self.ctx, _lib.load().bhip_klt_drop_all(self._h))

    def reset(self):
        if self._h:
            _check(self.ctx, _lib.load().bhip_klt_reset(self._h))

    def _list(self, which, out):
        out = [] if out is None else out
        if not self._h:
            return out
        ids, xy, fault, _ = _klt_fetch(self.ctx, self._h, which, 0)
        for i in range(len(ids)):
            t = PointTrack(float(xy[i, 0]), float(xy[i, 1]), int(ids[i]))
            t.fault = int(fault[i])
            out.append(t)
        return out

    def getActiveTracks(self, list=None): return self._list(0, list)
    def getNewTracks(self, list=None): return self._list(1, list)
    def getDroppedTracks(self, list=None): return self._list(2, list)
    def getAllTracks(self, list=None): return self.getActiveTracks(list)
    def getInactiveTracks(self, list=None): return [] if list is None else list   # KLT has none: a track with a problem is dropped


def _klt_fetch(ctx, h, which, seq, batch=1):
    """one list (0 active, 1 spawned, 2 dropped) of sequence seq of a bhip_klt with `batch` sequences
    -> (featureId int64 [n], xy float32 [n][2], fault int32 [n], error float32 [n])"""
    L = _lib.load()
    counts = [(C.c_int * batch)() for _ in range(3)]
    _check(ctx, L.bhip_klt_counts(h, *counts))
    n = counts[which][seq]
    ids = np.zeros(n, np.int64)
    xy = np.zeros((n, 2), np.float32)
    fault = np.zeros(n, np.int32)
    err = np.zeros(n, np.float32)
    if n:
        _check(ctx, L.bhip_klt_fetch(h, which, seq, ids.ctypes.data_as(_lib._llp), xy.ctypes.data_as(_lib._fp), fault.ctypes.data_as(_lib._ip),
                                     err.ctypes.data_as(_lib._fp)))
    return ids, xy, fault, err


class FactoryPointTracker:
    """G:factory/feature/tracker/FactoryPointTracker.java:99-145"""

    @staticmethod
    def klt(config, configExtract=None, featureRadius=None, imageType=GrayF32, derivType=None, ctx=None):
        """klt(int[] scaling, ConfigGeneralDetector, int featureRadius, imageType, derivType) or klt(PkltConfig, ConfigGeneralDetector, imageType,
        derivType): the first argument decides"""
        # derivType None = GImageDerivativeOps.getDerivativeType(imageType): GrayF32 for GrayF32, GrayS16 for GrayU8
        if not ((imageType is GrayF32 and derivType in (None, GrayF32)) or (imageType is GrayU8 and derivType in (None, GrayS16))):
            raise RuntimeError("only GrayF32 sequences (GrayF32 derivatives) and GrayU8 sequences (GrayS16 derivatives) are tracked on the GPU "
                               "(use the Java path)")
        if config is None:
            config = PkltConfig()
        if not isinstance(config, PkltConfig):
            config = PkltConfig(featureRadius, config)
        return PointTrackerKltPyramid(config.config, config.templateRadius, config.pyramidScaling, configExtract, ctx, imageType=imageType)
