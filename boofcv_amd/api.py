"""Host-side mirror of the reference's interfaces for the detect -> describe -> associate path, on top of the C ABI.

Names, argument meaning and error behaviour follow the Java reference (waicool20/BoofCV 0.35-SNAPSHOT) so that the parity
tests read like the reference's own tests; every call runs hand-written HIP kernels in libboofhip.so on an MI355X.

    F: = main/boofcv-feature/src/main/java/boofcv/   I: = main/boofcv-ip/src/main/java/boofcv/   T: = main/boofcv-types/src/main/java/boofcv/

  FactoryDetectDescribe.surfStable / surfFast   F:factory/feature/detdesc/FactoryDetectDescribe.java:118-135,209-226
  DetectDescribePoint                            F:abst/feature/detdesc/DetectDescribePoint.java:32-46
  FactoryAssociation.greedy / AssociateDescription   F:factory/feature/associate/FactoryAssociation.java:51-65 ; F:abst/feature/associate/AssociateDescription.java:42-61
  BOverride* hooks (static op classes)           I:alg/filter/convolve/BOverrideConvolveImage.java:37-83 etc.

Errors: BHIP_ERR_INVALID -> IllegalArgumentException, everything else -> RuntimeError (which is what a BOverride hook throws to make the
reference fall back to its Java code).
"""
import atexit
import ctypes as C
import math
import sys
import threading
import weakref
from dataclasses import dataclass

import numpy as np

from . import _lib

Double_MAX_VALUE = 1.7976931348623157e308
Float_MAX_VALUE = float(np.finfo(np.float32).max)


class IllegalArgumentException(ValueError):
    pass


def _check(ctx, status):
    if status == _lib.BHIP_OK:
        return
    msg = _lib.load().bhip_last_error(ctx._h if ctx is not None else None)
    msg = msg.decode(errors="replace") if msg else ""
    if status == _lib.BHIP_ERR_INVALID:
        raise IllegalArgumentException(msg or "invalid argument")
    raise RuntimeError("boofhip status %d: %s" % (status, msg))


class _NativeObject:
    """A Python object that owns one native handle (_h) created on a Context (ctx): bhip_surf, bhip_klt or bhip_bg, destroyed with the
    export named by _destroy.  close() (or garbage collection) destroys it; closing the context closes it first."""
    _destroy = None
    _h = None

    def _adopt(self, handle):
        self._h = handle
        self.ctx._children.add(self)

    def _closed(self):
        """what a subclass forgets with its handle"""

    def close(self):
        """Releases the native object (idempotent; safe after its context has been closed)."""
        if self._h:
            getattr(_lib.load(), self._destroy)(self._h)
            self._h = None
            self._closed()

    def __del__(self, _finalizing=sys.is_finalizing):   # (bound at definition: module globals are gone when this runs late in shutdown)
        try:
            if _finalizing():
                return   # the atexit hook below has closed what was alive; the native library ignores destroy calls after exit began
            self.close()
        except Exception:
            pass


class Context:
    """bhip_ctx: one per host thread per device.

    Lifetime: close() (or garbage collection) destroys the native context after closing every detect+describe object created on it; the
    native library tolerates any order anyway (include/boofhip.h, "handles may be destroyed in any order").  At interpreter exit an
    atexit hook closes every live context while the HIP runtime is still up; finalisers that run later do nothing."""
    _default = {}
    _live = weakref.WeakSet()

    def __init__(self, device=0, stream=None):
        L = _lib.load()
        h = C.c_void_p()
        if stream is None:
            st = L.bhip_ctx_create(device, C.byref(h))
        else:
            st = L.bhip_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h))
        if st != _lib.BHIP_OK:
            raise RuntimeError("bhip_ctx_create(device=%d) failed with status %d: no usable MI355X? (there is no CPU fallback)" % (device, st))
        self._h = h
        self.device = device
        self._children = weakref.WeakSet()
        Context._live.add(self)

    def synchronize(self):
        _check(self, _lib.load().bhip_ctx_synchronize(self._h))

    def lastError(self):
        msg = _lib.load().bhip_last_error(self._h)
        return msg.decode(errors="replace") if msg else ""

    def profile(self, on=True):
        """Bracket every kernel launch with HIP events on this context's stream."""
        _check(self, _lib.load().bhip_profile_enable(self._h, 1 if on else 0))

    def profileReset(self):
        _check(self, _lib.load().bhip_profile_reset(self._h))

    def profileReport(self):
        """{tag: dict(launches, ms, bytes, flops)} accumulated since the last reset."""
        L = _lib.load()
        n = L.bhip_profile_report(self._h, None, 0)
        buf = C.create_string_buffer(max(n, 1))
        L.bhip_profile_report(self._h, buf, n)
        out = {}
        for line in buf.value.decode().splitlines():
            tag, launches, ms, b, f = line.split()
            out[tag] = dict(launches=int(launches), ms=float(ms), bytes=float(b), flops=float(f))
        return out

    def close(self):
        if self._h:
            for child in list(self._children):
                child.close()
            _lib.load().bhip_ctx_destroy(self._h)
            self._h = None

    __del__ = _NativeObject.__del__

    @classmethod
    def _close_all(cls):
        for ctx in list(cls._live):
            try:
                ctx.close()
            except Exception:
                pass
        cls._default.clear()

    @classmethod
    def default(cls, device=0):
        if device not in cls._default:
            cls._default[device] = Context(device)
        return cls._default[device]


atexit.register(Context._close_all)   # runs before module teardown and before the HIP runtime's own exit handlers


class _PinnedPool:
    """Page-locked host blocks (bhip_host_alloc) for the arrays this wrapper hands out or fills on every call -- fetched key points and
    descriptors, match lists -- so that their copies are DMA transfers instead of staged pageable copies (what a JNI provider gets from direct
    ByteBuffers over the same allocator).  Blocks are recycled by size class when the numpy arrays built on them are garbage collected,
    from any thread.  A block still in use when the interpreter exits is left to the runtime, never freed under a live array."""
    _free = {}      # size class -> [address]
    _pooled = 0     # bytes sitting in _free
    _closed = False
    _lock = threading.RLock()   # guards the three above (reentrant: a garbage collection inside a locked section may run _release)
    MIN = 4096
    MAX_POOLED = 1 << 30   # blocks released beyond this go back to the runtime instead of the pool

    @classmethod
    def _size_class(cls, nbytes):
        c = cls.MIN   # 4K, 6K, 8K, 12K, 16K, 24K, ...: powers of two and the sizes half way between them
        while c < nbytes:
            c = c * 3 // 2 if c & (c - 1) == 0 else c * 4 // 3
        return c

    @classmethod
    def block(cls, ctx, nbytes):
        """-> (ctypes uint8 array over a pinned block of at least nbytes, or None when pinned memory is not to be had)"""
        if cls._closed or not ctx._h:
            return None
        size = cls._size_class(max(int(nbytes), 1))
        addr = None
        with cls._lock:
            if cls._free.get(size):
                addr = cls._free[size].pop()
                cls._pooled -= size
        if addr is None:
            p = C.c_void_p()
            if _lib.load().bhip_host_alloc(ctx._h, size, C.byref(p)) != _lib.BHIP_OK or not p.value:
                return None
            addr = p.value
        buf = (C.c_uint8 * size).from_address(addr)
        weakref.finalize(buf, cls._release, addr, size).atexit = False   # not at exit: numpy arrays may still point into the block
        return buf

    @classmethod
    def _release(cls, addr, size, _finalizing=sys.is_finalizing):
        if _finalizing():
            return   # the interpreter is going down: the runtime reclaims the block
        with cls._lock:
            if cls._closed:
                return   # the exit hook has run: as above
            pooled = cls._pooled + size <= cls.MAX_POOLED
            if pooled:
                cls._free.setdefault(size, []).append(addr)
                cls._pooled += size
        if not pooled:
            _lib.load().bhip_host_free(C.c_void_p(addr))

    @classmethod
    def arrays(cls, ctx, specs):
        """specs = [(shape, dtype), ...] -> numpy arrays carved out of ONE pinned block (64-byte aligned each); pageable arrays when no pinned
        memory is available.  Contents are uninitialised."""
        sizes = [int(np.prod(shape)) * np.dtype(dt).itemsize for shape, dt in specs]
        offs, total = [], 0
        for n in sizes:
            offs.append(total)
            total += (n + 63) & ~63
        buf = cls.block(ctx, total) if total else None
        if buf is None:
            return [np.empty(shape, dtype=dt) for shape, dt in specs]
        raw = np.frombuffer(buf, dtype=np.uint8)   # keeps `buf` (and with it the block) alive through .base
        return [raw[o:o + n].view(dt).reshape(shape) for o, n, (shape, dt) in zip(offs, sizes, specs)]

    @classmethod
    def _close(cls):
        L = _lib.load()
        with cls._lock:
            cls._closed = True
            blocks = [addr for lst in cls._free.values() for addr in lst]
            cls._free.clear()
            cls._pooled = 0
        for addr in blocks:
            L.bhip_host_free(C.c_void_p(addr))


atexit.register(_PinnedPool._close)   # registered after Context._close_all, so it runs before it (contexts are still alive)


# ------------------------------------------------------------------------------------------------------------------
# data types
# ------------------------------------------------------------------------------------------------------------------
def _check_extent(width, height, startIndex, stride, size):
    """The raw pointer goes to the C ABI: the view must lie inside its array (a Java array access would throw instead of reading past the end)."""
    if width < 0 or height < 0 or startIndex < 0 or stride < width:
        raise IllegalArgumentException("bad image geometry: width %d height %d startIndex %d stride %d" % (width, height, startIndex, stride))
    if width > 0 and height > 0 and startIndex + (height - 1) * stride + width > size:
        raise IllegalArgumentException("image view (startIndex %d, stride %d, %d x %d) exceeds its data array of %d elements" % (startIndex, stride, width, height, size))


class GrayF32:
    """T:struct/image/GrayF32.java:30 / ImageBase.java:34-52: pixel (x,y) = data[startIndex + y*stride + x]."""

    def __init__(self, width=0, height=0, data=None, startIndex=0, stride=None):
        self.width, self.height = int(width), int(height)
        self.stride = int(width if stride is None else stride)
        self.startIndex = int(startIndex)
        if data is None:
            data = np.zeros(self.startIndex + self.stride * self.height, dtype=np.float32)
        if data.dtype != np.float32 or not data.flags["C_CONTIGUOUS"] or data.ndim != 1:
            raise IllegalArgumentException("data must be a contiguous 1-D float32 array")
        _check_extent(self.width, self.height, self.startIndex, self.stride, data.size)
        self.data = data

    @staticmethod
    def wrap(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        return GrayF32(a.shape[1], a.shape[0], a.reshape(-1))

    def reshape(self, width, height):
        if width * height > self.data.size or self.startIndex != 0:
            self.data = np.zeros(width * height, dtype=np.float32)
            self.startIndex = 0
        self.width, self.height, self.stride = int(width), int(height), int(width)

    def subimage(self, x0, y0, x1, y1):
        if not (0 <= x0 <= x1 <= self.width and 0 <= y0 <= y1 <= self.height):   # ImageBase.subimage throws IllegalArgumentException
            raise IllegalArgumentException("sub-image (%d,%d)-(%d,%d) is outside the %d x %d image" % (x0, y0, x1, y1, self.width, self.height))
        return GrayF32(x1 - x0, y1 - y0, self.data, self.startIndex + y0 * self.stride + x0, self.stride)

    def array(self):
        return np.lib.stride_tricks.as_strided(self.data[self.startIndex:], shape=(self.height, self.width), strides=(4 * self.stride, 4))

    def get(self, x, y):
        if not (0 <= x < self.width and 0 <= y < self.height):
            raise IndexError("Requested pixel is out of bounds: %d %d" % (x, y))  # ImageAccessException
        return float(self.data[self.startIndex + y * self.stride + x])

    def set(self, x, y, v):
        if not (0 <= x < self.width and 0 <= y < self.height):
            raise IndexError("Requested pixel is out of bounds: %d %d" % (x, y))
        self.data[self.startIndex + y * self.stride + x] = v

    def _p(self):
        return self.data.ctypes.data_as(C.POINTER(C.c_float))


@dataclass
class Point2D_F64:
    x: float = 0.0
    y: float = 0.0


@dataclass
class Point2D_I16:
    x: int = 0
    y: int = 0


class TupleDesc_F64:
    """F:struct/feature/TupleDesc_F64.java:30"""

    def __init__(self, numFeatures=0, value=None):
        self.value = np.zeros(numFeatures, dtype=np.float64) if value is None else np.asarray(value, dtype=np.float64)

    def size(self):
        return len(self.value)

    def setTo(self, src):
        self.value = np.array(src.value, dtype=np.float64)


class _GrayInt:
    """Integer single-band images (T:struct/image/GrayU8.java, GrayS16.java, GrayS32.java): pixel (x,y) = data[startIndex + y*stride + x]."""
    dtype = None

    def __init__(self, width=0, height=0, data=None, startIndex=0, stride=None):
        self.width, self.height = int(width), int(height)
        self.stride = int(width if stride is None else stride)
        self.startIndex = int(startIndex)
        if data is None:
            data = np.zeros(self.startIndex + self.stride * self.height, dtype=self.dtype)
        if data.dtype != self.dtype or not data.flags["C_CONTIGUOUS"] or data.ndim != 1:
            raise IllegalArgumentException("data must be a contiguous 1-D %s array" % np.dtype(self.dtype).name)
        _check_extent(self.width, self.height, self.startIndex, self.stride, data.size)
        self.data = data

    @classmethod
    def wrap(cls, a):
        a = np.ascontiguousarray(a, dtype=cls.dtype)
        return cls(a.shape[1], a.shape[0], a.reshape(-1))

    def reshape(self, width, height):
        if width * height > self.data.size or self.startIndex != 0:
            self.data = np.zeros(width * height, dtype=self.dtype)
            self.startIndex = 0
        self.width, self.height, self.stride = int(width), int(height), int(width)

    def subimage(self, x0, y0, x1, y1):
        if not (0 <= x0 <= x1 <= self.width and 0 <= y0 <= y1 <= self.height):
            raise IllegalArgumentException("sub-image (%d,%d)-(%d,%d) is outside the %d x %d image" % (x0, y0, x1, y1, self.width, self.height))
        return type(self)(x1 - x0, y1 - y0, self.data, self.startIndex + y0 * self.stride + x0, self.stride)

    def array(self):
        it = np.dtype(self.dtype).itemsize
        return np.lib.stride_tricks.as_strided(self.data[self.startIndex:], shape=(self.height, self.width), strides=(it * self.stride, it))


class GrayU8(_GrayInt):
    dtype = np.uint8

    def _p(self):
        return self.data.ctypes.data_as(_lib._u8p)


class GrayS16(_GrayInt):
    dtype = np.int16

    def _p(self):
        return self.data.ctypes.data_as(_lib._i16p)


class GrayS32(_GrayInt):
    dtype = np.int32

    def _p(self):
        return self.data.ctypes.data_as(_lib._i32p)


class Planar:
    """T:struct/image/Planar.java: bands of one shape.  Planar(GrayF32, width, height, numBands) or Planar.wrap([bands])."""

    def __init__(self, bandType=None, width=0, height=0, numBands=0):
        if bandType is not None and bandType is not GrayF32:
            raise RuntimeError("only GrayF32 bands are implemented on the GPU")
        self.width, self.height = int(width), int(height)
        self.bands = [GrayF32(width, height) for _ in range(numBands)]

    @staticmethod
    def wrap(bands):
        p = Planar(GrayF32, bands[0].width, bands[0].height, 0)
        for b in bands:
            if b.width != p.width or b.height != p.height:
                raise IllegalArgumentException("bands must have the same shape")
        p.bands = list(bands)
        return p

    def getNumBands(self):
        return len(self.bands)

    def getBand(self, i):
        return self.bands[i]


class PlanarType:
    """ImageType.pl(numBands, GrayF32.class)"""

    def __init__(self, numBands, bandType=None):
        self.numBands, self.bandType = int(numBands), bandType or GrayF32


class BrightFeature(TupleDesc_F64):
    """F:struct/feature/BrightFeature.java:32: SURF descriptor + sign of the Laplacian."""

    def __init__(self, numFeatures=0, value=None, white=False):
        super().__init__(numFeatures, value)
        self.white = bool(white)

    def setTo(self, src):
        super().setTo(src)
        self.white = getattr(src, "white", False)


class TupleDesc_B:
    """F:struct/feature/TupleDesc_B.java:27-40: numBits packed into int32 words."""

    def __init__(self, numBits, data=None):
        self.numBits = int(numBits)
        n = (self.numBits + 31) // 32
        self.data = np.zeros(n, dtype=np.int32) if data is None else np.asarray(data, dtype=np.int32)


@dataclass
class AssociatedIndex:
    """F:struct/feature/AssociatedIndex.java:30-34"""
    src: int = 0
    dst: int = 0
    fitScore: float = 0.0


class MatchScoreType:
    NORM_ERROR = "NORM_ERROR"


# ------------------------------------------------------------------------------------------------------------------
# configuration (public mutable fields, null => defaults, as in the reference)
# ------------------------------------------------------------------------------------------------------------------
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


# ------------------------------------------------------------------------------------------------------------------
# detect + describe
# ------------------------------------------------------------------------------------------------------------------
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
        for im in images:
            _check_extent(im.width, im.height, im.startIndex, im.stride, im.data.size)   # the fields are mutable: validate what is handed over
        n = len(images)
        u8 = isinstance(images[0], GrayU8)
        if any(isinstance(im, GrayU8) != u8 for im in images):
            raise IllegalArgumentException("all images of a batch must have the same type")
        ptrs = (C.POINTER(C.c_uint8 if u8 else C.c_float) * n)(*[im._p() for im in images])
        starts = (C.c_int * n)(*[im.startIndex for im in images])
        strides = (C.c_int * n)(*[im.stride for im in images])
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
        b0 = input.getBand(0)
        for b in input.bands:
            if (b.startIndex, b.stride) != (b0.startIndex, b0.stride):
                raise IllegalArgumentException("bands must share startIndex and stride")   # Planar images do (ImageMultiBand layout)
        ptrs = (C.POINTER(C.c_float) * self.numBands)(*[b._p() for b in input.bands])
        self._cache = {}
        self._batch = 0
        for b in input.bands:
            _check_extent(input.width, input.height, b.startIndex, b.stride, b.data.size)
        _check(self.ctx, _lib.load().bhip_surf_detect_planar_f32(self._h, ptrs, self.numBands, b0.startIndex, b0.stride, input.width, input.height))
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


# ------------------------------------------------------------------------------------------------------------------
# association
# ------------------------------------------------------------------------------------------------------------------
class ScoreAssociateEuclideanSq_F64:
    """F:abst/feature/associate/ScoreAssociateEuclideanSq_F64.java -> DescriptorDistance.euclideanSq"""
    kind, sqrt = "l2", 0

    def getScoreType(self):
        return MatchScoreType.NORM_ERROR


class ScoreAssociateEuclidean_F64:
    kind, sqrt = "l2", 1

    def getScoreType(self):
        return MatchScoreType.NORM_ERROR


class ScoreAssociateHamming_B:
    kind, sqrt = "hamming", 0

    def getScoreType(self):
        return MatchScoreType.NORM_ERROR


class AssociateDescription:
    """WrapAssociateGreedy (F:abst/feature/associate/WrapAssociateGreedy.java:73-123) over AssociateGreedy on the GPU."""

    def __init__(self, score, maxError, backwardsValidation, ctx=None):
        self.ctx = ctx or Context.default()
        self.score = score
        self.maxFitError = float(maxError)
        self.backwardsValidation = bool(backwardsValidation)
        self.listSrc = None
        self.listDst = None
        self._matches = []
        self._unassocSrc = []
        self._pairs = np.zeros(0, dtype=np.int32)
        self._fit = np.zeros(0)
        self._nd = 0

    def setSource(self, listSrc):
        self.listSrc = listSrc

    def setDestination(self, listDst):
        self.listDst = listDst

    @staticmethod
    def _pack(lst, kind):
        if isinstance(lst, np.ndarray):
            return np.ascontiguousarray(lst, dtype=np.float64 if kind == "l2" else np.int32)
        if len(lst) == 0:
            return np.zeros((0, 1), dtype=np.float64 if kind == "l2" else np.int32)
        if kind == "l2":
            return np.ascontiguousarray(np.stack([np.asarray(d.value, dtype=np.float64) for d in lst]))
        return np.ascontiguousarray(np.stack([np.asarray(d.data, dtype=np.int32) for d in lst]))

    def associate(self):
        if self.listSrc is None:
            raise IllegalArgumentException("source features not specified")
        if self.listDst is None:
            raise IllegalArgumentException("destination features not specified")
        kind = self.score.kind
        src = self._pack(self.listSrc, kind)
        dst = self._pack(self.listDst, kind)
        ns, nd = len(src), len(dst)
        length = src.shape[1] if ns else (dst.shape[1] if nd else 1)
        if ns and nd and src.shape[1] != dst.shape[1]:
            raise IllegalArgumentException("descriptor lengths differ")
        pairs, fit = _PinnedPool.arrays(self.ctx, [((ns,), np.int32), ((ns,), np.float64)])
        pairs[:] = -1
        fit[:] = self.maxFitError
        L = _lib.load()
        if ns:
            if kind == "l2":
                _check(self.ctx, L.bhip_assoc_l2_f64(self.ctx._h, src.ctypes.data_as(_lib._dp), ns, dst.ctypes.data_as(_lib._dp), nd, length,
                                                     self.maxFitError, int(self.backwardsValidation), self.score.sqrt,
                                                     pairs.ctypes.data_as(_lib._ip), fit.ctypes.data_as(_lib._dp)))
            else:
                _check(self.ctx, L.bhip_assoc_hamming(self.ctx._h, src.ctypes.data_as(_lib._i32p), ns, dst.ctypes.data_as(_lib._i32p), nd, length,
                                                      self.maxFitError, int(self.backwardsValidation), pairs.ctypes.data_as(_lib._ip),
                                                      fit.ctypes.data_as(_lib._dp)))
        self._pairs, self._fit, self._nd = pairs, fit, nd
        self._matches = None      # the object lists are built when they are asked for (getMatches / getUnassociatedSource)
        self._unassocSrc = None

    @property
    def matches(self):
        if self._matches is None:
            idx = np.nonzero(self._pairs >= 0)[0]
            self._matches = [AssociatedIndex(i, d, f) for i, d, f in zip(idx.tolist(), self._pairs[idx].tolist(), self._fit[idx].tolist())]
        return self._matches

    @property
    def unassocSrc(self):
        if self._unassocSrc is None:
            self._unassocSrc = np.nonzero(self._pairs < 0)[0].tolist()
        return self._unassocSrc

    def getPairs(self):
        return self._pairs

    def getFitQuality(self):
        return self._fit

    def getMatches(self):
        return self.matches

    def getUnassociatedSource(self):
        return self.unassocSrc

    def getUnassociatedDestination(self):
        # FindUnassociated.checkDestination (F:alg/feature/associate/FindUnassociated.java:56-72)
        matched = np.zeros(self._nd, dtype=bool)
        for m in self.matches:
            matched[m.dst] = True
        return [i for i in range(self._nd) if not matched[i]]

    def setMaxScoreThreshold(self, score):
        self.maxFitError = float(score)

    def getScoreType(self):
        return self.score.getScoreType()

    def uniqueSource(self):
        return True

    def uniqueDestination(self):
        return self.backwardsValidation


class AssociateSurfBasic:
    """F:alg/feature/associate/AssociateSurfBasic.java:36-170: SURF features are split by the sign of the Laplacian (BrightFeature.white)
    and each sign is associated on its own -- features of different sign are never matched and each contraction is a quarter of the size."""

    def __init__(self, assoc):
        self.assoc = assoc
        self._src = ([], [])   # (positive, negative) lists of (index, feature)
        self._dst = ([], [])
        self.matches = []
        self.unassociatedSrc = []

    @staticmethod
    def _sort(features):
        pos, neg = [], []
        for i, f in enumerate(features):
            (pos if f.white else neg).append((i, f))
        return pos, neg

    def setSrc(self, src):
        self._src = self._sort(src)

    def setDst(self, dst):
        self._dst = self._sort(dst)

    def swapLists(self):
        self._src, self._dst = self._dst, self._src

    def associate(self):
        self.matches = []
        self.unassociatedSrc = []
        if not (self._src[0] or self._src[1]) or not (self._dst[0] or self._dst[1]):
            return
        for sign in (0, 1):   # positive, then negative
            s, d = self._src[sign], self._dst[sign]
            self.assoc.setSource([f for _, f in s])
            self.assoc.setDestination([f for _, f in d])
            self.assoc.associate()
            for a in self.assoc.getMatches():
                self.matches.append(AssociatedIndex(s[a.src][0], d[a.dst][0], a.fitScore))
            self.unassociatedSrc.extend(s[i][0] for i in self.assoc.getUnassociatedSource())

    def getMatches(self):
        return self.matches

    def totalDestination(self):
        return len(self._dst[0]) + len(self._dst[1])

    def getUnassociatedSrc(self):
        return self.unassociatedSrc

    def getAssoc(self):
        return self.assoc


class WrapAssociateSurfBasic:
    """F:abst/feature/associate/WrapAssociateSurfBasic.java:33-101"""

    def __init__(self, alg):
        self.alg = alg

    def setSource(self, listSrc):
        self.alg.setSrc(listSrc)

    def setDestination(self, listDst):
        self.alg.setDst(listDst)

    def associate(self):
        self.alg.associate()

    def getMatches(self):
        return self.alg.getMatches()

    def getUnassociatedSource(self):
        return self.alg.getUnassociatedSrc()

    def getUnassociatedDestination(self):
        # FindUnassociated.checkDestination (F:alg/feature/associate/FindUnassociated.java:56-72)
        n = self.alg.totalDestination()
        matched = np.zeros(n, dtype=bool)
        for m in self.alg.getMatches():
            matched[m.dst] = True
        return [i for i in range(n) if not matched[i]]

    def setMaxScoreThreshold(self, score):
        self.alg.getAssoc().setMaxScoreThreshold(score)

    def getScoreType(self):
        return self.alg.getAssoc().getScoreType()

    def uniqueSource(self):
        return self.alg.getAssoc().uniqueSource()

    def uniqueDestination(self):
        return self.alg.getAssoc().uniqueDestination()


class FactoryAssociation:
    @staticmethod
    def greedy(score, maxError, backwardsValidation, ctx=None):
        return AssociateDescription(score, maxError, backwardsValidation, ctx)

    @staticmethod
    def defaultScore(tupleType):
        """F:factory/feature/associate/FactoryAssociation.java:141-156"""
        if issubclass(tupleType, TupleDesc_F64):
            return ScoreAssociateEuclideanSq_F64()
        if tupleType is TupleDesc_B:
            return ScoreAssociateHamming_B()
        raise IllegalArgumentException("Unknown tuple type: %s" % tupleType)


# ------------------------------------------------------------------------------------------------------------------
# static op classes = what the BOverride* hooks replace
# ------------------------------------------------------------------------------------------------------------------
def _ctx(ctx):
    return ctx or Context.default()


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
            _check(ctx, _lib.load().bhip_integral_u8_s32(ctx._h, input._p(), input.startIndex, input.stride, input.width, input.height, transformed._p(),
                                                         transformed.startIndex, transformed.stride))
            return transformed
        if transformed is None:
            transformed = GrayF32(input.width, input.height)
        elif transformed.width != input.width or transformed.height != input.height:
            transformed.reshape(input.width, input.height)
        _check(ctx, _lib.load().bhip_integral_f32(ctx._h, input._p(), input.startIndex, input.stride, input.width, input.height, transformed._p(),
                                                  transformed.startIndex, transformed.stride))
        return transformed


class IntegralImageFeatureIntensity:
    @staticmethod
    def hessian(integral, skip, size, intensity, ctx=None):
        """F:alg/feature/detect/intensity/IntegralImageFeatureIntensity.java:43-56; intensity must be (width/skip) x (height/skip)."""
        ctx = _ctx(ctx)
        if isinstance(integral, GrayS32):
            _check(ctx, _lib.load().bhip_hessian_s32(ctx._h, integral._p(), integral.startIndex, integral.stride, integral.width, integral.height, skip, size,
                                                     intensity._p(), intensity.startIndex, intensity.stride))
            return
        _check(ctx, _lib.load().bhip_hessian_f32(ctx._h, integral._p(), integral.startIndex, integral.stride, integral.width, integral.height, skip, size,
                                                 intensity._p(), intensity.startIndex, intensity.stride))


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
            _check(self.ctx, L.bhip_nonmax_block_minmax_f32(self.ctx._h, intensity._p(), intensity.startIndex, intensity.stride, intensity.width,
                                                           intensity.height, self.radius, self.thresholdMin, self.threshold, self.border, 1,
                                                           1 if self.detectMax else 0, xyMin.ctypes.data_as(_lib._i16p), C.byref(nMin),
                                                           xyMax.ctypes.data_as(_lib._i16p), C.byref(nMax), cap))
            self.foundMinXY = xyMin[:nMin.value]
        else:
            _check(self.ctx, L.bhip_nonmax_block_f32(self.ctx._h, intensity._p(), intensity.startIndex, intensity.stride, intensity.width,
                                                    intensity.height, self.radius, self.threshold, self.border, xyMax.ctypes.data_as(_lib._i16p), cap,
                                                    C.byref(nMax)))
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
        _check(self.ctx, _lib.load().bhip_select_nbest_f32(self.ctx._h, intensityImage._p(), intensityImage.startIndex, intensityImage.stride,
                                                          intensityImage.width, intensityImage.height, xy.ctypes.data_as(_lib._i16p), len(xy),
                                                          int(self.target), 1 if positive else 0, out.ctypes.data_as(_lib._i16p), C.byref(n)))
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
        if (derivX.startIndex, derivX.stride) != (derivY.startIndex, derivY.stride):
            raise IllegalArgumentException("derivX and derivY must share startIndex and stride")
        intensity.reshape(derivX.width, derivX.height)
        L = _lib.load()
        args = (derivX._p(), derivY._p(), derivX.startIndex, derivX.stride, derivX.width, derivX.height, intensity._p(), intensity.startIndex,
                intensity.stride)
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
        _check(self.ctx, fn(self.ctx._h, image._p(), image.startIndex, image.stride, w, h, self.pixelTol, self.minContinuous, self.maxFeaturesFraction,
                            intensity._p() if intensity is not None else None, intensity.startIndex if intensity is not None else 0,
                            intensity.stride if intensity is not None else 0, low.ctypes.data_as(_lib._i16p), C.byref(nLow),
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
            _check(self.ctx, fn(self.ctx._h, C.byref(cfg), integral._p(), integral.startIndex, integral.stride, integral.width,
                                                           integral.height, out.ctypes.data_as(_lib._dp), cap, C.byref(n)))
            if n.value <= cap:
                self.foundPoints = out[:n.value].copy()
                return
            cap = n.value

    def getFoundPoints(self):
        return self.foundPoints


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
    for im in (src, dst):
        _check_extent(im.width, im.height, im.startIndex, im.stride, im.data.size)
    if dst.width != src.width or dst.height != src.height:
        raise IllegalArgumentException("Image shapes do not match")  # InputSanityCheck.checkSameShape
    _check(ctx, fn(ctx._h, kernel.data.ctypes.data_as(_lib._fp), kernel.width, kernel.offset, src._p(), src.startIndex, src.stride, src.width, src.height,
                   dst._p(), dst.startIndex, dst.stride))


class ConvolveImageNoBorder:
    """BOverrideConvolveImage.horizontal/vertical/convolve targets (I:alg/filter/convolve/ConvolveImageNoBorder.java:53-90)"""

    @staticmethod
    def convolve(kernel, input, output, ctx=None):
        ctx = _ctx(ctx)
        if output.width != input.width or output.height != input.height:
            raise IllegalArgumentException("Image shapes do not match")
        _check(ctx, _lib.load().bhip_conv2d_f32(ctx._h, kernel.data.ctypes.data_as(_lib._fp), kernel.width, kernel.offset, input._p(), input.startIndex,
                                                input.stride, input.width, input.height, output._p(), output.startIndex, output.stride))

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
        rc = fn(ctx._h, kp, kw, image._p(), image.startIndex, image.stride, image.width, image.height,
                dest._p(), dest.startIndex, dest.stride, dest.width, dest.height, int(skip))
        _check(ctx, rc)

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
            rc = L.bhip_pyramid_u8(self.ctx._h, taps.ctypes.data_as(_lib._i32p), len(taps), sc.ctypes.data_as(_lib._ip), n, input._p(),
                                   input.startIndex, input.stride, input.width, input.height, packed.ctypes.data_as(_lib._u8p))
        else:
            packed = np.zeros(total.value, dtype=np.float32)
            rc = L.bhip_pyramid_f32(self.ctx._h, self.kernel.data.ctypes.data_as(_lib._fp), self.kernel.width, sc.ctypes.data_as(_lib._ip), n, input._p(),
                                    input.startIndex, input.stride, input.width, input.height, packed.ctypes.data_as(_lib._fp))
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
    @staticmethod
    def mean(input, output, radiusX, radiusY=None, storage=None, ctx=None):
        """BOverrideBlurImageOps.mean target (I:alg/filter/blur/BlurImageOps.java:343-376)"""
        ctx = _ctx(ctx)
        radiusY = radiusX if radiusY is None else radiusY
        if radiusX <= 0 or radiusY <= 0:
            raise IllegalArgumentException("Radius must be > 0")
        if output is None:
            output = GrayF32(input.width, input.height)
        _check(ctx, _lib.load().bhip_mean_f32(ctx._h, input._p(), input.startIndex, input.stride, input.width, input.height, int(radiusX), int(radiusY),
                                              output._p(), output.startIndex, output.stride))
        return output

    @staticmethod
    def median(input, output, radius, ctx=None):
        """BOverrideBlurImageOps.median target (I:alg/filter/blur/BlurImageOps.java:752-765)"""
        ctx = _ctx(ctx)
        if radius <= 0:
            raise IllegalArgumentException("Radius must be > 0")
        if output is None:
            output = GrayF32(input.width, input.height)
        _check(ctx, _lib.load().bhip_median_f32(ctx._h, input._p(), input.startIndex, input.stride, input.width, input.height, int(radius), output._p(),
                                                output.startIndex, output.stride))
        return output

    @staticmethod
    def gaussian(input, output, sigma, radius, storage=None, ctx=None):
        """BOverrideBlurImageOps.gaussian target (I:alg/filter/blur/BlurImageOps.java:406-425)"""
        ctx = _ctx(ctx)
        if output is None:
            output = GrayF32(input.width, input.height)
        _check(ctx, _lib.load().bhip_gaussian_f32(ctx._h, input._p(), input.startIndex, input.stride, input.width, input.height, float(sigma), int(radius),
                                                  output._p(), output.startIndex, output.stride))
        return output


class BorderType:
    """T:struct/border/BorderType.java:28-64.  The gradients have a GPU path for EXTENDED (BoofDefaults.DERIV_BORDER_TYPE); the interpolation of
    ImageDistort has one for ZERO and EXTENDED, and DistortImageOps turns SKIP into EXTENDED with renderAll = false."""
    EXTENDED = "EXTENDED"
    SKIP, NORMALIZED, REFLECT, WRAP, ZERO = "SKIP", "NORMALIZED", "REFLECT", "WRAP", "ZERO"


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
        _check(ctx, getattr(_lib.load(), fn)(ctx._h, orig._p(), orig.startIndex, orig.stride, orig.width, orig.height, derivX._p(), derivY._p(),
                                             derivX.startIndex, derivX.stride, 2 if extended else 0 if border is None else 1))


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
            _check(self.ctx, _lib.load().bhip_brief_u8(self.ctx._h, im._p(), im.startIndex, im.stride, im.width, im.height, self.radius, npts,
                                                      self.samplePoints.ctypes.data_as(_lib._i32p), self.compare.ctypes.data_as(_lib._i32p),
                                                      xy.ctypes.data_as(_lib._dp), n, out.ctypes.data_as(_lib._i32p)))
            return out
        _check(self.ctx, _lib.load().bhip_brief_f32(self.ctx._h, im._p(), im.startIndex, im.stride, im.width, im.height, self.radius, npts,
                                                   self.samplePoints.ctypes.data_as(_lib._i32p), self.compare.ctypes.data_as(_lib._i32p),
                                                   xy.ctypes.data_as(_lib._dp), n, out.ctypes.data_as(_lib._i32p)))
        return out

    def process(self, c_x, c_y, feature):
        feature.data[:] = self.processAll([[c_x, c_y]])[0]


# ------------------------------------------------------------------------------------------------------------------
# pyramid KLT point tracker            G: = main/boofcv-geo/src/main/java/boofcv/
# ------------------------------------------------------------------------------------------------------------------
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


@dataclass
class ConfigGeneralDetector(ConfigExtract):
    """F:abst/feature/detect/interest/ConfigGeneralDetector.java:34-70"""
    maxFeatures: int = -1


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
        if (self.derivX.startIndex, self.derivX.stride) != (self.derivY.startIndex, self.derivY.stride):
            raise IllegalArgumentException("derivX and derivY must share startIndex and stride")
        for im in (self.image, self.derivX, self.derivY):
            _check_extent(im.width, im.height, im.startIndex, im.stride, im.data.size)
        d, dx, dy = (np.zeros((n, ln), np.float32) for _ in range(3))
        G = np.zeros((n, 3), np.float32)
        ok = np.zeros(n, np.uint8)
        cfg = self.config._c()
        im = self.image
        L = _lib.load()
        fn = L.bhip_klt_set_description_u8 if isinstance(im, GrayU8) else L.bhip_klt_set_description_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(cfg), int(radius), im._p(), im.startIndex, im.stride, self.derivX._p(),
                            self.derivY._p(), self.derivX.startIndex, self.derivX.stride, im.width, im.height,
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
        _check_extent(im.width, im.height, im.startIndex, im.stride, im.data.size)
        L = _lib.load()
        fn = L.bhip_klt_track_u8 if isinstance(im, GrayU8) else L.bhip_klt_track_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(cfg), int(radius), im._p(), im.startIndex, im.stride, im.width, im.height,
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
        _check_extent(image.width, image.height, image.startIndex, image.stride, image.data.size)
        if self._shape != (image.width, image.height) or not self._h:
            self._create(image.width, image.height)
        L = _lib.load()
        start, stride = (C.c_int * 1)(image.startIndex), (C.c_int * 1)(image.stride)
        if self.imageType is GrayU8:
            _check(self.ctx, L.bhip_klt_process_u8(self._h, (_lib._u8p * 1)(image._p()), start, stride))
        else:
            _check(self.ctx, L.bhip_klt_process_f32(self._h, (C.POINTER(C.c_float) * 1)(image._p()), start, stride))

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
        _check(self.ctx, fn(self.ctx._h, C.byref(c._c()), imageLeft._p(), imageLeft.startIndex, imageLeft.stride, imageRight._p(), imageRight.startIndex,
                            imageRight.stride, w, h, d._p(), d.startIndex, d.stride))

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


# ------------------------------------------------------------------------------------------------------------------
# image remap: ImageDistort (rules, deviations and what is refused: bhip_distort_map_u8 in include/boofhip.h)
# ------------------------------------------------------------------------------------------------------------------
class TemplateScoreType:
    """F:factory/feature/detect/template/TemplateScoreType.java:28-64"""
    SUM_ABSOLUTE_DIFFERENCE, SUM_SQUARE_ERROR, NCC, CORRELATION = "SUM_ABSOLUTE_DIFFERENCE", "SUM_SQUARE_ERROR", "NCC", "CORRELATION"
    _ORDINAL = {SUM_ABSOLUTE_DIFFERENCE: _lib.BHIP_TEMPLATE_SAD, SUM_SQUARE_ERROR: _lib.BHIP_TEMPLATE_SSE, NCC: _lib.BHIP_TEMPLATE_NCC,
                CORRELATION: _lib.BHIP_TEMPLATE_CORRELATION}


class TemplateMatchingIntensity:
    """TemplateIntensityImage<GrayU8 | GrayF32> over TemplateSumAbsoluteDifference / TemplateSumSquaredError / TemplateNCC
    (F:alg/feature/detect/template/TemplateIntensityImage.java:56-125).  Rules, limits and deviations: bhip_template_intensity_u8 in
    include/boofhip.h.  The intensity image is written as a whole by every process(), 0 in the border, also with a mask."""

    def __init__(self, type, imageType, ctx=None):
        self.type, self.imageType = type, imageType
        self.ctx = _ctx(ctx)
        self.image = None
        self.intensity = GrayF32(0, 0)
        self.borderX0 = self.borderY0 = self.borderX1 = self.borderY1 = 0

    def setInputImage(self, image):
        self.image = image

    def process(self, template, mask=None):
        image = self.image
        for what, im in (("image", image), ("template", template), ("mask", mask)):
            if im is not None and not isinstance(im, self.imageType):
                raise IllegalArgumentException("the %s must be a %s" % (what, self.imageType.__name__))
        if image is None:
            raise IllegalArgumentException("setInputImage() has not been called")
        self.intensity.reshape(image.width, image.height)
        self.borderX0, self.borderY0 = template.width // 2, template.height // 2
        self.borderX1, self.borderY1 = template.width - self.borderX0, template.height - self.borderY0
        out = self.intensity
        fn = _lib.load().bhip_template_intensity_u8 if self.imageType is GrayU8 else _lib.load().bhip_template_intensity_f32
        m = (mask._p(), mask.startIndex, mask.stride, mask.width, mask.height) if mask is not None else (None, 0, 0, 0, 0)
        _check(self.ctx, fn(self.ctx._h, TemplateScoreType._ORDINAL[self.type], image._p(), image.startIndex, image.stride, image.width, image.height,
                            template._p(), template.startIndex, template.stride, template.width, template.height, *m, out._p(), out.startIndex, out.stride))

    def getIntensity(self): return self.intensity
    def isBorderProcessed(self): return False
    def isMaximize(self): return self.type == TemplateScoreType.NCC
    def getBorderX0(self): return self.borderX0
    def getBorderX1(self): return self.borderX1
    def getBorderY0(self): return self.borderY0
    def getBorderY1(self): return self.borderY1


@dataclass
class Match:
    """F:struct/feature/Match.java:28-52: the template's top-left corner and the fit score, higher is better"""
    x: int = 0
    y: int = 0
    score: float = 0.0


class TemplateMatching:
    """F:alg/feature/detect/template/TemplateMatching.java:69-176: the intensity, the strict block non-maximum suppression on its sub-image
    and the N best by QuickSelect (bhip_template_select_f32 in include/boofhip.h: which matches are kept is pinned, their order is that of
    the restated routine; a match shows its own candidate's score)."""

    def __init__(self, match, ctx=None):
        self.match = match
        self.ctx = _ctx(ctx if ctx is not None else getattr(match, "ctx", None))
        if match.isMaximize():
            config = ConfigExtract(2, -Float_MAX_VALUE, 0, True)
        else:
            config = ConfigExtract(2, -Float_MAX_VALUE, 0, True, True, False)
        self.extractor = FactoryFeatureExtractor.nonmax(config, self.ctx)
        self.template = self.mask = None
        self.maxMatches = 0
        self.imageWidth = self.imageHeight = 0
        self.results = []

    def setMinimumSeparation(self, radius):
        self.extractor.setSearchRadius(radius)

    def setTemplate(self, template, mask, maxMatches):
        self.template, self.mask, self.maxMatches = template, mask, maxMatches

    def setImage(self, image):
        self.match.setInputImage(image)
        self.imageWidth, self.imageHeight = image.width, image.height

    def process(self):
        match = self.match
        if self.mask is None:
            match.process(self.template)
        else:
            match.process(self.template, self.mask)
        intensity = match.getIntensity()
        offsetX = offsetY = 0
        if not match.isBorderProcessed():
            x0, x1 = match.getBorderX0(), self.imageWidth - match.getBorderX1()
            y0, y1 = match.getBorderY0(), self.imageHeight - match.getBorderY1()
            intensity = intensity.subimage(x0, y0, x1 + 1, y1 + 1)
        else:
            offsetX, offsetY = match.getBorderX0(), match.getBorderY0()
        self.extractor.process(intensity)
        cand = np.ascontiguousarray(self.extractor.foundMaxXY if match.isMaximize() else self.extractor.foundMinXY, dtype=np.int16)
        n = len(cand)
        N = max(min(int(self.maxMatches), n), 0)
        xy, score, got = np.zeros((max(N, 1), 2), np.int16), np.zeros(max(N, 1), np.float32), C.c_int(0)
        _check(self.ctx, _lib.load().bhip_template_select_f32(self.ctx._h, intensity._p(), intensity.startIndex, intensity.stride, intensity.width,
                                                             intensity.height, cand.ctypes.data_as(_lib._i16p), n, int(self.maxMatches),
                                                             1 if match.isMaximize() else 0, xy.ctypes.data_as(_lib._i16p),
                                                             score.ctypes.data_as(_lib._fp), C.byref(got)))
        self.results = [Match(int(xy[i, 0]) - offsetX, int(xy[i, 1]) - offsetY, float(score[i])) for i in range(got.value)]

    def getResults(self):
        return self.results


class FactoryTemplateMatching:
    """F:factory/feature/detect/template/FactoryTemplateMatching.java:47-113"""

    @staticmethod
    def createIntensity(type, imageType, ctx=None):
        """IllegalArgumentException where the factory throws it (an image class it has no evaluator for, an unknown type); CORRELATION on
        GrayF32, which the factory answers with TemplateCorrelationFFT, raises RuntimeError: use the Java path."""
        name = getattr(imageType, "__name__", str(imageType))
        if type == TemplateScoreType.CORRELATION:
            if imageType is GrayF32:
                raise RuntimeError("TemplateCorrelationFFT is not implemented on the GPU (use the Java path)")
            raise IllegalArgumentException("Image type not supported. " + name)
        if type not in (TemplateScoreType.SUM_ABSOLUTE_DIFFERENCE, TemplateScoreType.SUM_SQUARE_ERROR, TemplateScoreType.NCC):
            raise IllegalArgumentException("Unknown")
        if imageType is not GrayU8 and imageType is not GrayF32:
            raise IllegalArgumentException("Image type not supported. " + name)
        return TemplateMatchingIntensity(type, imageType, ctx)

    @staticmethod
    def createMatcher(type, imageType, ctx=None):
        return TemplateMatching(FactoryTemplateMatching.createIntensity(type, imageType, ctx))


class InterpolationType:
    """I:alg/interpolate/InterpolationType.java"""
    NEAREST_NEIGHBOR, BILINEAR, BICUBIC, POLYNOMIAL4 = "NEAREST_NEIGHBOR", "BILINEAR", "BICUBIC", "POLYNOMIAL4"


_INTERP_CODE = {InterpolationType.NEAREST_NEIGHBOR: _lib.BHIP_INTERP_NEAREST_NEIGHBOR, InterpolationType.BILINEAR: _lib.BHIP_INTERP_BILINEAR}
_BORDER_CODE = {BorderType.ZERO: _lib.BHIP_BORDER_ZERO, BorderType.EXTENDED: _lib.BHIP_BORDER_EXTENDED}
_ALL_BORDERS = (BorderType.SKIP, BorderType.EXTENDED, BorderType.NORMALIZED, BorderType.REFLECT, BorderType.WRAP, BorderType.ZERO)


class InterpolatePixelS:
    """InterpolatePixelS<T> as FactoryInterpolation builds it: the interpolation rule, the image type and the border (None until setBorder)."""

    def __init__(self, type, imageType, borderType=None):
        self.type, self.imageType, self.borderType = type, imageType, None
        if borderType is not None:
            self.setBorder(borderType)

    def setBorder(self, borderType):
        """alg.setBorder(FactoryImageBorder.single(borderType, imageType)) (I:core/image/border/FactoryImageBorder.java:100-135)"""
        if borderType == BorderType.SKIP:
            raise IllegalArgumentException("Skip border can't be implemented here and has to be done externally")
        if borderType == BorderType.NORMALIZED:
            raise IllegalArgumentException("Normalized can't be supported by this border interface")
        if borderType not in _ALL_BORDERS:
            raise IllegalArgumentException("Border type not supported: %s" % borderType)
        if borderType not in _BORDER_CODE:
            raise RuntimeError("border %s is not implemented on the GPU (use the Java path)" % borderType)
        self.borderType = borderType

    def getBorder(self): return self.borderType
    def getImageType(self): return self.imageType


class FactoryInterpolation:
    """I:factory/interpolate/FactoryInterpolation.java"""

    @staticmethod
    def _typed(type, imageType, borderType):
        if imageType in (GrayF32, GrayU8):
            return InterpolatePixelS(type, imageType, borderType)
        if imageType in (GrayS16, GrayS32):
            raise RuntimeError("only GrayU8 and GrayF32 images are interpolated on the GPU (use the Java path)")
        raise RuntimeError("Unknown image type: %s" % getattr(imageType, "__name__", imageType))

    @staticmethod
    def bilinearPixelS(imageType, borderType=None):
        """:170-192"""
        return FactoryInterpolation._typed(InterpolationType.BILINEAR, imageType, borderType)

    @staticmethod
    def nearestNeighborPixelS(imageType):
        """:302-315"""
        return FactoryInterpolation._typed(InterpolationType.NEAREST_NEIGHBOR, imageType, None)

    @staticmethod
    def createPixelS(min, max, type, borderType, imageType):
        """:80-108"""
        if type == InterpolationType.NEAREST_NEIGHBOR:
            alg = FactoryInterpolation.nearestNeighborPixelS(imageType)
        elif type == InterpolationType.BILINEAR:
            return FactoryInterpolation.bilinearPixelS(imageType, borderType)
        elif type in (InterpolationType.BICUBIC, InterpolationType.POLYNOMIAL4):
            raise RuntimeError("%s interpolation is not implemented on the GPU (use the Java path)" % type)
        else:
            raise IllegalArgumentException("Add type: %s" % type)
        if borderType is not None:
            alg.setBorder(borderType)
        return alg


class PixelTransform:
    """PixelTransform<Point2D_F32> (T:struct/distort/PixelTransform.java): compute(x, y) -> (sx, sy), the source coordinates of destination
    pixel (x, y) as two np.float32.  A caller overrides compute(); such a transform is evaluated on the host into a map."""

    def compute(self, x, y):
        raise NotImplementedError


def _f32(v):
    return np.float32(v)


class PixelTransformAffine_F32(PixelTransform):
    """I:alg/distort/PixelTransformAffine_F32.java over AffinePointOps_F32.transform, as include/boofhip.h defines it (georegression's source is
    not part of the reference tree: the order of operations is the library's definition).  coeff = (a11, a12, a21, a22, tx, ty)."""
    _model = _lib.BHIP_DISTORT_AFFINE

    def __init__(self, a11=1, a12=0, a21=0, a22=1, tx=0, ty=0):
        self.coeff = np.array([a11, a12, a21, a22, tx, ty], dtype=np.float32)

    def compute(self, x, y):
        a11, a12, a21, a22, tx, ty = self.coeff
        x, y = _f32(x), _f32(y)
        return tx + a11 * x + a12 * y, ty + a21 * x + a22 * y


class PixelTransformHomography_F32(PixelTransform):
    """I:alg/distort/PixelTransformHomography_F32.java:33-76 over HomographyPointOps_F32.transform, as include/boofhip.h defines it (same caveat
    as PixelTransformAffine_F32).  coeff = a11 .. a33, row-major."""
    _model = _lib.BHIP_DISTORT_HOMOGRAPHY

    def __init__(self, coeff=(1, 0, 0, 0, 1, 0, 0, 0, 1)):
        self.coeff = np.array(coeff, dtype=np.float32).reshape(9)

    def compute(self, x, y):
        c = self.coeff
        x, y = _f32(x), _f32(y)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = c[6] * x + c[7] * y + c[8]
            return (c[0] * x + c[1] * y + c[2]) / z, (c[3] * x + c[4] * y + c[5]) / z


def _kernel_model(transform):
    """the model code when the kernel can evaluate `transform` itself: one of the two classes with compute() not overridden"""
    for cls in (PixelTransformAffine_F32, PixelTransformHomography_F32):
        if isinstance(transform, cls) and type(transform).compute is cls.compute:
            return cls._model
    return 0


def _host_map(transform, width, height):
    """ImageDistortCache_SB.init (I:alg/distort/ImageDistortCache_SB.java:111-134): the transform at every destination pixel, [height*width*2] float32"""
    if _kernel_model(transform):
        ys, xs = np.mgrid[0:height, 0:width].astype(np.int32)
        sx, sy = transform.compute(xs.astype(np.float32), ys.astype(np.float32))   # the same float32 operations, element by element
        return np.ascontiguousarray(np.stack([sx, sy], axis=-1), dtype=np.float32).reshape(-1)
    m = np.empty((height, width, 2), dtype=np.float32)
    for y in range(height):
        for x in range(width):
            m[y, x] = transform.compute(x, y)
    return m.reshape(-1)


class ImageDistort:
    """ImageDistort<T,T> as FactoryDistort.distortSB builds it (I:alg/distort/ImageDistort.java; ImageDistortBasic_SB.java:56-135 for cached =
    false, ImageDistortCache_SB.java:76-206 for cached = true).  An affine or homography model is evaluated in the kernel when cached is false;
    every other transform, and cached = true, is evaluated on the host into a map once per setModel / destination size.  Source, destination and
    mask must not overlap."""

    def __init__(self, cached, interp, outputType, ctx=None):
        self.cached, self.interp, self.outputType = bool(cached), interp, outputType
        self.ctx = ctx   # None: the default context, created by the first apply
        self.dstToSrc = None
        self.renderAll = True
        self._map, self._mapSize, self._dirty = None, None, True

    def setModel(self, dstToSrc):
        self.dstToSrc = dstToSrc
        self._dirty = True

    def getModel(self): return self.dstToSrc
    def setRenderAll(self, renderAll): self.renderAll = bool(renderAll)
    def getRenderAll(self): return self.renderAll

    def apply(self, srcImg, dstImg, *args):
        """apply(src, dst), apply(src, dst, mask) or apply(src, dst, dstX0, dstY0, dstX1, dstY1)"""
        T = self.outputType
        if not isinstance(srcImg, T) or not isinstance(dstImg, T):
            raise IllegalArgumentException("this ImageDistort takes %s images" % T.__name__)
        if self.dstToSrc is None:
            raise IllegalArgumentException("setModel has not been called")
        if self.interp.borderType is None:
            raise IllegalArgumentException("the interpolation has no border (the reference dereferences null at the first border pixel)")
        mask, crop = None, (0, 0, dstImg.width, dstImg.height)
        if len(args) == 1:
            mask = args[0]
            if not isinstance(mask, GrayU8) or (mask.width, mask.height) != (dstImg.width, dstImg.height):
                raise IllegalArgumentException("the mask is a GrayU8 image of the destination's size")
        elif len(args) == 4:
            crop = tuple(int(v) for v in args)
        elif args:
            raise TypeError("apply(src, dst), apply(src, dst, mask) or apply(src, dst, x0, y0, x1, y1)")
        L = _lib.load()
        self.ctx = _ctx(self.ctx)
        u8 = T is GrayU8
        model = 0 if self.cached else _kernel_model(self.dstToSrc)
        tail = (dstImg.width, dstImg.height) + crop + (_INTERP_CODE[self.interp.type], _BORDER_CODE[self.interp.borderType], 1 if self.renderAll else 0,
                                                         dstImg._p(), dstImg.startIndex, dstImg.stride, mask._p() if mask is not None else None,
                                                         mask.startIndex if mask is not None else 0, mask.stride if mask is not None else 0)
        head = (self.ctx._h, srcImg._p(), srcImg.startIndex, srcImg.stride, srcImg.width, srcImg.height)
        if model:
            fn = L.bhip_distort_model_u8 if u8 else L.bhip_distort_model_f32
            coeff = np.ascontiguousarray(self.dstToSrc.coeff, dtype=np.float32)
            _check(self.ctx, fn(*head, model, coeff.ctypes.data_as(_lib._fp), *tail))
            return
        if self._dirty or self._mapSize != (dstImg.width, dstImg.height):
            self._map = _host_map(self.dstToSrc, dstImg.width, dstImg.height)
            self._mapSize, self._dirty = (dstImg.width, dstImg.height), False
        fn = L.bhip_distort_map_u8 if u8 else L.bhip_distort_map_f32
        _check(self.ctx, fn(*head, self._map.ctypes.data_as(_lib._fp), *tail))


class FactoryDistort:
    """I:factory/distort/FactoryDistort.java"""

    @staticmethod
    def distortSB(cached, interp, outputType, ctx=None):
        """:96-122"""
        if outputType in (GrayS16, GrayS32):
            raise RuntimeError("only GrayU8 and GrayF32 images are distorted on the GPU (use the Java path)")
        if outputType not in (GrayF32, GrayU8):
            raise IllegalArgumentException("Output type not supported: %s" % getattr(outputType, "__name__", outputType))
        if not isinstance(interp, InterpolatePixelS):
            raise RuntimeError("only the single-band pixel interpolations are implemented on the GPU (use the Java path)")
        if interp.imageType is not outputType:
            raise RuntimeError("input and output of one type only on the GPU (use the Java path)")
        return ImageDistort(cached, interp, outputType, ctx)

    @staticmethod
    def distortPL(*args, **kwargs):
        raise RuntimeError("Planar images are not distorted on the GPU (use the Java path)")

    @staticmethod
    def distortIL(*args, **kwargs):
        raise RuntimeError("interleaved images are not distorted on the GPU (use the Java path)")


class DistortImageOps:
    """I:alg/distort/DistortImageOps.java"""

    @staticmethod
    def distortSingle(input, output, *args, ctx=None):
        """distortSingle(input, output, transform, interpType, borderType) (:105-122: SKIP becomes EXTENDED with renderAll = false) or
        distortSingle(input, output, renderAll, transform, interp) (:135-145)"""
        if isinstance(input, Planar):
            raise RuntimeError("Planar images are not distorted on the GPU (use the Java path)")
        if len(args) != 3:
            raise TypeError("distortSingle(input, output, transform, interpType, borderType) or distortSingle(input, output, renderAll, transform, interp)")
        if isinstance(args[0], (bool, np.bool_)):
            renderAll, transform, interp = args
        else:
            transform, interpType, borderType = args
            renderAll = borderType != BorderType.SKIP
            if not renderAll:
                borderType = BorderType.EXTENDED
            interp = FactoryInterpolation.createPixelS(0, 255, interpType, borderType, type(input))
        distorter = FactoryDistort.distortSB(False, interp, type(input), ctx)
        distorter.setRenderAll(renderAll)
        distorter.setModel(transform)
        distorter.apply(input, output)

    @staticmethod
    def affine(input, output, borderType, interpType, a11, a12, a21, a22, dx, dy, ctx=None):
        """:70-92.  Affine2D_F32.invert is georegression's, whose source is not part of the reference tree; it is computed here in float as
        div = a11*a22 - a12*a21; (a22, -a12, -a21, a11)/div; tx' = (a12*ty - a22*tx)/div, ty' = (a21*tx - a11*ty)/div -- the library's
        definition, like the model formulas."""
        a11, a12, a21, a22, tx, ty = (np.float32(v) for v in (a11, a12, a21, a22, dx, dy))
        with np.errstate(divide="ignore", invalid="ignore"):
            div = a11 * a22 - a12 * a21
            inv = PixelTransformAffine_F32(a22 / div, -a12 / div, -a21 / div, a11 / div, (a12 * ty - a22 * tx) / div, (a21 * tx - a11 * ty) / div)
        DistortImageOps.distortSingle(input, output, inv, interpType, borderType, ctx=ctx)


# ------------------------------------------------------------------------------------------------------------------
# boofcv.alg.background: stationary background models (F:alg/background/stationary/*.java, F:factory/background/*.java)
# ------------------------------------------------------------------------------------------------------------------
Float_MIN_VALUE = np.float32(1.401298464324817e-45)


class InterleavedType:
    """ImageType.il(numBands, InterleavedU8.class / InterleavedF32.class): named so that the factories can refuse it"""

    def __init__(self, numBands, bandType=None):
        self.numBands, self.bandType = int(numBands), bandType or GrayF32


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
            return frame._p(), frame.startIndex, 0, frame.stride, frame.width, frame.height, frame
        if not isinstance(frame, Planar) or frame.getNumBands() != self._bands or any(not isinstance(b, self.imageType.bandType) for b in frame.bands):
            raise IllegalArgumentException("this model takes Planar<%s> frames of %d bands" % (self.imageType.bandType.__name__, self._bands))
        a = np.ascontiguousarray(np.stack([b.array() for b in frame.bands]))
        ptr = a.ctypes.data_as(_lib._u8p if a.dtype == np.uint8 else _lib._fp)
        return ptr, 0, frame.width * frame.height, frame.width, frame.width, frame.height, a

    def _call(self, segment, frame, mask):
        L = _lib.load()
        u8 = self._pixel == _lib.BHIP_PIXEL_U8
        ptr, start, bandStride, stride, w, h, keep = self._frame(frame)
        mp, ms, mst = (mask._p(), mask.startIndex, mask.stride) if mask is not None else (None, 0, 0)
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


# ------------------------------------------------------------------------------------------------------------------
# dense optical flow: FactoryDenseOpticalFlow.flowKlt (rules, deviations and limits: bhip_flow_klt_dev_f32 in include/boofhip.h)
# ------------------------------------------------------------------------------------------------------------------
class ImageFlow:
    """F:struct/flow/ImageFlow.java:30-160.  data is float32 [height, width, 2]: (x, y) of every pixel's flow, x = NaN marks an invalid pixel.
    As in Java a new flow is (0, 0), reshape() keeps the elements it has (flat index y * width + x) and invalidateAll() touches x only."""

    class D:
        """ImageFlow.D: a view of one pixel's (x, y)"""

        def __init__(self, cell):
            self._c = cell

        x = property(lambda self: float(self._c[0]), lambda self, v: self._c.__setitem__(0, v))
        y = property(lambda self: float(self._c[1]), lambda self, v: self._c.__setitem__(1, v))

        def set(self, x, y=None):
            if y is None:
                x, y = x.x, x.y
            self._c[0], self._c[1] = x, y

        def markInvalid(self):
            self._c[0] = np.nan

        def getX(self): return self.x
        def getY(self): return self.y
        def isValid(self): return not math.isnan(self.x)

    def __init__(self, width, height):
        self._store = np.zeros((0, 2), dtype=np.float32)
        self.reshape(width, height)

    def reshape(self, width, height):
        width, height = int(width), int(height)
        n = width * height
        if len(self._store) < n:
            grown = np.zeros((n, 2), dtype=np.float32)
            grown[:len(self._store)] = self._store
            self._store = grown
        self.width, self.height = width, height
        self.data = self._store[:n].reshape(height, width, 2)

    def invalidateAll(self):
        self.data[:, :, 0] = np.nan

    def fillZero(self):
        self.data[...] = 0

    def isInBounds(self, x, y):
        return 0 <= x < self.width and 0 <= y < self.height

    def get(self, x, y):
        if not self.isInBounds(x, y):
            raise IllegalArgumentException("Requested pixel is out of bounds: %d %d" % (x, y))
        return ImageFlow.D(self.data[y, x])

    def unsafe_get(self, x, y):
        return ImageFlow.D(self.data[y, x])

    def isValid(self, x, y):
        return self.get(x, y).isValid()

    def getWidth(self): return self.width
    def getHeight(self): return self.height

    def setTo(self, flow):
        n = self.width * self.height
        self._store[:n] = flow._store[:n]


class DenseOpticalFlow:
    """DenseOpticalFlow<GrayF32 | GrayU8> as FactoryDenseOpticalFlow.flowKlt builds it: FlowKlt_to_DenseOpticalFlow
    (F:abst/flow/FlowKlt_to_DenseOpticalFlow.java:76-86) over DenseOpticalFlowKlt (F:alg/flow/DenseOpticalFlowKlt.java:62-131).
    Deviations: a flow whose size differs from the images raises IllegalArgumentException (the Java does not check and indexes with the flow's
    width); a position where the reference throws counts as a failed track.  y of an invalid pixel keeps what `flow` held, as in Java: the
    library writes 0 there and process() merges the kept values."""

    def __init__(self, config, radius, inputType, ctx=None):
        self.config, self.radius, self.inputType = config, int(radius), inputType
        self.ctx = _ctx(ctx)

    def _run(self, source, destination):
        """the flow of a freshly constructed ImageFlow: float32 [height, width, 2], invalid pixels (NaN, 0)"""
        w, h = source.width, source.height
        out = np.empty((h, w, 2), dtype=np.float32)
        scales = (C.c_int * len(self.config.pyramidScaling))(*self.config.pyramidScaling)
        fn = _lib.load().bhip_flow_klt_u8 if self.inputType is GrayU8 else _lib.load().bhip_flow_klt_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(self.config.config._c()), self.radius, scales, len(scales), source._p(), source.startIndex, source.stride,
                            destination._p(), destination.startIndex, destination.stride, w, h, out.ctypes.data_as(_lib._fp), 0, 2 * w))
        return out

    def process(self, source, destination, flow):
        if not isinstance(source, self.inputType) or not isinstance(destination, self.inputType):
            raise IllegalArgumentException("this algorithm takes %s images" % self.inputType.__name__)
        if source.width != destination.width or source.height != destination.height:
            raise IllegalArgumentException("Image shapes do not match")
        if flow.width != source.width or flow.height != source.height:
            raise IllegalArgumentException("the flow is %d x %d, the images are %d x %d" % (flow.width, flow.height, source.width, source.height))
        out = self._run(source, destination)
        invalid = np.isnan(out[:, :, 0])
        out[invalid, 1] = flow.data[invalid, 1]   # markInvalid() sets x only
        flow.data[...] = out

    def getInputType(self):
        return self.inputType


class FactoryDenseOpticalFlow:
    """F:factory/flow/FactoryDenseOpticalFlow.java"""

    @staticmethod
    def flowKlt(configKlt, radius, inputType, derivType, ctx=None):
        """flowKlt(configKlt, radius, inputType, derivType) (:61-82): configKlt None = new PkltConfig(), derivType None = the default derivative
        type (GrayF32 -> GrayF32, GrayU8 -> GrayS16).  radius is the template radius and the neighbourhood radius; configKlt.templateRadius is
        not read.  Type pairs the GPU does not have raise RuntimeError: use the Java path."""
        if configKlt is None:
            configKlt = PkltConfig()
        if isinstance(inputType, (PlanarType, InterleavedType)) or inputType is Planar:
            raise RuntimeError("only GrayF32 and GrayU8 images are implemented on the GPU (use the Java path)")
        if derivType is None:
            derivType = {GrayF32: GrayF32, GrayU8: GrayS16}.get(inputType)
        if (inputType, derivType) not in ((GrayF32, GrayF32), (GrayU8, GrayS16)):
            raise RuntimeError("only GrayF32 images with GrayF32 derivatives and GrayU8 images with GrayS16 derivatives are implemented on the GPU "
                               "(use the Java path)")
        return DenseOpticalFlow(configKlt, radius, inputType, ctx)

    @staticmethod
    def region(*args, **kwargs):
        raise RuntimeError("DenseOpticalFlowBlockPyramid is not implemented on the GPU (use the Java path)")

    @staticmethod
    def hornSchunck(*args, **kwargs):
        raise RuntimeError("HornSchunck is not implemented on the GPU (use the Java path)")

    @staticmethod
    def hornSchunckPyramid(*args, **kwargs):
        raise RuntimeError("HornSchunckPyramid is not implemented on the GPU (use the Java path)")

    @staticmethod
    def broxWarping(*args, **kwargs):
        raise RuntimeError("BroxWarpingSpacial is not implemented on the GPU (use the Java path)")
