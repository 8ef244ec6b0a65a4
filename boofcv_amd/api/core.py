"""What every family shares: the exception type, status checking, the context, native handle ownership and the page-locked
result pool.  Errors: BHIP_ERR_INVALID -> IllegalArgumentException, everything else -> RuntimeError (which is what a BOverride hook throws to
make the reference fall back to its Java code)."""
import atexit
import ctypes as C
import sys
import threading
import weakref

import numpy as np

from .. import _lib

__all__ = ["Context", "Double_MAX_VALUE", "Float_MAX_VALUE", "IllegalArgumentException"]


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


def _ctx(ctx):
    return ctx or Context.default()


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
