"""Image and feature data types (T:struct/image, T:struct/border, F:struct/feature, georegression's points) and the one place
where a host image view is turned into C arguments."""
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .core import IllegalArgumentException

__all__ = ["BorderType", "BrightFeature", "GrayF32", "GrayS16", "GrayS32", "GrayU8", "InterleavedType", "Planar", "PlanarType", "Point2D_F64",
           "Point2D_I16", "TupleDesc_B", "TupleDesc_F64"]


def _check_extent(width, height, startIndex, stride, size):
    """The raw pointer goes to the C ABI: the view must lie inside its array (a Java array access would throw instead of reading past the end)."""
    if width < 0 or height < 0 or startIndex < 0 or stride < width:
        raise IllegalArgumentException("bad image geometry: width %d height %d startIndex %d stride %d" % (width, height, startIndex, stride))
    if width > 0 and height > 0 and startIndex + (height - 1) * stride + width > size:
        raise IllegalArgumentException("image view (startIndex %d, stride %d, %d x %d) exceeds its data array of %d elements" % (startIndex, stride, width, height, size))


class _Gray:
    """Single-band images (T:struct/image/GrayF32.java:30, GrayU8.java, GrayS16.java, GrayS32.java / ImageBase.java:34-52):
    pixel (x,y) = data[startIndex + y*stride + x]."""
    dtype = None   # numpy element type
    _ptr = None    # ctypes pointer type of data

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
        if not (0 <= x0 <= x1 <= self.width and 0 <= y0 <= y1 <= self.height):   # ImageBase.subimage throws IllegalArgumentException
            raise IllegalArgumentException("sub-image (%d,%d)-(%d,%d) is outside the %d x %d image" % (x0, y0, x1, y1, self.width, self.height))
        return type(self)(x1 - x0, y1 - y0, self.data, self.startIndex + y0 * self.stride + x0, self.stride)

    def array(self):
        it = np.dtype(self.dtype).itemsize
        return np.lib.stride_tricks.as_strided(self.data[self.startIndex:], shape=(self.height, self.width), strides=(it * self.stride, it))

    def _p(self):
        return self.data.ctypes.data_as(self._ptr)

    # --- the C ABI's image arguments.  The fields are mutable, so what is handed over is validated here, at the call: C only sees a pointer.
    def _in(self):
        """-> (pointer, startIndex, stride, width, height)"""
        _check_extent(self.width, self.height, self.startIndex, self.stride, self.data.size)
        return self.data.ctypes.data_as(self._ptr), self.startIndex, self.stride, self.width, self.height

    def _out(self):
        """-> (pointer, startIndex, stride): an output, or one of several inputs whose common size is passed once"""
        return self._in()[:3]


class GrayF32(_Gray):
    dtype, _ptr = np.float32, _lib._fp

    def get(self, x, y):
        if not (0 <= x < self.width and 0 <= y < self.height):
            raise IndexError("Requested pixel is out of bounds: %d %d" % (x, y))  # ImageAccessException
        return float(self.data[self.startIndex + y * self.stride + x])

    def set(self, x, y, v):
        if not (0 <= x < self.width and 0 <= y < self.height):
            raise IndexError("Requested pixel is out of bounds: %d %d" % (x, y))
        self.data[self.startIndex + y * self.stride + x] = v


class GrayU8(_Gray):
    dtype, _ptr = np.uint8, _lib._u8p


class GrayS16(_Gray):
    dtype, _ptr = np.int16, _lib._i16p


class GrayS32(_Gray):
    dtype, _ptr = np.int32, _lib._i32p


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


class InterleavedType:
    """ImageType.il(numBands, InterleavedU8.class / InterleavedF32.class): named so that the factories can refuse it"""

    def __init__(self, numBands, bandType=None):
        self.numBands, self.bandType = int(numBands), bandType or GrayF32


class BorderType:
    """T:struct/border/BorderType.java:28-64.  The gradients have a GPU path for EXTENDED (BoofDefaults.DERIV_BORDER_TYPE); the interpolation of
    ImageDistort has one for ZERO and EXTENDED, and DistortImageOps turns SKIP into EXTENDED with renderAll = false."""
    EXTENDED = "EXTENDED"
    SKIP, NORMALIZED, REFLECT, WRAP, ZERO = "SKIP", "NORMALIZED", "REFLECT", "WRAP", "ZERO"


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
