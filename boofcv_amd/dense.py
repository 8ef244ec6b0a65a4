"""Dense descriptors: FactoryDescribeImageDense.hog / .sift (F:factory/feature/dense/FactoryDescribeImageDense.java:108-165), DescribeImageDense
(F:abst/feature/dense/DescribeImageDense.java), DescribeImageDenseHoG over DescribeDenseHogFastAlg / DescribeDenseHogAlg
(F:abst/feature/dense/DescribeImageDenseHoG.java, F:alg/feature/dense/*.java), DescribeImageDenseSift over DescribeDenseSiftAlg
(F:abst/feature/dense/DescribeImageDenseSift.java), DescribeImageDense_Convert, ConfigDenseHoG, ConfigDenseSift and DenseSampling.

A module beside the api package (like sift.py and hornschunck.py): it takes the image types and the view marshaller from boofcv_amd.api and adds
no name there.  ConfigSiftDescribe is sift.py's.

Counts, locations and their order equal the single-threaded Java result; HOG descriptors (and the fast variant's float cell histograms) equal it
bit for bit wherever Math.atan narrows to the same float, dense SIFT descriptors to the last ulp of Math.atan2.  Rules, refusals and limits: the
bhip_dense_* section of include/boofhip.h.  Not pinned against the jars (georegression and ddogleg are not part of the reference tree):
UtilAngle.atanSafe / domain2PI / dist, UtilGaussian.computePDF; Math.atan / Math.atan2 are the device library's.

Refused with IllegalArgumentException: surfFast / surfStable (GenericDenseDescribeImageDense describes every grid point through
DescribeRegionPoint with a fixed orientation and scale, an entry the SURF kernels do not have: they take the key points of their own detector);
Planar and interleaved image types (HOG would reduce the bands' gradients with MAX_F); pixel types other than GrayU8 and GrayF32; any other
DescribeRegionPoint behind DescribeImageDense."""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from .api.core import IllegalArgumentException, _check, _ctx
from .api.image import GrayF32, GrayU8, TupleDesc_F64
from .sift import ConfigSiftDescribe

__all__ = ["ConfigDenseHoG", "ConfigDenseSift", "DenseSampling", "Point2D_I32", "DescribeImageDense", "DescribeImageDenseHoG", "DescribeImageDenseSift",
           "FactoryDescribeImageDense"]


@dataclass
class Point2D_I32:
    x: int = 0
    y: int = 0


class DenseSampling:
    """F:factory/feature/dense/DenseSampling.java: the sample period in pixels along x and y (doubles)"""

    def __init__(self, periodX=0.0, periodY=0.0):
        self.periodX, self.periodY = float(periodX), float(periodY)


class ConfigDenseHoG:
    """F:factory/feature/dense/ConfigDenseHoG.java: 9, 8, 3, 3, 1, fastVariant = true"""

    def __init__(self, orientationBins=9, pixelsPerCell=8, cellsPerBlockX=3, cellsPerBlockY=3, stepBlock=1, fastVariant=True):
        self.orientationBins, self.pixelsPerCell = int(orientationBins), int(pixelsPerCell)
        self.cellsPerBlockX, self.cellsPerBlockY, self.stepBlock = int(cellsPerBlockX), int(cellsPerBlockY), int(stepBlock)
        self.fastVariant = bool(fastVariant)

    def checkValidity(self):
        pass


class ConfigDenseSift:
    """F:factory/feature/dense/ConfigDenseSift.java: sift = new ConfigSiftDescribe() (sigmaToPixels is not used), sampling = DenseSampling(6, 6)"""

    def __init__(self, sampling=None):
        self.sift = ConfigSiftDescribe()
        self.sampling = DenseSampling(6, 6) if sampling is None else sampling

    def checkValidity(self):
        if self.sampling is None:
            raise IllegalArgumentException("Most specify sampling")


def _hog_args(c):
    return (int(c.orientationBins), int(c.pixelsPerCell), int(c.cellsPerBlockX), int(c.cellsPerBlockY), int(c.stepBlock), 1 if c.fastVariant else 0)


def _sift_args(c):
    """-> (widthSubregion, widthGrid, numHistogramBins), (weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY)"""
    s = c.sift
    return ((int(s.widthSubregion), int(s.widthGrid), int(s.numHistogramBins)),
            (float(s.weightingSigmaFraction), float(s.maxDescriptorElementValue), float(c.sampling.periodX), float(c.sampling.periodY)))


def _raise(status, what):
    raise (RuntimeError if status == _lib.BHIP_ERR_UNSUPPORTED else IllegalArgumentException)(what)


class DescribeImageDense:
    """DescribeImageDense<T, TupleDesc_F64>: process(input), then getDescriptions() and getLocations() (the centre of every region); the arrays
    `descriptors` [n, dof] and `locations` [n, 2] hold the same"""

    def __init__(self, imageType, dof, ctx=None):
        self.imageType, self._dof, self._ctxArg = imageType, int(dof), ctx
        self.descriptors, self.locations = np.zeros((0, self._dof)), np.zeros((0, 2), np.int32)

    @property
    def ctx(self):
        if self._ctxArg is None:
            self._ctxArg = _ctx(None)
        return self._ctxArg

    def _layout(self, width, height):
        raise NotImplementedError

    def _call(self, input, src, desc, xy, n, cap):
        raise NotImplementedError

    def _run(self, input):
        if not isinstance(input, self.imageType):
            raise IllegalArgumentException("this descriptor takes %s images" % self.imageType.__name__)
        src = input._in()
        cap = self._layout(input.width, input.height)
        desc, xy, n = np.empty((max(cap, 1), self._dof), np.float64), np.empty((max(cap, 1), 2), np.int32), C.c_int(0)
        self._call(input, src, desc, xy, n, cap)
        assert n.value == cap, "the grid of a frame is the host's"
        return desc[:cap], xy[:cap]

    def process(self, input):
        self.descriptors, self.locations = self._run(input)

    def getDescriptions(self):
        return [TupleDesc_F64(self._dof, d) for d in self.descriptors]

    def getLocations(self):
        return [Point2D_I32(int(x), int(y)) for x, y in self.locations]

    def createDescription(self):
        return TupleDesc_F64(self._dof)

    def getDescriptionType(self):
        return TupleDesc_F64

    def getImageType(self):
        return self.imageType


class _HogCell:
    """DescribeDenseHogFastAlg.Cell"""

    def __init__(self, histogram):
        self.histogram = histogram


class DescribeImageDenseHoG(DescribeImageDense):
    """DescribeImageDenseHoG (behind DescribeImageDense_Convert for GrayU8).  getLocations() are the blocks' centres: process adds half the region
    to BaseDenseHog's top-left pixels, which `topLeft` keeps.  Fast variant: getCell / getCellRows / getCellCols / getDescriptorsInRegion of
    DescribeDenseHogFastAlg"""

    def __init__(self, config, imageType, ctx=None):
        self.config = config
        self._args = _hog_args(config)
        dof = C.c_int(0)
        s = _lib.load().bhip_dense_hog_layout(*self._args, 1, 1, None, None, C.byref(dof), None, 0)
        if s < 0:
            _raise(s, "stepBlock must be >= 1" if config.stepBlock <= 0 else "no dense HOG for this config (include/boofhip.h)")
        super().__init__(imageType, dof.value, ctx)
        self.topLeft = np.zeros((0, 2), np.int32)
        self._cells = np.zeros((0, 0, self._args[0]), np.float32)

    def _layout(self, width, height):
        n = _lib.load().bhip_dense_hog_layout(*self._args, width, height, None, None, None, None, 0)
        if n < 0:
            _raise(n, "no dense HOG for a %d x %d frame" % (width, height))
        return n

    def _call(self, input, src, desc, xy, n, cap):
        L = _lib.load()
        fn = L.bhip_dense_hog_u8 if isinstance(input, GrayU8) else L.bhip_dense_hog_f32
        cells = None
        if self.config.fastVariant:
            ppc = self._args[1]
            self._cells = np.zeros((input.height // ppc, input.width // ppc, self._args[0]), np.float32)
            cells = self._cells.ctypes.data_as(_lib._fp) if self._cells.size else None
        _check(self.ctx, fn(self.ctx._h, *self._args, *src, desc.ctypes.data_as(_lib._dp), xy.ctypes.data_as(_lib._i32p), C.byref(n), cap, cells))

    def process(self, input):
        self.descriptors, self.topLeft = self._run(input)
        rx, ry = self.getRegionWidthPixelX() // 2, self.getRegionWidthPixelY() // 2
        self.locations = self.topLeft + np.array([rx, ry], np.int32)

    def getRegionWidthPixelX(self):
        return self._args[1] * self._args[2]

    def getRegionWidthPixelY(self):
        return self._args[1] * self._args[3]

    def _fast(self):
        if not self.config.fastVariant:
            raise IllegalArgumentException("cells belong to the fast variant (DescribeDenseHogFastAlg)")

    def getCellRows(self):
        self._fast()
        return self._cells.shape[0]

    def getCellCols(self):
        self._fast()
        return self._cells.shape[1]

    def getCell(self, row, col):
        self._fast()
        return _HogCell(self._cells.reshape(-1, self._args[0])[row * self.getCellCols() + col])

    def getDescriptorsInRegion(self, pixelX0, pixelY0, pixelX1, pixelY1, output):
        """DescribeDenseHogFastAlg.getDescriptorsInRegion :129-143, the reference's indexing (y * cellCols) kept"""
        self._fast()
        ppc, cbx, cby = self._args[1], self._args[2], self._args[3]
        gridX0 = int(math.ceil(pixelX0 / float(ppc)))
        gridY0 = int(math.ceil(pixelY0 / float(ppc)))
        gridX1 = pixelX1 // ppc - cbx
        gridY1 = pixelY1 // ppc - cby
        for y in range(gridY0, gridY1 + 1):
            index = y * self.getCellCols() + gridX0
            for _ in range(gridX0, gridX1 + 1):
                if index < 0 or index >= len(self.descriptors):
                    raise IndexError(index)   # FastQueue.get
                output.append(TupleDesc_F64(self._dof, self.descriptors[index]))
                index += 1


class DescribeImageDenseSift(DescribeImageDense):
    """DescribeImageDenseSift: the GrayF32 gradient for GrayF32 frames, the GrayS16 one for GrayU8 (GImageDerivativeOps.getDerivativeType)"""

    def __init__(self, config, imageType, ctx=None):
        config.checkValidity()
        self.config = config
        grid, _ = _sift_args(config)
        dof = C.c_int(0)   # the config's own checks, on a frame and periods that pass theirs
        s = _lib.load().bhip_dense_sift_layout(*grid, 1.0, 1.0, 1024, 1024, None, None, C.byref(dof), None, 0)
        if s < 0:
            _raise(s, "no dense SIFT for this describe config (include/boofhip.h)")
        super().__init__(imageType, dof.value, ctx)

    def _layout(self, width, height):
        grid, rest = _sift_args(self.config)
        n = _lib.load().bhip_dense_sift_layout(*grid, rest[2], rest[3], width, height, None, None, None, None, 0)
        if n < 0:
            _raise(n, "no dense SIFT grid for a %d x %d frame with periods (%g, %g): a single row or column of descriptors divides by zero in the reference"
                   % (width, height, rest[2], rest[3]))
        return n

    def _call(self, input, src, desc, xy, n, cap):
        L = _lib.load()
        grid, rest = _sift_args(self.config)
        fn = L.bhip_dense_sift_u8 if isinstance(input, GrayU8) else L.bhip_dense_sift_f32
        _check(self.ctx, fn(self.ctx._h, *grid, *rest, *src, desc.ctypes.data_as(_lib._dp), xy.ctypes.data_as(_lib._i32p), C.byref(n), cap))


def _gray(imageType, what):
    if imageType not in (GrayF32, GrayU8):
        name = getattr(imageType, "__name__", type(imageType).__name__)
        raise IllegalArgumentException("%s on the GPU takes single-band GrayF32 or GrayU8 frames, not %s (Planar / interleaved inputs would need the "
                                       "MAX_F gradient reduction)" % (what, name))
    return imageType


class FactoryDescribeImageDense:
    @staticmethod
    def surfFast(config=None, imageType=GrayF32):
        raise IllegalArgumentException("dense SURF is not on the GPU: GenericDenseDescribeImageDense needs a describe entry at a fixed orientation and "
                                       "scale, which the SURF kernels (tied to their own detector's key points) do not have")

    surfStable = surfFast

    @staticmethod
    def sift(config=None, imageType=GrayF32, ctx=None):
        config = ConfigDenseSift() if config is None else config
        config.checkValidity()
        return DescribeImageDenseSift(config, _gray(imageType, "dense SIFT"), ctx)

    @staticmethod
    def hog(config=None, imageType=GrayF32, ctx=None):
        config = ConfigDenseHoG() if config is None else config
        config.checkValidity()
        return DescribeImageDenseHoG(config, _gray(imageType, "dense HOG"), ctx)
