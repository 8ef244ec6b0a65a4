"""Dense optical flow: FactoryDenseOpticalFlow.flowKlt (F:struct/flow, F:abst/flow, F:alg/flow, F:factory/flow).  Rules, deviations
and limits: bhip_flow_klt_dev_f32 in include/boofhip.h."""
import ctypes as C
import math

import numpy as np

from .. import _lib
from .core import IllegalArgumentException, _check, _ctx
from .image import GrayF32, GrayS16, GrayU8, InterleavedType, Planar, PlanarType
from .klt import PkltConfig

__all__ = ["DenseOpticalFlow", "FactoryDenseOpticalFlow", "ImageFlow"]


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
        _check(self.ctx, fn(self.ctx._h, C.byref(self.config.config._c()), self.radius, scales, len(scales), *source._out(), *destination._out(), w, h,
                            out.ctypes.data_as(_lib._fp), 0, 2 * w))
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
