"""Horn-Schunck dense optical flow: FactoryDenseOpticalFlow.hornSchunck (F:factory/flow/FactoryDenseOpticalFlow.java:122-138),
HornSchunck_to_DenseOpticalFlow (F:abst/flow/HornSchunck_to_DenseOpticalFlow.java:31-53) over HornSchunck_F32 / HornSchunck_U8
(F:alg/flow/HornSchunck.java, HornSchunck_F32.java, HornSchunck_U8.java), ConfigHornSchunck (F:factory/flow/ConfigHornSchunck.java:28-44).

A module beside the api package (like census.py, best5.py and enhance.py): it takes ImageFlow, the image types and the view marshaller from
boofcv_amd.api and adds no name there; api.FactoryDenseOpticalFlow.hornSchunck keeps refusing.  hornSchunckPyramid and broxWarping (in-place
successive over-relaxation) and region (a serial best-match search with order-dependent ties) stay on the Java path: their results depend on
raster order.

process() gives the single-threaded Java result bit for bit: the flow is reset to zero (resetOutput is true and has no setter) and iterated
numIterations times.  Rules and limits: bhip_flow_hs_dev_f32 in include/boofhip.h.  Deviations: derivY(width-1, height-1), which the reference
never writes, is 0, the value of a freshly constructed instance; HornSchunck_F32.computeDerivT's fourth tap (:114) reads image1's pixel
(x+1, y+1) whatever the two strides are; a flow whose size differs from the images raises IllegalArgumentException (the Java indexes past it);
numIterations <= 0 gives the zero flow, as the Java loop does."""
import numpy as np

from . import _lib
from .api.core import IllegalArgumentException, _check, _ctx
from .api.image import GrayF32, GrayU8

__all__ = ["ConfigHornSchunck", "DenseOpticalFlowHornSchunck", "FactoryDenseOpticalFlowHornSchunck"]


class ConfigHornSchunck:
    """F:factory/flow/ConfigHornSchunck.java: alpha -- larger values place more importance on flow smoothness; numIterations"""

    def __init__(self, alpha=20.0, numIterations=1000):
        self.alpha, self.numIterations = float(alpha), int(numIterations)

    def checkValidity(self):
        pass


class DenseOpticalFlowHornSchunck:
    """DenseOpticalFlow<GrayF32 | GrayU8> as FactoryDenseOpticalFlow.hornSchunck builds it"""

    def __init__(self, alpha, numIterations, inputType, ctx=None):
        self.alpha, self.numIterations, self.inputType = float(alpha), int(numIterations), inputType
        self.ctx = _ctx(ctx)

    def setNumIterations(self, numIterations):
        self.numIterations = int(numIterations)

    def process(self, source, destination, flow):
        if not isinstance(source, self.inputType) or not isinstance(destination, self.inputType):
            raise IllegalArgumentException("this algorithm takes %s images" % self.inputType.__name__)
        if source.width != destination.width or source.height != destination.height:
            raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape
        if flow.width != source.width or flow.height != source.height:
            raise IllegalArgumentException("the flow is %d x %d, the images are %d x %d" % (flow.width, flow.height, source.width, source.height))
        w, h = source.width, source.height
        out = np.empty((h, w, 2), dtype=np.float32)
        src, dst = source._out(), destination._out()   # validated before anything reaches C
        fn = _lib.load().bhip_flow_hs_u8 if self.inputType is GrayU8 else _lib.load().bhip_flow_hs_f32
        _check(self.ctx, fn(self.ctx._h, self.alpha, self.numIterations, *src, *dst, w, h, out.ctypes.data_as(_lib._fp), 0, 2 * w))
        flow.data[...] = out

    def getInputType(self):
        return self.inputType


class FactoryDenseOpticalFlowHornSchunck:
    """FactoryDenseOpticalFlow.hornSchunck on the GPU"""

    @staticmethod
    def hornSchunck(config, imageType, ctx=None):
        """hornSchunck(config, imageType) (:122-138): config None = new ConfigHornSchunck().  Image types the GPU does not have raise
        RuntimeError: use the Java path."""
        if config is None:
            config = ConfigHornSchunck()
        if imageType is not GrayF32 and imageType is not GrayU8:
            raise RuntimeError("Horn-Schunck runs on the GPU for GrayF32 and GrayU8 images only (use the Java path)")
        return DenseOpticalFlowHornSchunck(config.alpha, config.numIterations, imageType, ctx)
