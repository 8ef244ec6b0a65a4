"""Image remap: interpolation, pixel transforms and ImageDistort (I:alg/interpolate, I:factory/interpolate, T:struct/distort,
I:alg/distort, I:factory/distort).  Rules, deviations and what is refused: bhip_distort_map_u8 in include/boofhip.h."""

import numpy as np

from .. import _lib
from .core import IllegalArgumentException, _check, _ctx
from .image import BorderType, GrayF32, GrayS16, GrayS32, GrayU8, Planar

__all__ = ["DistortImageOps", "FactoryDistort", "FactoryInterpolation", "ImageDistort", "InterpolatePixelS", "InterpolationType", "PixelTransform",
           "PixelTransformAffine_F32", "PixelTransformHomography_F32"]


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
                                                         *dstImg._out(), *(mask._out() if mask is not None else (None, 0, 0)))
        head = (self.ctx._h, *srcImg._in())
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
