"""Image enhancement: EnhanceImageOps (I:alg/enhance/EnhanceImageOps.java) and the histogram it starts from
(I:alg/misc/ImageStatistics.java:299-306).
  EnhanceImageOps.equalize(histogram, transform)                                   :65-77     host integer logic, as in Java
  EnhanceImageOps.applyTransform(input, transform, output)                         :86-94     GrayU8
  EnhanceImageOps.equalizeLocal(input, radius, output, histogramLength, workArrays)  :176-232   GrayU8
  EnhanceImageOps.sharpen4 / sharpen8(input, output)                               :307-371   GrayU8 or GrayF32, input and output of one type
  ImageStatistics.histogram(input, minValue, histogram)                            GrayU8

A module beside the api package (like binaryops.py and lines.py): it takes the image types and the view marshaller from boofcv_amd.api and
adds no name there.  Method names, argument meaning, `output == None` declaring a new image, output.reshape for applyTransform /
equalizeLocal and checkSameShape for sharpen follow the reference; what the reference or the C boundary refuses raises
IllegalArgumentException before anything reaches C.  Results equal the single-threaded Java results bit for bit.  Deviations (the device
cannot throw): equalizeLocal ranks a pixel >= histogramLength like any other, histogram drops a pixel outside [minValue, minValue + length),
applyTransform writes 0 for a pixel beyond the table -- the reference throws ArrayIndexOutOfBoundsException in all three.  Refused: the
GrayU16 / GrayS8 / GrayS16 / GrayS32 forms, radius > 255, histogramLength outside 1 .. 256, overlapping input and output of equalizeLocal
and sharpen."""
import numpy as np

from . import _lib
from .api.core import IllegalArgumentException, _check, _ctx
from .api.image import GrayF32, GrayU8

__all__ = ["EnhanceImageOps", "ImageStatistics"]

PATHS = {"auto": _lib.BHIP_EQLOCAL_AUTO, "direct": _lib.BHIP_EQLOCAL_DIRECT, "sliding": _lib.BHIP_EQLOCAL_SLIDING}


def _u8(img, what):
    if not isinstance(img, GrayU8):
        raise IllegalArgumentException("%s: only the GrayU8 form runs on the GPU (GrayU16 / GrayS8 / GrayS16 / GrayS32 are not provided), got %s"
                                       % (what, type(img).__name__))
    return img


def _reshaped(input, output, what):
    """output.reshape(input.width, input.height), or a new image"""
    if output is None:
        return GrayU8(input.width, input.height)
    _u8(output, what)
    output.reshape(input.width, input.height)
    return output


def _no_overlap(input, output, what):
    if input.data is output.data or np.may_share_memory(input.array(), output.array()):
        raise IllegalArgumentException("input and output of %s must not overlap" % what)


def _table(values, what, writable=False):
    t = np.asarray(values)
    if t.ndim != 1 or not 1 <= t.size <= 256 or not np.issubdtype(t.dtype, np.integer):
        raise IllegalArgumentException("%s must be a 1-D integer array of 1 .. 256 entries" % what)
    if writable and not (isinstance(values, np.ndarray) and values.dtype == np.int32 and values.flags.c_contiguous and values.flags.writeable):
        raise IllegalArgumentException("%s must be a writable contiguous int32 array (it is filled in place)" % what)
    return t


def path_value(path):
    """"auto" / "direct" / "sliding" or a BHIP_EQLOCAL_* value -> the value"""
    p = PATHS.get(path, path)
    if p not in PATHS.values():
        raise IllegalArgumentException("equalizeLocal: path must be auto, direct or sliding")
    return p


def check_equalize_local(radius, histogramLength):
    if radius < 0:
        raise IllegalArgumentException("equalizeLocal: radius must be >= 0")
    if radius > 255:
        raise IllegalArgumentException("equalizeLocal: a radius beyond 255 is not supported")
    if not 1 <= histogramLength <= 256:
        raise IllegalArgumentException("equalizeLocal: histogramLength must be in 1 .. 256")


class ImageStatistics:
    @staticmethod
    def histogram(input, minValue, histogram, ctx=None):
        """ImageStatistics.histogram(GrayU8, minValue, int[]): `histogram` (a writable int32 numpy array of 1 .. 256 entries) is cleared and
        filled; -> histogram.  A pixel outside [minValue, minValue + len(histogram)) is dropped (the reference throws)."""
        _u8(input, "histogram")
        _table(histogram, "histogram", writable=True)
        if not 0 <= minValue <= 255:
            raise IllegalArgumentException("histogram: minValue must be in 0 .. 255")
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_histogram_u8(ctx._h, *input._in(), int(minValue), histogram.size, histogram.ctypes.data_as(_lib._ip)))
        return histogram


class EnhanceImageOps:
    """Static methods as in the reference; those that run on the GPU take an optional ctx= (the default context otherwise)."""

    @staticmethod
    def equalize(histogram, transform):
        """transform[i] = ((histogram[0] + .. + histogram[i]) * (len - 1)) / sum in Java's int arithmetic (a product beyond 2^31 wraps, the
        division truncates toward zero); a histogram that sums to 0 raises ZeroDivisionError (ArithmeticException)."""
        h = _table(histogram, "histogram")
        if len(transform) < h.size:
            raise IndexError("transform is shorter than the histogram")   # ArrayIndexOutOfBoundsException
        prefix = np.cumsum(h.astype(np.int64))
        total = int(((int(prefix[-1]) + 2 ** 31) % 2 ** 32) - 2 ** 31)
        if total == 0:
            raise ZeroDivisionError("/ by zero")
        maxValue = h.size - 1
        for i in range(h.size):
            s = ((int(prefix[i]) + 2 ** 31) % 2 ** 32) - 2 ** 31
            p = ((s * maxValue + 2 ** 31) % 2 ** 32) - 2 ** 31
            q = abs(p) // abs(total)
            transform[i] = q if (p < 0) == (total < 0) else -q
        return transform

    @staticmethod
    def applyTransform(input, transform, output=None, ctx=None):
        _u8(input, "applyTransform")
        t = np.ascontiguousarray(_table(transform, "transform"), np.int32)
        output = _reshaped(input, output, "applyTransform")
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_apply_transform_u8(ctx._h, *input._in(), t.ctypes.data_as(_lib._ip), t.size, *output._out()))
        return output

    @staticmethod
    def equalizeLocal(input, radius, output=None, histogramLength=256, workArrays=None, ctx=None, path="auto"):
        """workArrays is accepted and unused (the kernels keep no histogram between pixels that a caller could recycle).  path: "auto",
        or "direct" / "sliding" to force one of the two kernels (they give the same image)."""
        _u8(input, "equalizeLocal")
        check_equalize_local(radius, histogramLength)
        path = path_value(path)
        if output is not None and _u8(output, "equalizeLocal").data is input.data:
            raise IllegalArgumentException("input and output of equalizeLocal must not overlap")
        output = _reshaped(input, output, "equalizeLocal")
        _no_overlap(input, output, "equalizeLocal")
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_equalize_local_u8(ctx._h, *input._in(), int(radius), int(histogramLength), path, *output._out()))
        return output

    @staticmethod
    def _sharpen(rule, input, output, ctx):
        if not isinstance(input, (GrayU8, GrayF32)):
            raise IllegalArgumentException("sharpen%d: expected a GrayU8 or GrayF32 input, got %s" % (rule, type(input).__name__))
        if output is None:
            output = type(input)(input.width, input.height)
        if type(output) is not type(input):
            raise IllegalArgumentException("sharpen%d: input and output must be of one type" % rule)
        if (input.width, input.height) != (output.width, output.height):
            raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape
        _no_overlap(input, output, "sharpen%d" % rule)
        ctx = _ctx(ctx)
        fn = _lib.load().bhip_sharpen_u8 if isinstance(input, GrayU8) else _lib.load().bhip_sharpen_f32
        _check(ctx, fn(ctx._h, rule, *input._in(), *output._out()))
        return output

    @staticmethod
    def sharpen4(input, output=None, ctx=None):
        return EnhanceImageOps._sharpen(4, input, output, ctx)

    @staticmethod
    def sharpen8(input, output=None, ctx=None):
        return EnhanceImageOps._sharpen(8, input, output, ctx)
