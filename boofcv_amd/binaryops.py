"""Binary image operations: BinaryImageOps on GrayU8 0/1 images and GrayS32 label images (I:alg/filter/binary/BinaryImageOps.java).
  logicAnd / logicOr / logicXor / invert                       :69-145
  erode4 / dilate4 / erode8 / dilate8 (numTimes)               :158-361
  edge4 / edge8 (outsideZero), removePointNoise                :258-411
  contourLabels: the labelled image and getContours().size of contour(input, rule, output)   :457-469; the point lists are not produced
  relabel, labelToBinary                                       :509-578

A module beside the api package (like binary.py, census.py and best5.py): it takes the image types and the view marshaller from boofcv_amd.api
and adds no name there.  Method names, argument meaning and `output == None` declaring a new image follow the reference; shape mismatches and
erode4 with numTimes <= 0 raise IllegalArgumentException before anything reaches C.  Not implemented on the GPU and refused: thin, contour /
contourExternal (the ordered point lists are a serial walk), labelToClusters, clusterToBinary."""
import enum

import numpy as np

from . import _lib
from .api.core import IllegalArgumentException, _check, _ctx
from .api.image import GrayS32, GrayU8

__all__ = ["BinaryImageOps", "ConnectRule"]


class ConnectRule(enum.IntEnum):
    """T:struct/ConnectRule.java (values = BHIP_CONNECT_*)"""
    FOUR = _lib.BHIP_CONNECT_FOUR
    EIGHT = _lib.BHIP_CONNECT_EIGHT


def _same(a, b):
    if (a.width, a.height) != (b.width, b.height):
        raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape


def _declare(input, output, kind=GrayU8, inputKind=GrayU8):
    """InputSanityCheck.checkDeclare"""
    if not isinstance(input, inputKind):
        raise IllegalArgumentException("expected a %s input" % inputKind.__name__)
    if output is None:
        return kind(input.width, input.height)
    if not isinstance(output, kind):
        raise IllegalArgumentException("expected a %s output" % kind.__name__)
    _same(input, output)
    return output


def _unsupported(what):
    raise IllegalArgumentException("%s is not implemented on the GPU" % what)


class BinaryImageOps:
    """Static methods as in the reference; every one takes an optional ctx= (the default context otherwise)."""

    @staticmethod
    def _logic(op, inputA, inputB, output, ctx):
        if not isinstance(inputB, GrayU8):
            raise IllegalArgumentException("expected a GrayU8 input")
        output = _declare(inputA, output)
        _same(inputA, inputB)
        ctx = _ctx(ctx)
        a, b, o = inputA._in(), inputB._out(), output._out()
        _check(ctx, _lib.load().bhip_binary_logic_u8(ctx._h, op, a[0], a[1], a[2], *b, a[3], a[4], *o))
        return output

    @staticmethod
    def logicAnd(inputA, inputB, output=None, ctx=None):
        return BinaryImageOps._logic(_lib.BHIP_LOGIC_AND, inputA, inputB, output, ctx)

    @staticmethod
    def logicOr(inputA, inputB, output=None, ctx=None):
        return BinaryImageOps._logic(_lib.BHIP_LOGIC_OR, inputA, inputB, output, ctx)

    @staticmethod
    def logicXor(inputA, inputB, output=None, ctx=None):
        return BinaryImageOps._logic(_lib.BHIP_LOGIC_XOR, inputA, inputB, output, ctx)

    @staticmethod
    def invert(input, output=None, ctx=None):
        output = _declare(input, output)
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_binary_invert_u8(ctx._h, *input._in(), *output._out()))
        return output

    @staticmethod
    def _morph(op, input, numTimes, output, ctx):
        output = _declare(input, output)
        if op == _lib.BHIP_MORPH_ERODE4 and numTimes <= 0:
            raise IllegalArgumentException("numTimes must be >= 1")
        if output.data is input.data:
            raise IllegalArgumentException("input and output of a neighbourhood operation must not share their array")
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_binary_morph_u8(ctx._h, op, int(numTimes), *input._in(), *output._out()))
        return output

    @staticmethod
    def erode4(input, numTimes, output=None, ctx=None):
        return BinaryImageOps._morph(_lib.BHIP_MORPH_ERODE4, input, numTimes, output, ctx)

    @staticmethod
    def dilate4(input, numTimes, output=None, ctx=None):
        return BinaryImageOps._morph(_lib.BHIP_MORPH_DILATE4, input, numTimes, output, ctx)

    @staticmethod
    def erode8(input, numTimes, output=None, ctx=None):
        return BinaryImageOps._morph(_lib.BHIP_MORPH_ERODE8, input, numTimes, output, ctx)

    @staticmethod
    def dilate8(input, numTimes, output=None, ctx=None):
        return BinaryImageOps._morph(_lib.BHIP_MORPH_DILATE8, input, numTimes, output, ctx)

    @staticmethod
    def _edge(rule, input, output, outsideZero, ctx):
        output = _declare(input, output)
        if output.data is input.data:
            raise IllegalArgumentException("input and output of a neighbourhood operation must not share their array")
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_binary_edge_u8(ctx._h, int(rule), int(bool(outsideZero)), *input._in(), *output._out()))
        return output

    @staticmethod
    def edge4(input, output=None, outsideZero=True, ctx=None):
        return BinaryImageOps._edge(ConnectRule.FOUR, input, output, outsideZero, ctx)

    @staticmethod
    def edge8(input, output=None, outsideZero=True, ctx=None):
        return BinaryImageOps._edge(ConnectRule.EIGHT, input, output, outsideZero, ctx)

    @staticmethod
    def removePointNoise(input, output=None, ctx=None):
        output = _declare(input, output)
        if output.data is input.data:
            raise IllegalArgumentException("input and output of a neighbourhood operation must not share their array")
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_binary_remove_point_noise_u8(ctx._h, *input._in(), *output._out()))
        return output

    @staticmethod
    def contourLabels(input, rule, output=None, ctx=None):
        """The labelled image and getContours().size of BinaryImageOps.contour(input, rule, output); the point lists are not produced.
        `output` (a GrayS32 of the input's shape) is written; -> numBlobs.  Pass a GrayS32 to read the labels."""
        rule = ConnectRule(rule)
        output = _declare(input, output, GrayS32)
        ctx = _ctx(ctx)
        n = _lib._i(0)
        _check(ctx, _lib.load().bhip_label_blobs_u8_s32(ctx._h, int(rule), *input._in(), *output._out(), n))
        return n.value

    @staticmethod
    def relabel(input, labels, ctx=None):
        if not isinstance(input, GrayS32):
            raise IllegalArgumentException("expected a GrayS32 image")
        table = np.ascontiguousarray(labels, np.int32)
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_relabel_s32(ctx._h, *input._in(), table.ctypes.data_as(_lib._ip), len(table)))

    @staticmethod
    def labelToBinary(labelImage, binaryImage=None, *selection, ctx=None):
        """labelToBinary(labelImage, binaryImage), labelToBinary(labelImage, binaryImage, selectedBlobs: sequence of bool) or
        labelToBinary(labelImage, binaryImage, numLabels, *selected) as in the reference (:524-578)"""
        binaryImage = _declare(labelImage, binaryImage, GrayU8, GrayS32)
        table, n = None, 0
        if len(selection) == 1 and not isinstance(selection[0], (int, np.integer)):
            sel = np.ascontiguousarray(np.asarray(selection[0], bool), np.uint8)
            table, n = sel.ctypes.data_as(_lib._u8p), len(sel)
        elif selection:
            sel = np.zeros(int(selection[0]), np.uint8)
            for s in selection[1:]:
                if not 0 <= s < len(sel):
                    raise IndexError("selected label %d outside numLabels %d" % (s, len(sel)))   # ArrayIndexOutOfBoundsException
                sel[s] = 1
            table, n = sel.ctypes.data_as(_lib._u8p), len(sel)
        ctx = _ctx(ctx)
        _check(ctx, _lib.load().bhip_label_to_binary_s32_u8(ctx._h, *labelImage._in(), *binaryImage._out(), table, n))
        return binaryImage

    # ---- what stays on the Java path ----
    @staticmethod
    def thin(input, maxIterations, output=None, ctx=None):
        _unsupported("thin (BinaryThinning)")

    @staticmethod
    def contour(input, rule, output=None, ctx=None):
        _unsupported("contour (the point lists; contourLabels gives the labelled image and the count)")

    @staticmethod
    def contourExternal(input, rule, ctx=None):
        _unsupported("contourExternal")

    @staticmethod
    def labelToClusters(labelImage, numLabels, queue=None, ctx=None):
        _unsupported("labelToClusters")

    @staticmethod
    def clusterToBinary(clusters, binary, ctx=None):
        _unsupported("clusterToBinary")
