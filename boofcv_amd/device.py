"""Device-resident, batched forms of the boofcv-ip front end (bhip_*_dev_f32 of include/boofhip.h) on torch CUDA tensors.

torch is used for what it is good at here -- device memory and the current stream; every operation is one call into libboofhip.so
(hand-written HIP kernels).  A batch is a [B, H, W] float32 tensor whose last dimension is contiguous; rows may be strided (views work).
Names follow the reference classes the host-buffer forms in boofcv_amd/api/ mirror:

  DeviceImageOps.convolve*      ConvolveImageNoBorder / ConvolveImageNormalized      I:alg/filter/convolve/*.java
  DeviceImageOps.gaussian       BlurImageOps.gaussian                               I:alg/filter/blur/BlurImageOps.java:406-425
  DeviceImageOps.sobel / three  GradientSobel / GradientThree .process              I:alg/filter/derivative/GradientSobel.java:110-124,158-173
  DeviceImageOps.intensity      GradientToEdgeFeatures.intensityE / intensityAbs    F:alg/feature/detect/edge/GradientToEdgeFeatures.java:61-95
  DeviceImageOps.nonmax         NonMaxBlock.process (strict)                        F:alg/feature/detect/extract/NonMaxBlock.java:69-94
  DeviceImageOps.nonmaxMinMax   NonMaxBlockSearchStrict.Min / .Max / .MinMax        F:alg/feature/detect/extract/NonMaxBlockSearchStrict.java:56-248
  DeviceImageOps.fast           FastCornerDetector.process                          F:alg/feature/detect/intensity/FastCornerDetector.java:123-189
  DeviceImageOps.disparityBM    StereoDisparity.process (blockMatch, SAD, GrayU8)   F:factory/feature/disparity/FactoryStereoDisparity.java:62-144
  DeviceImageOps.templateIntensity  TemplateMatchingIntensity.process (SAD, SSE, NCC)   F:alg/feature/detect/template/TemplateIntensityImage.java:56-125
  DeviceImageOps.templateMatch  TemplateMatching.process                            F:alg/feature/detect/template/TemplateMatching.java:117-176
  DeviceImageOps.distort        ImageDistort.apply (distortSB, GrayU8 / GrayF32)    I:alg/distort/ImageDistortBasic_SB.java:56-135, ImageDistortCache_SB.java:76-206
  DeviceImageOps.pyramid        PyramidDiscreteSampleBlur.process                   I:alg/transform/pyramid/PyramidDiscreteSampleBlur.java:88-118
  DeviceImageOps.cornerIntensity  GradientCornerIntensity.process                   F:alg/feature/detect/intensity/impl/ImplSsdCorner_F32.java:62-196
  DeviceImageOps.denseFlowKlt   DenseOpticalFlow.process (flowKlt, GrayF32 / GrayU8)  F:factory/flow/FactoryDenseOpticalFlow.java:61-82
  DeviceImageOps.threshold      InputToBinary.process (FactoryThresholdBinary.threshold)  I:factory/filter/binary/FactoryThresholdBinary.java:318-372
  DeviceImageOps.meanU8 / gaussianU8  BlurImageOps.mean / gaussian on GrayU8           I:alg/filter/blur/BlurImageOps.java:75-141
  DeviceImageOps.binaryLogic / binaryInvert / erode / dilate / edge / removePointNoise   BinaryImageOps (GrayU8 0/1)   I:alg/filter/binary/BinaryImageOps.java:69-411
  DeviceImageOps.labelBlobs     the labelled image and blob count of BinaryImageOps.contour     I:alg/filter/binary/LinearContourLabelChang2004.java:96-152
  DeviceImageOps.relabel / labelToBinary   BinaryImageOps.relabel / labelToBinary                I:alg/filter/binary/BinaryImageOps.java:509-557
  DeviceImageOps.prewitt        GradientPrewitt.process                             I:alg/filter/derivative/GradientPrewitt.java:80-142
  DeviceImageOps.edgeNonMaxCrude4   GradientToEdgeFeatures.nonMaxSuppressionCrude4  F:alg/feature/detect/edge/impl/ImplEdgeNonMaxSuppressionCrude.java:50-242
  DeviceImageOps.houghBinaryPolar   HoughTransformBinary.computeParameters (polar)  F:alg/feature/detect/line/HoughTransformBinary.java:124-135
  DeviceImageOps.houghGradientFoot  HoughTransformGradient.transform (foot of norm) F:alg/feature/detect/line/HoughTransformGradient.java:184-252
  DeviceImageOps.nonmaxRelaxed  NonMaxBlock.process (NonMaxBlockSearchRelaxed.Max)  F:alg/feature/detect/extract/NonMaxBlockSearchRelaxed.java:69-98,227-251
  DeviceImageOps.meanShiftPeak  MeanShiftPeak.search                                F:alg/feature/detect/peak/MeanShiftPeak.java:103-160
  DeviceImageOps.histogram / equalizeTable / applyTransform   ImageStatistics.histogram, EnhanceImageOps.equalize / applyTransform   I:alg/enhance/EnhanceImageOps.java:65-94
  DeviceImageOps.equalizeLocal  EnhanceImageOps.equalizeLocal (GrayU8)              I:alg/enhance/EnhanceImageOps.java:176-232
  DeviceImageOps.sharpen        EnhanceImageOps.sharpen4 / sharpen8 (GrayU8, GrayF32)   I:alg/enhance/EnhanceImageOps.java:307-371
  DeviceImageOps.siftScaleSpace / siftDetect   SiftScaleSpace.initialize + computeNextOctave, SiftDetector.process   F:alg/feature/detect/interest/SiftDetector.java:165-191
  DeviceImageOps.siftDetectDescribe            CompleteSift.process (orientation histograms, 128-element descriptors)    F:alg/feature/detdesc/CompleteSift.java:89-134
  DeviceImageOps.denseHog / denseSift          DescribeDenseHogFastAlg / DescribeDenseHogAlg / DescribeDenseSiftAlg .process       F:alg/feature/dense/*.java
  DeviceImageOps.brief          DescribePointBrief.process                      F:alg/feature/describe/DescribePointBrief.java:73-89
  DeviceKltTracker              PointTrackerKltPyramid, batched over sequences      main/boofcv-geo/.../abst/feature/tracker/PointTrackerKltPyramid.java:139-348
  DeviceBackgroundModel         BackgroundStationaryBasic / Gaussian / Gmm, batched over streams   F:alg/background/stationary/*.java
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .api.background import ConfigBackgroundGmm
from .api.core import Context, IllegalArgumentException, _check, _NativeObject
from .api.klt import KltConfig, PkltConfig, _klt_fetch
from .api.template import TemplateScoreType

INTENSITY_E, INTENSITY_ABS, INTENSITY_SQ = 0, 1, 2


def _geom(t, dtype=torch.float32):
    """(ptr, imageStride, rowStride, W, H, B) of a [B,H,W] CUDA tensor of `dtype` with unit stride along x (strides in elements)"""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.dtype != dtype or not t.is_cuda:
        raise IllegalArgumentException("expected a [B,H,W] %s CUDA tensor" % str(dtype).replace("torch.", ""))
    B, H, W = t.shape
    if W > 1 and t.stride(2) != 1:
        raise IllegalArgumentException("the last dimension must be contiguous")
    if (B > 1 and t.stride(0) < 0) or (H > 1 and t.stride(1) < 0):
        raise IllegalArgumentException("strides must not be negative")
    return C.c_void_p(t.data_ptr()), (t.stride(0) if B > 1 else H * t.stride(1)), t.stride(1) if H > 1 else max(W, t.stride(1)), W, H, B


class DeviceImageOps:
    """All calls are asynchronous on the context's stream (create the Context on torch's current stream to mix with torch ops)."""

    def __init__(self, ctx=None, device=0):
        self.ctx = ctx or Context(device, stream=torch.cuda.current_stream(device).cuda_stream)
        self.L = _lib.load()
        self.device = torch.device("cuda", self.ctx.device)

    def _like(self, t):
        return torch.empty(t.shape, dtype=torch.float32, device=t.device)

    def _conv(self, fn, kernel, offset, src, out):
        k = np.ascontiguousarray(kernel, np.float32)
        out = self._like(src) if out is None else out
        ip, iis, irs, W, H, B = _geom(src)
        op, ois, ors, W2, H2, B2 = _geom(out)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("input and output shapes differ")
        _check(self.ctx, fn(self.ctx._h, k.ctypes.data_as(_lib._fp), len(k), int(offset), ip, iis, irs, W, H, B, op, ois, ors))
        return out

    def convolveHorizontal(self, kernel, offset, src, out=None):
        return self._conv(self.L.bhip_conv_h_dev_f32, kernel, offset, src, out)

    def convolveVertical(self, kernel, offset, src, out=None):
        return self._conv(self.L.bhip_conv_v_dev_f32, kernel, offset, src, out)

    def convolveNormalizedHorizontal(self, kernel, offset, src, out=None):
        return self._conv(self.L.bhip_conv_norm_h_dev_f32, kernel, offset, src, out)

    def convolveNormalizedVertical(self, kernel, offset, src, out=None):
        return self._conv(self.L.bhip_conv_norm_v_dev_f32, kernel, offset, src, out)

    def gaussian(self, src, sigma, radius, out=None):
        out = self._like(src) if out is None else out
        ip, iis, irs, W, H, B = _geom(src)
        op, ois, ors, _, _, _ = _geom(out)
        _check(self.ctx, self.L.bhip_gaussian_dev_f32(self.ctx._h, ip, iis, irs, W, H, B, float(sigma), int(radius), op, ois, ors))
        return out

    def _u8_out(self, src, out, B, H, W):
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.uint8, device=src.device)
        op, ois, ors, W2, H2, B2 = _geom(out, torch.uint8)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("input and output shapes differ")
        return out, op, ois, ors

    def threshold(self, src, config, out=None):
        """InputToBinary.process of FactoryThresholdBinary.threshold(config, GrayU8 | GrayF32) on uint8 or float32 frames [B,H,W] of any row / image
        stride -> the uint8 0/1 images [B,H,W] (`out`, any stride, is written in place and as a whole).  config: a binary.ConfigThreshold; the
        types and image types binary.InputToBinary refuses are refused here too.  No host synchronisation."""
        from . import binary
        u8 = src.dtype == torch.uint8
        binary.InputToBinary(config, binary.GrayU8 if u8 else binary.GrayF32)   # the refusals
        ip, iis, irs, W, H, B = _geom(src, torch.uint8 if u8 else torch.float32)
        out, op, ois, ors = self._u8_out(src, out, B, H, W)
        fn = self.L.bhip_threshold_dev_u8 if u8 else self.L.bhip_threshold_dev_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(config._c()), ip, iis, irs, W, H, B, op, ois, ors))
        return out

    def meanU8(self, src, radiusX, radiusY=None, out=None):
        """BlurImageOps.mean on uint8 frames [B,H,W]"""
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        out, op, ois, ors = self._u8_out(src, out, B, H, W)
        _check(self.ctx, self.L.bhip_mean_dev_u8(self.ctx._h, ip, iis, irs, W, H, B, int(radiusX), int(radiusX if radiusY is None else radiusY), op, ois, ors))
        return out

    def gaussianU8(self, src, radius, out=None):
        """BlurImageOps.gaussian(GrayU8, -1, radius) on uint8 frames [B,H,W]"""
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        out, op, ois, ors = self._u8_out(src, out, B, H, W)
        _check(self.ctx, self.L.bhip_gaussian_dev_u8(self.ctx._h, ip, iis, irs, W, H, B, int(radius), op, ois, ors))
        return out

    # ---- BinaryImageOps on uint8 0/1 frames [B,H,W] and int32 label images (boofcv_amd/binaryops.py has the host-view forms) ----
    def binaryLogic(self, op, a, b, out=None):
        """BinaryImageOps.logicAnd / logicOr / logicXor: op is "and", "or", "xor" or a BHIP_LOGIC_* value.  `out` may be `a` or `b`."""
        op = {"and": _lib.BHIP_LOGIC_AND, "or": _lib.BHIP_LOGIC_OR, "xor": _lib.BHIP_LOGIC_XOR}.get(op, op)
        ap, ais, ars, W, H, B = _geom(a, torch.uint8)
        bp, bis, brs, W2, H2, B2 = _geom(b, torch.uint8)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("Image shapes do not match")
        out, op_, ois, ors = self._u8_out(a, out, B, H, W)
        _check(self.ctx, self.L.bhip_binary_logic_dev_u8(self.ctx._h, int(op), ap, ais, ars, bp, bis, brs, W, H, B, op_, ois, ors))
        return out

    def binaryInvert(self, src, out=None):
        """BinaryImageOps.invert; `out` may be `src`"""
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        out, op, ois, ors = self._u8_out(src, out, B, H, W)
        _check(self.ctx, self.L.bhip_binary_invert_dev_u8(self.ctx._h, ip, iis, irs, W, H, B, op, ois, ors))
        return out

    def _morph(self, op, src, numTimes, out):
        if op == _lib.BHIP_MORPH_ERODE4 and numTimes <= 0:
            raise IllegalArgumentException("numTimes must be >= 1")
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        out, op_, ois, ors = self._u8_out(src, out, B, H, W)
        _check(self.ctx, self.L.bhip_binary_morph_dev_u8(self.ctx._h, op, int(numTimes), ip, iis, irs, W, H, B, op_, ois, ors))
        return out

    def erode(self, src, rule, numTimes=1, out=None):
        """BinaryImageOps.erode4 / erode8(input, numTimes, output): rule 4 or 8.  Input and output must not overlap."""
        return self._morph({4: _lib.BHIP_MORPH_ERODE4, 8: _lib.BHIP_MORPH_ERODE8}[int(rule)], src, numTimes, out)

    def dilate(self, src, rule, numTimes=1, out=None):
        """BinaryImageOps.dilate4 / dilate8(input, numTimes, output)"""
        return self._morph({4: _lib.BHIP_MORPH_DILATE4, 8: _lib.BHIP_MORPH_DILATE8}[int(rule)], src, numTimes, out)

    def edge(self, src, rule, outsideZero=True, out=None):
        """BinaryImageOps.edge4 / edge8(input, output, outsideZero)"""
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        out, op, ois, ors = self._u8_out(src, out, B, H, W)
        _check(self.ctx, self.L.bhip_binary_edge_dev_u8(self.ctx._h, int(rule), int(bool(outsideZero)), ip, iis, irs, W, H, B, op, ois, ors))
        return out

    def removePointNoise(self, src, out=None):
        """BinaryImageOps.removePointNoise"""
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        out, op, ois, ors = self._u8_out(src, out, B, H, W)
        _check(self.ctx, self.L.bhip_binary_remove_point_noise_dev_u8(self.ctx._h, ip, iis, irs, W, H, B, op, ois, ors))
        return out

    def labelBlobs(self, src, rule, out=None, numBlobs=None):
        """The labelled image and the blob count of BinaryImageOps.contour(input, rule, output) on uint8 frames [B,H,W] -> (labels int32 [B,H,W],
        numBlobs int32 [B]), both on the device: 0 for background, blobs numbered 1..N per image in the raster order of their first pixel.
        `out` (int32, any stride) is written in place.  The contour point lists are not produced.  No host synchronisation."""
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.int32, device=src.device)
        op, ois, ors, W2, H2, B2 = _geom(out, torch.int32)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("input and output shapes differ")
        if numBlobs is None:
            numBlobs = torch.empty((B,), dtype=torch.int32, device=src.device)
        if numBlobs.dtype != torch.int32 or numBlobs.shape != (B,) or not numBlobs.is_contiguous() or not numBlobs.is_cuda:
            raise IllegalArgumentException("numBlobs must be a contiguous int32 CUDA tensor [B]")
        _check(self.ctx, self.L.bhip_label_blobs_dev_u8_s32(self.ctx._h, int(rule), ip, iis, irs, W, H, B, op, ois, ors, C.c_void_p(numBlobs.data_ptr())))
        return out, numBlobs

    def relabel(self, labels, table):
        """BinaryImageOps.relabel in place on int32 label images [B,H,W]; table: int32 CUDA tensor [numLabels].  A pixel outside the table stays."""
        ip, iis, irs, W, H, B = _geom(labels, torch.int32)
        if table.dtype != torch.int32 or table.dim() != 1 or not table.is_contiguous() or not table.is_cuda:
            raise IllegalArgumentException("the table must be a contiguous 1-D int32 CUDA tensor")
        _check(self.ctx, self.L.bhip_relabel_dev_s32(self.ctx._h, ip, iis, irs, W, H, B, C.c_void_p(table.data_ptr()), table.numel()))
        return labels

    def labelToBinary(self, labels, selected=None, out=None):
        """BinaryImageOps.labelToBinary(labelImage, binaryImage[, selectedBlobs]); selected: uint8 / bool CUDA tensor [numLabels] or None"""
        ip, iis, irs, W, H, B = _geom(labels, torch.int32)
        out, op, ois, ors = self._u8_out(labels, out, B, H, W)
        sp, n = None, 0
        if selected is not None:
            if selected.dtype == torch.bool:
                selected = selected.to(torch.uint8)
            if selected.dtype != torch.uint8 or selected.dim() != 1 or not selected.is_contiguous() or not selected.is_cuda:
                raise IllegalArgumentException("selected must be a contiguous 1-D uint8 or bool CUDA tensor")
            sp, n = C.c_void_p(selected.data_ptr()), selected.numel()
        _check(self.ctx, self.L.bhip_label_to_binary_dev_s32_u8(self.ctx._h, ip, iis, irs, W, H, B, op, ois, ors, sp, n))
        return out

    # ---- EnhanceImageOps on uint8 (sharpen: also float32) frames [B,H,W] (boofcv_amd/enhance.py has the host-view forms) ----
    def _table(self, t, B, what, length=None):
        """a contiguous int32 CUDA tensor [length] (shared by the batch) or [B, length] -> (pointer, ints between two images' tables, length)"""
        if t.dtype != torch.int32 or t.dim() not in (1, 2) or not t.is_contiguous() or not t.is_cuda or not 1 <= t.shape[-1] <= 256:
            raise IllegalArgumentException("%s must be a contiguous int32 CUDA tensor [length] or [B, length] with 1 <= length <= 256" % what)
        if t.dim() == 2 and t.shape[0] != B:
            raise IllegalArgumentException("%s holds %d tables for %d images" % (what, t.shape[0], B))
        if length is not None and t.shape[-1] != length:
            raise IllegalArgumentException("%s must have %d entries" % (what, length))
        return C.c_void_p(t.data_ptr()), (t.shape[-1] if t.dim() == 2 else 0), t.shape[-1]

    def histogram(self, src, minValue=0, length=256, out=None):
        """ImageStatistics.histogram(GrayU8, minValue, int[length]) on uint8 frames [B,H,W] of any row / image stride -> int32 [B, length] on
        the device (`out`, contiguous, is cleared and filled in place).  A pixel outside [minValue, minValue + length) is dropped where the
        reference throws.  No host synchronisation."""
        if not 1 <= length <= 256 or not 0 <= minValue <= 255:
            raise IllegalArgumentException("histogram: length must be in 1 .. 256 and minValue in 0 .. 255")
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        if out is None:
            out = torch.empty((B, length), dtype=torch.int32, device=src.device)
        if out.dim() != 2:
            raise IllegalArgumentException("the histograms must be an int32 CUDA tensor [B, length]")
        hp, _, _ = self._table(out, B, "the histograms", length)
        _check(self.ctx, self.L.bhip_histogram_dev_u8(self.ctx._h, ip, iis, irs, W, H, B, int(minValue), int(length), hp))
        return out

    def equalizeTable(self, histograms, out=None):
        """EnhanceImageOps.equalize on int32 histograms [B, length] (or [length]) on the device -> the transform tables of the same shape (`out`
        may be `histograms`).  A histogram that sums to 0 gives zeros where the reference throws.  No host synchronisation."""
        B = histograms.shape[0] if histograms.dim() == 2 else 1
        hp, _, length = self._table(histograms, B, "the histograms")
        if out is None:
            out = torch.empty_like(histograms)
        if out.shape != histograms.shape:
            raise IllegalArgumentException("histograms and tables differ in shape")
        tp, _, _ = self._table(out, B, "the tables", length)
        _check(self.ctx, self.L.bhip_equalize_table_dev(self.ctx._h, hp, length, B, tp))
        return out

    def applyTransform(self, src, table, out=None):
        """EnhanceImageOps.applyTransform on uint8 frames [B,H,W] of any row / image stride: out = (byte)table[src].  table: int32 on the
        device, [B, length] (one table per image, as equalizeTable gives) or [length] (shared by the batch).  `out` (any stride) is written
        in place and as a whole and may be `src`; a pixel beyond the table gives 0 where the reference throws.  No host synchronisation."""
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        tp, ts, length = self._table(table, B, "the table")
        out, op, ois, ors = self._u8_out(src, out, B, H, W)
        _check(self.ctx, self.L.bhip_apply_transform_dev_u8(self.ctx._h, ip, iis, irs, W, H, B, tp, ts, length, op, ois, ors))
        return out

    def equalizeLocal(self, src, radius, histogramLength=256, out=None, path="auto"):
        """EnhanceImageOps.equalizeLocal(input, radius, output, histogramLength, null) on uint8 frames [B,H,W] of any row / image stride -> the
        uint8 images [B,H,W] (`out`, any stride, is written in place and as a whole; it must not overlap `src`).  0 <= radius <= 255,
        1 <= histogramLength <= 256; a pixel >= histogramLength is ranked like any other where the reference throws.  path: "auto", or
        "direct" / "sliding" to force one of the two kernels (the same image either way; "direct" is refused when its tile does not fit
        LDS).  No host synchronisation."""
        from . import enhance
        enhance.check_equalize_local(radius, histogramLength)
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        out, op, ois, ors = self._u8_out(src, out, B, H, W)
        _check(self.ctx, self.L.bhip_equalize_local_dev_u8(self.ctx._h, ip, iis, irs, W, H, B, int(radius), int(histogramLength), enhance.path_value(path), op, ois, ors))
        return out

    def sharpen(self, src, rule, out=None):
        """EnhanceImageOps.sharpen4 / sharpen8(input, output): rule 4 or 8, on uint8 or float32 frames [B,H,W] of any row / image stride -> images
        of the same type (`out`, any stride, is written in place and as a whole; it must not overlap `src`).  No host synchronisation."""
        if int(rule) not in (4, 8):
            raise IllegalArgumentException("sharpen: rule must be 4 or 8")
        dt = src.dtype
        if dt not in (torch.uint8, torch.float32):
            raise IllegalArgumentException("sharpen: expected uint8 or float32 frames")
        ip, iis, irs, W, H, B = _geom(src, dt)
        if out is None:
            out = torch.empty((B, H, W), dtype=dt, device=src.device)
        op, ois, ors, W2, H2, B2 = _geom(out, dt)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("input and output shapes differ")
        fn = self.L.bhip_sharpen_dev_u8 if dt == torch.uint8 else self.L.bhip_sharpen_dev_f32
        _check(self.ctx, fn(self.ctx._h, int(rule), ip, iis, irs, W, H, B, op, ois, ors))
        return out

    def _grad(self, fn, src, border, dx, dy):
        """border: None = frame untouched (as the reference with a null border), 0 = ImageBorderValue(0), "EXTENDED" = BorderType.EXTENDED (Sobel
        only).  float32 -> float32, uint8 -> int16."""
        fn_f32, fn_u8 = fn
        u8 = src.dtype == torch.uint8
        fn, dt = (fn_u8, torch.int16) if u8 else (fn_f32, torch.float32)
        if dx is None:
            # with a border policy every pixel is written; without one the frame keeps what the caller put there (zeros here, filled on
            # torch's stream: make sure that fill is ordered before the kernel when the ctx runs on another stream)
            if border is None:
                dx, dy = torch.zeros(src.shape, dtype=dt, device=src.device), torch.zeros(src.shape, dtype=dt, device=src.device)
                torch.cuda.current_stream(src.device).synchronize()
            else:
                dx, dy = torch.empty(src.shape, dtype=dt, device=src.device), torch.empty(src.shape, dtype=dt, device=src.device)
        ip, iis, irs, W, H, B = _geom(src, src.dtype if u8 else torch.float32)
        xp, ois, ors, _, _, _ = _geom(dx, dt)
        yp, ois2, ors2, _, _, _ = _geom(dy, dt)
        if (ois, ors) != (ois2, ors2):
            raise IllegalArgumentException("derivX and derivY must share their layout")
        _check(self.ctx, fn(self.ctx._h, ip, iis, irs, W, H, B, xp, yp, ois, ors, 0 if border is None else 2 if border == "EXTENDED" else 1))
        return dx, dy

    def sobel(self, src, border=0, dx=None, dy=None):
        """float32 -> float32 (GradientSobel.process(GrayF32, ...)) or uint8 -> int16 (GradientSobel.process(GrayU8, GrayS16, GrayS16, ...))"""
        return self._grad((self.L.bhip_sobel_dev_f32, self.L.bhip_sobel_dev_u8_s16), src, border, dx, dy)

    def three(self, src, border=0, dx=None, dy=None):
        return self._grad((self.L.bhip_three_dev_f32, self.L.bhip_three_dev_u8_s16), src, border, dx, dy)

    def prewitt(self, src, border="EXTENDED", dx=None, dy=None):
        """GradientPrewitt.process: float32 -> float32 or uint8 -> int16; border as _grad describes (FactoryDerivative.prewitt's default is
        EXTENDED)"""
        return self._grad((self.L.bhip_prewitt_dev_f32, self.L.bhip_prewitt_dev_u8_s16), src, border, dx, dy)

    def intensity(self, kind, dx, dy, out=None):
        """float32 derivatives: intensityE / intensityAbs / the squared magnitude (INTENSITY_*); int16 derivatives: intensityAbs only"""
        s16 = dx.dtype == torch.int16
        out = self._like(dx) if out is None else out
        xp, dis, drs, W, H, B = _geom(dx, dx.dtype if s16 else torch.float32)
        yp, dis2, drs2, W2, H2, B2 = _geom(dy, dx.dtype if s16 else torch.float32)
        if (dis, drs) != (dis2, drs2):
            raise IllegalArgumentException("derivX and derivY must share their layout")
        op, ois, ors, W3, H3, B3 = _geom(out)
        if (W, H, B) != (W2, H2, B2) or (W, H, B) != (W3, H3, B3):
            raise IllegalArgumentException("Image shapes do not match")
        if s16:
            if int(kind) != INTENSITY_ABS:
                raise IllegalArgumentException("only intensityAbs is implemented for GrayS16 derivatives on the GPU")
            _check(self.ctx, self.L.bhip_gradient_intensity_abs_dev_s16(self.ctx._h, xp, yp, dis, drs, W, H, B, op, ois, ors))
        else:
            _check(self.ctx, self.L.bhip_gradient_intensity_dev_f32(self.ctx._h, int(kind), xp, yp, dis, drs, W, H, B, op, ois, ors))
        return out

    def _derivs(self, dx, dy):
        """(ptrX, ptrY, imageStride, rowStride, W, H, B, int16?) of a derivative pair (float32 or int16) that shares one layout"""
        if dx.dtype not in (torch.float32, torch.int16) or dy.dtype != dx.dtype:
            raise IllegalArgumentException("derivatives are float32 (GrayF32) or int16 (GrayS16) and of one type; GrayS32 is not implemented on the GPU")
        xp, dis, drs, W, H, B = _geom(dx, dx.dtype)
        yp, dis2, drs2, W2, H2, B2 = _geom(dy, dx.dtype)
        if (dis, drs) != (dis2, drs2):
            raise IllegalArgumentException("derivX and derivY must share their layout")
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("Image shapes do not match")
        return xp, yp, dis, drs, W, H, B, dx.dtype == torch.int16

    def edgeNonMaxCrude4(self, intensity, dx, dy, out=None):
        """GradientToEdgeFeatures.nonMaxSuppressionCrude4(intensity, derivX, derivY, output) on float32 or int16 derivatives -> float32 [B,H,W];
        intensity and out must not overlap"""
        xp, yp, dis, drs, W, H, B, s16 = self._derivs(dx, dy)
        ip, iis, irs, W2, H2, B2 = _geom(intensity)
        out = self._like(intensity) if out is None else out
        op, ois, ors, W3, H3, B3 = _geom(out)
        if (W, H, B) != (W2, H2, B2) or (W, H, B) != (W3, H3, B3):
            raise IllegalArgumentException("Image shapes do not match")
        fn = self.L.bhip_edge_nonmax_crude4_dev_s16 if s16 else self.L.bhip_edge_nonmax_crude4_dev_f32
        _check(self.ctx, fn(self.ctx._h, ip, iis, irs, xp, yp, dis, drs, W, H, B, op, ois, ors))
        return out

    def houghPolarBins(self, width, height, rangeResolution):
        """HoughParametersPolar.initialize -> (numBinsRange, r_max)"""
        n, r = C.c_int(), C.c_float()
        if self.L.bhip_hough_polar_bins(int(width), int(height), float(rangeResolution), C.byref(n), C.byref(r)) != 0:
            raise IllegalArgumentException("bad image size")
        return n.value, r.value

    def houghBinaryPolar(self, binary, rangeResolution=2.0, numBinsAngle=180, cosTable=None, sinTable=None, out=None):
        """HoughTransformBinary.computeParameters with HoughParametersPolar(rangeResolution, numBinsAngle) on uint8 frames [B,H,W] -> the
        transform float32 [B, numBinsAngle, numBinsRange] (`out`, any row / image stride, is written as a whole).  cosTable / sinTable: the
        numBinsAngle float32 values of the trigonometric table (default: lines.CachedSineCosine_F32(0, (float)Math.PI, numBinsAngle))."""
        bp, bis, brs, W, H, B = _geom(binary, torch.uint8)
        if cosTable is None or sinTable is None:
            from . import lines
            table = lines.CachedSineCosine_F32(0.0, np.float32(np.pi), int(numBinsAngle))
            cosTable, sinTable = table.c, table.s
        c, s = np.ascontiguousarray(cosTable, np.float32), np.ascontiguousarray(sinTable, np.float32)
        if len(c) != numBinsAngle or len(s) != numBinsAngle:
            raise IllegalArgumentException("the tables have numBinsAngle entries")
        R, _ = self.houghPolarBins(W, H, rangeResolution)
        if out is None:
            if R <= 0 or numBinsAngle <= 0:
                raise IllegalArgumentException("the transform has no bins")
            if R * numBinsAngle > 1 << 28:
                raise RuntimeError("transform too large for the GPU path")
            out = torch.empty((B, int(numBinsAngle), R), dtype=torch.float32, device=binary.device)
        tp, tis, trs, TW, TH, TB = _geom(out)
        if TB != B:
            raise IllegalArgumentException("one transform per image")
        _check(self.ctx, self.L.bhip_hough_binary_polar_dev_u8(self.ctx._h, bp, bis, brs, W, H, B, float(rangeResolution), int(numBinsAngle),
                                                             c.ctypes.data_as(_lib._fp), s.ctypes.data_as(_lib._fp), tp, tis, trs, TW, TH))
        return out

    def houghGradientFoot(self, dx, dy, binary, out=None, cap=None, counts=None):
        """HoughTransformGradient.transform(derivX, derivY, binary) with HoughParametersFootOfNorm up to the transform image, on float32 or int16
        derivatives and uint8 frames [B,H,W] -> (transform float32 [B,H,W], edge pixel counts int32 [B]).  cap: the edge pixels per image that
        vote (default: all; a smaller cap bounds the scratch -- compare counts with it)."""
        xp, yp, dis, drs, W, H, B, s16 = self._derivs(dx, dy)
        bp, bis, brs, W2, H2, B2 = _geom(binary, torch.uint8)
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.float32, device=binary.device)
        tp, tis, trs, W3, H3, B3 = _geom(out)
        if (W, H, B) != (W2, H2, B2) or (W, H, B) != (W3, H3, B3):
            raise IllegalArgumentException("Image shapes do not match")
        if counts is None:
            counts = torch.empty((B,), dtype=torch.int32, device=binary.device)
        if counts.dtype != torch.int32 or counts.shape != (B,) or not counts.is_contiguous() or not counts.is_cuda:
            raise IllegalArgumentException("counts must be a contiguous int32 CUDA tensor [B]")
        fn = self.L.bhip_hough_gradient_foot_dev_s16 if s16 else self.L.bhip_hough_gradient_foot_dev_f32
        _check(self.ctx, fn(self.ctx._h, xp, yp, dis, drs, bp, bis, brs, W, H, B, tp, tis, trs, W * H if cap is None else int(cap), C.c_void_p(counts.data_ptr())))
        return out, counts

    def nonmaxRelaxed(self, intensity, radius, threshold, border=0, cap=None):
        """NonMaxBlock.process with NonMaxBlockSearchRelaxed.Max -> (xy int16 [B, cap, 2], counts int32 [B]) on the device, in block-raster order
        and raster order within a block; a count may exceed cap (default: every pixel inside the border)"""
        ip, iis, irs, W, H, B = _geom(intensity)
        if cap is None:
            cap = max(1, max(W - 2 * border, 0) * max(H - 2 * border, 0))
        xy = torch.empty((B, max(cap, 1), 2), dtype=torch.int16, device=intensity.device)
        n = torch.empty((B,), dtype=torch.int32, device=intensity.device)
        _check(self.ctx, self.L.bhip_nonmax_block_relaxed_dev_f32(self.ctx._h, ip, iis, irs, W, H, B, int(radius), float(threshold), int(border),
                                                                C.c_void_p(xy.data_ptr()), int(cap), C.c_void_p(n.data_ptr())))
        return xy[:, :cap], n

    def meanShiftPeak(self, image, xy, counts=None, radius=3, weights=None, maxIterations=10, convergenceTol=0.001):
        """MeanShiftPeak.search from the integer peaks xy int16 [B, cap, 2] (the first min(counts[b], cap) of image b; counts None: all) on float32
        images [B,H,W] -> (peaks float32 [B, cap, 2], intensity float32 [B, cap]: the image at the integer peak).  weights: the (2*radius+1)^2
        kernel of a WeightPixel_F32 (default: lines.weightPixelGaussian(radius)); radius <= 0: no refinement.  Rows past counts[b] are not written."""
        ip, iis, irs, W, H, B = _geom(image)
        if xy.dtype != torch.int16 or xy.dim() != 3 or xy.shape[0] != B or xy.shape[2] != 2 or not xy.is_contiguous() or not xy.is_cuda:
            raise IllegalArgumentException("xy must be a contiguous int16 CUDA tensor [B, cap, 2]")
        cap = xy.shape[1]
        if counts is not None and (counts.dtype != torch.int32 or counts.shape != (B,) or not counts.is_contiguous() or not counts.is_cuda):
            raise IllegalArgumentException("counts must be a contiguous int32 CUDA tensor [B]")
        wp = None
        if radius > 0:
            if weights is None:
                from . import lines
                weights = lines.weightPixelGaussian(int(radius))
            w = np.ascontiguousarray(weights, np.float32).reshape(-1)
            if w.size != (2 * radius + 1) ** 2:
                raise IllegalArgumentException("the weight table has (2*radius+1)^2 entries")
            wp = w.ctypes.data_as(_lib._fp)
        peak = torch.empty((B, cap, 2), dtype=torch.float32, device=image.device)
        inten = torch.empty((B, cap), dtype=torch.float32, device=image.device)
        _check(self.ctx, self.L.bhip_mean_shift_peak_dev_f32(self.ctx._h, ip, iis, irs, W, H, B, C.c_void_p(xy.data_ptr()),
                                                           C.c_void_p(counts.data_ptr()) if counts is not None else None, cap, int(radius),
                                                           int(maxIterations), float(convergenceTol), wp, C.c_void_p(peak.data_ptr()),
                                                           C.c_void_p(inten.data_ptr())))
        return peak, inten

    def nonmax(self, intensity, radius, threshold, border, cap=None):
        """-> (xy int16 [B, cap, 2], counts int32 [B]) on the device; lists are in the reference's block-raster order"""
        ip, iis, irs, W, H, B = _geom(intensity)
        if cap is None:
            step = radius + 1
            cap = max(1, ((max(W - 2 * border, 0) + step - 1) // step) * ((max(H - 2 * border, 0) + step - 1) // step))
        xy = torch.empty((B, cap, 2), dtype=torch.int16, device=intensity.device)
        n = torch.empty((B,), dtype=torch.int32, device=intensity.device)
        _check(self.ctx, self.L.bhip_nonmax_block_dev_f32(self.ctx._h, ip, iis, irs, W, H, B, int(radius), float(threshold), int(border),
                                                        C.c_void_p(xy.data_ptr()), cap, C.c_void_p(n.data_ptr())))
        return xy, n

    def nonmaxMinMax(self, intensity, radius, thresholdMin, thresholdMax, border, detectMin=True, detectMax=True, cap=None):
        """NonMaxBlockSearchStrict.Min / .Max / .MinMax -> (xyMin int16 [B, cap, 2], nMin int32 [B], xyMax, nMax) on the device, each list in
        block-raster order; a side that is not detected has counts of 0"""
        ip, iis, irs, W, H, B = _geom(intensity)
        if cap is None:
            step = radius + 1
            cap = max(1, ((max(W - 2 * border, 0) + step - 1) // step) * ((max(H - 2 * border, 0) + step - 1) // step))
        xyMin, xyMax = (torch.empty((B, cap, 2), dtype=torch.int16, device=intensity.device) for _ in range(2))
        nMin, nMax = (torch.empty((B,), dtype=torch.int32, device=intensity.device) for _ in range(2))
        _check(self.ctx, self.L.bhip_nonmax_block_minmax_dev_f32(self.ctx._h, ip, iis, irs, W, H, B, int(radius), float(thresholdMin), float(thresholdMax),
                                                               int(border), 1 if detectMin else 0, 1 if detectMax else 0, C.c_void_p(xyMin.data_ptr()),
                                                               C.c_void_p(nMin.data_ptr()), C.c_void_p(xyMax.data_ptr()), C.c_void_p(nMax.data_ptr()), cap))
        return xyMin, nMin, xyMax, nMax

    def fast(self, src, pixelTol, minContinuous, maxFeaturesFraction=0.1, intensity=True, cap=None):
        """FastCornerDetector.process on uint8 or float32 frames -> (intensity float32 [B, H, W] | None, xyLow int16 [B, cap, 2], nLow int32 [B],
        xyHigh, nHigh): dark and bright corners in raster order.  intensity: True allocates it, False / None is process(image), a float32
        tensor (any row stride) is written in place.  A count may exceed cap; only the first cap pairs are written."""
        u8 = src.dtype == torch.uint8
        ip, iis, irs, W, H, B = _geom(src, torch.uint8 if u8 else torch.float32)
        inten = None
        if intensity is True:
            inten = torch.empty((B, H, W), dtype=torch.float32, device=src.device)
        elif intensity is not None and intensity is not False:
            inten = intensity
        op, ois, ors = None, 0, 0
        if inten is not None:
            op, ois, ors, W2, H2, B2 = _geom(inten)
            if (W, H, B) != (W2, H2, B2):
                raise IllegalArgumentException("input and intensity shapes differ")
        if cap is None:
            # the detector stops after the row that reaches the limit, so a list is never longer than the limit plus that row
            cap = max(1, min(max(W - 6, 0) * max(H - 6, 0), int(maxFeaturesFraction * W * H) + W))
        xyLow, xyHigh = (torch.empty((B, cap, 2), dtype=torch.int16, device=src.device) for _ in range(2))
        nLow, nHigh = (torch.empty((B,), dtype=torch.int32, device=src.device) for _ in range(2))
        fn = self.L.bhip_fast_dev_u8 if u8 else self.L.bhip_fast_dev_f32
        _check(self.ctx, fn(self.ctx._h, ip, iis, irs, W, H, B, int(pixelTol) if u8 else float(pixelTol), int(minContinuous), float(maxFeaturesFraction), op, ois,
                            ors, C.c_void_p(xyLow.data_ptr()), C.c_void_p(nLow.data_ptr()), C.c_void_p(xyHigh.data_ptr()), C.c_void_p(nHigh.data_ptr()),
                            cap))
        return inten, xyLow, nLow, xyHigh, nHigh

    def disparityBM(self, left, right, config=None, subpixel=True, out=None):
        """StereoDisparity.process of FactoryStereoDisparity.blockMatch (SAD) on uint8 pairs [B,H,W] -> the disparity [B,H,W]: float32 when subpixel,
        uint8 otherwise (config.subpixel is not read; `out`, any row / image stride, is written in place and as a whole).  config: a
        ConfigDisparityBM, None = the reference defaults."""
        lp, lis, lrs, W, H, B = _geom(left, torch.uint8)
        rp, ris, rrs, W2, H2, B2 = _geom(right, torch.uint8)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("Image shapes do not match")
        dt = torch.float32 if subpixel else torch.uint8
        if out is None:
            out = torch.empty((B, H, W), dtype=dt, device=left.device)
        op, ois, ors, W3, H3, B3 = _geom(out, dt)
        if (W, H, B) != (W3, H3, B3):
            raise IllegalArgumentException("input and disparity shapes differ")
        fn = self.L.bhip_disparity_bm_dev_u8_f32 if subpixel else self.L.bhip_disparity_bm_dev_u8_u8
        _check(self.ctx, fn(self.ctx._h, C.byref(config._c()) if config is not None else None, lp, lis, lrs, rp, ris, rrs, W, H, B, op, ois, ors))
        return out

    def census(self, src, variant, out=None):
        """FilterImageInterface.process of FactoryCensusTransform.variant(variant, GrayU8) on uint8 frames [B,H,W] of any row / image stride ->
        the census words [B,H,W]: uint8 (BLOCK_3_3), int32 (BLOCK_5_5) or int64 (the other variants).  variant: a census.CensusVariants, or a
        sample list [(x, y)] (at most 64, offsets within -7 .. 7) for sample_S64 -> int64.  `out`, any stride, is written in place and as a
        whole.  No host synchronisation."""
        from . import census
        ip, iis, irs, W, H, B = _geom(src, torch.uint8)
        samples = None
        if isinstance(variant, (list, tuple, np.ndarray)):
            samples = [tuple(p) for p in variant]
        else:
            try:
                variant = census.CensusVariants(variant)
            except ValueError:
                raise IllegalArgumentException("Unknown type %s" % (variant,))
            if variant not in (census.CensusVariants.BLOCK_3_3, census.CensusVariants.BLOCK_5_5):
                samples = census._variant_samples(variant)
        dt = torch.int64 if samples is not None else torch.uint8 if variant == census.CensusVariants.BLOCK_3_3 else torch.int32
        if out is None:
            out = torch.empty((B, H, W), dtype=dt, device=src.device)
        op, ois, ors, W2, H2, B2 = _geom(out, dt)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("input and output shapes differ")
        if samples is not None:
            xy, p, n = census._samples_arg(samples)
            _check(self.ctx, self.L.bhip_census_sample_dev_u8_s64(self.ctx._h, p, n, ip, iis, irs, W, H, B, op, ois, ors))
        else:
            fn = self.L.bhip_census_dev_u8_u8 if dt == torch.uint8 else self.L.bhip_census_dev_u8_s32
            _check(self.ctx, fn(self.ctx._h, ip, iis, irs, W, H, B, op, ois, ors))
        return out

    def disparityBMCensus(self, left, right, config=None, variant=_lib.BHIP_CENSUS_BLOCK_5_5, subpixel=True, out=None):
        """StereoDisparity.process of FactoryStereoDisparity.blockMatch with errorType = CENSUS and configCensus.variant = variant on uint8 pairs
        [B,H,W] -> the disparity [B,H,W]: float32 when subpixel, uint8 otherwise (config.subpixel and config.errorType are not read; `out`, any
        row / image stride, is written in place and as a whole).  config: a ConfigDisparityBM, None = the reference defaults."""
        lp, lis, lrs, W, H, B = _geom(left, torch.uint8)
        rp, ris, rrs, W2, H2, B2 = _geom(right, torch.uint8)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("Image shapes do not match")
        dt = torch.float32 if subpixel else torch.uint8
        if out is None:
            out = torch.empty((B, H, W), dtype=dt, device=left.device)
        op, ois, ors, W3, H3, B3 = _geom(out, dt)
        if (W, H, B) != (W3, H3, B3):
            raise IllegalArgumentException("input and disparity shapes differ")
        fn = self.L.bhip_disparity_bm_census_dev_u8_f32 if subpixel else self.L.bhip_disparity_bm_census_dev_u8_u8
        _check(self.ctx, fn(self.ctx._h, C.byref(config._c()) if config is not None else None, int(variant), lp, lis, lrs, rp, ris, rrs, W, H, B, op, ois, ors))
        return out

    def disparityBM5(self, left, right, config=None, variant=None, subpixel=True, out=None):
        """StereoDisparity.process of FactoryStereoDisparity.blockMatchBest5 on uint8 pairs [B,H,W] -> the disparity [B,H,W]: float32 when subpixel,
        uint8 otherwise.  variant None: errorType = SAD; a census.CensusVariants: errorType = CENSUS with that variant (config.subpixel and
        config.errorType are not read; `out`, any row / image stride, is written in place and as a whole).  config: a ConfigDisparityBMBest5 or
        ConfigDisparityBM, None = the reference defaults."""
        lp, lis, lrs, W, H, B = _geom(left, torch.uint8)
        rp, ris, rrs, W2, H2, B2 = _geom(right, torch.uint8)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("Image shapes do not match")
        dt = torch.float32 if subpixel else torch.uint8
        if out is None:
            out = torch.empty((B, H, W), dtype=dt, device=left.device)
        op, ois, ors, W3, H3, B3 = _geom(out, dt)
        if (W, H, B) != (W3, H3, B3):
            raise IllegalArgumentException("input and disparity shapes differ")
        cfg = C.byref(config._c()) if config is not None else None
        if variant is None:
            fn = self.L.bhip_disparity_bm5_dev_u8_f32 if subpixel else self.L.bhip_disparity_bm5_dev_u8_u8
            _check(self.ctx, fn(self.ctx._h, cfg, lp, lis, lrs, rp, ris, rrs, W, H, B, op, ois, ors))
        else:
            fn = self.L.bhip_disparity_bm5_census_dev_u8_f32 if subpixel else self.L.bhip_disparity_bm5_census_dev_u8_u8
            _check(self.ctx, fn(self.ctx._h, cfg, int(variant), lp, lis, lrs, rp, ris, rrs, W, H, B, op, ois, ors))
        return out

    def denseFlowKlt(self, prev, curr, config=None, radius=3, out=None, tracks=None, form=_lib.BHIP_FLOW_FORM_AUTO):
        """DenseOpticalFlow.process of FactoryDenseOpticalFlow.flowKlt on float32 or uint8 pairs [B,H,W] -> the flow [B,H,W,2] float32, invalid
        pixels (NaN, 0).  config: a PkltConfig (its KltConfig and pyramidScaling; templateRadius is not read), None = the reference defaults.
        `out`: any image / row stride with (x, y) adjacent, written in place.  tracks: None, True (allocated) or a contiguous int32 [B,H,W,4]
        tensor that receives every pixel's own track {fault, error, dx, dy} (the three floats as their bit patterns); returned second when given.
        form: BHIP_FLOW_FORM_AUTO / _LANE / _WAVE selects the track kernel (same results)."""
        config = config or PkltConfig()
        u8 = prev.dtype == torch.uint8
        dt = torch.uint8 if u8 else torch.float32
        pp, pis, prs, W, H, B = _geom(prev, dt)
        cp, cis, crs, W2, H2, B2 = _geom(curr, dt)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("Image shapes do not match")
        if out is None:
            out = torch.empty((B, H, W, 2), dtype=torch.float32, device=prev.device)
        if out.dim() != 4 or out.dtype != torch.float32 or not out.is_cuda or tuple(out.shape) != (B, H, W, 2):
            raise IllegalArgumentException("the flow must be a [%d,%d,%d,2] float32 CUDA tensor" % (B, H, W))
        if out.stride(3) != 1 or out.stride(2) != 2 or (H > 1 and out.stride(1) < 2 * W) or (B > 1 and out.stride(0) < 0):
            raise IllegalArgumentException("the flow's (x, y) pairs and pixels of a row must be adjacent")
        ois = out.stride(0) if B > 1 else H * out.stride(1)
        ors = out.stride(1) if H > 1 else max(2 * W, out.stride(1))
        if tracks is True:
            tracks = torch.empty((B, H, W, 4), dtype=torch.int32, device=prev.device)
        if tracks is not None and (tracks.dtype != torch.int32 or tuple(tracks.shape) != (B, H, W, 4) or not tracks.is_contiguous() or not tracks.is_cuda):
            raise IllegalArgumentException("tracks must be a contiguous [%d,%d,%d,4] int32 CUDA tensor" % (B, H, W))
        scales = (C.c_int * len(config.pyramidScaling))(*config.pyramidScaling)
        fn = self.L.bhip_flow_klt_dev_u8 if u8 else self.L.bhip_flow_klt_dev_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(config.config._c()), int(radius), scales, len(scales), pp, pis, prs, cp, cis, crs, W, H, B,
                            C.c_void_p(out.data_ptr()), ois, ors, C.c_void_p(tracks.data_ptr()) if tracks is not None else None, int(form)))
        return out if tracks is None else (out, tracks)

    def denseFlowStats(self):
        """(pixels, Lucas-Kanade iterations) of the last denseFlowKlt on this context (synchronises)"""
        n, it = C.c_longlong(), C.c_longlong()
        _check(self.ctx, self.L.bhip_flow_klt_stats(self.ctx._h, C.byref(n), C.byref(it)))
        return n.value, it.value

    def denseFlowHornSchunck(self, prev, curr, alpha=20.0, numIterations=1000, out=None, derivs=None, itersPerLaunch=0):
        """DenseOpticalFlow.process of FactoryDenseOpticalFlow.hornSchunck on float32 or uint8 pairs [B,H,W] -> the flow [B,H,W,2] float32.
        `out`: any image / row stride with (x, y) adjacent, written in place.  derivs: None, True (allocated) or a contiguous float32 [B,3,H,W]
        tensor that receives derivX, derivY, derivT (the GrayS16 values of uint8 pairs as floats); returned second when given.  itersPerLaunch:
        0 = the library's choice, 1 .. BHIP_FLOW_HS_MAX_FUSED forces how many iterations one launch fuses (same results)."""
        u8 = prev.dtype == torch.uint8
        dt = torch.uint8 if u8 else torch.float32
        pp, pis, prs, W, H, B = _geom(prev, dt)
        cp, cis, crs, W2, H2, B2 = _geom(curr, dt)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("Image shapes do not match")
        if out is None:
            out = torch.empty((B, H, W, 2), dtype=torch.float32, device=prev.device)
        if out.dim() != 4 or out.dtype != torch.float32 or not out.is_cuda or tuple(out.shape) != (B, H, W, 2):
            raise IllegalArgumentException("the flow must be a [%d,%d,%d,2] float32 CUDA tensor" % (B, H, W))
        if out.stride(3) != 1 or out.stride(2) != 2 or (H > 1 and out.stride(1) < 2 * W) or (B > 1 and out.stride(0) < 0):
            raise IllegalArgumentException("the flow's (x, y) pairs and pixels of a row must be adjacent")
        ois = out.stride(0) if B > 1 else H * out.stride(1)
        ors = out.stride(1) if H > 1 else max(2 * W, out.stride(1))
        if derivs is True:
            derivs = torch.empty((B, 3, H, W), dtype=torch.float32, device=prev.device)
        if derivs is not None and (derivs.dtype != torch.float32 or tuple(derivs.shape) != (B, 3, H, W) or not derivs.is_contiguous() or not derivs.is_cuda):
            raise IllegalArgumentException("derivs must be a contiguous [%d,3,%d,%d] float32 CUDA tensor" % (B, H, W))
        fn = self.L.bhip_flow_hs_dev_u8 if u8 else self.L.bhip_flow_hs_dev_f32
        _check(self.ctx, fn(self.ctx._h, float(alpha), int(numIterations), pp, pis, prs, cp, cis, crs, W, H, B, C.c_void_p(out.data_ptr()), ois, ors,
                            C.c_void_p(derivs.data_ptr()) if derivs is not None else None, int(itersPerLaunch)))
        return out if derivs is None else (out, derivs)

    def siftLayout(self, width, height, configSS=None):
        """bhip_sift_layout -> (dims [(w, h)] of the octaves SiftScaleSpace computes for a width x height frame, scaleFloats, dogFloats): a frame's
        scale images are numScales+3 dense images per octave of plane = (w*h + 3) & ~3 floats each, octave after octave; its DoG images
        numScales+2 per octave in the same way"""
        from . import sift
        c = sift._cfg(configSS, None)
        dims = (C.c_int * 128)()
        sf, df = C.c_longlong(0), C.c_longlong(0)
        n = self.L.bhip_sift_layout(C.byref(c), int(width), int(height), dims, 64, C.byref(sf), C.byref(df))
        if n < 0:
            raise (RuntimeError if n == _lib.BHIP_ERR_UNSUPPORTED else IllegalArgumentException)("no SIFT scale space for a %d x %d frame with this config" % (width, height))
        return [(dims[2 * i], dims[2 * i + 1]) for i in range(n)], sf.value, df.value

    def siftScaleSpace(self, src, configSS=None):
        """SiftScaleSpace.initialize and every computeNextOctave on uint8 or float32 frames [B,H,W] of any row / image stride -> (scale float32
        [B, scaleFloats], dog float32 [B, dogFloats], dims) in the layout of siftLayout (padding floats are 0).  siftImages() cuts a frame's
        buffers into its images.  No host synchronisation."""
        from . import sift
        u8 = src.dtype == torch.uint8
        ip, iis, irs, W, H, B = _geom(src, torch.uint8 if u8 else torch.float32)
        dims, sf, df = self.siftLayout(W, H, configSS)
        scale = torch.zeros((B, sf), dtype=torch.float32, device=src.device)
        dog = torch.zeros((B, df), dtype=torch.float32, device=src.device)
        fn = self.L.bhip_sift_scale_space_dev_u8 if u8 else self.L.bhip_sift_scale_space_dev_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(sift._cfg(configSS, None)), ip, iis, irs, W, H, B, C.c_void_p(scale.data_ptr()), C.c_void_p(dog.data_ptr())))
        return scale, dog, dims

    @staticmethod
    def siftImages(buf, dims, perOctave):
        """the images of one frame's buffer (a 1-D tensor or array laid out by siftLayout): [[image [h, w]] * perOctave] per octave"""
        out, off = [], 0
        for w, h in dims:
            plane = (w * h + 3) & ~3
            out.append([buf[off + i * plane:off + i * plane + w * h].reshape(h, w) for i in range(perOctave)])
            off += perOctave * plane
        return out

    def siftDetect(self, src, configSS=None, configDet=None, cap=4096):
        """SiftDetector.process on uint8 or float32 frames [B,H,W] of any row / image stride -> (x, y, scale float64 [B, cap], white uint8 [B, cap],
        where int16 [B, cap, 4] = octave, DoG index, pixel x, pixel y in that octave, count int32 [B]) on the device, every frame's detections
        in the reference's order.  A count may exceed cap; only the first cap records are written.  No host synchronisation."""
        from . import sift
        u8 = src.dtype == torch.uint8
        ip, iis, irs, W, H, B = _geom(src, torch.uint8 if u8 else torch.float32)
        cap = int(cap)
        x, y, scale = (torch.empty((B, max(cap, 0)), dtype=torch.float64, device=src.device) for _ in range(3))
        white = torch.empty((B, max(cap, 0)), dtype=torch.uint8, device=src.device)
        where = torch.empty((B, max(cap, 0), 4), dtype=torch.int16, device=src.device)
        count = torch.empty((B,), dtype=torch.int32, device=src.device)
        fn = self.L.bhip_sift_detect_dev_u8 if u8 else self.L.bhip_sift_detect_dev_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(sift._cfg(configSS, configDet)), ip, iis, irs, W, H, B, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()),
                            C.c_void_p(scale.data_ptr()), C.c_void_p(white.data_ptr()), C.c_void_p(where.data_ptr()), C.c_void_p(count.data_ptr()), cap))
        return x, y, scale, white, where, count

    def siftDetectDescribe(self, src, config=None, cap=4096):
        """CompleteSift.process (FactoryDetectDescribe.sift(config); None: new ConfigCompleteSift()) on uint8 or float32 frames [B,H,W] of any row /
        image stride -> (x, y, scale, orientation float64 [B, cap], white uint8 [B, cap], descriptors float64 [B, cap, dof], count int32 [B]) on
        the device: every frame's features in the reference's order, the descriptors in the layout associateL2 reads.  A count may exceed cap;
        only the first cap records are written.  No host synchronisation."""
        from . import sift
        if config is None:
            config = sift.ConfigCompleteSift()
        u8 = src.dtype == torch.uint8
        ip, iis, irs, W, H, B = _geom(src, torch.uint8 if u8 else torch.float32)
        cap = int(cap)
        dc = sift._desc_cfg(config.orientation, config.describe)
        dof = self.L.bhip_csift_dof(C.byref(dc))
        if dof < 0:
            raise (RuntimeError if dof == _lib.BHIP_ERR_UNSUPPORTED else IllegalArgumentException)("no SIFT descriptor for this orientation / describe config")
        x, y, scale, ori = (torch.empty((B, max(cap, 0)), dtype=torch.float64, device=src.device) for _ in range(4))
        white = torch.empty((B, max(cap, 0)), dtype=torch.uint8, device=src.device)
        desc = torch.empty((B, max(cap, 0), dof), dtype=torch.float64, device=src.device)
        count = torch.empty((B,), dtype=torch.int32, device=src.device)
        fn = self.L.bhip_csift_dev_u8 if u8 else self.L.bhip_csift_dev_f32
        _check(self.ctx, fn(self.ctx._h, C.byref(sift._cfg(config.scaleSpace, config.detector)), C.byref(dc), ip, iis, irs, W, H, B, C.c_void_p(x.data_ptr()),
                            C.c_void_p(y.data_ptr()), C.c_void_p(scale.data_ptr()), C.c_void_p(ori.data_ptr()), C.c_void_p(white.data_ptr()),
                            C.c_void_p(desc.data_ptr()), C.c_void_p(count.data_ptr()), cap))
        return x, y, scale, ori, white, desc, count

    def _dense(self, src, cap, layout, call, extra=()):
        u8 = src.dtype == torch.uint8
        ip, iis, irs, W, H, B = _geom(src, torch.uint8 if u8 else torch.float32)
        dof = C.c_int(0)
        n = layout(W, H, C.byref(dof))
        if n < 0:
            raise (RuntimeError if n == _lib.BHIP_ERR_UNSUPPORTED else IllegalArgumentException)("no dense descriptors for a %d x %d frame with this config" % (W, H))
        cap = n if cap is None else int(cap)
        desc = torch.empty((B, max(cap, 0), dof.value), dtype=torch.float64, device=src.device)
        xy = torch.empty((B, max(cap, 0), 2), dtype=torch.int32, device=src.device)
        count = torch.empty((B,), dtype=torch.int32, device=src.device)
        _check(self.ctx, call(u8)(ip, iis, irs, W, H, B, C.c_void_p(desc.data_ptr()), C.c_void_p(xy.data_ptr()), C.c_void_p(count.data_ptr()), cap, *extra))
        return desc, xy, count

    def denseHog(self, src, config=None, cap=None, cells=None):
        """DescribeDenseHogFastAlg / DescribeDenseHogAlg (FactoryDescribeImageDense.hog(config); None: new ConfigDenseHoG()) on uint8 or float32 frames
        [B,H,W] of any row / image stride -> (descriptors float64 [B, cap, dof], xy int32 [B, cap, 2]: the blocks' top-left pixels, count int32 [B]) on
        the device, in the reference's row-major order, the descriptors in the layout associateL2 reads.  cap None: room for all of them; a count
        may exceed cap, only the first cap records are written.  cells (fast variant): a contiguous float32 [B, H // pixelsPerCell,
        W // pixelsPerCell, orientationBins] CUDA tensor that receives the cell histograms.  No host synchronisation."""
        from . import dense
        config = dense.ConfigDenseHoG() if config is None else config
        a = dense._hog_args(config)
        if cells is not None:
            B, H, W = (1,) + tuple(src.shape) if src.dim() == 2 else tuple(src.shape)
            if not config.fastVariant:
                raise IllegalArgumentException("only the fast variant has cell histograms")
            if cells.dtype != torch.float32 or not cells.is_cuda or not cells.is_contiguous() or tuple(cells.shape) != (B, H // a[1], W // a[1], a[0]):
                raise IllegalArgumentException("cells is a contiguous [B, H // pixelsPerCell, W // pixelsPerCell, orientationBins] float32 CUDA tensor")
        return self._dense(src, cap, lambda W, H, dof: self.L.bhip_dense_hog_layout(*a, W, H, None, None, dof, None, 0),
                           lambda u8: (lambda *r: (self.L.bhip_dense_hog_dev_u8 if u8 else self.L.bhip_dense_hog_dev_f32)(self.ctx._h, *a, *r)),
                           (None if cells is None else C.c_void_p(cells.data_ptr()),))

    def denseSift(self, src, config=None, cap=None):
        """DescribeDenseSiftAlg behind DescribeImageDenseSift (FactoryDescribeImageDense.sift(config); None: new ConfigDenseSift()) on uint8 (GrayS16
        gradient) or float32 frames [B,H,W] of any row / image stride -> (descriptors float64 [B, cap, dof], xy int32 [B, cap, 2]: the window centres,
        count int32 [B]) on the device, as denseHog.  No host synchronisation."""
        from . import dense
        config = dense.ConfigDenseSift() if config is None else config
        g, rest = dense._sift_args(config)
        return self._dense(src, cap, lambda W, H, dof: self.L.bhip_dense_sift_layout(*g, rest[2], rest[3], W, H, None, None, dof, None, 0),
                           lambda u8: (lambda *r: (self.L.bhip_dense_sift_dev_u8 if u8 else self.L.bhip_dense_sift_dev_f32)(self.ctx._h, *g, *rest, *r)))

    def distortBuildMap(self, model, coeff, dw, dh, out=None):
        """bhip_distort_build_map: the [dh,dw,2] float32 map of an affine (model 1, six coefficients) or homography (model 2, nine) model"""
        coeff = np.ascontiguousarray(coeff, np.float32).reshape(-1)
        if out is None:
            out = torch.empty((int(dh), int(dw), 2), dtype=torch.float32, device=self.device)
        if out.dtype != torch.float32 or tuple(out.shape) != (int(dh), int(dw), 2) or not out.is_contiguous() or not out.is_cuda:
            raise IllegalArgumentException("the map is a contiguous [dh,dw,2] float32 CUDA tensor")
        if coeff.size != {1: 6, 2: 9}.get(int(model), -1):
            raise IllegalArgumentException("model 1 (affine) takes 6 coefficients, model 2 (homography) 9")
        _check(self.ctx, self.L.bhip_distort_build_map(self.ctx._h, int(model), coeff.ctypes.data_as(_lib._fp), int(dw), int(dh), C.c_void_p(out.data_ptr())))
        return out

    def distort(self, src, map=None, model=None, coeff=None, interp=_lib.BHIP_INTERP_BILINEAR, border=_lib.BHIP_BORDER_EXTENDED, renderAll=True, out=None,
                mask=None, crop=None, shape=None):
        """ImageDistort.apply on [B,H,W] uint8 / float32 frames of any row / image stride -> `out` of the same type, [B,dh,dw].  The source
        coordinates come from `map`, a contiguous [dh,dw,2] (shared by the batch) or [B,dh,dw,2] float32 tensor of (x, y) pairs, or from
        `model` (1 affine, 2 homography) with `coeff`, evaluated in the kernel; then the destination size is out's, or `shape` = (dh, dw), or the
        source's.  interp / border: the BHIP_INTERP_* / BHIP_BORDER_* codes.  renderAll = False leaves the pixels whose source lies outside the
        image as they are in `out`.  mask: a [B,dh,dw] uint8 tensor, written 1 / 0.  crop = (x0, y0, x1, y1).  src, out and mask must not overlap."""
        dt = src.dtype
        if dt not in (torch.uint8, torch.float32):
            raise RuntimeError("only uint8 and float32 frames are distorted on the GPU (use the Java path)")
        sp, sis, srs, sw, sh, B = _geom(src, dt)
        if (map is None) == (model is None):
            raise IllegalArgumentException("give a map or a model")
        if map is not None:
            if map.dtype != torch.float32 or not map.is_cuda or map.dim() not in (3, 4) or map.shape[-1] != 2 or not map.is_contiguous():
                raise IllegalArgumentException("the map is a contiguous [dh,dw,2] or [B,dh,dw,2] float32 CUDA tensor")
            if map.dim() == 4 and map.shape[0] != B:
                raise IllegalArgumentException("one map, or one per image")
            dh, dw = int(map.shape[-3]), int(map.shape[-2])
            mis = 2 * dh * dw if map.dim() == 4 else 0
        elif out is not None:
            dh, dw = int(out.shape[-2]), int(out.shape[-1])
        else:
            dh, dw = (sh, sw) if shape is None else (int(shape[0]), int(shape[1]))
        if out is None:
            if not renderAll or crop is not None:
                out = torch.zeros((B, dh, dw), dtype=dt, device=src.device)
                torch.cuda.current_stream(src.device).synchronize()   # the fill runs on torch's stream: order it before the kernel
            else:
                out = torch.empty((B, dh, dw), dtype=dt, device=src.device)
        op, ois, ors, W2, H2, B2 = _geom(out, dt)
        if (W2, H2, B2) != (dw, dh, B):
            raise IllegalArgumentException("the destination has the map's size and the source's batch")
        mp, mis2, mrs = None, 0, 0
        if mask is not None:
            mp, mis2, mrs, W3, H3, B3 = _geom(mask, torch.uint8)
            if (W3, H3, B3) != (dw, dh, B):
                raise IllegalArgumentException("the mask has the destination's shape")
        x0, y0, x1, y1 = (0, 0, dw, dh) if crop is None else (int(v) for v in crop)
        tail = (dw, dh, x0, y0, x1, y1, int(interp), int(border), 1 if renderAll else 0, op, ois, ors, mp, mis2, mrs)
        if map is not None:
            fn = self.L.bhip_distort_map_dev_u8 if dt == torch.uint8 else self.L.bhip_distort_map_dev_f32
            _check(self.ctx, fn(self.ctx._h, sp, sis, srs, sw, sh, B, C.c_void_p(map.data_ptr()), mis, *tail))
        else:
            coeff = np.ascontiguousarray(coeff, np.float32).reshape(-1)
            if coeff.size != {1: 6, 2: 9}.get(int(model), -1):
                raise IllegalArgumentException("model 1 (affine) takes 6 coefficients, model 2 (homography) 9")
            fn = self.L.bhip_distort_model_dev_u8 if dt == torch.uint8 else self.L.bhip_distort_model_dev_f32
            _check(self.ctx, fn(self.ctx._h, sp, sis, srs, sw, sh, B, int(model), coeff.ctypes.data_as(_lib._fp), *tail))
        return out

    def _template(self, t, dtype, B, what):
        """(ptr, imageStride, rowStride, w, h) of a template or mask: [h,w] is shared by the batch (image stride 0), [B,h,w] is one per image"""
        p, tis, trs, tw, th, tb = _geom(t, dtype)
        if t.dim() == 2:
            tis = 0
        elif tb != B:
            raise IllegalArgumentException("%s: one per image of the batch, or a single [h,w] one" % what)
        return p, tis, trs, tw, th

    def templateIntensity(self, images, template, mask=None, score="SUM_ABSOLUTE_DIFFERENCE", out=None):
        """TemplateMatchingIntensity.process(template[, mask]) of FactoryTemplateMatching.createIntensity(score, GrayU8 | GrayF32) on uint8 or
        float32 images [B,H,W] -> the intensity float32 [B,H,W], 0 in the border (`out`, any row / image stride, is written in place and as a
        whole).  template / mask: [th,tw] shared by the batch or [B,th,tw]; same dtype as the images.  score: a TemplateScoreType name."""
        if score not in TemplateScoreType._ORDINAL:
            raise IllegalArgumentException("Unknown")
        if images.dtype not in (torch.uint8, torch.float32):
            raise IllegalArgumentException("Image type not supported. " + str(images.dtype))
        dt = images.dtype
        ip, iis, irs, W, H, B = _geom(images, dt)
        if template.dtype != dt or (mask is not None and mask.dtype != dt):
            raise IllegalArgumentException("image, template and mask must have one type")
        tp, tis, trs, tw, th = self._template(template, dt, B, "template")
        mp, mis, mrs, mw, mh = self._template(mask, dt, B, "mask") if mask is not None else (None, 0, 0, 0, 0)
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.float32, device=images.device)
        op, ois, ors, W2, H2, B2 = _geom(out)
        if (W, H, B) != (W2, H2, B2):
            raise IllegalArgumentException("input and intensity shapes differ")
        fn = self.L.bhip_template_intensity_dev_u8 if dt == torch.uint8 else self.L.bhip_template_intensity_dev_f32
        _check(self.ctx, fn(self.ctx._h, TemplateScoreType._ORDINAL[score], ip, iis, irs, W, H, B, tp, tis, trs, tw, th, mp, mis, mrs, mw, mh, op, ois, ors))
        return out

    def templateMatch(self, images, template, mask=None, score="SUM_ABSOLUTE_DIFFERENCE", maxMatches=1, radius=2, cap=None):
        """TemplateMatching (setMinimumSeparation(radius), setTemplate(template, mask, maxMatches), setImage, process, getResults) on every image
        of a batch: templateIntensity, the strict block non-maximum suppression on the intensity sub-image (nonmaxMinMax) and the N best
        (bhip_template_select_dev_f32) -> (xy int16 [B, maxMatches, 2] top-left corners, scores float32 [B, maxMatches], counts int32 [B],
        candidates int32 [B]); rows past counts[b] are 0.  cap: candidates kept per image (default: one per suppression block, at most
        BHIP_TEMPLATE_MAX_CANDIDATES); where candidates[b] > cap the list was cut and the matches are those of the cut list."""
        maximize = score == "NCC"
        inten = self.templateIntensity(images, template, mask, score)
        th, tw = template.shape[-2:]
        B, H, W = inten.shape
        sub = inten[:, th // 2:th // 2 + H - th + 1, tw // 2:tw // 2 + W - tw + 1]
        if cap is None:
            step = radius + 1
            cap = max(1, min(((sub.shape[2] + step - 1) // step) * ((sub.shape[1] + step - 1) // step), _lib.BHIP_TEMPLATE_MAX_CANDIDATES))
        fmax = float(np.finfo(np.float32).max)
        xyMin, nMin, xyMax, nMax = self.nonmaxMinMax(sub, radius, fmax, -fmax, 0, detectMin=not maximize, detectMax=maximize, cap=cap)
        cxy, cn = (xyMax, nMax) if maximize else (xyMin, nMin)
        xy = torch.zeros((B, max(maxMatches, 1), 2), dtype=torch.int16, device=images.device)
        scores = torch.zeros((B, max(maxMatches, 1)), dtype=torch.float32, device=images.device)
        counts = torch.empty((B,), dtype=torch.int32, device=images.device)
        torch.cuda.current_stream(images.device).synchronize()   # the zero fills run on torch's stream: order them before the kernel of the ctx
        sp, sis, srs, w, h, _ = _geom(sub)
        _check(self.ctx, self.L.bhip_template_select_dev_f32(self.ctx._h, sp, sis, srs, w, h, B, C.c_void_p(cxy.data_ptr()), C.c_void_p(cn.data_ptr()), cap,
                                                           int(maxMatches), 1 if maximize else 0, C.c_void_p(xy.data_ptr()),
                                                           C.c_void_p(scores.data_ptr()), C.c_void_p(counts.data_ptr())))
        return xy[:, :maxMatches], scores[:, :maxMatches], counts, cn

    def cornerIntensity(self, kind, radius, kappa, dx, dy, out=None, weighted=False):
        """kind: 0 Shi-Tomasi, 1 Harris.  float32 derivatives: ImplSsdCorner_F32 / ImplSsdCornerWeighted_F32; int16 derivatives:
        ImplSsdCorner_S16 / ImplSsdCornerWeighted_S16.  The intensity is float32."""
        s16 = dx.dtype == torch.int16
        dt = torch.int16 if s16 else torch.float32
        out = torch.empty(dx.shape, dtype=torch.float32, device=dx.device) if out is None else out
        xp, dis, drs, W, H, B = _geom(dx, dt)
        yp, dis2, drs2, _, _, _ = _geom(dy, dt)
        if (dis, drs) != (dis2, drs2):
            raise IllegalArgumentException("derivX and derivY must share their layout")
        op, ois, ors, _, _, _ = _geom(out)
        if s16:
            st = self.L.bhip_corner_intensity_dev_s16(self.ctx._h, int(kind), int(radius), float(kappa), 1 if weighted else 0, xp, yp, dis, drs, W, H, B, op,
                                                      ois, ors)
        elif weighted:
            st = self.L.bhip_corner_intensity_weighted_dev_f32(self.ctx._h, int(kind), int(radius), float(kappa), xp, yp, dis, drs, W, H, B, op, ois, ors)
        else:
            st = self.L.bhip_corner_intensity_dev_f32(self.ctx._h, int(kind), int(radius), float(kappa), xp, yp, dis, drs, W, H, B, op, ois, ors)
        _check(self.ctx, st)
        return out

    def pyramidLayout(self, width, height, scales):
        s = np.ascontiguousarray(scales, np.int32)
        dims = np.zeros(2 * len(s), np.int32)
        offs = np.zeros(len(s), np.int64)
        total = C.c_longlong()
        if self.L.bhip_pyramid_layout(width, height, s.ctypes.data_as(_lib._ip), len(s), dims.ctypes.data_as(_lib._ip), offs.ctypes.data_as(_lib._llp),
                                      C.byref(total)) != 0:
            raise IllegalArgumentException("bad pyramid scales")
        return dims.reshape(-1, 2), offs, total.value

    def pyramid(self, kernel, scales, src):
        """-> list of [B, h_i, w_i] layer views into one packed [B, total] tensor.  float32 frames with a Kernel1D_F32, or uint8 frames with a
        Kernel1D_S32 (PyramidDiscreteSampleBlur<GrayU8>)"""
        u8 = src.dtype == torch.uint8
        k = np.ascontiguousarray(kernel, np.int32 if u8 else np.float32)
        s = np.ascontiguousarray(scales, np.int32)
        ip, iis, irs, W, H, B = _geom(src, torch.uint8 if u8 else torch.float32)
        dims, offs, total = self.pyramidLayout(W, H, s)
        out = torch.empty((B, total), dtype=src.dtype if u8 else torch.float32, device=src.device)
        if u8:
            _check(self.ctx, self.L.bhip_pyramid_dev_u8(self.ctx._h, k.ctypes.data_as(_lib._i32p), len(k), s.ctypes.data_as(_lib._ip), len(s), ip, iis, irs, W, H, B,
                                                      C.c_void_p(out.data_ptr())))
        else:
            _check(self.ctx, self.L.bhip_pyramid_dev_f32(self.ctx._h, k.ctypes.data_as(_lib._fp), len(k), s.ctypes.data_as(_lib._ip), len(s), ip, iis, irs, W, H, B,
                                                       C.c_void_p(out.data_ptr())))
        return [out[:, int(offs[i]):int(offs[i]) + int(dims[i][0]) * int(dims[i][1])].view(B, int(dims[i][1]), int(dims[i][0])) for i in range(len(s))]

    def brief(self, img, radius, samplePoints, compare, xy, start):
        """xy: [N,2] float64 device tensor, start: host prefix (B+1) -> [N, ceil(numPoints/32)] int32 words"""
        ip, iis, irs, W, H, B = _geom(img)
        sp = np.ascontiguousarray(samplePoints, np.int32)
        cp = np.ascontiguousarray(compare, np.int32)
        st = np.ascontiguousarray(start, np.int32)
        if len(st) != B + 1:
            raise IllegalArgumentException("start must have batch+1 entries")
        words = (len(cp) + 31) // 32
        out = torch.empty((xy.shape[0], words), dtype=torch.int32, device=img.device)
        _check(self.ctx, self.L.bhip_brief_dev_f32(self.ctx._h, ip, iis, irs, W, H, B, int(radius), len(cp), sp.ctypes.data_as(_lib._i32p),
                                                 cp.ctypes.data_as(_lib._i32p), C.c_void_p(xy.data_ptr()), st.ctypes.data_as(_lib._ip),
                                                 C.c_void_p(out.data_ptr())))
        return out


class DeviceKltTracker(_NativeObject):
    """PointTrackerKltPyramid (G:abst/feature/tracker/PointTrackerKltPyramid.java:139-348, as FactoryPointTracker.klt builds it) for B independent
    GrayF32 or GrayU8 sequences at once, on one bhip_klt: process(frames) takes a [B,H,W] float32 or uint8 CUDA tensor (the first call decides; a
    uint8 tracker has a uint8 pyramid and int16 derivatives) and queues pyramid, Sobel (EXTENDED border), tracking,
    re-description and the list update on the context's stream without a host synchronisation; spawn() detects Shi-Tomasi corners
    (radius 1, unweighted) with the strict non-max extractor (detectRadius, detectThreshold, detectBorder) and starts tracks on them
    (maxFeatures <= 0).  Sequence b's results equal those of a single-sequence tracker fed with frames[b]."""
    _destroy = "bhip_klt_destroy"

    def __init__(self, scales, templateRadius, config=None, detectRadius=1, detectThreshold=0.0, ctx=None, detectBorder=None, device=0):
        self.ctx = ctx or Context(device, stream=torch.cuda.current_stream(device).cuda_stream)
        self.L = _lib.load()
        self.scales = [int(s) for s in scales]
        self.templateRadius = int(templateRadius)
        self.config = config or KltConfig()
        self.detectRadius, self.detectThreshold = int(detectRadius), float(detectThreshold)
        # FactoryDetectPoint.createGeneral + GeneralFeatureDetector: ignoreBorder + radius, at least the Shi-Tomasi window radius (1)
        self.detectBorder = max(self.detectRadius, 1) if detectBorder is None else int(detectBorder)
        self._shape = None
        self._dtype = None

    def _need(self):
        if not self._h:
            raise IllegalArgumentException("process() has not been called")

    def process(self, frames):
        u8 = frames.dtype == torch.uint8
        dtype = torch.uint8 if u8 else torch.float32
        if self._dtype is not None and dtype != self._dtype:
            raise IllegalArgumentException("this tracker has been fed %s frames" % str(self._dtype).replace("torch.", ""))
        ptr, imageStride, stride, W, H, B = _geom(frames, dtype)
        if self._shape != (W, H, B) or not self._h:
            self.close()
            h = C.c_void_p()
            cfg = self.config._c()
            sc = (C.c_int * len(self.scales))(*self.scales)
            create = self.L.bhip_klt_create_u8 if u8 else self.L.bhip_klt_create
            _check(self.ctx, create(self.ctx._h, C.byref(cfg), self.templateRadius, sc, len(self.scales), self.detectRadius, self.detectThreshold,
                                    self.detectBorder, W, H, B, C.byref(h)))
            self._adopt(h)
            self._shape, self._dtype = (W, H, B), dtype
        _check(self.ctx, (self.L.bhip_klt_process_dev_u8 if u8 else self.L.bhip_klt_process_dev_f32)(self._h, ptr, imageStride, stride))

    def spawn(self):
        self._need()
        _check(self.ctx, self.L.bhip_klt_spawn(self._h, -1))

    def addTracks(self, seq, xy):
        """addTrack(x, y) on sequence seq[i] for every i, in order -> uint8 [n] (0 where the reference returns null)"""
        self._need()
        seq = np.ascontiguousarray(seq, np.int32)
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        ok = np.zeros(len(seq), np.uint8)
        _check(self.ctx, self.L.bhip_klt_add_tracks(self._h, seq.ctypes.data_as(_lib._ip), xy.ctypes.data_as(_lib._dp), len(seq), ok.ctypes.data_as(_lib._u8p)))
        return ok

    def dropTracks(self, seq, featureId):
        self._need()
        seq = np.ascontiguousarray(seq, np.int32)
        ids = np.ascontiguousarray(featureId, np.int64)
        ok = np.zeros(len(seq), np.uint8)
        _check(self.ctx, self.L.bhip_klt_drop_tracks(self._h, seq.ctypes.data_as(_lib._ip), ids.ctypes.data_as(_lib._llp), len(seq), ok.ctypes.data_as(_lib._u8p)))
        return ok

    def dropAllTracks(self):
        self._need()
        _check(self.ctx, self.L.bhip_klt_drop_all(self._h))

    def reset(self):
        self._need()
        _check(self.ctx, self.L.bhip_klt_reset(self._h))

    def counts(self):
        """-> (active, spawned, dropped) int32 [B] each"""
        self._need()
        B = self._shape[2]
        out = [np.zeros(B, np.int32) for _ in range(3)]
        _check(self.ctx, self.L.bhip_klt_counts(self._h, *[o.ctypes.data_as(_lib._ip) for o in out]))
        return tuple(out)

    def stats(self):
        """-> (tracks, iterations, borderIterations) of the last process() over all sequences"""
        self._need()
        v = [C.c_longlong() for _ in range(3)]
        _check(self.ctx, self.L.bhip_klt_stats(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _fetch(self, which, seq):
        self._need()
        ids, xy, fault, err = _klt_fetch(self.ctx, self._h, which, int(seq), self._shape[2])
        return dict(featureId=ids, xy=xy, fault=fault, error=err)

    def active(self, seq):
        """tracks of getActiveTracks() of sequence seq, in list order: dict(featureId, xy, fault, error)"""
        return self._fetch(0, seq)

    def spawned(self, seq):
        return self._fetch(1, seq)

    def dropped(self, seq):
        return self._fetch(2, seq)

    def templates(self, seq, layer, which=0):
        """PyramidKltFeature.desc[layer] of every track of a list (which: 0 active, 1 spawned, 2 dropped) of sequence seq, in list order
        -> (templates float32 [n][3][(2r+1)^2] = desc, derivX, derivY; G float32 [n][3] = Gxx, Gyy, Gxy)"""
        self._need()
        n = int(self.counts()[(0, 1, 2)[which]][seq])
        ln = (2 * self.templateRadius + 1) ** 2
        t, G = np.zeros((n, 3, ln), np.float32), np.zeros((n, 3), np.float32)
        if n:
            _check(self.ctx, self.L.bhip_klt_fetch_templates(self._h, int(which), int(seq), int(layer), t.ctypes.data_as(_lib._fp), G.ctypes.data_as(_lib._fp)))
        return t, G

    def layer(self, seq, layer, which=0):
        """layer of the image pyramid (which 0) / derivX (1) / derivY (2) of sequence seq, as a host array"""
        self._need()
        sc = np.asarray(self.scales, dtype=np.int32)
        dims = np.zeros(2 * len(sc), dtype=np.int32)
        self.L.bhip_pyramid_layout(self._shape[0], self._shape[1], sc.ctypes.data_as(_lib._ip), len(sc), dims.ctypes.data_as(_lib._ip), None, None)
        shape = (int(dims[2 * layer + 1]), int(dims[2 * layer]))
        if self._dtype == torch.uint8:   # uint8 image pyramid, int16 derivatives
            if which == 0:
                out = np.zeros(shape, np.uint8)
                _check(self.ctx, self.L.bhip_klt_fetch_layer_u8(self._h, int(seq), int(layer), out.ctypes.data_as(_lib._u8p)))
            else:
                out = np.zeros(shape, np.int16)
                _check(self.ctx, self.L.bhip_klt_fetch_layer_s16(self._h, int(seq), int(layer), int(which), out.ctypes.data_as(_lib._i16p)))
            return out
        out = np.zeros(shape, np.float32)
        _check(self.ctx, self.L.bhip_klt_fetch_layer(self._h, int(seq), int(layer), int(which), out.ctypes.data_as(_lib._fp)))
        return out


class DeviceBackgroundModel(_NativeObject):
    """FactoryBackgroundModel.stationaryBasic / stationaryGaussian / stationaryGmm for S independent camera streams at once, on one bhip_bg
    (F:factory/background/FactoryBackgroundModel.java:47-64,112-141,193-225; stream s is one Java object).

    algorithm   "basic", "gaussian" or "gmm", with config a ConfigBackgroundBasic / ConfigBackgroundGaussian / ConfigBackgroundGmm (None: the
                GMM defaults); the factory's rules hold (stationaryBasic does not forward config.unknownValue)
    dtype       torch.uint8 or torch.float32
    bands       0: Gray frames [S,T,H,W]; 1..4: Planar frames [S,T,B,H,W]
    update()    updateBackground(frame_t[, mask_t]) for the T frames of every stream in one launch that keeps each pixel's model in registers;
                masks: None, True (allocated) or a uint8 [S,T,H,W] tensor -> the masks
    segment()   segment(frame, mask) with frames [S,(B,)H,W] -> uint8 [S,H,W]
    Frames and masks may be strided views (unit stride along x).  The handle is created at the first call, for its stream count and frame size."""
    ALGORITHMS = ("basic", "gaussian", "gmm")
    _destroy = "bhip_bg_destroy"

    def __init__(self, algorithm, config=None, dtype=torch.uint8, bands=0, ctx=None, device=0):
        if algorithm not in self.ALGORITHMS:
            raise IllegalArgumentException("algorithm must be one of %s" % (self.ALGORITHMS,))
        if dtype not in (torch.uint8, torch.float32):
            raise RuntimeError("only uint8 and float32 frames are implemented on the GPU (use the Java path)")
        if config is None and algorithm == "gmm":
            config = ConfigBackgroundGmm()
        elif config is None:
            raise IllegalArgumentException("ConfigBackgroundBasic / ConfigBackgroundGaussian: threshold has no default")
        else:
            config.checkValidity()
        self.ctx = ctx or Context(device, stream=torch.cuda.current_stream(device).cuda_stream)
        self.L = _lib.load()
        self.device = torch.device("cuda", self.ctx.device)
        self.algorithm, self.config, self.dtype, self.bands = algorithm, config, dtype, int(bands)
        self._shape = None          # (S, H, W)
        self._unknown = None if algorithm == "basic" else config.unknownValue

    def _create(self, S, H, W):
        if self._h:
            if self._shape != (S, H, W):
                raise IllegalArgumentException("this model was created for %d streams of %d x %d frames" % (self._shape[0], self._shape[2], self._shape[1]))
            return
        c = self.config
        family = _lib.BHIP_IMAGE_PLANAR if self.bands else _lib.BHIP_IMAGE_GRAY
        pixel = _lib.BHIP_PIXEL_U8 if self.dtype == torch.uint8 else _lib.BHIP_PIXEL_F32
        h = C.c_void_p()
        if self.algorithm == "basic":
            cfg = _lib.BgBasicCfg(c.learnRate, c.threshold, c.unknownValue)
            st = self.L.bhip_bg_create_basic(self.ctx._h, C.byref(cfg), family, pixel, self.bands, W, H, S, C.byref(h))
        elif self.algorithm == "gaussian":
            cfg = _lib.BgGaussianCfg(c.learnRate, c.threshold, c.initialVariance, c.minimumDifference, c.unknownValue)
            st = self.L.bhip_bg_create_gaussian(self.ctx._h, C.byref(cfg), family, pixel, self.bands, W, H, S, C.byref(h))
        else:
            cfg = _lib.BgGmmCfg(c.learningPeriod, c.initialVariance, c.decayCoefient, c.maxDistance, c.numberOfGaussian, c.significantWeight, c.unknownValue)
            st = self.L.bhip_bg_create_gmm(self.ctx._h, C.byref(cfg), family, pixel, self.bands, W, H, S, C.byref(h))
        _check(self.ctx, st)
        self._adopt(h)
        self._shape = (S, H, W)
        if self.algorithm == "basic" and self._unknown is not None:
            _check(self.ctx, self.L.bhip_bg_set_unknown_value(self._h, self._unknown))

    def setUnknownValue(self, unknownValue):
        if unknownValue < 0 or unknownValue > 255:
            raise IllegalArgumentException("out of range. 0 to 255")
        self._unknown = int(unknownValue)
        if self._h:
            _check(self.ctx, self.L.bhip_bg_set_unknown_value(self._h, self._unknown))

    def set(self, name, value):
        """a setter of the Java class on every stream: threshold, learn_rate, initial_variance, minimum_difference, learning_period,
        significant_weight, max_distance"""
        if not self._h:
            raise IllegalArgumentException("the model is created by the first update() or segment()")
        _check(self.ctx, getattr(self.L, "bhip_bg_set_" + name)(self._h, float(value)))

    def _frames(self, t, lead, what):
        """t: [S, (T,) (B,) H, W] with `lead` leading dimensions -> (ptr, strides of the leading dimensions + band, row stride, sizes)"""
        nd = lead + (1 if self.bands else 0) + 2
        if t.dim() != nd or t.dtype != self.dtype or not t.is_cuda:
            raise IllegalArgumentException("%s: expected a %d-dimensional %s CUDA tensor" % (what, nd, str(self.dtype).replace("torch.", "")))
        if self.bands and t.shape[lead] != self.bands:
            raise IllegalArgumentException("%s: expected %d bands" % (what, self.bands))
        if t.shape[-1] > 1 and t.stride(-1) != 1:
            raise IllegalArgumentException("the last dimension must be contiguous")
        if any(t.shape[i] > 1 and t.stride(i) < 0 for i in range(nd)):
            raise IllegalArgumentException("strides must not be negative")
        W = t.shape[-1]
        row = t.stride(-2) if t.shape[-2] > 1 else max(W, t.stride(-2))
        band = t.stride(lead) if self.bands else 0
        return C.c_void_p(t.data_ptr()), [t.stride(i) for i in range(lead)], band, row

    def _masks(self, m, shape, what):
        if m.dtype != torch.uint8 or not m.is_cuda or tuple(m.shape) != tuple(shape):
            raise IllegalArgumentException("%s: expected a uint8 CUDA tensor of shape %s" % (what, tuple(shape)))
        if m.shape[-1] > 1 and m.stride(-1) != 1:
            raise IllegalArgumentException("the last dimension must be contiguous")
        W = m.shape[-1]
        return C.c_void_p(m.data_ptr()), [m.stride(i) for i in range(m.dim() - 2)], (m.stride(-2) if m.shape[-2] > 1 else max(W, m.stride(-2)))

    def update(self, frames, masks=None):
        ptr, (ss, fs), band, row = self._frames(frames, 2, "frames")
        S, T, H, W = frames.shape[0], frames.shape[1], frames.shape[-2], frames.shape[-1]
        self._create(S, H, W)
        if masks is True:
            masks = torch.empty((S, T, H, W), dtype=torch.uint8, device=frames.device)
        mp, mss, mfs, mrow = None, 0, 0, 0
        if masks is not None:
            mp, (mss, mfs), mrow = self._masks(masks, (S, T, H, W), "masks")
        fn = self.L.bhip_bg_update_dev_u8 if self.dtype == torch.uint8 else self.L.bhip_bg_update_dev_f32
        _check(self.ctx, fn(self._h, ptr, ss, fs, band, row, T, mp, mss, mfs, mrow))
        return masks

    def segment(self, frames, out=None):
        ptr, (ss,), band, row = self._frames(frames, 1, "frames")
        S, H, W = frames.shape[0], frames.shape[-2], frames.shape[-1]
        self._create(S, H, W)
        if out is None:
            out = torch.empty((S, H, W), dtype=torch.uint8, device=frames.device)
        mp, (mss,), mrow = self._masks(out, (S, H, W), "out")
        fn = self.L.bhip_bg_segment_dev_u8 if self.dtype == torch.uint8 else self.L.bhip_bg_segment_dev_f32
        _check(self.ctx, fn(self._h, ptr, ss, band, row, mp, mss, mrow))
        return out

    def reset(self, stream=None):
        if self._h:
            _check(self.ctx, self.L.bhip_bg_reset(self._h, -1 if stream is None else int(stream)))

    def model(self, stream):
        """the model of one stream in the reference's layout (include/boofhip.h, bhip_bg_fetch_model), as a float32 NumPy array:
        Basic [bands][H][W], Gaussian [2*bands][H][W], GMM [H][W*modelStride]"""
        if not self._h:
            raise IllegalArgumentException("the model is created by the first update() or segment()")
        n = C.c_longlong()
        _check(self.ctx, self.L.bhip_bg_model_floats(self._h, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        _check(self.ctx, self.L.bhip_bg_fetch_model(self._h, int(stream), out.ctypes.data_as(_lib._fp)))
        _, H, W = self._shape
        return out.reshape(H, -1) if self.algorithm == "gmm" else out.reshape(-1, H, W)

    def storeModel(self, stream, model):
        """the inverse of model(): installs a model (the stream counts as initialised afterwards)"""
        if not self._h:
            raise IllegalArgumentException("the model is created by the first update() or segment()")
        n = C.c_longlong()
        _check(self.ctx, self.L.bhip_bg_model_floats(self._h, C.byref(n)))
        a = np.ascontiguousarray(model, np.float32).reshape(-1)
        if a.size != n.value:
            raise IllegalArgumentException("the model of a stream has %d floats" % n.value)
        _check(self.ctx, self.L.bhip_bg_store_model(self._h, int(stream), a.ctypes.data_as(_lib._fp)))
