"""NumPy / plain Python restatement of the thresholding family (FactoryThresholdBinary.threshold on GrayU8 / GrayF32), following the Java:

  ConfigLength.computeI                      T:struct/ConfigLength.java:53-80
  ImplThresholdImageOps.threshold            I:alg/filter/binary/impl/ImplThresholdImageOps.java:46-134
  localMean / localGaussian                  :226-323 (GrayU8), :424-520 (GrayF32)
  BlurImageOps.mean / gaussian on GrayU8     I:alg/filter/blur/BlurImageOps.java:75-141 -> ConvolveImageMean, ImplConvolveMean, ConvolveImageNormalized,
                                             ConvolveNormalized_JustBorder_SB, ConvolveNormalizedNaive_SB
  ... and on GrayF32 (float sums in the reference's order)
  GThresholdImageOps.computeOtsu             I:alg/filter/binary/GThresholdImageOps.java:105-142
  GlobalBinaryFilter.process                 I:abst/filter/binary/GlobalBinaryFilter.java:57-62
  ThresholdBlock (geometry, stages)          I:alg/filter/binary/ThresholdBlock.java:90-170
  ThresholdBlockMinMax_U8 / _F32, ThresholdBlockMean_U8 / _F32, ThresholdBlockOtsu, ComputeOtsu

Images are (H, W) arrays, uint8 or float32; results are uint8 0/1 arrays.  Test code: clarity over speed."""
import numpy as np

from corner_ref import gaussian_kernel_s32

F = np.float32
(FIXED, GLOBAL_ENTROPY, GLOBAL_OTSU, GLOBAL_LI, GLOBAL_HUANG, LOCAL_GAUSSIAN, LOCAL_MEAN, LOCAL_OTSU, BLOCK_MIN_MAX, BLOCK_MEAN, BLOCK_OTSU, LOCAL_SAVOLA,
 LOCAL_NICK) = range(13)   # ThresholdType ordinals


def java_d2i(v):
    """(int) of a double"""
    v = float(v)
    if v != v:
        return 0
    return int(max(-2147483648.0, min(2147483647.0, v)))


def compute_i(length, fraction, total):
    """ConfigLength.computeI"""
    size = max(fraction * total, length) if fraction >= 0 else length
    return int(size + 0.5) if size >= 0 else -1


def select_block_size(width, height, requested):
    """ThresholdBlock.selectBlockSize -> (blockWidth, blockHeight); ZeroDivisionError where Java throws ArithmeticException"""
    bh = height if height < requested else height // (height // requested)
    bw = width if width < requested else width // (width // requested)
    return bw, bh


# ---------------- global ----------------
def threshold(img, thr, down):
    """GThresholdImageOps.threshold(input, output, double threshold, down)"""
    if img.dtype == np.uint8:
        t = java_d2i(thr)
        a = img.astype(np.int64)
    else:
        t = F(thr)
        a = img
    with np.errstate(invalid="ignore"):
        return (a <= t if down else a > t).astype(np.uint8)


def compute_otsu(histogram, length, totalPixels):
    """GThresholdImageOps.computeOtsu(int[], int, int)"""
    dlength = float(length)
    s = 0.0
    for i in range(length):
        s += (i / dlength) * int(histogram[i])
    sumB, wB, varMax, thr = 0.0, 0, 0.0, 0
    for i in range(length):
        wB += int(histogram[i])
        if wB == 0:
            continue
        wF = totalPixels - wB
        if wF == 0:
            break
        sumB += (i / dlength) * int(histogram[i])
        mB = sumB / wB
        mF = (s - sumB) / wF
        varBetween = float(wB) * float(wF) * (mB - mF) * (mB - mF)
        if varBetween > varMax:
            varMax, thr = varBetween, i
    return thr


def global_otsu(img, scale, down, minValue=0, maxValue=255):
    """GlobalBinaryFilter.Otsu.process on GrayU8"""
    hist = np.bincount(img.reshape(-1).astype(np.int64) - minValue, minlength=1 + maxValue - minValue)
    otsu = compute_otsu(hist, len(hist), img.size) + minValue
    s = scale if down else (0.0 if scale <= 0.0 else 1.0 / scale)
    return threshold(img, float(otsu) * s, down)


# ---------------- GrayU8 blurs ----------------
def _norm_s32(a, k, axis):
    """(total + weight/2) / weight over the taps inside the image: what the interior (divisor = kernel sum), the JustBorder and the Naive form all compute"""
    a = np.moveaxis(np.asarray(a, np.int64), axis, 0)
    n, kw, r = a.shape[0], len(k), len(k) // 2
    out = np.empty_like(a)
    for p in range(n):
        lo, hi = max(0, r - p), min(kw, n - p + r)
        total = np.zeros(a.shape[1:], np.int64)
        weight = 0
        for t in range(lo, hi):
            total += a[p - r + t] * int(k[t])
            weight += int(k[t])
        out[p] = (total + weight // 2) // weight
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def mean_u8(img, radiusX, radiusY=None):
    """BlurImageOps.mean(GrayU8): horizontal into a GrayU8 storage image, vertical on that"""
    radiusY = radiusX if radiusY is None else radiusY
    if radiusX <= 0 or radiusY <= 0:
        raise ValueError("Radius must be > 0")
    h = _norm_s32(img, np.ones(2 * radiusX + 1, np.int64), 1)
    return _norm_s32(h, np.ones(2 * radiusY + 1, np.int64), 0)


def mean_u8_literal(img, radius):
    """The same, loop by loop as ConvolveImageMean.horizontal / vertical dispatch: ConvolveImageNormalized (Naive) when the kernel is wider than
    the image, else ConvolveNormalized_JustBorder_SB for the border and ImplConvolveMean's running totals for the interior.  Small images only."""
    def one_pass(a):   # along the last axis
        H, W = a.shape
        kw = 2 * radius + 1
        out = np.zeros((H, W), np.int64)
        for y in range(H):
            row = [int(v) for v in a[y]]
            if kw > W:
                for x in range(W):
                    s, e = max(x - radius, 0), min(x - radius + kw, W)
                    weight = e - s
                    out[y, x] = (sum(row[s:e]) + weight // 2) // weight
                continue
            for x in range(radius):                       # left border: taps kw - (radius + 1 + x) .. kw
                taps = radius + 1 + x
                out[y, x] = (sum(row[:taps]) + taps // 2) // taps
            for x in range(W - radius, W):                # right border: kEnd = W - (x - radius) taps
                taps = W - (x - radius)
                out[y, x] = (sum(row[x - radius:]) + taps // 2) // taps
            total = sum(row[:kw])
            out[y, radius] = (total + kw // 2) // kw
            for i in range(kw, W):
                total -= row[i - kw]
                total += row[i]
                out[y, i - radius] = (total + kw // 2) // kw
        return out.astype(np.uint8)
    h = one_pass(np.asarray(img))
    return one_pass(h.T).T


def box_mean_u8_single_division(img, radius):
    """NOT the reference: one 2-D box sum over the clipped window with one rounding division (what a plausible GPU version would do)"""
    a = np.asarray(img, np.int64)
    H, W = a.shape
    out = np.empty((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            win = a[max(0, y - radius):min(H, y + radius + 1), max(0, x - radius):min(W, x + radius + 1)]
            out[y, x] = (win.sum() + win.size // 2) // win.size
    return out.astype(np.uint8)


def gaussian_u8(img, radius):
    """BlurImageOps.gaussian(GrayU8, -1, radius)"""
    k = gaussian_kernel_s32(radius)
    return _norm_s32(_norm_s32(img, k, 1), k, 0)


# ---------------- GrayF32 blurs: float sums in the reference's order ----------------
def _norm_f32(a, k, axis, normalized_interior):
    """ConvolveImageNormalized with a Kernel1D_F32 of offset width/2: Naive when the kernel is at least as wide as the image, else
    ConvolveImageNoBorder inside (total, taps in increasing order) and JustBorder (total / weight) in the border"""
    a = np.moveaxis(np.asarray(a, F), axis, 0)
    k = np.asarray(k, F)
    n, kw, r = a.shape[0], len(k), len(k) // 2
    out = np.empty_like(a)
    naive = kw >= n
    with np.errstate(all="ignore"):
        for p in range(n):
            lo, hi = max(0, r - p), min(kw, n - p + r)
            total = np.zeros(a.shape[1:], F)
            weight = F(0)
            for t in range(lo, hi):
                total = total + a[p - r + t] * k[t]
                weight = F(weight + k[t])
            interior = not naive and r <= p < n - r
            out[p] = total / weight if (not interior or normalized_interior) else total
    return np.moveaxis(out, 0, axis)


def gaussian_f32(img, kernel):
    """BlurImageOps.gaussian(GrayF32, -1, radius); kernel = FactoryKernelGaussian.gaussian(Kernel1D_F32, -1, radius)"""
    return _norm_f32(_norm_f32(img, kernel, 1, False), kernel, 0, False)


def _mean_f32_pass(a, radius, axis):
    a = np.moveaxis(np.asarray(a, F), axis, 0)
    n, kw = a.shape[0], 2 * radius + 1
    k = np.full(kw, F(1.0) / F(kw), F)   # FactoryKernel.table1D_F32(radius, true)
    if kw > n:
        return np.moveaxis(_norm_f32(a, k, 0, True), 0, axis)
    out = _norm_f32(a, k, 0, True)       # the border rows are kept, the interior is overwritten
    divisor = F(kw)
    with np.errstate(all="ignore"):
        total = np.zeros(a.shape[1:], F)
        for i in range(kw):
            total = total + a[i]
        out[radius] = total / divisor
        for i in range(kw, n):
            total = total - a[i - kw]
            total = total + a[i]
            out[i - radius] = total / divisor
    return np.moveaxis(out, 0, axis)


def mean_f32(img, radius):
    """BlurImageOps.mean(GrayF32): ConvolveImageMean.horizontal then vertical, running float totals"""
    if radius <= 0:
        raise ValueError("Radius must be > 0")
    return _mean_f32_pass(_mean_f32_pass(img, radius, 1), radius, 0)


# ---------------- local ----------------
def _local_compare(img, blur, scale, down):
    scale = F(scale)   # the filters hand their double to a float parameter
    with np.errstate(all="ignore"):
        if down:
            return (img.astype(F) <= blur.astype(F) * scale).astype(np.uint8)
        return (img.astype(F) * scale > blur.astype(F)).astype(np.uint8)


def local_radius(img, length, fraction):
    return compute_i(length, fraction, min(img.shape[1], img.shape[0])) // 2


def local_mean(img, length, fraction, scale, down, blur=None):
    """ThresholdImageOps.localMean; blur: another mean (the order-sensitivity check hands in the single-division box mean)"""
    radius = local_radius(img, length, fraction)
    if blur is None:
        blur = mean_u8(img, radius) if img.dtype == np.uint8 else mean_f32(img, radius)
    return _local_compare(img, blur, scale, down)


def local_gaussian(img, length, fraction, scale, down, kernel_f32=None):
    radius = local_radius(img, length, fraction)
    if radius <= 0:
        raise ValueError("Sigma must be > 0")
    blur = gaussian_u8(img, radius) if img.dtype == np.uint8 else gaussian_f32(img, kernel_f32)
    return _local_compare(img, blur, scale, down)


# ---------------- blocks ----------------
class ComputeOtsu:
    """I:alg/filter/binary/ComputeOtsu.java"""

    def __init__(self, useOtsu2, tuning, down, scale):
        self.useOtsu2, self.tuning, self.down, self.scale = useOtsu2, float(tuning), down, float(scale)
        self.threshold = self.variance = 0.0

    def compute(self, histogram, length, totalPixels):
        dlength = float(length)
        s = 0.0
        for i in range(length):
            s += (i / dlength) * int(histogram[i])
        sumB, wB = 0.0, 0
        self.variance = self.threshold = 0.0
        selectedMB = selectedMF = 0.0
        for i in range(length):
            wB += int(histogram[i])
            if wB == 0:
                continue
            wF = totalPixels - wB
            if wF == 0:
                break
            f = i / dlength
            sumB += f * int(histogram[i])
            mB = sumB / wB
            mF = (s - sumB) / wF
            varBetween = float(wB) * float(wF) * (mB - mF) * (mB - mF)
            if varBetween > self.variance:
                self.variance = varBetween
                if self.useOtsu2:
                    selectedMB, selectedMF = mB, mF
                else:
                    self.threshold = float(i)
        if self.useOtsu2:
            self.threshold = length * (selectedMB + selectedMF) / 2.0
        self.variance += 0.001
        adjustment = java_d2i(self.tuning * self.threshold * self.tuning * self.threshold / self.variance + 0.5)
        self.threshold += -adjustment if self.down else adjustment
        self.threshold = float(java_d2i(self.scale * max(self.threshold, 0.0) + 0.5))
        return self.threshold


def block_geometry(width, height, requested):
    """-> (bw, bh, nbx, nby, rect) with rect(bx, by) = (x0, y0, x1, y1): the last block of a direction takes the remainder"""
    bw, bh = select_block_size(width, height, requested)
    nbx, nby = width // bw, height // bh

    def rect(bx, by):
        return bx * bw, by * bh, (width if bx == nbx - 1 else (bx + 1) * bw), (height if by == nby - 1 else (by + 1) * bh)
    return bw, bh, nbx, nby, rect


def _raster_sum_f32(block, pairwise):
    if pairwise:   # NOT the reference: numpy's pairwise summation, for the order-sensitivity check
        return F(np.sum(block, dtype=F))
    s = F(0)
    with np.errstate(all="ignore"):
        for v in block.reshape(-1):
            s = F(s + v)
    return s


def block_stats(img, kind, requested, scale=1.0, pairwise=False):
    """computeStatistics: MIN_MAX -> (nby, nbx, 2), MEAN -> (nby, nbx) (uint8 values as int64, or float32), OTSU -> (nby, nbx, 256) int64"""
    H, W = img.shape
    bw, bh, nbx, nby, rect = block_geometry(W, H, requested)
    u8 = img.dtype == np.uint8
    if kind == BLOCK_MIN_MAX:
        stats = np.zeros((nby, nbx, 2), np.int64 if u8 else F)
    elif kind == BLOCK_MEAN:
        stats = np.zeros((nby, nbx), np.int64 if u8 else F)
    else:
        stats = np.zeros((nby, nbx, 256), np.int64)
    for by in range(nby):
        for bx in range(nbx):
            x0, y0, x1, y1 = rect(bx, by)
            blk = img[y0:y1, x0:x1]
            if kind == BLOCK_MIN_MAX:
                mn = mx = blk[0, 0]
                for v in blk.reshape(-1):   # `if (v < min) .. else if (v > max)`: a NaN first pixel stays in both
                    if v < mn:
                        mn = v
                    elif v > mx:
                        mx = v
                stats[by, bx] = (mn, mx)
            elif kind == BLOCK_MEAN:
                w, h = x1 - x0, y1 - y0
                if u8:
                    s = int(blk.astype(np.int64).sum())
                    stats[by, bx] = java_d2i(float(scale) * s / (w * h) + 0.5) & 0xFF   # (byte), read back & 0xFF
                else:
                    with np.errstate(all="ignore"):
                        stats[by, bx] = F(F(scale) * _raster_sum_f32(blk, pairwise)) / F(w * h)
            else:
                stats[by, bx] = np.bincount(blk.reshape(-1), minlength=256)
    return stats


def threshold_block(img, kind, requested, scale, down, local=True, minimumSpread=10.0, useOtsu2=True, tuning=0.0, pairwise=False):
    """ThresholdBlock.process with the processor of `kind`"""
    H, W = img.shape
    bw, bh, nbx, nby, rect = block_geometry(W, H, requested)
    u8 = img.dtype == np.uint8
    stats = block_stats(img, kind, requested, scale, pairwise)
    out = np.zeros((H, W), np.uint8)
    a, b = (1, 0) if down else (0, 1)
    otsu = ComputeOtsu(useOtsu2, tuning, down, scale)
    for by in range(nby):
        for bx in range(nbx):
            x0, y0, x1, y1 = rect(bx, by)
            if local:
                bx0, by0, bx1, by1 = max(0, bx - 1), max(0, by - 1), min(nbx - 1, bx + 1), min(nby - 1, by + 1)
            else:
                bx0, by0, bx1, by1 = bx, by, bx, by
            px = img[y0:y1, x0:x1]
            with np.errstate(all="ignore"):
                if kind == BLOCK_MIN_MAX:
                    if u8:
                        mn, mx = 2147483647, -2147483647
                    else:
                        mn, mx = F(np.finfo(F).max), F(-np.finfo(F).max)
                    for y in range(by0, by1 + 1):
                        for x in range(bx0, bx1 + 1):
                            lmn, lmx = stats[y, x]
                            if lmn < mn:
                                mn = lmn
                            if lmx > mx:
                                mx = lmx
                    if u8:
                        if int(mx) - int(mn) <= java_d2i(minimumSpread):
                            res = np.ones(px.shape, np.uint8)
                        else:
                            average = java_d2i(float(scale) * ((int(mx) + int(mn)) // 2))   # max + min >= 0: // is Java's /
                            res = (px.astype(np.int64) <= average) if down else (px.astype(np.int64) > average)
                    else:
                        if F(mx - mn) <= F(minimumSpread):
                            res = np.ones(px.shape, np.uint8)
                        else:
                            average = F(F(scale) * F(mx + mn)) / F(2.0)
                            res = (px <= average) if down else (px > average)
                elif kind == BLOCK_MEAN:
                    count = (by1 - by0 + 1) * (bx1 - bx0 + 1)
                    if u8:
                        mean = 0
                        for y in range(by0, by1 + 1):
                            for x in range(bx0, bx1 + 1):
                                mean += int(stats[y, x])
                        mean //= count
                        le = px.astype(np.int64) <= mean
                    else:
                        mean = F(0)
                        for y in range(by0, by1 + 1):
                            for x in range(bx0, bx1 + 1):
                                mean = F(mean + stats[y, x])
                        mean = F(mean / F(count))
                        le = px <= mean
                    res = np.where(le, a, b)
                else:
                    histogram = stats[by0:by1 + 1, bx0:bx1 + 1].reshape(-1, 256).sum(axis=0)
                    thr = otsu.compute(histogram, 256, int(histogram.sum()))
                    res = np.where(px.astype(np.float64) <= thr, a, b)
            out[y0:y1, x0:x1] = res
    return out


# ---------------- the factory ----------------
def threshold_config(img, cfg, kernel_f32=None):
    """FactoryThresholdBinary.threshold(config, type).process(img); cfg: anything with the ConfigThreshold fields of the mirror (type as an ordinal,
    width a ConfigLength with length / fraction).  kernel_f32: the Kernel1D_F32 of a GrayF32 LOCAL_GAUSSIAN."""
    t = int(cfg.type)
    H, W = img.shape
    side = min(W, H)
    if t == FIXED:
        return threshold(img, cfg.fixedThreshold, cfg.down)
    if t == GLOBAL_OTSU:
        return global_otsu(img, cfg.scale, cfg.down, cfg.minPixelValue, cfg.maxPixelValue)
    if t == LOCAL_MEAN:
        return local_mean(img, cfg.width.length, cfg.width.fraction, cfg.scale, cfg.down)
    if t == LOCAL_GAUSSIAN:
        return local_gaussian(img, cfg.width.length, cfg.width.fraction, cfg.scale, cfg.down, kernel_f32)
    if t in (BLOCK_MIN_MAX, BLOCK_MEAN, BLOCK_OTSU):
        requested = compute_i(cfg.width.length, cfg.width.fraction, side)
        return threshold_block(img, t, requested, cfg.scale, cfg.down, cfg.thresholdFromLocalBlocks, getattr(cfg, "minimumSpread", 10.0),
                               getattr(cfg, "useOtsu2", True), getattr(cfg, "tuning", 0.0))
    raise ValueError("not restated: %d" % t)


# ---------------- the inputs the CPU and GPU tests share ----------------
def image_u8(width, height, seed):
    """a ramp with noise: every block has texture, neighbouring means differ"""
    rng = np.random.default_rng(seed)
    ramp = np.add.outer(np.arange(height) * 5, np.arange(width) * 3) % 200
    return np.clip(ramp + rng.integers(-45, 56, (height, width)), 0, 255).astype(np.uint8)


def image_f32(width, height, seed):
    """uniform in [0, 255) with all 24 significant bits in use, so float sums depend on their order"""
    rng = np.random.default_rng(seed)
    return (rng.random((height, width), dtype=np.float32) * F(255)).astype(F)


BLOCK_MEAN_F32_INPUT = dict(width=67, height=37, seed=11, requested=8)   # the GrayF32 BLOCK_MEAN case of tests/test_gpu_threshold.py
LOCAL_MEAN_U8_INPUT = dict(width=67, height=37, seed=11, length=11)       # the GrayU8 LOCAL_MEAN case
