"""FactoryDescribeImageDense.hog (both variants) and .sift restated in float32 / float64 scalars in the reference's loop order:
DescribeDenseHogFastAlg (F:alg/feature/dense/DescribeDenseHogFastAlg.java:80-215), DescribeDenseHogAlg (F:alg/feature/dense/DescribeDenseHogAlg.java:
121-339), DescribeDenseSiftAlg (F:alg/feature/dense/DescribeDenseSiftAlg.java:120-198), DescribeSiftCommon.trilinearInterpolation /
normalizeDescriptor and UtilFeature.normalizeL2 (through sift_describe_ref), GradientThree with the EXTENDED border (GrayF32: sift_describe_ref's;
GrayU8 -> GrayS16: b - a on clamped reads, kernel -1 0 1 without a divisor, I:alg/filter/derivative/GradientThree.java:53,86-101).

Every ordered sum exists twice: in Java's scatter order (the loops as written) and as a gather per element over only the samples that reach it
(the form a kernel uses); tests/test_dense_reference.py compares the two bit for bit.  Math.atan / Math.atan2 are the C library's math.atan /
math.atan2, one pixel at a time (unpinned against Java's to the last ulp); UtilAngle.atanSafe / domain2PI / dist (georegression) and
UtilGaussian.computePDF (ddogleg) are restated from their contract, unpinned.

`stats` records (new_stats()): atanMargin, for every pixel with dx != 0 the distance of the double atan(dy / dx) from the nearest midpoint between
adjacent floats, in double ulps (the smallest seen); axisPos / axisNeg, pixels with dx == 0 and dy >= 0 / dy < 0; clipped, descriptor elements
> 0.2 after the first normalisation; splitLow / splitHigh, standard-HOG pixel visits with i <= pixelsPerCell/2 / beyond."""
import math

import numpy as np

import sift_describe_ref as sd

f32, f64 = np.float32, np.float64
F_PI, F_PId2 = f32(math.pi), f32(math.pi / 2.0)


def new_stats():
    return dict(atanMargin=math.inf, axisPos=0, axisNeg=0, clipped=0, splitLow=0, splitHigh=0, pixels=0)


# ---------------- gradients ----------------
def gradient_f32(img):
    """GrayF32, or GrayU8 converted first (DescribeImageDense_Convert): FactoryDerivative.three, EXTENDED"""
    return sd.gradient_three(np.asarray(img).astype(f32))


def gradient_s16(img):
    """GradientThree.process(GrayU8, GrayS16, GrayS16, EXTENDED) read through getF"""
    a = np.asarray(img).astype(np.int32)
    h, w = a.shape
    xs, ys = np.arange(w), np.arange(h)
    dx = a[:, np.clip(xs + 1, 0, w - 1)] - a[:, np.clip(xs - 1, 0, w - 1)]
    dy = a[np.clip(ys + 1, 0, h - 1), :] - a[np.clip(ys - 1, 0, h - 1), :]
    return dx.astype(np.int16).astype(f32), dy.astype(np.int16).astype(f32)


# ---------------- shared ----------------
def normalize_l2(d):
    """UtilFeature.normalizeL2 :101-114"""
    norm = 0.0
    for v in d:
        norm += float(v) * float(v)
    if norm == 0:
        return d
    return d / math.sqrt(norm)


def normalize_descriptor(d, maxValue, stats=None):
    """DescribeSiftCommon.normalizeDescriptor :84-98"""
    d = normalize_l2(np.array(d, f64))
    if stats is not None:
        stats["clipped"] += int((d > maxValue).sum())
    d = np.where(d > maxValue, maxValue, d)
    return normalize_l2(d)


def atan_margin(a):
    """distance of the double a from the nearest midpoint between adjacent floats, in ulps of a"""
    f = f32(a)
    lo, hi = float(np.nextafter(f, f32(-np.inf))), float(np.nextafter(f, f32(np.inf)))
    mid_lo, mid_hi = (lo + float(f)) / 2.0, (hi + float(f)) / 2.0
    return min(abs(a - mid_lo), abs(a - mid_hi)) / math.ulp(a)


def atan_safe(y, x, stats=None):
    """UtilAngle.atanSafe(float, float): x == 0 -> +-pi/2 by y >= 0, else (float)Math.atan(y / x) with the quotient in float"""
    y, x = f32(y), f32(x)
    if x == 0:
        if stats is not None:
            stats["axisPos" if y >= 0 else "axisNeg"] += 1
        return F_PId2 if y >= 0 else f32(-F_PId2)
    a = math.atan(float(f32(y / x)))
    if stats is not None:
        stats["atanMargin"] = min(stats["atanMargin"], atan_margin(a))
    return f32(a)


# ---------------- HOG ----------------
class Hog:
    def __init__(self, orientationBins=9, pixelsPerCell=8, cellsPerBlockX=3, cellsPerBlockY=3, stepBlock=1, fastVariant=True):
        if stepBlock <= 0:
            raise ValueError("stepBlock must be >= 1")
        self.bins, self.ppc, self.cbx, self.cby, self.step, self.fast = int(orientationBins), int(pixelsPerCell), int(cellsPerBlockX), int(cellsPerBlockY), int(stepBlock), bool(fastVariant)
        self.dof = self.bins * self.cbx * self.cby
        self.angleBinSize = f32(F_PI / f32(self.bins))
        self.weights = None if self.fast else self.weight_block_pixels()

    def args(self):
        return (self.bins, self.ppc, self.cbx, self.cby, self.step, int(self.fast))

    # ---- the grid ----
    def layout(self, width, height):
        """-> (perRow, perCol, [(x, y)]) in the reference's row-major order; the location is the block's top-left pixel"""
        ppc = self.ppc
        if self.fast:
            cellCols, cellRows = width // ppc, height // ppc
            rows = list(range(0, cellRows - (self.cby - 1), self.step))
            cols = list(range(0, cellCols - (self.cbx - 1), self.step))
            locs = [(c * ppc, r * ppc) for r in rows for c in cols]
        else:
            ys = list(range(0, height - ppc * self.cby + 1, ppc * self.step))
            xs = list(range(0, width - ppc * self.cbx + 1, ppc * self.step))
            rows, cols = ys, xs
            locs = [(x, y) for y in ys for x in xs]
        if not locs:
            return 0, 0, []
        return len(cols), len(rows), locs

    # ---- per pixel ----
    def pixel_features(self, dx, dy, stats=None):
        """-> findex0 float32 [h, w] (angle / angleBinSize) and the float sum dx*dx + dy*dy"""
        h, w = dx.shape
        findex = np.zeros((h, w), f32)
        for y in range(h):
            for x in range(w):
                angle = f32(atan_safe(dy[y, x], dx[y, x], stats) + F_PId2)
                findex[y, x] = f32(angle / self.angleBinSize)
        if stats is not None:
            stats["pixels"] += h * w
        return findex, (dx * dx + dy * dy).astype(f32)

    # ---- fast variant ----
    def cell_histograms(self, findex, sumsq):
        """computeCellHistograms :175-215, Java's loops -> float32 [cellRows, cellCols, bins]"""
        h, w = findex.shape
        ppc, bins = self.ppc, self.bins
        cellRows, cellCols = h // ppc, w // ppc
        cells = np.zeros((cellRows, cellCols, bins), f32)
        magnitude = np.sqrt(sumsq.astype(f64)).astype(f32)
        for ci in range(cellRows):
            for cj in range(cellCols):
                hist = [f32(0)] * bins
                for k in range(ppc):
                    for l in range(ppc):
                        findex0 = findex[ci * ppc + k, cj * ppc + l]
                        m = magnitude[ci * ppc + k, cj * ppc + l]
                        index0 = int(findex0)
                        weight1 = f32(findex0 - f32(index0))
                        index0 %= bins
                        index1 = (index0 + 1) % bins
                        hist[index0] = f32(hist[index0] + f32(m * f32(f32(1.0) - weight1)))
                        hist[index1] = f32(hist[index1] + f32(m * weight1))
                cells[ci, cj] = hist
        return cells

    def cell_histograms_gather(self, findex, sumsq):
        """the same, one (cell, bin) at a time over the cell's pixels in raster order"""
        h, w = findex.shape
        ppc, bins = self.ppc, self.bins
        cellRows, cellCols = h // ppc, w // ppc
        cells = np.zeros((cellRows, cellCols, bins), f32)
        magnitude = np.sqrt(sumsq.astype(f64)).astype(f32)
        index = findex.astype(np.int64)           # (int): toward zero, the values are >= 0
        weight1 = (findex - index.astype(f32)).astype(f32)
        index0 = index % bins
        index1 = (index0 + 1) % bins
        first = (magnitude * (f32(1.0) - weight1)).astype(f32)
        second = (magnitude * weight1).astype(f32)
        for ci in range(cellRows):
            for cj in range(cellCols):
                sl = (slice(ci * ppc, ci * ppc + ppc), slice(cj * ppc, cj * ppc + ppc))
                i0, i1, a, b = index0[sl].reshape(-1), index1[sl].reshape(-1), first[sl].reshape(-1), second[sl].reshape(-1)
                for bin_ in range(bins):
                    acc = f32(0)
                    for p in range(ppc * ppc):
                        if i0[p] == bin_:
                            acc = f32(acc + a[p])
                        if i1[p] == bin_:
                            acc = f32(acc + b[p])
                    cells[ci, cj, bin_] = acc
        return cells

    def block_descriptor(self, cells, row, col, stats=None):
        """computeDescriptor :150-169"""
        d = np.array([cells[row + i, col + j, k] for i in range(self.cby) for j in range(self.cbx) for k in range(self.bins)], f64)
        return normalize_descriptor(d, 0.2, stats)

    # ---- standard variant ----
    def weight_block_pixels(self):
        """computeWeightBlockPixels :121-161"""
        rows, cols = self.cby * self.ppc, self.cbx * self.ppc
        offsetRow = 0.5 if rows % 2 == 0 else 0.0
        offsetCol = 0.5 if cols % 2 == 0 else 0.0
        radiusRow, radiusCol = rows // 2, cols // 2
        weights = np.zeros(rows * cols, f64)
        index = 0
        with np.errstate(all="ignore"):
            for row in range(rows):
                pdfRow = _pdf(radiusRow, row - radiusRow + offsetRow)
                for col in range(cols):
                    pdfCol = _pdf(radiusCol, col - radiusCol + offsetCol)
                    weights[index] = pdfCol * pdfRow
                    index += 1
            mx = 0.0
            for v in weights:
                if v > mx:
                    mx = float(v)
            return weights / f64(mx)

    def _spatial(self, i):
        ppc = self.ppc
        if i <= ppc // 2:
            w1 = (i + ppc / 2.0) / ppc
            return 1.0 - w1, w1, 0.0
        w2 = (i - ppc / 2.0) / ppc
        return 0.0, 1.0 - w2, w2

    def add_to_histogram(self, hist, cellX, cellY, orientationIndex, magnitude):
        """addToHistogram :330-339"""
        if cellX < 0 or cellX >= self.cbx:
            return
        if cellY < 0 or cellY >= self.cby:
            return
        hist[(cellY * self.cbx + cellX) * self.bins + orientationIndex] += magnitude

    def compute_cell_histogram(self, findex, magnitude, hist, pixelX0, pixelY0, cellX, cellY, stats=None):
        """computeCellHistogram :237-321 as written; findex = orientation / angleBinSize (float), magnitude a double per pixel"""
        bins, ppc, cbx = self.bins, self.ppc, self.cbx
        add = self.add_to_histogram
        for i in range(ppc):
            indexBlock = (cellY * ppc + i) * ppc * cbx + cellX * ppc
            sy = self._spatial(i)
            for j in range(ppc):
                sx = self._spatial(j)
                if stats is not None:
                    stats["splitLow" if i <= ppc // 2 else "splitHigh"] += 1
                findex0 = findex[pixelY0 + i, pixelX0 + j]
                m = float(magnitude[pixelY0 + i, pixelX0 + j])
                m *= float(self.weights[indexBlock + j])
                index0 = int(findex0)
                oriWeight1 = float(f32(findex0 - f32(index0)))
                index0 %= bins
                index1 = (index0 + 1) % bins
                for b in range(3):
                    for a in range(3):
                        add(hist, cellX + a - 1, cellY + b - 1, index0, (1.0 - oriWeight1) * m * sx[a] * sy[b])
                        add(hist, cellX + a - 1, cellY + b - 1, index1, oriWeight1 * m * sx[a] * sy[b])

    def std_descriptor_raw(self, findex, sumsq, x, y, stats=None):
        """process :209-222 for the block at (x, y), before the normalisation"""
        hist = [0.0] * self.dof
        magnitude = np.sqrt(np.asarray(sumsq).astype(f64))   # Math.sqrt of the widened float sum (IEEE: one correct rounding)
        for cellY in range(self.cby):
            for cellX in range(self.cbx):
                self.compute_cell_histogram(findex, magnitude, hist, x + cellX * self.ppc, y + cellY * self.ppc, cellX, cellY, stats)
        return np.array(hist, f64)

    def std_descriptor_raw_gather(self, findex, sumsq, x, y):
        """the same, one element at a time: the cells next to the element's in row-major order, their pixels in raster order, contributions with
        a zero spatial weight (+0.0 in the reference) skipped"""
        bins, ppc, cbx, cby = self.bins, self.ppc, self.cbx, self.cby
        out = np.zeros(self.dof, f64)
        spatial = [self._spatial(i) for i in range(ppc)]
        for e in range(self.dof):
            tcell, bin_ = divmod(e, bins)
            ty, tx = divmod(tcell, cbx)
            acc = 0.0
            for sy in range(cby):
                for sx in range(cbx):
                    a, d = tx - sx, ty - sy
                    if a < -1 or a > 1 or d < -1 or d > 1:
                        continue
                    for i in range(ppc):
                        wy = spatial[i][d + 1]
                        if wy == 0:
                            continue
                        for j in range(ppc):
                            wx = spatial[j][a + 1]
                            if wx == 0:
                                continue
                            py, px = y + sy * ppc + i, x + sx * ppc + j
                            findex0 = findex[py, px]
                            index0 = int(findex0)
                            oriWeight1 = float(f32(findex0 - f32(index0)))
                            index0 %= bins
                            index1 = (index0 + 1) % bins
                            magnitude = math.sqrt(float(sumsq[py, px])) * float(self.weights[(sy * ppc + i) * ppc * cbx + sx * ppc + j])
                            if index0 == bin_:
                                acc += (1.0 - oriWeight1) * magnitude * wx * wy
                            if index1 == bin_:
                                acc += oriWeight1 * magnitude * wx * wy
            out[e] = acc
        return out

    # ---- a frame ----
    def process(self, img, stats=None):
        """-> dict(xy int32 [n, 2], desc float64 [n, dof], cells float32 [cellRows, cellCols, bins] or None, perRow, perCol)"""
        dx, dy = gradient_f32(img)
        h, w = dx.shape
        findex, sumsq = self.pixel_features(dx, dy, stats)
        perRow, perCol, locs = self.layout(w, h)
        cells = self.cell_histograms(findex, sumsq) if self.fast else None
        desc = []
        for (x, y) in locs:
            if self.fast:
                desc.append(self.block_descriptor(cells, y // self.ppc, x // self.ppc, stats))
            else:
                desc.append(normalize_descriptor(self.std_descriptor_raw(findex, sumsq, x, y, stats), 0.2, stats))
        return dict(xy=np.array(locs, np.int32).reshape(-1, 2), desc=np.array(desc, f64).reshape(len(locs), self.dof), cells=cells, perRow=perRow, perCol=perCol)

    def descriptors_in_region(self, n, cellCols, pixelX0, pixelY0, pixelX1, pixelY1):
        """getDescriptorsInRegion :129-143 -> indices into the list of n descriptors (the reference's indexing, y * cellCols included)"""
        gridX0 = int(math.ceil(pixelX0 / float(self.ppc)))
        gridY0 = int(math.ceil(pixelY0 / float(self.ppc)))
        gridX1 = pixelX1 // self.ppc - self.cbx
        gridY1 = pixelY1 // self.ppc - self.cby
        out = []
        for y in range(gridY0, gridY1 + 1):
            index = y * cellCols + gridX0
            for x in range(gridX0, gridX1 + 1):
                if index < 0 or index >= n:
                    raise IndexError(index)
                out.append(index)
                index += 1
        return out


def _pdf(sigma, sample):
    """UtilGaussian.computePDF(0, sigma, sample); sigma 0 (a side of one pixel) gives NaN as the arithmetic does"""
    if sigma == 0:
        return math.nan   # -d*d / 0 is NaN or -inf, and exp of either over 0 is NaN
    return sd.pdf(float(sigma), float(sample))


# ---------------- dense SIFT ----------------
class DenseSift:
    def __init__(self, widthSubregion=4, widthGrid=4, numHistogramBins=8, weightingSigmaFraction=0.5, maxDescriptorElementValue=0.2, periodX=6.0, periodY=6.0):
        self.d = sd.Describe(widthSubregion, widthGrid, numHistogramBins, 1.0, weightingSigmaFraction, maxDescriptorElementValue)
        self.periodX, self.periodY = float(periodX), float(periodY)
        self.dof = self.d.dof
        self.widthPixels = self.d.ws * self.d.wg

    def args(self):
        return (self.d.ws, self.d.wg, self.d.nb)

    def layout(self, width, height):
        """process :120-146 -> (numX, numY, [(x, y)]); ZeroDivisionError where Java throws ArithmeticException"""
        radius = self.widthPixels // 2
        X0, X1, Y0, Y1 = radius, width - radius, radius, height - radius
        numX, numY = int((X1 - X0) / self.periodX), int((Y1 - Y0) / self.periodY)
        locs = []
        for i in range(numY):
            y = _jdiv((Y1 - Y0) * i, numY - 1) + Y0
            for j in range(numX):
                x = _jdiv((X1 - X0) * j, numX - 1) + X0
                locs.append((x, y))
        if not locs:
            return 0, 0, []
        return numX, numY, locs

    def precompute_angles(self, dx, dy, stats=None):
        """precomputeAngles :151-164"""
        h, w = dx.shape
        angle = np.zeros((h, w), f64)
        for y in range(h):
            for x in range(w):
                angle[y, x] = _a2(dy[y, x], dx[y, x])
        if stats is not None:
            stats["pixels"] += h * w
            stats["axisPos"] += int(((dx == 0) & (dy >= 0)).sum())
            stats["axisNeg"] += int(((dx == 0) & (dy < 0)).sum())
        magnitude = np.sqrt((dx * dx + dy * dy).astype(f64)).astype(f32)
        return sd.domain2pi(angle), magnitude

    def _window(self, angle, magnitude, cx, cy):
        wp, radius = self.widthPixels, self.widthPixels // 2
        a = angle[cy - radius:cy - radius + wp, cx - radius:cx - radius + wp].reshape(-1)
        m = magnitude[cy - radius:cy - radius + wp, cx - radius:cx - radius + wp].reshape(-1)
        assert len(a) == wp * wp, "window outside the image"
        weight = (self.d.gaussianWeight * m).astype(f32)
        i, j = np.mgrid[0:wp, 0:wp]
        subY, subX = i.reshape(-1).astype(f32) / f32(self.d.ws), j.reshape(-1).astype(f32) / f32(self.d.ws)
        return weight, subX, subY, a

    def descriptor_raw(self, angle, magnitude, cx, cy):
        """computeDescriptor :172-195 before the normalisation: every element's sum over the samples in raster order (the vector form of
        sift_describe_ref.Describe.compute_raw)"""
        d = self.d
        weight, subX, subY, a = self._window(angle, magnitude, cx, cy)
        grid = np.arange(d.wg).astype(f32)
        wy = 1.0 - np.abs(subY[:, None] - grid[None, :]).astype(f64)
        wx = 1.0 - np.abs(subX[:, None] - grid[None, :]).astype(f64)
        wh = 1.0 - sd.angle_dist(a[:, None], (np.arange(d.nb) * d.binWidth)[None, :]) / d.binWidth
        v = ((weight.astype(f64)[:, None, None, None] * wx[:, None, :, None]) * wy[:, :, None, None]) * wh[:, None, None, :]
        ok = (wy > 0)[:, :, None, None] & (wx > 0)[:, None, :, None] & (wh > 0)[:, None, None, :]
        v = np.where(ok, v, 0.0).reshape(len(weight), -1)
        return np.cumsum(np.vstack([np.zeros((1, v.shape[1])), v]), axis=0)[-1]

    def descriptor_raw_loops(self, angle, magnitude, cx, cy):
        """the same with the reference's loops: trilinearInterpolation per sample"""
        weight, subX, subY, a = self._window(angle, magnitude, cx, cy)
        out = np.zeros(self.dof)
        for s in range(len(weight)):
            self.d.trilinear(weight[s], subX[s], subY[s], float(a[s]), out)
        return out

    def descriptor_raw_gather(self, angle, magnitude, cx, cy):
        """the same, one element at a time over the (2 * widthSubregion - 1)^2 samples that can reach it, in raster order"""
        d = self.d
        ws, wg, nb, sw = d.ws, d.wg, d.nb, self.widthPixels
        weight, subX, subY, a = self._window(angle, magnitude, cx, cy)
        out = np.zeros(self.dof)
        for e in range(self.dof):
            k, ij = e % nb, e // nb
            j, i = ij % wg, ij // wg
            angleBin = k * d.binWidth
            acc = 0.0
            for sy in range(max(ws * (i - 1), 0), min(ws * (i + 1), sw - 1) + 1):
                wy = 1.0 - float(np.abs(subY[sy * sw] - f32(i)))
                if wy <= 0:
                    continue
                for sx in range(max(ws * (j - 1), 0), min(ws * (j + 1), sw - 1) + 1):
                    wx = 1.0 - float(np.abs(subX[sx] - f32(j)))
                    if wx <= 0:
                        continue
                    whist = 1.0 - float(sd.angle_dist(float(a[sy * sw + sx]), angleBin)) / d.binWidth
                    if whist <= 0:
                        continue
                    acc += float(weight[sy * sw + sx]) * wx * wy * whist
            out[e] = acc
        return out

    def process(self, img, u8=False, stats=None):
        """-> dict(xy int32 [n, 2] (window centres), desc float64 [n, dof], perRow, perCol)"""
        dx, dy = gradient_s16(img) if u8 else gradient_f32(img)
        h, w = dx.shape
        numX, numY, locs = self.layout(w, h)
        angle, magnitude = self.precompute_angles(dx, dy, stats)
        desc = [normalize_descriptor(self.descriptor_raw(angle, magnitude, x, y), self.d.maxValue, stats) for (x, y) in locs]
        return dict(xy=np.array(locs, np.int32).reshape(-1, 2), desc=np.array(desc, f64).reshape(len(locs), self.dof), perRow=numX, perCol=numY)


def _jdiv(a, b):
    """Java int division: toward zero; b == 0 raises"""
    if b == 0:
        raise ZeroDivisionError("/ by zero")
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _a2(y, x):
    """Math.atan2(float, float) of one pixel: the C library's, the zero-argument cases as the Java specification fixes them"""
    y, x = float(y), float(x)
    if x == 0.0 or y == 0.0:
        return float(sd.atan2(y, x))
    return math.atan2(y, x)
