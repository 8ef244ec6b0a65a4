"""CompleteSift restated in numpy float32 / float64 in the reference's loop order: OrientationHistogramSift
(F:alg/feature/orientation/OrientationHistogramSift.java:135-309), DescribePointSift / DescribeSiftCommon
(F:alg/feature/describe/DescribePointSift.java:105-165, DescribeSiftCommon.java:60-131), CompleteSift.detectFeatures / handleDetection
(F:alg/feature/detdesc/CompleteSift.java:97-134), InterpolateArray, UtilFeature.normalizeL2, FastHessianFeatureDetector.polyPeak(double),
FactoryKernelGaussian.gaussian2D_F32(sigma, radius, false, false), KernelMath.maxAbs / divide.

The detector, the scale space and the gradient's interior come from sift_ref and the oracle binding (orc.gradient("three", ...)); the frame of
the gradient (BorderType.EXTENDED) is written out here.  Per-sample values are computed for a whole window at once, element by element with
the reference's expressions; every sum that the reference takes over samples is taken in raster order (np.cumsum along the sample axis is
sequential; a sample outside a bin contributes +0.0, which changes no partial sum).  UtilAngle.domain2PI / dist / bound are georegression's,
restated from their contract; Math.exp / sqrt / atan2 / sin / cos are the C library's (unpinned against Java's to the last ulp).

Statistics for the preconditions of the GPU tests are collected into the dict `stats` (new_stats())."""
import math

import numpy as np

import sift_ref as sr
from oracle import pyoracle as orc

f32, f64 = np.float32, np.float64
PI2 = 2.0 * math.pi


# ---------------- georegression UtilAngle, from its contract ----------------
def domain2pi(a):
    a = np.asarray(a, f64)
    return np.where(a < 0, a + PI2, a)


def angle_dist(a, b):
    d = np.asarray(a, f64) - b
    d = np.where(d > math.pi, d - PI2, np.where(d < -math.pi, PI2 + d, d))
    return np.abs(d)


def bound(a):
    a = math.fmod(a, PI2)
    if a > math.pi:
        return a - PI2
    if a < -math.pi:
        return a + PI2
    return a


def atan2(y, x):
    """Math.atan2, elementwise.  The C library follows the same special-case table as Java's specification (C99 F.9.1.4); the cases with a
    zero argument are selected explicitly all the same, as the kernels do"""
    y, x = np.asarray(y, f64), np.asarray(x, f64)
    with np.errstate(all="ignore"):
        r = np.arctan2(y, x)
    pi_y = np.copysign(math.pi, y)
    r = np.where((y == 0) & (x > 0), y, r)
    r = np.where((y == 0) & (x < 0), pi_y, r)
    r = np.where((x == 0) & (y > 0), math.pi / 2, r)
    r = np.where((x == 0) & (y < 0), -math.pi / 2, r)
    r = np.where((x == 0) & (y == 0), np.where(np.signbit(x), pi_y, y), r)
    return r


def poly_peak(lower, middle, upper):
    """FastHessianFeatureDetector.polyPeak(double) :352-366"""
    a = 0.5 * lower - middle + 0.5 * upper
    b = 0.5 * upper - 0.5 * lower
    if a == 0.0:
        return 0.0
    return -b / (2.0 * a)


# ---------------- the gradient of CompleteSift: FactoryDerivative.three(GrayF32, null), EXTENDED border ----------------
def gradient_three(img):
    """-> derivX, derivY float32.  Interior: the oracle's GradientThree (checked against (a - b) * 0.5f); frame: the generic border convolution
    total = 0; total += ext(x+k-1) * kernel[k] with kernel (-0.5, 0, 0.5) (ConvolveJustBorder_General_SB), and the unrolled three taps
    total = a*k0; total += b*k1; total += c*k2 on the second row / column (DerivativeHelperFunctions.processBorder*)"""
    img = np.ascontiguousarray(img, f32)
    h, w = img.shape
    gx, gy = orc.gradient("three", orc.Gray.from_array(img), False)
    gx, gy = gx.array().copy(), gy.array().copy()
    xs, ys = np.arange(w), np.arange(h)
    xl, xr = np.clip(xs - 1, 0, w - 1), np.clip(xs + 1, 0, w - 1)
    yt, yb = np.clip(ys - 1, 0, h - 1), np.clip(ys + 1, 0, h - 1)
    k0, k1, k2 = f32(-0.5), f32(0), f32(0.5)
    bx = ((f32(0) + img[:, xl] * k0) + img * k1) + img[:, xr] * k2
    by = ((f32(0) + img[yt, :] * k0) + img * k1) + img[yb, :] * k2
    assert bx.dtype == f32 and by.dtype == f32
    inner = np.zeros((h, w), bool)
    inner[1:h - 1, 1:w - 1] = True
    fast_x = (img[:, xr] - img[:, xl]) * f32(0.5)
    fast_y = (img[yb, :] - img[yt, :]) * f32(0.5)
    assert np.array_equal(gx[inner].view(np.uint32), fast_x[inner].view(np.uint32)) and np.array_equal(gy[inner].view(np.uint32), fast_y[inner].view(np.uint32))
    dx, dy = np.where(inner, gx, bx), np.where(inner, gy, by)
    return np.ascontiguousarray(dx, f32), np.ascontiguousarray(dy, f32)


def new_stats():
    return dict(binMargin=math.inf, axisSamples=0, oriSamples=0, pixelMargin=math.inf, thresholdMargin=math.inf, inside=0, outside=0, negativeCoordinate=0,
                anglesPerDetection={}, maxR=0, detections=0, features=0)


# ---------------- OrientationHistogramSift ----------------
class Orientation:
    def __init__(self, histogramSize=36, sigmaEnlarge=2.0):
        self.N, self.sigmaEnlarge = int(histogramSize), float(sigmaEnlarge)
        self.histAngleBin = 2.0 * math.pi / self.N
        self.step = 0.1
        self.table = np.array([math.exp(-0.5 * (i * self.step)) for i in range(int(4 * 4 / self.step))], f64)
        self.mag, self.hx, self.hy = (np.zeros(self.N) for _ in range(3))
        self.angles, self.peakAngle = [], 0.0

    def compute_weight(self, deltaX, deltaY, sigma):
        """computeWeight :298-309 with InterpolateArray.interpolate, elementwise"""
        deltaX, deltaY = np.asarray(deltaX, f64), np.asarray(deltaY, f64)
        d = ((deltaX * deltaX + deltaY * deltaY) / (sigma * sigma)) / self.step
        index = np.minimum(d, 1e9).astype(np.int64)
        ok = (d >= 0) & (index < len(self.table) - 1)
        idx = np.where(ok, index, 0)
        w = d - idx
        value = self.table[idx] * (1.0 - w) + self.table[idx + 1] * w
        return np.where(ok, value, 0.0)

    def compute_histogram(self, derivX, derivY, c_x, c_y, sigma, stats=None):
        """computeHistogram :155-201"""
        h, w = derivX.shape
        r = int(math.ceil(sigma * self.sigmaEnlarge))
        x0, y0, x1, y1 = max(c_x - r, 0), max(c_y - r, 0), min(c_x + r + 1, w), min(c_y + r + 1, h)
        dx = np.ascontiguousarray(derivX[y0:y1, x0:x1], f32).reshape(-1)
        dy = np.ascontiguousarray(derivY[y0:y1, x0:x1], f32).reshape(-1)
        ys, xs = np.mgrid[y0:y1, x0:x1]
        magnitude = np.sqrt((dx * dx + dy * dy).astype(f64))
        theta = domain2pi(atan2(dy, dx))
        weight = self.compute_weight((xs - c_x).reshape(-1), (ys - c_y).reshape(-1), sigma)
        q = theta / self.histAngleBin
        hbin = q.astype(np.int64) % self.N
        n = len(dx)
        out = []
        for v in (magnitude * weight, dx.astype(f64) * weight, dy.astype(f64) * weight):
            M = np.zeros((n + 1, self.N))
            M[np.arange(1, n + 1), hbin] = v
            out.append(np.cumsum(M, axis=0)[-1])
        self.mag, self.hx, self.hy = out
        if stats is not None:
            stats["maxR"] = max(stats["maxR"], r)
            stats["oriSamples"] += n
            axis = (dx == 0) | (dy == 0)
            generic = ~axis & (np.abs(dx) != np.abs(dy))
            stats["axisSamples"] += int(axis.sum())
            if generic.any():
                stats["binMargin"] = min(stats["binMargin"], float(np.abs(q[generic] - np.rint(q[generic])).min()))

    def find_histogram_peaks(self, stats=None):
        """findHistogramPeaks :206-249"""
        N, mag = self.N, self.mag
        peaks, self.angles, self.peakAngle = [], [], 0.0
        largest, largestIndex = 0.0, -1
        before, current = mag[N - 2], mag[N - 1]
        for i in range(N):
            after = mag[i]
            if current > before and current > after:
                ci = N + i - 1 if i - 1 < 0 else (i - 1) % N
                peaks.append(ci)
                if current > largest:
                    largest, largestIndex = current, ci
            before, current = current, after
        if largestIndex < 0:
            return
        threshold = largest * 0.8
        for index in peaks:
            current = mag[index]
            if stats is not None and index != largestIndex:
                stats["thresholdMargin"] = min(stats["thresholdMargin"], abs(float(current) - threshold) / threshold)
            if current >= threshold:
                angle = self.compute_angle(index)
                self.angles.append(angle)
                if index == largestIndex:
                    self.peakAngle = angle

    def compute_angle(self, index1):
        N = self.N
        index0 = N + index1 - 1 if index1 - 1 < 0 else (index1 - 1) % N
        index2 = (index1 + 1) % N
        offset = poly_peak(float(self.mag[index0]), float(self.mag[index1]), float(self.mag[index2]))
        return self.interpolate_angle(index0, index1, index2, offset)

    def interpolate_angle(self, index0, index1, index2, offset):
        angle1 = float(atan2(self.hy[index1], self.hx[index1]))
        other = index0 if offset < 0 else index2
        delta = float(angle_dist(float(atan2(self.hy[other], self.hx[other])), angle1))
        return bound(angle1 + delta * offset)

    def process(self, derivX, derivY, c_x, c_y, sigma, stats=None):
        x, y = int(c_x + 0.5), int(c_y + 0.5)
        self.compute_histogram(derivX, derivY, x, y, sigma, stats)
        self.find_histogram_peaks(stats)
        return list(self.angles)


# ---------------- DescribeSiftCommon / DescribePointSift ----------------
def pdf(sigma, sample):
    """UtilGaussian.computePDF(0, sigma, sample) (ddogleg), as the library's tables restate it"""
    return math.exp(-sample * sample / (2.0 * sigma * sigma)) / (sigma * math.sqrt(2.0 * math.pi))


def gaussian_weight_kernel(sigma, radius):
    """createGaussianWeightKernel :103-108"""
    k1 = np.array([pdf(sigma, i - 0.5) for i in range(radius, -radius, -1)], f64).astype(f32)
    ker = (k1[:, None] * k1[None, :]).astype(f32).reshape(-1)
    return ker / np.abs(ker).max()


class Describe:
    def __init__(self, widthSubregion=4, widthGrid=4, numHistogramBins=8, sigmaToPixels=1.0, weightingSigmaFraction=0.5, maxDescriptorElementValue=0.2):
        self.ws, self.wg, self.nb = int(widthSubregion), int(widthGrid), int(numHistogramBins)
        self.sigmaToPixels, self.maxValue = float(sigmaToPixels), float(maxDescriptorElementValue)
        self.binWidth = 2.0 * math.pi / self.nb
        window = self.ws * self.wg
        self.gaussianWeight = gaussian_weight_kernel(window * float(weightingSigmaFraction), window // 2)
        assert self.gaussianWeight.dtype == f32

    @property
    def dof(self):
        return self.wg * self.wg * self.nb

    def canonical_radius(self):
        return self.wg * self.ws // 2

    def trilinear(self, weight, sampleX, sampleY, angle, descriptor):
        """trilinearInterpolation :113-131, one sample, the reference's loops"""
        weight, sampleX, sampleY = f32(weight), f32(sampleX), f32(sampleY)
        for i in range(self.wg):
            wy = 1.0 - float(np.abs(sampleY - f32(i)))
            if wy <= 0:
                continue
            for j in range(self.wg):
                wx = 1.0 - float(np.abs(sampleX - f32(j)))
                if wx <= 0:
                    continue
                for k in range(self.nb):
                    wh = 1.0 - float(angle_dist(angle, k * self.binWidth)) / self.binWidth
                    if wh <= 0:
                        continue
                    descriptor[(i * self.wg + j) * self.nb + k] += float(weight) * wx * wy * wh

    def _samples(self, derivX, derivY, c_x, c_y, sigma, orientation, stats):
        h, w = derivX.shape
        c, s = math.cos(orientation), math.sin(orientation)
        sw = self.wg * self.ws
        sampleRadius = float(sw // 2)
        sampleToPixels = sigma * self.sigmaToPixels
        sy, sx = np.mgrid[0:sw, 0:sw]
        sy, sx = sy.reshape(-1), sx.reshape(-1)
        subY, subX = sy.astype(f32) / f32(self.ws), sx.astype(f32) / f32(self.ws)
        y = sampleToPixels * (sy - sampleRadius)
        x = sampleToPixels * (sx - sampleRadius)
        fx = x * c - y * s + c_x + 0.5
        fy = x * s + y * c + c_y + 0.5
        px, py = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)
        inb = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        pxc, pyc = np.where(inb, px, 0), np.where(inb, py, 0)
        dX, dY = derivX[pyc, pxc].astype(f32), derivY[pyc, pxc].astype(f32)
        adjDX = c * dX.astype(f64) + s * dY.astype(f64)
        adjDY = -s * dX.astype(f64) + c * dY.astype(f64)
        angle = domain2pi(atan2(adjDY, adjDX))
        weightGradient = np.sqrt((dX * dX + dY * dY).astype(f64)).astype(f32)
        weight = self.gaussianWeight * weightGradient
        assert weight.dtype == f32
        if stats is not None:
            stats["inside"] += int(inb.sum())
            stats["outside"] += int((~inb).sum())
            stats["negativeCoordinate"] += int((((fx > -1) & (fx < 0)) | ((fy > -1) & (fy < 0))).sum())
            m = min(float(np.abs(fx - np.rint(fx)).min()), float(np.abs(fy - np.rint(fy)).min()))
            stats["pixelMargin"] = min(stats["pixelMargin"], m)
        return inb, weight, subX, subY, angle

    def compute_raw(self, derivX, derivY, c_x, c_y, sigma, orientation, stats=None):
        """computeRawDescriptor :118-165: all samples at once, the sum over samples in raster order for every element"""
        inb, weight, subX, subY, angle = self._samples(derivX, derivY, c_x, c_y, sigma, orientation, stats)
        grid = np.arange(self.wg).astype(f32)
        wy = 1.0 - np.abs(subY[:, None] - grid[None, :]).astype(f64)                                  # [ns, i]
        wx = 1.0 - np.abs(subX[:, None] - grid[None, :]).astype(f64)                                  # [ns, j]
        wh = 1.0 - angle_dist(angle[:, None], (np.arange(self.nb) * self.binWidth)[None, :]) / self.binWidth   # [ns, k]
        v = ((weight.astype(f64)[:, None, None, None] * wx[:, None, :, None]) * wy[:, :, None, None]) * wh[:, None, None, :]
        ok = inb[:, None, None, None] & (wy > 0)[:, :, None, None] & (wx > 0)[:, None, :, None] & (wh > 0)[:, None, None, :]
        v = np.where(ok, v, 0.0).reshape(len(weight), -1)
        return np.cumsum(np.vstack([np.zeros((1, v.shape[1])), v]), axis=0)[-1]

    def compute_raw_loops(self, derivX, derivY, c_x, c_y, sigma, orientation):
        """the same with the reference's loops (slow: the witness that compute_raw keeps their order)"""
        inb, weight, subX, subY, angle = self._samples(derivX, derivY, c_x, c_y, sigma, orientation, None)
        d = np.zeros(self.dof)
        for i in range(len(weight)):
            if inb[i]:
                self.trilinear(weight[i], subX[i], subY[i], float(angle[i]), d)
        return d

    @staticmethod
    def normalize_l2(d):
        """UtilFeature.normalizeL2 :101-114"""
        norm = 0.0
        for v in d:
            norm += float(v) * float(v)
        if norm == 0:
            return d
        return d / math.sqrt(norm)

    def normalize(self, d, maxValue=None):
        """normalizeDescriptor :84-98"""
        maxValue = self.maxValue if maxValue is None else maxValue
        d = self.normalize_l2(np.array(d, f64))
        d = np.where(d > maxValue, maxValue, d)
        return self.normalize_l2(d)

    def process(self, derivX, derivY, c_x, c_y, sigma, orientation, stats=None):
        return self.normalize(self.compute_raw(derivX, derivY, c_x, c_y, sigma, orientation, stats))


# ---------------- CompleteSift ----------------
def complete(ss, det, ori, desc, img, stats=None, space=None):
    """CompleteSift.process -> dict(x, y, scale, orientation float64 [n], white uint8 [n], desc float64 [n, dof], anglesPerDetection int [detections]),
    in the reference's order: detection order, then the order of the angle list"""
    space = space if space is not None else sr.scale_space(ss, img)
    xy, scale, white, where = sr.detect(ss, det, None, None, space)
    grads = {}
    out = dict(x=[], y=[], scale=[], orientation=[], white=[], desc=[], anglesPerDetection=[])
    by_octave = {o: octv for o, octv, _ in space}
    for i in range(len(scale)):
        o, j = int(where[i, 0]), int(where[i, 1])
        if (o, j) not in grads:
            grads[(o, j)] = gradient_three(by_octave[o][j])
        dX, dY = grads[(o, j)]
        p2i = math.pow(2.0, o)
        localX, localY, localSigma = xy[i, 0] / p2i, xy[i, 1] / p2i, scale[i] / p2i
        angles = ori.process(dX, dY, localX, localY, localSigma, stats)
        out["anglesPerDetection"].append(len(angles))
        for a in angles:
            out["desc"].append(desc.process(dX, dY, localX, localY, localSigma, a, stats))
            out["x"].append(xy[i, 0]); out["y"].append(xy[i, 1]); out["scale"].append(scale[i]); out["white"].append(white[i]); out["orientation"].append(a)
    n = len(out["x"])
    res = dict(x=np.array(out["x"], f64), y=np.array(out["y"], f64), scale=np.array(out["scale"], f64), orientation=np.array(out["orientation"], f64),
               white=np.array(out["white"], np.uint8), desc=np.array(out["desc"], f64).reshape(n, desc.dof),
               anglesPerDetection=np.array(out["anglesPerDetection"], np.int64))
    if stats is not None:
        stats["detections"], stats["features"] = len(scale), n
        for k in out["anglesPerDetection"]:
            stats["anglesPerDetection"][k] = stats["anglesPerDetection"].get(k, 0) + 1
    return res
