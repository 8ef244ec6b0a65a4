"""A numpy restatement of the reference's Hough line detectors (single-threaded classes), line by line, with float32 and float64 scalars
exactly where Java has float and double.  F: = main/boofcv-feature/src/main/java/boofcv, I: = main/boofcv-ip/src/main/java/boofcv.

  prewitt                      I:alg/filter/derivative/GradientPrewitt.java:80-142, impl/GradientPrewitt_Shared.java, the generic border convolution
  intensity_abs                F:alg/feature/detect/edge/impl/ImplGradientToEdgeFeatures.java:63-81, 151-169
  nonmax_crude4                F:alg/feature/detect/edge/impl/ImplEdgeNonMaxSuppressionCrude.java inner4 :50-115, border4 :155-242
  HoughParametersPolar / FootOfNorm, hough_binary, hough_gradient      F:alg/feature/detect/line/*.java
  nonmax_relaxed               F:alg/feature/detect/extract/NonMaxBlock.java:69-94, NonMaxBlockSearchRelaxed.java:69-98, 227-251
  MeanShiftPeak                F:alg/feature/detect/peak/MeanShiftPeak.java:103-160 over ImplBilinearPixel_F32 with ImageBorderValue(0)
  ImageLinePruneMerge          F:alg/feature/detect/line/ImageLinePruneMerge.java, LineImageOps.convert
  detect_binary / detect_gradient   HoughBinary_to_DetectLine.detect, HoughGradient_to_DetectLine.detect

Images are [H,W] arrays.  The vectorised parts are element-wise float32 / float64 array operations (numpy does not contract a*b+c), so
each element is what the scalar Java loop computes; every order-dependent float sum is a scalar loop.  georegression / ddogleg are not in
the reference tree: CachedSineCosine_F32, UtilAngle, Intersection2D_F32, Distance2D_F32 and UtilGaussian.computePDF are restated from
their documented behaviour, as in boofcv_amd/lines.py (DESIGN.md lists them as unpinned)."""
import functools
import math

import numpy as np

import fast_ref
import threshold_ref

F = np.float32
D = np.float64
FLOAT_MAX = np.finfo(np.float32).max
INT_MAX, INT_MIN = 2147483647, -2147483648


def java_f2i(v):
    """Java's (int) of float / double values (array): NaN -> 0, saturating, truncation toward zero"""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        t = np.trunc(v.astype(D))
        out = np.where(np.isnan(t), 0.0, np.clip(t, INT_MIN, INT_MAX))
    return out.astype(np.int64).astype(np.int32)


def wrap_i32(v):
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


# ---------------- gradient, edge features ----------------
def _padded(img, border):
    """the image with one pixel around it as the border policy reads it: 1 = ImageBorderValue(0), 2 = EXTENDED"""
    return np.pad(img, 1, mode="edge") if border == 2 else np.pad(img, 1, mode="constant")


def prewitt(img, border, dx=None, dy=None):
    """border 0: frame untouched (dx, dy keep what they hold), 1: value 0, 2: EXTENDED.  uint8 -> int16, float32 -> float32"""
    h, w = img.shape
    u8 = img.dtype == np.uint8
    dt = np.int16 if u8 else F
    dx = np.zeros((h, w), dt) if dx is None else dx.copy()
    dy = np.zeros((h, w), dt) if dy is None else dy.copy()
    a = img.astype(np.int32) if u8 else img.astype(F)
    if h > 2 and w > 2:
        a11, a12, a13 = a[:-2, :-2], a[:-2, 1:-1], a[:-2, 2:]
        a21, a23 = a[1:-1, :-2], a[1:-1, 2:]
        a31, a32, a33 = a[2:, :-2], a[2:, 1:-1], a[2:, 2:]
        wv = a33 - a11
        v = a31 - a13
        dy[1:-1, 1:-1] = (a32 + wv + v - a12).astype(dt)
        dx[1:-1, 1:-1] = (a23 + wv - v - a21).astype(dt)
    if border:
        p = _padded(a, border)
        kx = [-1, 0, 1, -1, 0, 1, -1, 0, 1]
        ky = [-1, -1, -1, 0, 0, 0, 1, 1, 1]
        tx = np.zeros((h, w), np.int32 if u8 else F)
        ty = np.zeros((h, w), np.int32 if u8 else F)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(3):
                for j in range(3):
                    win = p[i:i + h, j:j + w]
                    tx = tx + win * (kx[i * 3 + j] if u8 else F(kx[i * 3 + j]))   # total += get(x+j, y+i) * k, row-major kernel order
                    ty = ty + win * (ky[i * 3 + j] if u8 else F(ky[i * 3 + j]))
        frame = np.ones((h, w), bool)
        frame[1:-1, 1:-1] = False
        dx[frame] = tx.astype(dt)[frame]
        dy[frame] = ty.astype(dt)[frame]
    return dx, dy


def intensity_abs(dx, dy):
    if dx.dtype == np.int16:
        return (np.abs(dx.astype(np.int32)) + np.abs(dy.astype(np.int32))).astype(F)
    return (np.abs(dx) + np.abs(dy)).astype(F)


def nonmax_crude4(intensity, dx, dy):
    """inner4 and border4, pixel by pixel"""
    h, w = intensity.shape
    out = np.zeros((h, w), F)

    def get(x, y):   # ImageBorderValue(0)
        return intensity[y, x] if 0 <= x < w and 0 <= y < h else F(0)

    for y in range(h):
        for x in range(w):
            sx = 1 if dx[y, x] > 0 else -1
            sy = 1 if dy[y, x] > 0 else -1
            middle = intensity[y, x]
            left, right = get(x - sx, y - sy), get(x + sx, y + sy)
            out[y, x] = F(0) if (left > middle or right > middle) else middle
    return out


# ---------------- georegression / ddogleg restatements ----------------
def cached_sine_cosine(min_angle, max_angle, size):
    lo, hi = F(min_angle), F(max_angle)
    c, s = np.zeros(size, F), np.zeros(size, F)
    with np.errstate(all="ignore"):
        for i in range(size):
            angle = F(F(F(hi - lo) * F(i)) / F(size - 1)) + lo
            c[i] = F(math.cos(float(angle))) if np.isfinite(angle) else F(np.nan)
            s[i] = F(math.sin(float(angle))) if np.isfinite(angle) else F(np.nan)
    return c, s


def weight_gaussian(radius):
    """WeightPixelGaussian_F32.setRadius(radius, radius, true): gaussian2D_F32((float)sigmaForRadius(radius, 0), radius, true, true)"""
    sigma = float(F((radius * 2.0 + 1.0) / (5.0 + 0.8 * 0)))
    k1 = [F(math.exp(-float(i) * float(i) / (2.0 * sigma * sigma)) / (sigma * math.sqrt(2.0 * math.pi))) for i in range(radius, -radius - 1, -1)]
    k2 = [F(a * b) for a in k1 for b in k1]
    total = F(0)
    for v in k2:
        total = F(total + v)
    return np.array([F(v / total) for v in k2], F)


# ---------------- parameterisations ----------------
class Polar:
    def __init__(self, range_resolution, num_bins_angle):
        self.range_resolution, self.num_bins_angle = float(range_resolution), int(num_bins_angle)
        self.c, self.s = cached_sine_cosine(0.0, F(math.pi), self.num_bins_angle)

    def initialize(self, width, height):
        self.origin_x, self.origin_y = width // 2, height // 2
        prod = int(wrap_i32(self.origin_x * self.origin_x + self.origin_y * self.origin_y))
        with np.errstate(all="ignore"):
            self.r_max = F(np.sqrt(D(prod)))
            bins = np.ceil(D(self.r_max) / D(self.range_resolution))
        self.num_bins_range = int(java_f2i(bins))
        return self.num_bins_range, self.num_bins_angle   # transform width, height

    def is_transform_valid(self, x, y):
        return True

    def transform_to_line(self, x, y):
        w2 = self.num_bins_range // 2
        with np.errstate(all="ignore"):
            r = F(F(self.r_max * F(F(x) - F(w2))) / F(w2))
        c, s = self.c[int(y)], self.s[int(y)]
        return F(F(r * c) + F(self.origin_x)), F(F(r * s) + F(self.origin_y)), F(-s), c


class FootOfNorm:
    def __init__(self, min_distance_from_origin):
        self.min_distance = int(min_distance_from_origin)

    def initialize(self, width, height):
        self.origin_x, self.origin_y = width // 2, height // 2
        return width, height

    def is_transform_valid(self, x, y):
        return abs(x - self.origin_x) >= self.min_distance or abs(y - self.origin_x) >= self.min_distance   # originX twice, as the reference

    def transform_to_line(self, x, y):
        x, y = F(x), F(y)
        return x, y, F(-F(y - F(self.origin_y))), F(x - F(self.origin_x))

    def parameterize(self, x, y, dx, dy):
        """arrays of edge pixels: int x, y; float32 derivatives -> float32 parameter (x, y)"""
        px, py = (x - self.origin_x).astype(F), (y - self.origin_y).astype(F)
        with np.errstate(all="ignore"):
            v = (px * dx + py * dy) / (dx * dx + dy * dy)
            return v * dx + F(self.origin_x), v * dy + F(self.origin_y)


# ---------------- transforms ----------------
def hough_binary(binary, par):
    """HoughTransformBinary.computeParameters after the fill with 0 -> the GrayF32 transform [numBinsAngle, numBinsRange].  The linear index
    i*stride + col is Java's; an index outside the array is dropped (Java throws)."""
    h, w = binary.shape
    tw, th = par.initialize(w, h)
    counts = np.zeros(tw * th, np.int64)
    ys, xs = np.nonzero(binary)   # raster order
    x, y = (xs - par.origin_x).astype(F), (ys - par.origin_y).astype(F)
    w2 = tw // 2
    for i in range(th):
        p = (x * par.c[i] + y * par.s[i]).astype(D)   # a float sum, widened
        with np.errstate(all="ignore"):
            col = wrap_i32(java_f2i(np.floor(p * D(w2) / D(par.r_max))).astype(np.int64) + w2)
        index = i * tw + col.astype(np.int64)
        index = index[(index >= 0) & (index < tw * th)]
        np.add.at(counts, index, 1)
    assert counts.max(initial=0) <= 1 << 24   # n increments of a float by 1 are exact up to 2^24
    return counts.astype(F).reshape(th, tw)


def gradient_votes(dx, dy, binary, par):
    """the (cell, weight) contributions of HoughTransformGradient.transform in the order Java adds them; cell -1: outside the transform"""
    h, w = binary.shape
    par.initialize(w, h)
    ys, xs = np.nonzero(binary)
    px, py = par.parameterize(xs, ys, dx[ys, xs].astype(F), dy[ys, xs].astype(F))
    x0, y0 = java_f2i(px), java_f2i(py)
    with np.errstate(all="ignore"):
        wx, wy = px - x0.astype(F), py - y0.astype(F)
        one = F(1)
        weights = np.stack([(one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy], axis=1).astype(F)
    x1, y1 = wrap_i32(x0.astype(np.int64) + 1), wrap_i32(y0.astype(np.int64) + 1)
    cx = np.stack([x0, x1, x0, x1], axis=1).astype(np.int64)
    cy = np.stack([y0, y0, y1, y1], axis=1).astype(np.int64)
    inside = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
    cell = np.where(inside, cy * w + cx, -1)
    return cell.reshape(-1), weights.reshape(-1)


def sum_votes(cell, weight, shape, reverse=False):
    """transform.data[index] += amount, one contribution after the other"""
    out = np.zeros(shape[0] * shape[1], F)
    order = range(len(cell) - 1, -1, -1) if reverse else range(len(cell))
    with np.errstate(all="ignore"):
        for k in order:
            c = cell[k]
            if c >= 0:
                out[c] = out[c] + weight[k]
    return out.reshape(shape)


def hough_gradient(dx, dy, binary, par, reverse=False):
    cell, weight = gradient_votes(dx, dy, binary, par)
    return sum_votes(cell, weight, binary.shape, reverse)


# ---------------- relaxed block NMS ----------------
def nonmax_relaxed(img, radius, threshold, border=0):
    """NonMaxBlock.process with NonMaxBlockSearchRelaxed.Max -> int16 [n, 2]"""
    img = np.asarray(img, F)
    h, w = img.shape
    threshold = F(threshold)
    found = []

    def check_local_max(x_c, y_c, peak):
        x0, x1, y0, y1 = max(x_c - radius, 0), min(x_c + radius, w - 1), max(y_c - radius, 0), min(y_c + radius, h - 1)
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                if img[y, x] > peak:
                    return
        found.append((x_c, y_c))

    end_x, end_y, step = w - border, h - border, radius + 1
    for by in range(border, end_y, step):
        y1 = min(by + step, end_y)
        for bx in range(border, end_x, step):
            x1 = min(bx + step, end_x)
            peaks, peak = [], threshold
            for y in range(by, y1):
                for x in range(bx, x1):
                    v = img[y, x]
                    if v > peak:
                        peak, peaks = v, [(x, y)]
                    elif v == peak:
                        peaks.append((x, y))
            if peaks and peak != FLOAT_MAX:
                for x, y in peaks:
                    check_local_max(x, y, peak)
    return np.array(found, np.int16).reshape(-1, 2)


def nonmax_relaxed_naive(img, radius, threshold, border=0):
    """the naive relaxed rule of GenericNonMaxTests: every pixel inside the border that is >= the threshold and not below any pixel of its
    clipped window -> a set of (x, y)"""
    img = np.asarray(img, F)
    h, w = img.shape
    out = set()
    for y in range(border, h - border):
        for x in range(border, w - border):
            v = img[y, x]
            if not v >= F(threshold) or v == FLOAT_MAX:
                continue
            win = img[max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1]
            if not np.any(win > v):
                out.add((x, y))
    return out


# ---------------- mean shift ----------------
class MeanShiftPeak:
    def __init__(self, image, radius, max_iterations=10, convergence_tol=0.001):
        self.img = np.asarray(image, F)
        self.h, self.w = self.img.shape
        self.radius, self.max_iterations, self.tol = int(radius), int(max_iterations), F(convergence_tol)
        self.weights = weight_gaussian(self.radius) if self.radius > 0 else None

    def _pixel(self, x, y):
        return self.img[y, x] if 0 <= x < self.w and 0 <= y < self.h else F(0)

    def _fast_bounds(self, x, y):
        return not (x < 0 or y < 0 or x > F(self.w - 2) or y > F(self.h - 2))

    def _get_fast(self, x, y):
        xt, yt = int(java_f2i(x)), int(java_f2i(y))
        ax, ay = F(x - F(xt)), F(y - F(yt))
        one = F(1)
        val = F(F(F(one - ax) * F(one - ay)) * self._pixel(xt, yt))
        val = F(val + F(F(ax * F(one - ay)) * self._pixel(xt + 1, yt)))
        val = F(val + F(F(ax * ay) * self._pixel(xt + 1, yt + 1)))
        val = F(val + F(F(F(one - ax) * ay) * self._pixel(xt, yt + 1)))
        return val

    def _get_border(self, x, y):
        xf, yf = F(np.floor(x)), F(np.floor(y))
        xt, yt = int(java_f2i(xf)), int(java_f2i(yf))
        ax, ay = F(x - xf), F(y - yf)
        one = F(1)
        val = F(F(F(one - ax) * F(one - ay)) * self._pixel(xt, yt))
        val = F(val + F(F(ax * F(one - ay)) * self._pixel(xt + 1, yt)))
        val = F(val + F(F(ax * ay) * self._pixel(xt + 1, yt + 1)))
        val = F(val + F(F(F(one - ax) * ay) * self._pixel(xt, yt + 1)))
        return val

    def _get(self, x, y):
        return self._get_fast(x, y) if self._fast_bounds(x, y) else self._get_border(x, y)

    def search(self, cx, cy):
        """-> (peakX, peakY) float32"""
        peak_x, peak_y = F(cx), F(cy)
        if self.radius <= 0:
            return peak_x, peak_y
        offset = F(-self.radius)
        width = 2 * self.radius + 1
        with np.errstate(all="ignore"):
            for _ in range(self.max_iterations):
                total, sum_x, sum_y = F(0), F(0), F(0)
                k = 0
                fast = self._fast_bounds(F(peak_x + offset), F(peak_y + offset)) and self._fast_bounds(F(peak_x - offset), F(peak_y - offset))
                for yy in range(width):
                    y = F(offset + F(yy))
                    for xx in range(width):
                        x = F(offset + F(xx))
                        wgt = self.weights[k]
                        k += 1
                        value = self._get_fast(F(peak_x + x), F(peak_y + y)) if fast else self._get(F(peak_x + x), F(peak_y + y))
                        weight = F(wgt * value)
                        total = F(total + weight)
                        sum_x = F(sum_x + F(weight * x))
                        sum_y = F(sum_y + F(weight * y))
                if total == 0:
                    break
                cx, cy = F(peak_x + F(sum_x / total)), F(peak_y + F(sum_y / total))
                dx, dy = F(cx - peak_x), F(cy - peak_y)
                peak_x, peak_y = cx, cy
                if abs(dx) < self.tol and abs(dy) < self.tol:
                    break
        return peak_x, peak_y


# ---------------- merge ----------------
PI_F, PID2_F = F(math.pi), F(math.pi / 2.0)


def atan_safe(y, x):
    if x == 0:
        return PID2_F if y >= 0 else F(-PID2_F)
    with np.errstate(all="ignore"):
        return F(math.atan(float(F(y / x))))


def dist_half(a, b):
    r = F(abs(F(a - b)))
    return r if float(r) <= math.pi / 2 else F(PI_F - r)


def point_distance(ax, ay, bx, by):
    dx, dy = F(bx - ax), F(by - ay)
    return F(math.sqrt(float(F(F(dx * dx) + F(dy * dy)))))


def intersect_lines(a, b):
    """lines (px, py, sx, sy): Intersection2D_F32.intersection(LineParametric2D_F32, LineParametric2D_F32)"""
    t_b = F(F(a[2] * F(b[1] - a[1])) - F(a[3] * F(b[0] - a[0])))
    bottom = F(F(a[3] * b[2]) - F(b[3] * a[2]))
    if bottom == 0:
        return None
    t_b = F(t_b / bottom)
    return F(F(b[2] * t_b) + b[0]), F(F(b[3] * t_b) + b[1])


def intersect_segments(l0, l1):
    a0, b0 = F(l0[2] - l0[0]), F(l0[3] - l0[1])
    a1, b1 = F(l1[2] - l1[0]), F(l1[3] - l1[1])
    top = F(F(b0 * F(l1[0] - l0[0])) + F(a0 * F(l0[1] - l1[1])))
    bottom = F(F(a0 * b1) - F(b0 * a1))
    if bottom == 0:
        return None
    t_1 = F(top / bottom)
    if t_1 < 0 or t_1 > 1:
        return None
    top = F(F(b1 * F(l0[0] - l1[0])) + F(a1 * F(l1[1] - l0[1])))
    bottom = F(F(a1 * b0) - F(b1 * a0))
    with np.errstate(all="ignore"):
        t_0 = F(top / bottom)
    if t_0 < 0 or t_0 > 1:
        return None
    return F(l1[0] + F(a1 * t_1)), F(l1[1] + F(b1 * t_1))


def segment_distance(line, px, py):
    a, b = F(line[2] - line[0]), F(line[3] - line[1])
    t = F(F(a * F(px - line[0])) + F(b * F(py - line[1])))
    with np.errstate(all="ignore"):
        t = F(t / F(F(a * a) + F(b * b)))
    if t < 0:
        return point_distance(line[0], line[1], px, py)
    if t > 1:
        return point_distance(line[2], line[3], px, py)
    return point_distance(F(line[0] + F(t * a)), F(line[1] + F(t * b)), px, py)


def convert_to_segment(l, width, height):
    """LineImageOps.convert"""
    inside = []
    f = lambda *v: tuple(F(x) for x in v)
    for side in (f(0, 0, 1, 0), f(0, 0, 0, 1), f(width - 1, height - 1, -1, 0), f(width - 1, height - 1, 0, -1)):
        a = intersect_lines(side, l)
        if a is None:
            continue
        if a[0] >= 0 and a[0] <= F(F(width) - F(0.999)) and a[1] >= 0 and a[1] <= F(F(height) - F(0.999)):
            if not any(float(point_distance(p[0], p[1], a[0], a[1])) < 1e-4 for p in inside):
                inside.append(a)
    if len(inside) != 2:
        return None
    return inside[0] + inside[1]


def _float_compare(a, b):
    if a < b:
        return -1
    if a > b:
        return 1
    ia, ib = int(np.array(a, F).view(np.int32)), int(np.array(b, F).view(np.int32))
    return 0 if ia == ib else -1 if ia < ib else 1


def _sort_by_intensity(data):
    def cmp(o1, o2):
        if o1[1] < o2[1]:
            return 1
        if o1[1] > o2[1]:
            return -1
        if o1[0][0] < o2[0][0]:
            return -1
        if o1[0][0] > o2[0][0]:
            return 1
        return _float_compare(o1[0][1], o2[0][1])
    data.sort(key=functools.cmp_to_key(cmp))


def merge_lines(lines, intensity, merge_angle, merge_distance, max_lines, width, height):
    """HoughTransform*.mergeLines: pruneSimilar((float) mergeAngle, (float) mergeDistance, width, height), pruneNBest(maxLines)"""
    tol_angle, tol_dist = F(merge_angle), F(merge_distance)
    data = [[l, F(v)] for l, v in zip(lines, intensity)]
    _sort_by_intensity(data)
    theta = [atan_safe(d[0][3], d[0][2]) for d in data]
    segments = [convert_to_segment(d[0], width, height) for d in data]
    for i in range(len(segments)):
        a = segments[i]
        if a is None:
            continue
        for j in range(i + 1, len(segments)):
            b = segments[j]
            if b is None:
                continue
            if dist_half(theta[i], theta[j]) > tol_angle:
                continue
            p = intersect_segments(a, b)
            close = p is not None and p[0] >= 0 and p[1] >= 0 and p[0] < width and p[1] < height
            if not close:
                if segment_distance(a, b[0], b[1]) > tol_dist and segment_distance(a, b[2], b[3]) > tol_dist:
                    continue
                if segment_distance(b, b[0], b[1]) > tol_dist and segment_distance(b, b[2], b[3]) > tol_dist:
                    continue
            if data[j][1] > data[i][1]:
                data[i][1] = data[j][1]
            segments[j] = None
    data = [d for d, s in zip(data, segments) if s is not None]
    if len(data) > max_lines:
        _sort_by_intensity(data)
        data = data[:max_lines]
    return [d[0] for d in data]


# ---------------- whole detectors ----------------
def binary_transform_lines(binary, par, radius, min_counts, max_lines, merge_angle=math.pi * 0.05, merge_distance=10.0):
    """HoughTransformBinary.transform(binary) -> (lines [(px, py, sx, sy)], linesAll, foundIntensity, transform); min_counts: (length, fraction)"""
    h, w = binary.shape
    transform = hough_binary(binary, par)
    length, fraction = min_counts
    total = transform.shape[0] * transform.shape[1]
    threshold = F(max(fraction * total, length) if fraction >= 0 else length)
    peaks = nonmax_relaxed(transform, radius, threshold, 0)
    lines_all, found = [], []
    for x, y in peaks:
        if not par.is_transform_valid(int(x), int(y)):
            continue
        lines_all.append(par.transform_to_line(F(x), F(y)))
        found.append(transform[y, x])
    merged = list(lines_all) if max_lines <= 0 else merge_lines(lines_all, found, merge_angle, merge_distance, max_lines, w, h)
    return merged, lines_all, np.array(found, F), transform


def detect_binary(img, range_resolution=2.0, num_bins_angle=180, radius=1, min_counts=(1.0, 0.001), max_lines=10):
    """HoughBinary_to_DetectLine.detect with ConfigThreshold.global(GLOBAL_OTSU) on a GrayU8"""
    binary = threshold_ref.global_otsu(img, 1.0, True)
    return binary_transform_lines(binary, Polar(range_resolution, num_bins_angle), radius, min_counts, max_lines)[0]


def gradient_transform_lines(dx, dy, binary, par, radius, min_counts, max_lines, refine_radius=3, merge_angle=math.pi * 0.05, merge_distance=10.0):
    """HoughTransformGradient.transform(derivX, derivY, binary) -> (lines, linesAll, foundIntensity, transform)"""
    h, w = binary.shape
    transform = hough_gradient(dx, dy, binary, par)
    _, peaks = fast_ref.nonmax_block(transform, radius, F(0), F(min_counts), 0, False, True)   # the strict extractor
    refine = MeanShiftPeak(transform, refine_radius)
    lines_all, found = [], []
    for x, y in peaks:
        x, y = int(x), int(y)
        if not par.is_transform_valid(x, y):
            continue
        px, py = F(x), F(y)
        rx, ry = refine.search(px, py)
        with np.errstate(all="ignore"):
            if point_distance(px, py, rx, ry) < F(refine_radius * 2):
                px, py = rx, ry
        lines_all.append(par.transform_to_line(px, py))
        found.append(transform[y, x])
    merged = list(lines_all) if max_lines <= 0 else merge_lines(lines_all, found, merge_angle, merge_distance, max_lines, w, h)
    return merged, lines_all, np.array(found, F), transform


def detect_gradient(img, radius=2, min_counts=5, min_distance=5, threshold_edge=30.0, max_lines=0, refine_radius=3):
    """HoughGradient_to_DetectLine.detect: Prewitt (EXTENDED), intensityAbs, nonMaxSuppressionCrude4, threshold (down = false), transform"""
    dx, dy = prewitt(img, 2)
    inten = intensity_abs(dx, dy)
    binary = threshold_ref.threshold(nonmax_crude4(inten, dx, dy), F(threshold_edge), False)
    return gradient_transform_lines(dx, dy, binary, FootOfNorm(min_distance), radius, min_counts, max_lines, refine_radius)[0]
