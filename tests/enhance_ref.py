"""A plain numpy / Python restatement of the reference's image enhancement, the oracle of tests/test_gpu_enhance.py
(checked itself by tests/test_enhance_reference.py):

  EnhanceImageOps.equalize / applyTransform / equalizeLocal      main/boofcv-ip/src/main/java/boofcv/alg/enhance/EnhanceImageOps.java:65-232
  ImplEnhanceHistogram: equalizeLocalNaive / Inner / Row / Col / localHistogram   .../enhance/impl/ImplEnhanceHistogram.java:111-417
  ImplEnhanceFilter: sharpenInner4 / 8, sharpenBorder4 / 8, safeGet               .../enhance/impl/ImplEnhanceFilter.java:43-475
  ImageStatistics.histogram(GrayU8, minValue, int[])                              .../misc/impl/ImplImageStatistics.java:206-221

Two layers.  The LITERAL functions walk the reference's loops in their order with its index arithmetic (images are [H,W] arrays, x the
column); an index outside a histogram raises IndexError where Java throws.  The ONE-RULE functions (rank_local, sharpen_rule) state each
output pixel by itself; they are what the kernels implement, and the CPU test shows that they equal the literal loops."""
import numpy as np


def _i32(v):
    """a Python int wrapped to Java's int"""
    return ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _idiv(a, b):
    """Java's int division: truncation toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _byte(v):
    return int(v) & 0xFF


# ---------------- histogram, equalize, applyTransform ----------------
def histogram(img, minValue, length, drop=False):
    """ImplImageStatistics.histogram: h[(pixel & 0xFF) - minValue]++.  drop: leave out what Java's array would refuse (the GPU form)."""
    h = [0] * length
    for v in np.asarray(img, np.uint8).ravel().tolist():
        i = v - minValue
        if 0 <= i < length:
            h[i] += 1
        elif not drop:
            raise IndexError(i)
    return np.array(h, np.int32)


def equalize(hist):
    """EnhanceImageOps.equalize :65-77 -> transform"""
    n = len(hist)
    transform = [0] * n
    s = 0
    for i in range(n):
        s = _i32(s + int(hist[i]))
        transform[i] = s
    maxValue = n - 1
    if s == 0:
        raise ZeroDivisionError
    for i in range(n):
        transform[i] = _idiv(_i32(transform[i] * maxValue), s)
    return np.array(transform, np.int32)


def applyTransform(img, transform, drop=False):
    """ImplEnhanceHistogram.applyTransform(GrayU8): (byte)transform[pixel & 0xFF].  drop: 0 beyond the table (the GPU form)."""
    img = np.asarray(img, np.uint8)
    out = np.zeros(img.shape, np.uint8)
    for y in range(img.shape[0]):
        for x in range(img.shape[1]):
            v = int(img[y, x])
            if v >= len(transform):
                if not drop:
                    raise IndexError(v)
                continue
            out[y, x] = _byte(transform[v])
    return out


# ---------------- equalizeLocal: the five loops, literally ----------------
def _localHistogram(img, x0, y0, x1, y1, hist):
    for i in range(len(hist)):
        hist[i] = 0
    for i in range(y0, y1):
        for x in range(x0, x1):
            hist[int(img[i, x])] += 1   # IndexError where Java throws


def _prefix(hist, transform):
    s = 0
    for i in range(len(hist)):
        s += hist[i]
        transform[i] = s


def equalizeLocalNaive(img, radius, out, length):
    H, W = img.shape
    width = 2 * radius + 1
    maxValue = length - 1
    hist = [0] * length
    for y in range(H):
        y0 = y - radius
        y1 = y + radius + 1
        if y0 < 0:
            y0 = 0
            y1 = width
            if y1 > H:
                y1 = H
        elif y1 > H:
            y1 = H
            y0 = y1 - width
            if y0 < 0:
                y0 = 0
        for x in range(W):
            x0 = x - radius
            x1 = x + radius + 1
            if x0 < 0:
                x0 = 0
                x1 = width
                if x1 > W:
                    x1 = W
            elif x1 > W:
                x1 = W
                x0 = x1 - width
                if x0 < 0:
                    x0 = 0
            _localHistogram(img, x0, y0, x1, y1, hist)
            inputValue = int(img[y, x])
            s = 0
            for i in range(inputValue + 1):
                s += hist[i]
            area = (y1 - y0) * (x1 - x0)
            out[y, x] = _byte(_idiv(s * maxValue, area))


def equalizeLocalInner(img, radius, out, length):
    H, W = img.shape
    width = 2 * radius + 1
    area = width * width
    maxValue = length - 1
    hist = [0] * length
    for y in range(radius, H - radius):
        _localHistogram(img, 0, y - radius, width, y + radius + 1, hist)
        inputValue = int(img[y, radius])
        s = 0
        for i in range(inputValue + 1):
            s += hist[i]
        out[y, radius] = _byte(_idiv(s * maxValue, area))
        xOld, xNew = 0, width   # indexOld / indexNew relative to the row start
        for x in range(radius + 1, W - radius):
            for i in range(-radius, radius + 1):
                hist[int(img[y + i, xOld])] -= 1
            for i in range(-radius, radius + 1):
                hist[int(img[y + i, xNew])] += 1
            inputValue = int(img[y, x])
            s = 0
            for i in range(inputValue + 1):
                s += hist[i]
            out[y, x] = _byte(_idiv(s * maxValue, area))
            xOld += 1
            xNew += 1


def equalizeLocalRow(img, radius, startY, out, length):
    H, W = img.shape
    width = 2 * radius + 1
    area = width * width
    maxValue = length - 1
    hist = [0] * length
    transform = [0] * length
    hist0 = startY
    hist1 = startY + width
    if hist1 > H:
        hist1 = H
        hist0 = hist1 - width
    region0 = startY
    region1 = startY + radius
    _localHistogram(img, 0, hist0, width, hist1, hist)
    _prefix(hist, transform)
    for y in range(region0, region1):
        for x in range(0, radius + 1):
            out[y, x] = _byte(_idiv(transform[int(img[y, x])] * maxValue, area))
    for x in range(radius + 1, W - radius - 1):
        col = x - radius - 1
        for y in range(hist0, hist1):
            hist[int(img[y, col])] -= 1
        col += width
        for y in range(hist0, hist1):
            hist[int(img[y, col])] += 1
        _prefix(hist, transform)
        for y in range(radius):
            out[region0 + y, x] = _byte(_idiv(transform[int(img[region0 + y, x])] * maxValue, area))
    _localHistogram(img, W - width, hist0, W, hist1, hist)
    _prefix(hist, transform)
    for y in range(region0, region1):
        for x in range(W - radius - 1, W):
            out[y, x] = _byte(_idiv(transform[int(img[y, x])] * maxValue, area))


def equalizeLocalCol(img, radius, startX, out, length):
    H, W = img.shape
    width = 2 * radius + 1
    area = width * width
    maxValue = length - 1
    hist = [0] * length
    transform = [0] * length
    hist0 = startX
    hist1 = startX + width
    if hist1 > W:
        hist1 = W
        hist0 = hist1 - width
    _localHistogram(img, hist0, 0, hist1, width, hist)
    _prefix(hist, transform)
    for x in range(radius):
        out[radius, startX + x] = _byte(_idiv(transform[int(img[radius, startX + x])] * maxValue, area))
    for y in range(radius + 1, H - radius):
        row = y - radius - 1
        for x in range(hist0, hist1):
            hist[int(img[row, x])] -= 1
        row += width
        for x in range(hist0, hist1):
            hist[int(img[row, x])] += 1
        _prefix(hist, transform)
        for x in range(radius):
            out[y, startX + x] = _byte(_idiv(transform[int(img[y, startX + x])] * maxValue, area))


def equalizeLocal(img, radius, length):
    """EnhanceImageOps.equalizeLocal(GrayU8, radius, output, histogramLength, null) :176-232: the three-way dispatch -> (output, branch)"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    width = radius * 2 + 1
    if W >= width and H >= width:
        equalizeLocalInner(img, radius, out, length)
        equalizeLocalRow(img, radius, 0, out, length)
        equalizeLocalRow(img, radius, H - radius, out, length)
        equalizeLocalCol(img, radius, 0, out, length)
        equalizeLocalCol(img, radius, W - radius, out, length)
        return out, "inner"
    if W < width and H < width:
        out[...] = applyTransform(img, equalize(histogram(img, 0, length)))
        return out, "whole"
    equalizeLocalNaive(img, radius, out, length)
    return out, "naive"


# ---------------- equalizeLocal: the one rule ----------------
def window(c, r, n):
    """[lo, hi) of the window of coordinate c on an axis of n pixels: shifted, not cropped, to stay inside"""
    w = 2 * r + 1
    lo = max(0, min(c - r, n - w))
    return lo, min(n, lo + w)


def rank_local(img, radius, length):
    """out(x,y) = (byte)((#{window pixels <= in(x,y)} * (length-1)) / window area); a value >= length is ranked like any other"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        y0, y1 = window(y, radius, H)
        for x in range(W):
            x0, x1 = window(x, radius, W)
            cnt = int(np.count_nonzero(img[y0:y1, x0:x1] <= img[y, x]))
            out[y, x] = _byte((cnt * (length - 1)) // ((x1 - x0) * (y1 - y0)))
    return out


# ---------------- sharpen: the loops, in their write order ----------------
def _num(dtype):
    """the arithmetic of a pixel type: Java int for GrayU8, float32 operation by operation for GrayF32"""
    return (lambda v: int(v)) if dtype == np.uint8 else (lambda v: np.float32(v))


def _safeGet(img, x, y):
    H, W = img.shape
    x = 0 if x < 0 else W - 1 if x >= W else x
    y = 0 if y < 0 else H - 1 if y >= H else y
    return img[y, x]


def _clamp(a, lo, hi):
    if a > hi:
        a = hi
    elif a < lo:
        a = lo
    return a


def _sharpen_literal(img, rule):
    img = np.asarray(img)
    n = _num(img.dtype)
    H, W = img.shape
    lo, hi = n(0), n(255)
    out = np.zeros((H, W), img.dtype)
    g = lambda x, y: n(_safeGet(img, x, y))
    v = lambda x, y: n(img[y, x])

    def eight(get, x, y):
        a11, a12, a13 = get(x - 1, y - 1), get(x, y - 1), get(x + 1, y - 1)
        a21, a22, a23 = get(x - 1, y), get(x, y), get(x + 1, y)
        a31, a32, a33 = get(x - 1, y + 1), get(x, y + 1), get(x + 1, y + 1)
        return n(9) * a22 - (a11 + a12 + a13 + a21 + a23 + a31 + a32 + a33)

    b, c = H - 1, W - 1
    with np.errstate(all="ignore"):
        # sharpenInner
        for y in range(1, H - 1):
            for x in range(1, W - 1):
                if rule == 4:
                    a = n(5) * v(x, y) - (v(x - 1, y) + v(x + 1, y) + v(x, y - 1) + v(x, y + 1))
                else:
                    a = eight(v, x, y)
                out[y, x] = _clamp(a, lo, hi)
        # sharpenBorder: every x top then bottom, then every y in 1 .. H-2 left then right
        for x in range(W):
            if rule == 4:
                a = n(4) * g(x, 0) - (g(x - 1, 0) + g(x + 1, 0) + g(x, 1))
            else:
                a = eight(g, x, 0)
            out[0, x] = _clamp(a, lo, hi)
            if rule == 4:
                a = n(4) * g(x, b) - (g(x - 1, b) + g(x + 1, b) + g(x, b - 1))
            else:
                a = eight(g, x, b)
            out[b, x] = _clamp(a, lo, hi)
        for y in range(1, H - 1):
            if rule == 4:
                a = n(4) * g(0, y) - (g(1, y) + g(0, y - 1) + g(0, y + 1))
            else:
                a = eight(g, 0, y)
            out[y, 0] = _clamp(a, lo, hi)
            if rule == 4:
                a = n(4) * g(c, y) - (g(c - 1, y) + g(c, y - 1) + g(c, y + 1))
            else:
                a = eight(g, c, y)
            out[y, c] = _clamp(a, lo, hi)
    return out


def sharpen4(img):
    return _sharpen_literal(img, 4)


def sharpen8(img):
    return _sharpen_literal(img, 8)


# ---------------- sharpen: the one rule ----------------
def sharpen_owner(x, y, W, H):
    """which formula's write is the last one on pixel (x, y)"""
    if 1 <= y <= H - 2:
        return "RIGHT" if x == W - 1 else "LEFT" if x == 0 else "INNER"
    return "BOTTOM" if y == H - 1 else "TOP"


def sharpen_rule(img, rule, fused=False):
    """every pixel by itself from the owner table; fused: the multiply and the subtraction as ONE rounding (what a contracted FMA would give),
    for the test that shows the inputs tell the two apart"""
    img = np.asarray(img)
    n = _num(img.dtype)
    H, W = img.shape
    lo, hi = n(0), n(255)
    out = np.zeros((H, W), img.dtype)
    g = lambda x, y: n(_safeGet(img, x, y))

    def finish(k, c, s):
        if fused and img.dtype == np.float32:
            return np.float32(np.float64(k) * np.float64(c) - np.float64(s))   # exact in float64: one rounding to float32
        return n(k) * c - s

    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                c = g(x, y)
                if rule == 8:
                    s = g(x - 1, y - 1) + g(x, y - 1) + g(x + 1, y - 1) + g(x - 1, y) + g(x + 1, y) + g(x - 1, y + 1) + g(x, y + 1) + g(x + 1, y + 1)
                    a = finish(9, c, s)
                else:
                    o = sharpen_owner(x, y, W, H)
                    if o == "INNER":
                        a = finish(5, c, g(x - 1, y) + g(x + 1, y) + g(x, y - 1) + g(x, y + 1))
                    elif o == "TOP":
                        a = finish(4, c, g(x - 1, 0) + g(x + 1, 0) + g(x, 1))
                    elif o == "BOTTOM":
                        a = finish(4, c, g(x - 1, y) + g(x + 1, y) + g(x, y - 1))
                    elif o == "LEFT":
                        a = finish(4, c, g(1, y) + g(0, y - 1) + g(0, y + 1))
                    else:
                        a = finish(4, c, g(x - 1, y) + g(x, y - 1) + g(x, y + 1))
                out[y, x] = _clamp(a, lo, hi)
    return out


def convolve_clamped(img, kernel):
    """the 3x3 convolution of the inner pixels with an integer kernel, clamped to [0, 255] (TestImplEnhanceFilter's expected image); the frame is 0"""
    img = np.asarray(img)
    H, W = img.shape
    acc = np.zeros((H, W), np.float64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            acc[1:H - 1, 1:W - 1] += kernel[dy + 1][dx + 1] * img[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx].astype(np.float64)
    acc = np.clip(acc, 0, 255)
    acc[0, :] = acc[-1, :] = 0
    acc[:, 0] = acc[:, -1] = 0
    return acc


KERNEL_ENHANCE4 = ((0, -1, 0), (-1, 5, -1), (0, -1, 0))
KERNEL_ENHANCE8 = ((-1, -1, -1), (-1, 9, -1), (-1, -1, -1))
