"""SiftScaleSpace + SiftDetector + NonMaxLimiter + WrapSiftDetector restated in numpy float32 / float64 with the reference's tap and loop
order (F:alg/feature/detect/interest/SiftScaleSpace.java, SiftDetector.java:165-331, F:abst/feature/detect/extract/NonMaxLimiter.java:62-84,
I:alg/transform/pyramid/impl/ImplPyramidOps.java:44-85, I:alg/interpolate/impl/ImplBilinearPixel_F32.java:48-90,
I:alg/filter/convolve/ConvolveImageSparse.java:41-80).

Pieces the oracle binding already restates are called there: the Gaussian kernel (FactoryKernelGaussian), the two normalised convolution
passes (ConvolveImageNormalized, its naive form for kernels as wide as the image included) and the strict block non-maximum suppression.
Everything else is written out here.  Math.pow is Python's pow: unpinned against Java's, like the library's host pow."""
import math

import numpy as np

from oracle import pyoracle as orc

from template_ref import quick_select_index

f32 = np.float32


class ConfigSS:
    """ConfigSiftScaleSpace: 0, 5, 3, 2.75f"""

    def __init__(self, firstOctave=0, lastOctave=5, numScales=3, sigma0=float(f32(2.75))):
        self.firstOctave, self.lastOctave, self.numScales, self.sigma0 = firstOctave, lastOctave, numScales, float(sigma0)


class ConfigDet:
    """ConfigSiftDetector: ConfigExtract(2, 0, 1, true, true, true), maxFeaturesPerScale 0, edgeR 10"""

    def __init__(self, radius=2, threshold=0.0, maxFeaturesPerScale=0, edgeR=10.0):
        self.radius, self.threshold, self.maxFeaturesPerScale, self.edgeR = radius, float(f32(threshold)), maxFeaturesPerScale, float(edgeR)


def sigma_scale(ss, octave, scale):
    """SiftScaleSpace.computeSigmaScale(octave, scale) :162-164"""
    return ss.sigma0 * math.pow(2, octave + scale / float(ss.numScales))


def kernels(ss):
    """kernelSigma0 and kernelSigmaToK[0 .. numScales+1] (:127-141)"""
    levelK = math.pow(2, 1.0 / ss.numScales)
    k0 = orc.gaussian1d_f32(ss.sigma0, -1)
    ks = [orc.gaussian1d_f32(sigma_scale(ss, 0, i - 1) * math.sqrt(levelK - 1.0), -1) for i in range(1, ss.numScales + 3)]
    return k0, ks


def apply_gaussian(img, k):
    """applyGaussian :241-245: horizontalNormalized into tempBlur, then verticalNormalized"""
    g = orc.Gray.from_array(img)
    t = orc.conv("norm_h", k, len(k) // 2, g)
    return orc.conv("norm_v", k, len(k) // 2, t).array().copy()


def scale_image_up(img, scale):
    """ImplPyramidOps.scaleImageUp with ImplBilinearPixel_F32.get and an EXTENDED border.  get_fast and get_border are one expression on
    non-negative coordinates: floor = truncation, and a clamped read is the plain read wherever get_fast is taken (x <= width - 2)"""
    img = np.asarray(img, f32)
    h, w = img.shape
    fdiv = f32(1) / f32(scale)
    xs = np.arange(w * scale, dtype=np.int32).astype(f32) * fdiv
    ys = np.arange(h * scale, dtype=np.int32).astype(f32) * fdiv
    xf, yf = np.floor(xs), np.floor(ys)
    ax, ay = (xs - xf)[None, :], (ys - yf)[:, None]
    x0 = np.clip(xf.astype(np.int64), 0, w - 1); x1 = np.clip(xf.astype(np.int64) + 1, 0, w - 1)
    y0 = np.clip(yf.astype(np.int64), 0, h - 1); y1 = np.clip(yf.astype(np.int64) + 1, 0, h - 1)
    one = f32(1)
    val = ((one - ax) * (one - ay)) * img[np.ix_(y0, x0)]
    val = val + (ax * (one - ay)) * img[np.ix_(y0, x1)]
    val = val + (ax * ay) * img[np.ix_(y1, x1)]
    val = val + ((one - ax) * ay) * img[np.ix_(y1, x0)]
    assert val.dtype == f32
    return val


def scale_down2(img):
    """ImplPyramidOps.scaleDown2: every other pixel, width / 2 x height / 2"""
    h, w = img.shape
    return np.ascontiguousarray(img[0:2 * (h // 2):2, 0:2 * (w // 2):2])


def layout(ss, width, height):
    """[(octave, width, height)] of the octaves initialize / computeNextOctave produce for a frame size"""
    if ss.firstOctave < 0:
        w, h = width * (-2 * ss.firstOctave), height * (-2 * ss.firstOctave)
    else:
        w, h = width, height
        for _ in range(ss.firstOctave):
            w, h = w // 2, h // 2
    out = [(ss.firstOctave, w, h)]
    o = ss.firstOctave
    while True:
        o += 1
        if o > ss.lastOctave or w <= 5 or h <= 5:
            return out
        w, h = w // 2, h // 2
        out.append((o, w, h))


def to_float(img):
    """WrapSiftDetector.detect: GrayF32 as it is, GrayU8 by GConvertImage.convert (& 0xFF to float)"""
    img = np.asarray(img)
    assert img.dtype in (np.uint8, np.float32)
    return img.astype(f32)


def scale_space(ss, img):
    """-> [(octave index, [numScales+3 scale images], [numScales+2 DoG images])] for every octave the reference computes"""
    img = to_float(img)
    k0, ks = kernels(ss)
    if ss.firstOctave < 0:
        t0 = apply_gaussian(scale_image_up(img, -2 * ss.firstOctave), k0)
    else:
        t0 = apply_gaussian(img, k0)
        for _ in range(ss.firstOctave):
            t0 = scale_down2(apply_gaussian(t0, k0))
    out = []
    o = ss.firstOctave
    while True:
        octv = [t0]
        for i in range(1, ss.numScales + 3):
            octv.append(apply_gaussian(octv[i - 1], ks[i - 1]))
        dog = [octv[i] - octv[i - 1] for i in range(1, ss.numScales + 3)]
        out.append((o, octv, dog))
        o += 1
        if o > ss.lastOctave:
            break
        if octv[ss.numScales].shape[1] <= 5 or octv[ss.numScales].shape[0] <= 5:
            break
        t0 = scale_down2(octv[ss.numScales])
    return out


def nonmax_limiter(dog, det):
    """NonMaxLimiter.process: [(intensity, max, x, y)], all minima then all maxima in block-raster order, then the QuickSelect cut.  The
    minima of the image are the maxima of its (exact) negation, thresholdMin = -threshold"""
    g = orc.Gray.from_array(dog)
    gn = orc.Gray.from_array(-np.asarray(dog, f32))
    mins = orc.nonmax(gn, det.radius, det.threshold, 1)
    maxs = orc.nonmax(g, det.radius, det.threshold, 1)
    found = [(f32(-dog[y, x]), False, int(x), int(y)) for x, y in mins] + [(f32(dog[y, x]), True, int(x), int(y)) for x, y in maxs]
    full = list(found)
    if det.maxFeaturesPerScale > 0 and len(found) > det.maxFeaturesPerScale:
        idx = quick_select_index([f32(-e[0]) for e in found], det.maxFeaturesPerScale, len(found))
        found = [found[idx[i]] for i in range(det.maxFeaturesPerScale)]
    return found, full


def is_scale_space_extremum(lower, upper, cx, cy, value, sign):
    """:229-249"""
    h, w = lower.shape
    if cx <= 1 or cy <= 1 or cx >= w - 1 or cy >= h - 1:
        return False
    sign = f32(sign)
    value = f32(value) * sign
    for y in (-1, 0, 1):
        for x in (-1, 0, 1):
            if f32(lower[cy + y, cx + x]) * sign >= value:
                return False
            if f32(upper[cy + y, cx + x]) * sign >= value:
                return False
    return True


def _kernel_dd():
    """KernelMath.convolve1D_F32([-1,0,1], [-1,0,1])"""
    a = [f32(-1), f32(0), f32(1)]
    out = []
    for j in range(-2, 3):
        s = f32(0)
        for k in range(3):
            if 0 <= j + k < 3:
                s = f32(s + a[2 - k] * a[j + k])
        out.append(s)
    return out


KERNEL_DD = _kernel_dd()
KERNEL_XY = [[f32(a * b) for b in (f32(-1), f32(0), f32(1))] for a in (f32(-1), f32(0), f32(1))]   # KernelMath.convolve2D(kernelD, kernelD)


def _ext(img, x, y):
    h, w = img.shape
    return f32(img[min(max(y, 0), h - 1), min(max(x, 0), w - 1)])


def sparse_derivs(img, x, y):
    """derivXX, derivXY, derivYY .compute(x, y): ConvolveImageSparse.horizontal / convolve / vertical, float sums in tap order"""
    xx = f32(0)
    for i in range(5):
        xx = f32(xx + _ext(img, x + i - 2, y) * KERNEL_DD[i])
    yy = f32(0)
    for i in range(5):
        yy = f32(yy + _ext(img, x, y + i - 2) * KERNEL_DD[i])
    xy = f32(0)
    for i in range(3):
        for j in range(3):
            xy = f32(xy + _ext(img, x + j - 1, y + i - 1) * KERNEL_XY[i][j])
    return xx, xy, yy


def edge_threshold(edgeR):
    return (edgeR + 1) * (edgeR + 1) / edgeR


def is_edge(img, x, y, edgeR):
    """:311-331"""
    thr = edge_threshold(float(edgeR))
    if thr <= 0:
        return False
    xx, xy, yy = (float(v) for v in sparse_derivs(img, x, y))
    Tr = xx + yy
    det = xx * yy - xy * xy
    if det <= 0:
        return True
    return Tr * Tr >= thr * det


def poly_peak(lower, middle, upper):
    """FastHessianFeatureDetector.polyPeak(float) :336-350"""
    a = f32(f32(f32(0.5) * lower) - middle) + f32(f32(0.5) * upper)
    a = f32(a)
    b = f32(f32(f32(0.5) * upper) - f32(f32(0.5) * lower))
    if a == f32(0):
        return f32(0)
    return f32(f32(-b) / f32(f32(2) * a))


def feature_candidate(lower, target, upper, x, y, value, maximum, pixelScaleToInput, sigmas):
    """processFeatureCandidate :262-299 after the edge test -> (x, y, scale, white)"""
    sign = f32(1) if maximum else f32(-1)
    value = f32(f32(value) * sign)
    x0 = f32(target[y, x - 1]) * sign; x2 = f32(target[y, x + 1]) * sign
    y0 = f32(target[y - 1, x]) * sign; y2 = f32(target[y + 1, x]) * sign
    s0 = f32(lower[y, x]) * sign; s2 = f32(upper[y, x]) * sign
    px = pixelScaleToInput * float(f32(f32(x) + poly_peak(x0, value, x2)))
    py = pixelScaleToInput * float(f32(f32(y) + poly_peak(y0, value, y2)))
    si = float(poly_peak(s0, value, s2))
    sl, st, su = sigmas
    scale = sl * (-si) + (1 + si) * st if si < 0 else su * si + (1 - si) * st
    return px, py, scale, not maximum


def detect(ss, det, img, stats=None, space=None):
    """SiftDetector.process -> (xy float64 [n,2], scale float64 [n], white uint8 [n], where int16 [n,4] = octave, j, pixel x, pixel y), in
    the reference's order.  stats (a dict) counts the list entries and those the frame test, the 18-neighbour test and the edge test reject; stats['lists'] holds every
    scale's uncut NMS list"""
    space = space if space is not None else scale_space(ss, img)
    xy, sc, wh, where = [], [], [], []
    if stats is not None:
        stats.update(nms=0, frame=0, extremum=0, edge=0, kept=0, lists=[])
    for o, octv, dog in space:
        p2i = math.pow(2.0, o)
        for j in range(1, ss.numScales + 1):
            sig = (sigma_scale(ss, o, j - 1), sigma_scale(ss, o, j), sigma_scale(ss, o, j + 1))
            lower, target, upper = dog[j - 1], dog[j], dog[j + 1]
            found, full = nonmax_limiter(target, det)
            if stats is not None:
                stats["nms"] += len(found)
                stats["lists"].append(full)
            for inten, mx, x, y in found:
                value = inten if mx else f32(-inten)
                if not is_scale_space_extremum(lower, upper, x, y, value, 1.0 if mx else -1.0):
                    if stats is not None:
                        h, w = lower.shape
                        stats["frame" if x <= 1 or y <= 1 or x >= w - 1 or y >= h - 1 else "extremum"] += 1
                    continue
                if is_edge(target, x, y, det.edgeR):
                    if stats is not None:
                        stats["edge"] += 1
                    continue
                px, py, s, w = feature_candidate(lower, target, upper, x, y, value, mx, p2i, sig)
                xy.append((px, py)); sc.append(s); wh.append(1 if w else 0); where.append((o, j, x, y))
    if stats is not None:
        stats["kept"] = len(sc)
    return (np.array(xy, np.float64).reshape(-1, 2), np.array(sc, np.float64), np.array(wh, np.uint8), np.array(where, np.int16).reshape(-1, 4))
