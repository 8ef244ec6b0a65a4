"""NumPy reference of the FAST corner detector and the strict min / max block non-maximum suppression, written from the rules the
reference implements (not from its generated decision trees).

    F: = main/boofcv-feature/src/main/java/boofcv/   I: = main/boofcv-ip/src/main/java/boofcv/

  circle()            DiscretizedCircle.imageOffsets(3, stride)     I:misc/DiscretizedCircle.java:39-77
  classify / score    ImplFastCorner{9..12}_{U8,F32}.checkPixel as the rule GenericFastCorner.compareToNaiveDetection checks the trees
                      against; ImplFastHelper_U8 / _F32.scoreLower / scoreUpper (F:alg/feature/detect/intensity/impl/ImplFastHelper_*.java:47-81)
  fast()              FastCornerDetector.process                    F:alg/feature/detect/intensity/FastCornerDetector.java:123-189
  nonmax_block()      NonMaxBlock.process + NonMaxBlockSearchStrict F:alg/feature/detect/extract/NonMaxBlock.java:69-94, NonMaxBlockSearchStrict.java:56-248
  general_detector()  GeneralFeatureDetector.process                F:alg/feature/detect/interest/GeneralFeatureDetector.java:107-161
"""
import math

import numpy as np

FLOAT_MAX = np.float32(np.finfo(np.float32).max)


def java_round(v):
    return int(math.floor(v + 0.5))   # Math.round(double)


def circle(radius=3.0):
    """the loop of DiscretizedCircle.imageOffsets, keeping (dx, dy) instead of dy * stride + dx (the stride only has to be wide enough
    for the offsets to be distinct, which every image stride >= 7 is)"""
    pi2 = math.pi * 2.0
    circumference = pi2 * radius
    num = int(math.ceil(circumference))
    num -= num % 4
    step = pi2 / num
    wide = 1000
    out, prev, ang = [], 0, 0.0
    while ang < pi2:
        x, y = java_round(math.cos(ang) * radius), java_round(math.sin(ang) * radius)
        pixel = y * wide + x
        if pixel != prev:
            out.append((x, y))
        prev = pixel
        ang += step
    return out


CIRCLE = circle()


def java_f2i(f):
    """Java's (int) of a float array: toward zero, saturating, NaN -> 0"""
    f = np.asarray(f, np.float32)
    out = np.zeros(f.shape, np.int64)
    ok = ~np.isnan(f)
    t = np.trunc(f[ok].astype(np.float64))
    out[ok] = np.clip(t, -2147483648.0, 2147483647.0).astype(np.int64)
    return out


def _ring(img):
    h, w = img.shape
    return np.stack([img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE]), img[3:h - 3, 3:w - 3]


def _has_run(mask, n):
    """mask [16, ...] bool: some n cyclically contiguous entries are all set"""
    found = np.zeros(mask.shape[1:], bool)
    for s in range(16):
        run = np.ones(mask.shape[1:], bool)
        for k in range(n):
            run &= mask[(s + k) % 16]
        found |= run
    return found


def classify_score(img, tol, n):
    """interior pixels only -> (cls int8 [h-6, w-6]: -1 dark, +1 bright, 0; score float32, 0 where cls == 0)"""
    assert len(CIRCLE) == 16 and 9 <= n <= 12 and tol >= 0
    if img.dtype == np.uint8:
        ring, c = _ring(img.astype(np.int64))
        lower, upper = c - int(tol), c + int(tol)
    else:
        assert img.dtype == np.float32
        ring, c = _ring(img)
        lower, upper = c - np.float32(tol), c + np.float32(tol)   # float arithmetic
    bright, dark = ring > upper, ring < lower
    cls = np.zeros(c.shape, np.int8)
    cls[_has_run(bright, n)] = 1
    cls[_has_run(dark, n)] = -1   # exclusive with the above for n >= 9, tol >= 0
    assert not np.any(_has_run(bright, n) & _has_run(dark, n))
    used = np.where(cls[None] > 0, bright, dark) & (cls[None] != 0)
    count = used.sum(axis=0)
    if img.dtype == np.uint8:
        total = (ring * used).sum(axis=0)
        score = (total - c * count).astype(np.float32)
    else:
        total = np.zeros(c.shape, np.int64)   # `int total; total += v;` == total = (int)((float)total + v), in circle order
        with np.errstate(all="ignore"):
            for i in range(16):
                total = np.where(used[i], java_f2i(total.astype(np.float32) + ring[i]), total)
            score = total.astype(np.float32) - c * count.astype(np.float32)
        score = np.where(cls != 0, score, np.float32(0)).astype(np.float32)
    return cls, score


def max_features(fraction, w, h):
    return int(fraction * w * h)   # (int)(maxFeaturesFraction*image.width*image.height), left to right in double


def fast(img, tol, n, fraction=1.0, intensity=True):
    """-> (intensity float32 [h, w] or None, low int16 [nLow, 2], high int16 [nHigh, 2], stopRow).  The intensity is 0 in the 3-pixel
    border and in the rows after the stop row (a fresh reference detector)."""
    h, w = img.shape
    inten = np.zeros((h, w), np.float32)
    empty = np.zeros((0, 2), np.int16)
    if w < 7 or h < 7:
        return (inten if intensity else None), empty, empty.copy(), max(h - 4, 0)
    cls, score = classify_score(img, tol, n)
    limit = max_features(fraction, w, h)
    running = np.cumsum((cls != 0).sum(axis=1))
    hit = np.nonzero(running >= limit)[0]
    stop = 3 + (int(hit[0]) if len(hit) else h - 7)
    cls, score = cls[:stop - 2], score[:stop - 2]
    inten[3:stop + 1, 3:w - 3] = score
    lists = []
    for want in (-1, 1):
        ys, xs = np.nonzero(cls == want)   # raster order
        lists.append(np.stack([xs + 3, ys + 3], axis=1).astype(np.int16).reshape(-1, 2))
    return (inten if intensity else None), lists[0], lists[1], stop


def _window_ok(img, x, y, r, peak, minimum):
    h, w = img.shape
    x0, x1, y0, y1 = max(x - r, 0), min(x + r, w - 1), max(y - r, 0), min(y + r, h - 1)
    win = img[y0:y1 + 1, x0:x1 + 1]
    other = np.ones(win.shape, bool)
    other[y - y0, x - x0] = False
    return not np.any((win <= peak if minimum else win >= peak) & other)


def nonmax_block(img, radius, threshold_min, threshold_max, border, detect_min, detect_max):
    """the block algorithm as written: per (radius+1)^2 block the first extreme value (strict compare, raster order), threshold and
    marker test, then the clipped (2*radius+1)^2 window -> (minimums int16 [n, 2], maximums int16 [m, 2]) in block-raster order"""
    img = np.asarray(img, np.float32)
    h, w = img.shape
    end_x, end_y, step = w - border, h - border, radius + 1
    mins, maxs = [], []
    for y in range(border, end_y, step):
        y1 = min(y + step, end_y)
        for x in range(border, end_x, step):
            x1 = min(x + step, end_x)
            blk = img[y:y1, x:x1]
            if detect_max:
                k = int(np.argmax(blk))   # first largest in raster order
                py, px = divmod(k, blk.shape[1])
                v = blk[py, px]
                if v > -FLOAT_MAX and v >= threshold_max and v != FLOAT_MAX and _window_ok(img, x + px, y + py, radius, v, False):
                    maxs.append((x + px, y + py))
            if detect_min:
                k = int(np.argmin(blk))
                py, px = divmod(k, blk.shape[1])
                v = blk[py, px]
                if v < FLOAT_MAX and v <= threshold_min and v != -FLOAT_MAX and _window_ok(img, x + px, y + py, radius, v, True):
                    mins.append((x + px, y + py))
    return np.array(mins, np.int16).reshape(-1, 2), np.array(maxs, np.int16).reshape(-1, 2)


def nonmax_brute(img, radius, threshold, border, minimum):
    """every pixel inside the border that passes the threshold, is not the exclusion marker and is a strict extremum of its clipped
    window, sorted into block-raster order (at most one per block can pass)"""
    img = np.asarray(img, np.float32)
    h, w = img.shape
    step = radius + 1
    out = []
    for y in range(border, h - border):
        for x in range(border, w - border):
            v = img[y, x]
            if minimum:
                if not (v <= threshold) or v == -FLOAT_MAX:
                    continue
            elif not (v >= threshold) or v == FLOAT_MAX:
                continue
            if _window_ok(img, x, y, radius, v, minimum):
                out.append(((y - border) // step, (x - border) // step, x, y))
    out.sort()
    return np.array([(x, y) for _, _, x, y in out], np.int16).reshape(-1, 2)


def general_detector(img, tol, n, fraction, radius, threshold, ignore_border, detect_min, detect_max, max_feat, exclude_min, exclude_max, select):
    """FactoryDetectPoint.createFast(configFast, configDetector, imageType).process(image): createGeneral adds the radius to the ignore
    border (at least FAST's own 3), thresholdMin = -threshold, and a config without maximums gets the Min search.
    select(intensity, corners int16 [k, 2], N, positive) -> int16 [<= N, 2] is SelectNBestFeatures, called for every side with N > 0.
    -> (intensity with the exclusion marks, minimums, maximums)"""
    if not detect_max:
        detect_min = True
    inten, _, _, _ = fast(img, tol, n, fraction, True)
    border = max(ignore_border + radius, 3)
    empty = np.zeros((0, 2), np.int16)
    num_min = num_max = -1
    if max_feat > 0:
        num_min = max_feat if exclude_min is None else max_feat - len(exclude_min)   # FAST has minimums and maximums
        num_max = max_feat if exclude_max is None else max_feat - len(exclude_max)
        if num_min <= 0 and num_max <= 0:
            return inten, empty, empty.copy()
    for lst, mark in ((exclude_min, -FLOAT_MAX), (exclude_max, FLOAT_MAX)):
        if lst is not None:
            for x, y in lst:
                inten[y, x] = mark
    mins, maxs = nonmax_block(inten, radius, -threshold, threshold, border, detect_min, detect_max)
    if num_min > 0:
        mins = select(inten, mins, num_min, False)
    if num_max > 0:
        maxs = select(inten, maxs, num_max, True)
    return inten, mins, maxs
