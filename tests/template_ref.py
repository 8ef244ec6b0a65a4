"""NumPy restatement of the reference's template matching, for the tests (tests/test_template_reference.py checks it against the reference's own
tests, tests/test_gpu_template.py compares the GPU with it bit for bit).  It imports nothing of the library under test.

    F: = main/boofcv-feature/src/main/java/boofcv/
    TemplateIntensityImage.process              F:alg/feature/detect/template/TemplateIntensityImage.java:56-125
    TemplateSumAbsoluteDifference.U8 / .F32     F:alg/feature/detect/template/TemplateSumAbsoluteDifference.java:46-128
    TemplateSumSquaredError.U8 / .F32           F:alg/feature/detect/template/TemplateSumSquaredError.java:46-144
    TemplateNCC.U8 / .F32                       F:alg/feature/detect/template/TemplateNCC.java:54-274
    TemplateMatching.process                    F:alg/feature/detect/template/TemplateMatching.java:117-176

The evaluators are vectorised across the output positions and loop over the template elements in row-major order on np.float32 / np.int32
arrays, so every position sees the reference's order of operations (NumPy does not fuse a multiply into an add, and its int32 arrays wrap as
Java's int does).  An image is a 2-D uint8 (GrayU8) or float32 (GrayF32) array.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fast_ref  # noqa: E402  (the strict block non-maximum suppression, Min and Max)

SAD, SSE, NCC, CORRELATION = "SUM_ABSOLUTE_DIFFERENCE", "SUM_SQUARE_ERROR", "NCC", "CORRELATION"
SCORES = (SAD, SSE, NCC)
F_EPS = np.float32(2.0 ** -21)   # UtilEjml.F_EPS = (float)Math.pow(2, -21); EJML is not in the reference tree: parity unpinned against the jar
FLOAT_MAX = float(np.finfo(np.float32).max)
f32 = np.float32


def is_maximize(score):
    return score == NCC


def borders(tw, th):
    """(borderX0, borderY0, borderX1, borderY1)"""
    return tw // 2, th // 2, tw - tw // 2, th - th // 2


def ncc_template_stats(template):
    """TemplateNCC.setupTemplate: (area, templateMean, templateSigma), sequential fp32"""
    th, tw = template.shape
    area = f32(tw * th)
    mean = f32(0)
    for v in template.reshape(-1):
        mean = f32(mean + f32(v))
    mean = f32(mean / area)
    sigma = f32(0)
    for v in template.reshape(-1):
        diff = f32(f32(v) - mean)
        sigma = f32(sigma + f32(diff * diff))
    return area, mean, f32(np.sqrt(f32(sigma / area)))


def _evaluate_all(image, template, mask, score):
    """evaluate(x, y) / evaluateMask(x, y) for every x < w, y < h -> float32 [h, w]"""
    H, W = image.shape
    th, tw = template.shape
    h, w = H - th + 1, W - tw + 1
    u8 = image.dtype == np.uint8
    work = np.int32 if u8 else np.float32
    img = image.astype(work)
    tpl = template.astype(work)
    msk = None if mask is None else mask.astype(work)
    total = np.zeros((h, w), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if score in (SAD, SSE):
            div = f32(f32(255.0) * f32(255.0))
            for j in range(th):
                row = np.zeros((h, w), work)
                for i in range(tw):
                    win = img[j:j + h, i:i + w]
                    e = win - tpl[j, i]
                    if score == SAD:
                        term = np.abs(e) if msk is None else msk[j, i] * np.abs(e)
                    else:
                        term = e * e if msk is None else (msk[j, i] * e) * e
                    row = row + term
                rowf = row.astype(np.float32)
                total = total + (rowf if score == SAD else rowf / div)
            return total
        area, tmean, tsigma = ncc_template_stats(template)
        isum = np.zeros((h, w), work)
        for j in range(th):
            for i in range(tw):
                isum = isum + img[j:j + h, i:i + w]
        imean = isum.astype(np.float32) / area
        sigma = np.zeros((h, w), np.float32)
        top = np.zeros((h, w), np.float32)
        for j in range(th):
            for i in range(tw):
                diff = img[j:j + h, i:i + w].astype(np.float32) - imean
                sigma = sigma + diff * diff
                t = f32(f32(tpl[j, i]) - tmean)
                if msk is None:
                    top = top + diff * t
                else:
                    top = top + (f32(msk[j, i]) * diff) * t
        sigma = np.sqrt(sigma / area)
        return top / (F_EPS + sigma * tsigma)


def intensity(image, template, mask=None, score=SAD):
    """getIntensity() after setInputImage(image); process(template[, mask]) on a fresh object: float32 [H, W], 0 in the border"""
    image, template = np.asarray(image), np.asarray(template)
    assert image.dtype in (np.uint8, np.float32) and template.dtype == image.dtype and score in SCORES
    assert mask is None or (np.asarray(mask).shape == template.shape and np.asarray(mask).dtype == image.dtype)
    H, W = image.shape
    th, tw = template.shape
    assert 1 <= tw <= W and 1 <= th <= H
    out = np.zeros((H, W), np.float32)
    bx0, by0 = tw // 2, th // 2
    out[by0:by0 + H - th + 1, bx0:bx0 + W - tw + 1] = _evaluate_all(image, template, None if mask is None else np.asarray(mask), score)
    return out


def quick_select_index(data, k, n):
    """the project's restatement of org.ddogleg.sorting.QuickSelect.selectIndex(data, k, n, indexes) (oracle/boof_oracle.hpp quickSelectIndex):
    permutes data[0:n] in place and returns indexes"""
    idx = list(range(n))

    def swp(a, b):
        data[a], data[b] = data[b], data[a]
        idx[a], idx[b] = idx[b], idx[a]
    l, ir = 0, n - 1
    while True:
        if ir <= l + 1:
            if ir == l + 1 and data[ir] < data[l]:
                swp(l, ir)
            return idx
        mid, lp1 = (l + ir) >> 1, l + 1
        swp(mid, lp1)
        if data[l] > data[ir]:
            swp(l, ir)
        if data[lp1] > data[ir]:
            swp(lp1, ir)
        if data[l] > data[lp1]:
            swp(l, lp1)
        i, j = lp1, ir
        a, index_a = data[lp1], idx[lp1]
        while True:
            i += 1
            while data[i] < a:
                i += 1
            j -= 1
            while data[j] > a:
                j -= 1
            if j < i:
                break
            swp(i, j)
        data[lp1], data[j] = data[j], a
        idx[lp1], idx[j] = idx[j], index_a
        if j >= k:
            ir = j - 1
        if j <= k:
            l = i


def candidates(sub, maximize, radius=2):
    """the extractor of TemplateMatching on the intensity sub-image: ConfigExtract(2, -Float.MAX_VALUE, 0, true) maxima, or
    ConfigExtract(2, -Float.MAX_VALUE, 0, true, true, false) minima (thresholdMin = Float.MAX_VALUE) -> int16 [n, 2]"""
    mins, maxs = fast_ref.nonmax_block(sub, radius, FLOAT_MAX, -FLOAT_MAX, 0, not maximize, maximize)
    return maxs if maximize else mins


def select(sub, cand, max_matches, maximize):
    """TemplateMatching.process after the extractor -> (xy int16 [N, 2], score float32 [N]).  Match i shows -scores[indexes[i]], its own
    candidate's score, as TestTemplateMatching asserts; the restated selectIndex permutes the array it is given, so it gets a copy"""
    n = len(cand)
    sgn = f32(-1.0) if maximize else f32(1.0)
    scores = [f32(sgn * f32(sub[y, x])) for x, y in cand]
    N = min(max_matches, n)
    idx = quick_select_index(list(scores), N, n)
    xy = np.array([cand[idx[i]] for i in range(N)], np.int16).reshape(-1, 2)
    sc = np.array([-scores[idx[i]] for i in range(N)], np.float32)
    return xy, sc


def match(image, template, mask, score, max_matches, radius=2):
    """TemplateMatching: setMinimumSeparation(radius), setTemplate(template, mask, maxMatches), setImage(image), process(), getResults() ->
    (xy int16 [N, 2] top-left corners, score float32 [N], the intensity sub-image, the candidates)"""
    inten = intensity(image, template, mask, score)
    th, tw = np.asarray(template).shape
    H, W = inten.shape
    sub = inten[th // 2:th // 2 + H - th + 1, tw // 2:tw // 2 + W - tw + 1]
    cand = candidates(sub, is_maximize(score), radius)
    xy, sc = select(sub, cand, max_matches, is_maximize(score))
    return xy, sc, sub, cand


class JavaRandom:
    """java.util.Random: the documented linear congruential generator (nextInt(bound), nextFloat)"""

    def __init__(self, seed):
        self.seed = (int(seed) ^ 0x5DEECE66D) & ((1 << 48) - 1)

    def next(self, bits):
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        return self.seed >> (48 - bits)

    def nextInt(self, bound):
        if (bound & -bound) == bound:
            return (bound * self.next(31)) >> 31
        while True:
            bits = self.next(31)
            val = bits % bound
            if bits - val + (bound - 1) < (1 << 31):
                return val

    def nextFloat(self):
        return f32(self.next(24) / float(1 << 24))


def fill_uniform(img, rand, lo, hi):
    """ImageMiscOps.fillUniform(GrayU8 | GrayF32, rand, min, max), in place: min <= X < max"""
    flat = img.reshape(-1)
    if img.dtype == np.uint8:
        for i in range(flat.size):
            flat[i] = rand.nextInt(hi - lo) + lo
    else:
        rng = f32(f32(hi) - f32(lo))
        for i in range(flat.size):
            flat[i] = f32(f32(rand.nextFloat() * rng) + f32(lo))
