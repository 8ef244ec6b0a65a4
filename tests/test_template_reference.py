"""CPU checks of the template matching reference (tests/template_ref.py) against the reference implementation's own tests
(GeneralTemplateMatchTests with Random(344), a 30x40 image and a 5x8 template; TestTemplateMatching), against a naive per-pixel scalar loop,
and of the public surface the GPU path is reached through (header, ctypes table, Python mirror).  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import template_ref as tr   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("bhip_template_intensity_u8", "bhip_template_intensity_f32", "bhip_template_intensity_dev_u8", "bhip_template_intensity_dev_f32",
               "bhip_template_select_f32", "bhip_template_select_dev_f32")
DTYPES = (np.uint8, np.float32)
f32 = np.float32


class Fixture:
    """GeneralTemplateMatchTests' constructor: rand = Random(344), image 30x40, template and mask 5x8, template filled uniformly from 50..60"""

    def __init__(self, dtype):
        self.rand = tr.JavaRandom(344)
        self.image = np.zeros((40, 30), dtype)
        self.template = np.zeros((8, 5), dtype)
        self.mask = np.zeros((8, 5), dtype)
        tr.fill_uniform(self.template, self.rand, 50, 60)

    def noise(self):
        tr.fill_uniform(self.image, self.rand, 0, 200)

    def set_template(self, x, y):
        self.image[y:y + 8, x:x + 5] = self.template


def found(inten, tw, th, score):
    """checkExpected's extractor on the sub-image without the border"""
    H, W = inten.shape
    bx0, by0, bx1, by1 = tr.borders(tw, th)
    sub = inten[by0:H - by1 + 1, bx0:W - bx1 + 1]
    return [tuple(p) for p in tr.candidates(sub, tr.is_maximize(score)).tolist()]


def check_expected(inten, tw, th, score, points, strict=False):
    f = found(inten, tw, th, score)
    assert len(f) >= len(points)
    for p in points:
        assert f.count(p) == 1, (p, f)
    if strict:
        assert len(f) == len(points)


def test_java_random_first_values():
    """java.util.Random(344): the template of the reference's tests lies in 50 <= T < 60, and the generator is the documented LCG"""
    r = tr.JavaRandom(0)
    assert r.nextInt(1 << 31 - 1) >= 0
    r = tr.JavaRandom(42)
    assert [r.nextInt(10) for _ in range(5)] == [0, 3, 8, 4, 0]   # new Random(42).nextInt(10) x 5
    for dt in DTYPES:
        t = Fixture(dt).template
        assert t.min() >= 50 and t.max() < 60 and len(np.unique(t)) > 3


@pytest.mark.parametrize("score", tr.SCORES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_borders(score, dtype):
    """border_nomask / border_Mask, and the border of the intensity image is 0 (fillBorder)"""
    fx = Fixture(dtype)
    fx.noise()
    assert tr.borders(5, 8) == (2, 4, 3, 4)
    for mask in (None, np.ones((8, 5), dtype)):
        inten = tr.intensity(fx.image, fx.template, mask, score)
        assert inten.shape == (40, 30) and inten.dtype == np.float32
        inner = np.zeros((40, 30), bool)
        inner[4:4 + 33, 2:2 + 26] = True
        assert not inten[~inner].any()


@pytest.mark.parametrize("score", tr.SCORES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_case(score, dtype):
    """singleCase: one match at (10,12); an all-ones mask gives the same answer.  negativeCase: no perfect zero elsewhere for SAD / SSE"""
    fx = Fixture(dtype)
    fx.noise()
    neg = tr.intensity(fx.image, fx.template, None, score)
    if score != tr.NCC:
        assert (neg[4:37, 2:28] != 0).all()
    fx.set_template(10, 12)
    a = tr.intensity(fx.image, fx.template, None, score)
    check_expected(a, 5, 8, score, [(10, 12)])
    b = tr.intensity(fx.image, fx.template, np.ones((8, 5), dtype), score)
    check_expected(b, 5, 8, score, [(10, 12)])
    assert np.array_equal(a.view(np.int32), b.view(np.int32))   # m = 1 multiplies exactly
    if score != tr.NCC:
        assert a[12 + 4, 10 + 2] == 0


@pytest.mark.parametrize("score", tr.SCORES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_same_size_img_template(score, dtype):
    fx = Fixture(dtype)
    fx.noise()
    for mask in (None, np.ones((40, 30), dtype)):
        inten = tr.intensity(fx.image, fx.image, mask, score)
        check_expected(inten, 30, 40, score, [(0, 0)], strict=True)
        assert np.count_nonzero(inten) <= 1


@pytest.mark.parametrize("score", tr.SCORES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("value", [0, 30])
def test_uniform_image(score, dtype, value):
    """uniformImage: every value is finite; NCC of a flat window is exactly 0 (top = 0, the denominator is EPS)"""
    fx = Fixture(dtype)
    fx.image[:] = value
    fx.set_template(5, 7)
    for mask in (None, np.ones((8, 5), dtype)):
        inten = tr.intensity(fx.image, fx.template, mask, score)
        assert np.isfinite(inten).all()
        if score == tr.NCC:
            assert inten[4 + 30, 2 + 20] == 0   # a window of the flat part


@pytest.mark.parametrize("score", tr.SCORES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_mask(score, dtype):
    fx = Fixture(dtype)
    fx.noise()
    fx.set_template(10, 12)
    inten = tr.intensity(fx.image, fx.template, np.zeros((8, 5), dtype), score)
    assert np.abs(inten).max() <= 1e-4
    assert not inten.any()


@pytest.mark.parametrize("score", tr.SCORES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_multiple_cases(score, dtype):
    fx = Fixture(dtype)
    fx.noise()
    fx.set_template(10, 12)
    fx.set_template(20, 16)
    for mask in (None, np.ones((8, 5), dtype)):
        check_expected(tr.intensity(fx.image, fx.template, mask, score), 5, 8, score, [(10, 12), (20, 16)])


def _fill_border(a, value, r):
    a[:r, :] = value
    a[-r:, :] = value
    a[:, :r] = value
    a[:, -r:] = value


@pytest.mark.parametrize("score", tr.SCORES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_differentiate(score, dtype):
    """maskDifferentiate: with the changed template border masked out the match at (10,12) stands out more"""
    fx = Fixture(dtype)
    fx.noise()
    x, y, tw, th = 10, 12, 15, 15
    template = np.zeros((th, tw), dtype)
    tr.fill_uniform(template, fx.rand, 0, 200)
    _fill_border(template, 150, 2)
    fx.image[y - th // 2:y - th // 2 + th, x - tw // 2:x - tw // 2 + tw] = template
    _fill_border(template, 20, 2)
    _fill_border(template, 50, 1)
    maximize = tr.is_maximize(score)

    def fractions(inten):
        # ImageStatistics over the whole intensity image, border included; mean in double
        lo, hi, value, average = inten.min(), inten.max(), inten[y, x], f32(inten.astype(np.float64).mean())
        if maximize:
            return (value - lo) / (hi - lo), (average - lo) / (hi - lo)
        return (hi - value) / (hi - lo), (hi - average) / (hi - lo)

    value_no, average_no = fractions(tr.intensity(fx.image, template, None, score))
    mask = np.full((th, tw), 100 if dtype == np.uint8 else 1, dtype)
    _fill_border(mask, 0, 2)
    value_mask, average_mask = fractions(tr.intensity(fx.image, template, mask, score))
    assert value_mask >= value_no
    assert (value_mask / average_mask) * 0.9 > value_no / average_no


# ---- the restatement against a naive per-pixel scalar loop ----
def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def evaluate_scalar(image, template, mask, score, tlx, tly):
    """one evaluate(tl_x, tl_y) / evaluateMask as the Java reads, scalars only"""
    th, tw = template.shape
    u8 = image.dtype == np.uint8
    if score in (tr.SAD, tr.SSE):
        total, div = f32(0), f32(f32(255.0) * f32(255.0))
        for yy in range(th):
            row = 0 if u8 else f32(0)
            for xx in range(tw):
                if u8:
                    e = int(image[tly + yy, tlx + xx]) - int(template[yy, xx])
                    m = 1 if mask is None else int(mask[yy, xx])
                    row = _i32(row + (_i32(m * abs(e)) if score == tr.SAD else _i32(_i32(m * e) * e)))
                else:
                    e = f32(image[tly + yy, tlx + xx] - template[yy, xx])
                    if score == tr.SAD:
                        term = f32(abs(e)) if mask is None else f32(mask[yy, xx] * f32(abs(e)))
                    else:
                        term = f32(e * e) if mask is None else f32(f32(mask[yy, xx] * e) * e)
                    row = f32(row + term)
            rowf = f32(row)
            total = f32(total + (rowf if score == tr.SAD else f32(rowf / div)))
        return total
    area, tmean, tsigma = tr.ncc_template_stats(template)
    s = 0 if u8 else f32(0)
    for yy in range(th):
        for xx in range(tw):
            s = _i32(s + int(image[tly + yy, tlx + xx])) if u8 else f32(s + image[tly + yy, tlx + xx])
    mean = f32(f32(s) / area)
    top, sigma = f32(0), f32(0)
    for yy in range(th):
        for xx in range(tw):
            diff = f32(f32(image[tly + yy, tlx + xx]) - mean)
            sigma = f32(sigma + f32(diff * diff))
            t = f32(f32(template[yy, xx]) - tmean)
            top = f32(top + (f32(diff * t) if mask is None else f32(f32(f32(mask[yy, xx]) * diff) * t)))
    sigma = f32(np.sqrt(f32(sigma / area)))
    return f32(top / f32(tr.F_EPS + f32(sigma * tsigma)))


@pytest.mark.parametrize("score", tr.SCORES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [False, True])
def test_restatement_equals_the_scalar_loop(score, dtype, masked):
    rng = np.random.default_rng(5)
    if dtype == np.uint8:
        image = rng.integers(0, 256, (11, 13), dtype=np.uint8)
        template = rng.integers(0, 256, (3, 4), dtype=np.uint8)
        mask = rng.choice(np.array([0, 1, 3, 255], np.uint8), (3, 4))
    else:
        image = (rng.random((11, 13)) * 255).astype(np.float32)
        image[2, 3] = -7.25
        template = (rng.random((3, 4)) * 255).astype(np.float32)
        mask = rng.choice(np.array([0, 0.5, 1, 2.75], np.float32), (3, 4))
    m = mask if masked else None
    with np.errstate(over="ignore"):
        got = tr.intensity(image, template, m, score)
        for y in range(11 - 3 + 1):
            for x in range(13 - 4 + 1):
                want = evaluate_scalar(image, template, m, score, x, y)
                assert got[y + 1, x + 2].view(np.int32) == np.float32(want).view(np.int32), (x, y)
    assert not got[0].any() and not got[:, :2].any() and not got[-1].any() and not got[:, -1].any()   # rows 1..9 and columns 2..11 are evaluated


def test_masked_u8_sse_wraps_at_32_bits():
    """a row of 130 elements with mask 255 and error 255: 130 * 255 * 65025 = 2155578750 > 2^31 - 1, Java's int row total is negative"""
    image = np.full((1, 130), 255, np.uint8)
    template = np.zeros((1, 130), np.uint8)
    mask = np.full((1, 130), 255, np.uint8)
    with np.errstate(over="ignore"):
        got = tr.intensity(image, template, mask, tr.SSE)[0, 65]
    assert got == f32(f32(2155578750 - (1 << 32)) / f32(65025.0)) and got < 0
    assert got == evaluate_scalar(image, template, mask, tr.SSE, 0, 0)


# ---- TestTemplateMatching ----
def _dummy(expected, width=30, height=40):
    inten = np.zeros((height, width), np.float32)
    for x, y, s in expected:
        inten[y, x] = s
    return inten


def _check_results(xy, score, expected, ox, oy):
    assert len(xy) == len(expected)
    left = {(x - ox, y - oy): s for x, y, s in expected}
    for (x, y), s in zip(xy.tolist(), score.tolist()):
        assert left.pop((x, y)) == s


def test_template_matching_no_border():
    """basicTest_NOBORDER: the intensity has an unprocessed border of (4,5); the match at (0,0) lies inside it"""
    inten = _dummy([(10, 11, 15), (17, 15, 18), (0, 0, 18)])
    sub = inten[5:40 - 5 + 1, 4:30 - 4 + 1]
    xy, sc = tr.select(sub, tr.candidates(sub, True), 10, True)
    _check_results(xy, sc, [(10, 11, 15), (17, 15, 18)], 4, 5)


def test_template_matching_max_matches():
    """maxMatches: the two best of four, on the whole image (isBorderProcessed() = true only subtracts the offset)"""
    inten = _dummy([(10, 11, 15), (16, 15, 18), (0, 0, 19), (22, 30, 15)])
    cand = tr.candidates(inten, True)
    assert len(cand) == 4
    xy, sc = tr.select(inten, cand, 2, True)
    assert sorted(map(tuple, xy.tolist())) == [(0, 0), (16, 15)]
    assert sorted(sc.tolist()) == [18.0, 19.0]
    # all of them, which still goes through selectIndex (N == n): the same set, permuted
    xy, sc = tr.select(inten, cand, 10, True)
    assert sorted(map(tuple, xy.tolist())) == sorted(map(tuple, cand.tolist())) and len(sc) == 4


def test_template_and_image_same_size():
    """templateAndImageSameSize: a 1x1 sub-image whose only pixel is the match"""
    image = np.arange(30 * 40, dtype=np.float32).reshape(40, 30)
    xy, sc, sub, cand = tr.match(image, image, None, tr.SAD, 10)
    assert sub.shape == (1, 1) and xy.tolist() == [[0, 0]] and sc.tolist() == [-0.0]
    xy, sc, sub, cand = tr.match(image, image, None, tr.NCC, 10)
    assert xy.tolist() == [[0, 0]] and sc[0] > 0


def test_match_finds_the_planted_templates():
    fx = Fixture(np.uint8)
    fx.noise()
    fx.set_template(10, 12)
    fx.set_template(20, 16)
    for score in tr.SCORES:
        xy, sc, sub, cand = tr.match(fx.image, fx.template, None, score, 2)
        assert sorted(map(tuple, xy.tolist())) == [(10, 12), (20, 16)]
    xy, sc, sub, cand = tr.match(fx.image, fx.template, None, tr.SAD, 0)
    assert len(xy) == 0 and len(sc) == 0
    assert len(tr.select(sub, cand[:0], 3, False)[0]) == 0   # n == 0: no matches


def test_quick_select_keeps_the_k_smallest():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 7, 50):
        for k in sorted({0, 1, n // 2, n}):
            data = [f32(v) for v in rng.integers(0, 20, n)]
            orig = list(data)
            idx = tr.quick_select_index(data, k, n)
            assert sorted(idx) == list(range(n))
            assert [orig[i] for i in idx] == data                 # data is permuted the same way
            assert sorted(data[:k]) == sorted(orig)[:k]


# ---- the public surface ----
def test_header_ctypes_and_jni_name_the_new_exports():
    from boofcv_amd import _lib
    header = open(os.path.join(ROOT, "include", "boofhip.h")).read()
    jni = open(os.path.join(ROOT, "integration", "jni", "boofhip_jni.c")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and name in jni, name
    assert (_lib.BHIP_TEMPLATE_SAD, _lib.BHIP_TEMPLATE_SSE, _lib.BHIP_TEMPLATE_NCC, _lib.BHIP_TEMPLATE_CORRELATION) == (0, 1, 2, 3)
    for name, value in (("BHIP_TEMPLATE_MAX_WIDTH", _lib.BHIP_TEMPLATE_MAX_WIDTH), ("BHIP_TEMPLATE_MAX_CANDIDATES", _lib.BHIP_TEMPLATE_MAX_CANDIDATES)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert _lib.BHIP_TEMPLATE_MAX_WIDTH >= 64


def test_factory_refusals_and_properties_without_a_gpu():
    from boofcv_amd import api

    class NoGpu:
        _h = None
    T = api.TemplateScoreType
    for t in (T.SUM_ABSOLUTE_DIFFERENCE, T.SUM_SQUARE_ERROR, T.NCC):
        for it in (api.GrayU8, api.GrayF32):
            alg = api.FactoryTemplateMatching.createIntensity(t, it, ctx=NoGpu())
            assert alg.isMaximize() == (t == T.NCC) and alg.isBorderProcessed() is False
            m = api.FactoryTemplateMatching.createMatcher(t, it, ctx=NoGpu())
            assert m.extractor.canDetectMaximums() == (t == T.NCC) and m.extractor.canDetectMinimums() == (t != T.NCC)
            assert m.extractor.getSearchRadius() == 2
            m.setMinimumSeparation(5)
            assert m.extractor.getSearchRadius() == 5
        for it in (api.GrayS16, api.GrayS32):
            with pytest.raises(api.IllegalArgumentException):
                api.FactoryTemplateMatching.createIntensity(t, it, ctx=NoGpu())
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryTemplateMatching.createIntensity("MUTUAL_INFORMATION", api.GrayU8, ctx=NoGpu())
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryTemplateMatching.createIntensity(T.CORRELATION, api.GrayU8, ctx=NoGpu())
    with pytest.raises(RuntimeError, match="use the Java path") as e:
        api.FactoryTemplateMatching.createIntensity(T.CORRELATION, api.GrayF32, ctx=NoGpu())
    assert not isinstance(e.value, api.IllegalArgumentException)
    with pytest.raises(RuntimeError, match="use the Java path"):
        api.FactoryTemplateMatching.createMatcher(T.CORRELATION, api.GrayF32, ctx=NoGpu())
    # types that differ are refused before anything reaches the library
    alg = api.FactoryTemplateMatching.createIntensity(T.NCC, api.GrayU8, ctx=NoGpu())
    alg.setInputImage(api.GrayU8(30, 40))
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayF32(5, 8))
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayU8(5, 8), api.GrayF32(5, 8))
    assert api.Match(3, 4, 1.5) == api.Match(3, 4, 1.5)
