"""CPU: tests/disparity_ref.py (the NumPy reference of the GPU block matching) against the reference's own tests, and the new Python surface.

    FT: = main/boofcv-feature/src/test/java/boofcv/

  ChecksSelectErrorWithChecksWta (maxError, testRightToLeftValidation, confidenceFlatRegion, confidenceMultiplePeak)
                                  FT:alg/feature/disparity/block/select/ChecksSelectErrorWithChecksWta.java:65-219
  addSubpixelBias                 FT:alg/feature/disparity/block/select/TestSelectErrorSubpixel.java:86-109
  BasicDisparityTests             FT:alg/feature/disparity/block/score/BasicDisparityTests.java:68-142 (as ChecksDisparityBM.basicTest configures it)
"""
import numpy as np
import pytest

import disparity_ref as dr

W_, H_ = 20, 25   # ChecksSelectErrorWithChecksWta.w, .h


def _selector(scores, minDisparity, maxDisparity, radiusX, maxError, rtol, texture, subpixel, y=3):
    """createSelector(maxError, rtol, texture).configure(disparity, min, max, radiusX).process(y, scores) on an image filled with `reject`,
    as init() does; -> getDisparity(x, y) of the test (Math.round)"""
    reject = (maxDisparity - minDisparity) + 1
    disparity = np.full((H_, W_), reject, np.float32 if subpixel else np.uint8)
    dr.select_row(np.asarray(scores), W_, minDisparity, maxDisparity, radiusX, maxError, rtol, texture, subpixel, disparity[y])
    return lambda x: int(np.floor(float(disparity[y, x]) + 0.5)), reject


@pytest.mark.parametrize("subpixel", [False, True], ids=["DispU8", "S32_F32"])
def test_selector_max_error(subpixel):
    scores = np.zeros(W_ * 10, np.int64)
    for d in range(10):
        for x in range(W_):
            scores[W_ * d + x] = 5 if d == 0 else x
    get, reject = _selector(scores, 0, 10, 2, 2, -1, -1, subpixel)
    assert get(1 + 2) == 1
    assert abs(get(2 + 2) - 1) <= 1
    assert get(3 + 2) == reject and get(4 + 2) == reject
    get, _ = _selector(scores, 0, 10, 2, 20, -1, -1, subpixel)
    assert abs(get(3 + 2) - 1) <= 1 and abs(get(4 + 2) - 1) <= 1


@pytest.mark.parametrize("subpixel", [False, True], ids=["DispU8", "S32_F32"])
@pytest.mark.parametrize("minDisparity", [0, 2])
def test_selector_right_to_left_validation(subpixel, minDisparity):
    maxDisparity, r = 10, 2
    rangeDisparity = maxDisparity - minDisparity
    scores = np.zeros(W_ * rangeDisparity, np.int64)
    for d in range(rangeDisparity):
        for x in range(W_):
            scores[W_ * d + x] = abs(d - 5)
    get, reject = _selector(scores, minDisparity, maxDisparity, r, -1, 1, -1, subpixel)
    for i in range(r + minDisparity):                                   # "outside the border should be 'reject'"
        assert get(i + r) == reject
    for i in range(r):                                                  # the columns process() never writes: what init() filled in
        assert get(i) == reject
    for i in range(r + minDisparity, r + 4 + minDisparity):
        assert get(i) == reject
    assert get(4 + r + minDisparity) == 4
    for i in range(r + minDisparity + 5, W_ - r):
        assert get(i) == 5
    get, reject = _selector(scores, minDisparity, maxDisparity, 2, -1, 0, -1, subpixel)
    assert get(4 + r + minDisparity) == reject


@pytest.mark.parametrize("subpixel", [False, True], ids=["DispU8", "S32_F32"])
def test_selector_confidence_flat_region(subpixel):
    scores = np.zeros(W_ * 10, np.int64)
    for d in range(10):
        for x in range(W_):
            scores[W_ * d + x] = 3 + abs(2 - d)
    get, reject = _selector(scores, 0, 10, 2, -1, -1, 3, subpixel)
    assert get(4 + 2) == reject


@pytest.mark.parametrize("subpixel", [False, True], ids=["DispU8", "S32_F32"])
@pytest.mark.parametrize("minValue,minDisparity", [(3, 0), (0, 0), (3, 2), (0, 2)])
def test_selector_confidence_multiple_peak(subpixel, minValue, minDisparity):
    r = 2
    scores = np.zeros(W_ * 10, np.int64)
    for d in range(10):
        for x in range(W_):
            scores[W_ * d + x] = minValue + (d % 3)
    get, reject = _selector(scores, minDisparity, 10, r, -1, -1, 3, subpixel)
    for i in range(r + minDisparity + 3, W_ - r):
        assert get(i) == reject


def test_add_subpixel_bias():
    columnScore = np.zeros(20, np.int64)
    columnScore[4], columnScore[5], columnScore[6] = 100, 50, 200
    v, interpolated = dr.set_disparity_subpixel(columnScore, 20, 5)
    assert interpolated and 4 < v < 5 and v.dtype == np.float32
    assert v == np.float32(5) + np.float32(-100) / np.float32(2 * 200)
    columnScore[4], columnScore[6] = 200, 100
    v, _ = dr.set_disparity_subpixel(columnScore, 20, 5)
    assert 5 < v < 6
    # the ends of the search and the rejection value are stored as they are
    assert dr.set_disparity_subpixel(columnScore, 20, 0) == (np.float32(0), False)
    assert dr.set_disparity_subpixel(columnScore, 20, 19) == (np.float32(19), False)
    assert dr.set_disparity_subpixel(columnScore, 20, 21) == (np.float32(21), False)


@pytest.mark.parametrize("minDisparity", [0, 6])
def test_basic_disparity_tests(minDisparity):
    """checkGradient (min 0, disparity 5) / checkMinimumDisparity (min 6, disparity 4); radius 2 x 3, checks off, subpixel = false"""
    w, h, maxDisparity = 50, 60, 40
    disparity = 5 if minDisparity == 0 else 4
    yy, xx = np.mgrid[0:h, 0:w]
    left, right = (10 + xx + yy).astype(np.uint8), (10 + xx + disparity + yy).astype(np.uint8)
    out, cls = dr.block_match(left, right, minDisparity, maxDisparity - minDisparity, 2, 3, 0, -1, 0.0, subpixel=False)
    fill = maxDisparity - minDisparity                  # the test's image starts at 0; the wrapper's at getInvalidValue()
    borderX, borderY = 2, 3
    assert (out[:borderY] == fill).all() and (out[h - borderY:] == fill).all()
    for y in range(borderY, h - borderY):
        assert (out[y, :borderX + minDisparity] == fill).all() and (out[y, w - borderX:] == fill).all()
        if minDisparity == 0:
            assert (out[y, borderX + disparity:w - borderX] == disparity).all()
        else:
            assert (out[y, borderX + minDisparity:w - borderX].astype(int) + minDisparity == minDisparity).all()
    assert (cls[borderY:h - borderY, borderX + minDisparity:w - borderX] == dr.VALID_INT).all()
    assert dr.class_counts(cls)[dr.BORDER] == w * h - (h - 2 * borderY) * (w - 2 * borderX - minDisparity)


@pytest.mark.parametrize("minDisparity", [0, 4])
def test_cumulative_sum_cost_equals_the_four_loop_cost(minDisparity):
    W, H, rx, ry, rangeDisparity = 30, 9, 3, 1, 12
    rng = np.random.RandomState(234)
    left, right = rng.randint(0, 256, (H, W)).astype(np.uint8), rng.randint(0, 256, (H, W)).astype(np.uint8)
    scores = dr.sad_scores(left, right, minDisparity, minDisparity + rangeDisparity, rx, ry)
    assert sorted(scores) == list(range(ry, H - ry))
    n = 0
    for y, row in scores.items():
        for c in range(minDisparity, W - (2 * rx + 1) + 1):
            for i in range(min(c - minDisparity + 1, rangeDisparity)):
                assert row[W * i + (c - minDisparity)] == dr.naive_cost(left, right, y, c, i, minDisparity, rx, ry)
                n += 1
    assert n > 1000


def test_texture_products_wrap_like_java_ints():
    """range = 3, best = 1: no disparity is left for the second best, secondBest = Integer.MAX_VALUE and 10000 * (secondBest - scoreBest) wraps to a
    negative int, so the pixel is rejected; a 64-bit evaluation accepts it"""
    W = 12
    scores = np.zeros(W * 3, np.int64)
    scores[0 * W:1 * W], scores[1 * W:2 * W], scores[2 * W:3 * W] = 50, 10, 50
    out, cls = np.full(W, 3, np.uint8), np.zeros(W, np.uint8)
    dr.select_row(scores, W, 0, 3, 1, -1, -1, 0.15, False, out, cls)
    full = range(2 + 1, W - 1)                           # columns with lm == 3 (block start c >= 2), as pixels c + rx
    assert all(cls[x] == dr.REJECT_TEXTURE and out[x] == 4 for x in full)
    assert dr.i32(10000 * (dr.INT_MAX - 10)) < 0 <= dr.i32(1500 * 10) and 10000 * (dr.INT_MAX - 10) > 1500 * 10
    assert cls[1] == dr.VALID_INT and cls[2] == dr.VALID_INT and out[2] == 1      # lm = 1, 2: the test does not run
    out32, cls32 = np.full(W, 3, np.float32), np.zeros(W, np.uint8)
    dr.select_row(scores, W, 0, 3, 1, -1, -1, 0.0, True, out32, cls32)
    assert all(cls32[x] == dr.VALID_INTERP and out32[x] == 1.0 for x in full)     # texture off: kept, and c0 == c2 interpolates to 1


def test_right_to_left_search_clipped_by_the_image():
    """selectRightToLeft stops at localMax = min(W - rw, col + maxDisparity) - col - minDisparity: when the image clips it, the j whose left block
    would start at column W - rw is left out although that block exists"""
    W, rw, maxDisparity = 12, 3, 4
    scores = np.full(W * maxDisparity, 9, np.int64)
    col = 7                                              # left starts 7 .. 10 exist (W - rw = 9 is the last block start: j <= 2)
    scores[W * 2 + col + 2] = 1                          # j = 2: left block at column 9 = W - rw, the best of all
    scores[W * 1 + col + 1] = 5                          # j = 1
    assert dr.select_right_to_left(col, scores, W, rw, 0, maxDisparity) == 1
    assert dr.select_right_to_left(col - 3, scores, W, rw, 0, maxDisparity) == 0           # not clipped: 4 candidates, all 9
    scores[W * 3 + (col - 3) + 3] = 2
    assert dr.select_right_to_left(col - 3, scores, W, rw, 0, maxDisparity) == 3
    assert dr.select_right_to_left(W - rw, scores, W, rw, 0, maxDisparity) == 0            # localMax = 0: j = 0 alone


def test_block_match_refusals_of_the_reference():
    img = np.zeros((20, 60), np.uint8)
    base = dict(minDisparity=0, rangeDisparity=10, regionRadiusX=2, regionRadiusY=2)
    dr.block_match(img, img, **base)
    dr.block_match(img, img, **dict(base, rangeDisparity=56))
    for kw in (dict(minDisparity=-1), dict(rangeDisparity=0), dict(rangeDisparity=57), dict(minDisparity=50, rangeDisparity=7), dict(regionRadiusY=10)):
        with pytest.raises(ValueError):
            dr.block_match(img, img, **dict(base, **kw))
    with pytest.raises(ValueError):
        dr.block_match(np.zeros((9, 300), np.uint8), np.zeros((9, 300), np.uint8), rangeDisparity=254, regionRadiusX=2, regionRadiusY=1, subpixel=False)
    out, _ = dr.block_match(np.zeros((9, 300), np.uint8), np.zeros((9, 300), np.uint8), rangeDisparity=253, regionRadiusX=2, regionRadiusY=1, subpixel=False)
    assert out.dtype == np.uint8


SCENES = [(131, 19, 0, 100, 3, 2, 30, 1, .15), (259, 17, 5, 120, 4, 3, 30, 0, .1)]


@pytest.mark.parametrize("case", SCENES, ids=lambda c: "%dx%d" % c[:2])
def test_scene_has_every_class(case):
    """the pairs of tests/test_gpu_disparity.py: at least 10 pixels of each of the five classes that are not the border, so that a GPU result
    cannot be equal to the reference by rejecting everything"""
    W, H, minD, rng, rx, ry, mpe, rtol, tex = case
    left, right = dr.stereo_scene(W, H, minD, rng, 1)
    assert left.shape == right.shape == (H, W) and left.dtype == right.dtype == np.uint8
    disp, cls = dr.block_match(left, right, minD, rng, rx, ry, mpe, rtol, tex, subpixel=True)
    counts = dr.class_counts(cls)
    print(dict(zip(dr.CLASS_NAMES, counts)))
    assert counts[dr.BORDER] == W * H - (H - 2 * ry) * (W - 2 * rx - minD)
    assert all(c >= 10 for c in counts[1:]), counts
    assert (disp[cls == dr.BORDER] == rng).all()
    rejected = (cls == dr.REJECT_ERROR) | (cls == dr.REJECT_RTOL) | (cls == dr.REJECT_TEXTURE)
    assert (disp[rejected] == rng + 1).all()
    valid = disp[(cls == dr.VALID_INT) | (cls == dr.VALID_INTERP)]
    assert (valid >= 0).all() and (valid < rng).all()
    frac = disp[cls == dr.VALID_INTERP]
    assert (frac != np.floor(frac)).sum() >= 10
    u8, cls8 = dr.block_match(left, right, minD, rng, rx, ry, mpe, rtol, tex, subpixel=False)
    assert ((cls8 == dr.VALID_INT) == ((cls == dr.VALID_INT) | (cls == dr.VALID_INTERP))).all()


def test_wrap_scene_rejects_through_the_wrapped_product():
    """the 48 x 11, range 3 pair of tests/test_gpu_disparity.py: every texture rejection there has best == 1 with lm == 3, i.e. comes from the
    wrapped product, and there are at least 10 of them"""
    left, right = dr.stereo_scene(48, 11, 0, 3, 1)
    _, cls = dr.block_match(left, right, 0, 3, 2, 2, 0, -1, .15, subpixel=True)
    n = 0
    for y, row in dr.sad_scores(left, right, 0, 3, 2, 2).items():
        for c in range(2, 48 - 5 + 1):
            if cls[y, c + 2] == dr.REJECT_TEXTURE:
                assert int(np.argmin(row[c + 48 * np.arange(3)])) == 1
                n += 1
    assert n >= 10 and n == dr.class_counts(cls)[dr.REJECT_TEXTURE]


def test_config_defaults_and_validity():
    from boofcv_amd import api, _lib
    c = api.ConfigDisparityBM()
    assert (c.minDisparity, c.rangeDisparity, c.regionRadiusX, c.regionRadiusY, c.maxPerPixelError, c.validateRtoL, c.texture, c.subpixel, c.errorType) == \
        (0, 100, 3, 3, 0, 1, 0.15, True, api.DisparityError.SAD)
    c.checkValidity()
    for kw in (dict(minDisparity=-1), dict(rangeDisparity=0)):
        with pytest.raises(api.IllegalArgumentException):
            api.ConfigDisparityBM(**kw).checkValidity()
    assert not api.DisparityError.isCorrelation(api.DisparityError.SAD) and not api.DisparityError.isCorrelation(api.DisparityError.CENSUS)
    assert api.DisparityError.isCorrelation(api.DisparityError.NCC)
    d = _lib.DisparityBmCfg()
    _lib.load().bhip_disparity_bm_cfg_default(d)
    assert (d.minDisparity, d.rangeDisparity, d.regionRadiusX, d.regionRadiusY, d.maxPerPixelError, d.validateRtoL, d.texture) == (0, 100, 3, 3, 0.0, 1, 0.15)
    s = c._c()
    assert (s.minDisparity, s.rangeDisparity, s.regionRadiusX, s.regionRadiusY, s.maxPerPixelError, s.validateRtoL, s.texture) == (0, 100, 3, 3, 0.0, 1, 0.15)


def test_factory_refusals():
    from boofcv_amd import api
    F, Cfg, IAE = api.FactoryStereoDisparity, api.ConfigDisparityBM, api.IllegalArgumentException
    # where FactoryStereoDisparity.blockMatch and the constructors it calls throw IllegalArgumentException
    with pytest.raises(IAE, match="must be GrayF32"):
        F.blockMatch(Cfg(subpixel=True), api.GrayU8, api.GrayU8)
    with pytest.raises(IAE, match="must be GrayU8"):
        F.blockMatch(Cfg(subpixel=False), api.GrayU8, api.GrayF32)
    with pytest.raises(IAE, match="Unsupported error type"):
        F.blockMatch(Cfg(errorType=None), api.GrayU8, api.GrayF32)
    with pytest.raises(IAE, match="Unsupported image type"):
        F.blockMatch(Cfg(), api.GrayS32, api.GrayF32)
    with pytest.raises(IAE, match="Min disparity"):
        F.blockMatch(Cfg(minDisparity=-1), api.GrayU8, api.GrayF32)
    with pytest.raises(IAE, match="Max disparity"):
        F.blockMatch(Cfg(minDisparity=0, rangeDisparity=0), api.GrayU8, api.GrayF32)
    with pytest.raises(IAE, match="Min disparity"):
        F.blockMatch(Cfg(minDisparity=3, rangeDisparity=0), api.GrayU8, api.GrayF32)
    # what the reference has and the GPU does not: not an IllegalArgumentException, so that a caller can tell the two apart
    for call in (lambda: F.blockMatch(Cfg(errorType=api.DisparityError.CENSUS), api.GrayU8, api.GrayF32),
                 lambda: F.blockMatch(Cfg(errorType=api.DisparityError.NCC), api.GrayU8, api.GrayF32),
                 lambda: F.blockMatch(Cfg(), api.GrayF32, api.GrayF32),
                 lambda: F.blockMatch(Cfg(), api.GrayS16, api.GrayF32),
                 lambda: F.blockMatchBest5(None, api.GrayU8, api.GrayF32),
                 lambda: F.sgm(None, api.GrayU8, api.GrayF32),
                 lambda: F.regionSparseWta(0, 10, 2, 2, 30, 0.1, True, api.GrayU8)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert not isinstance(e.value, IAE)
