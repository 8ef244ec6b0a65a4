"""tests/hough_ref.py against the reference's own known-answer tests, re-expressed (no GPU):
  CommonHoughBinaryChecks.obviousLines as TestHoughParametersPolar.Binary configures it      F: src/test .../detect/line/*.java
  CommonHoughGradientChecks.obviousLines as TestHoughParametersFootOfNorm.Gradient configures it (GrayS16 and GrayF32 derivatives; GrayS32 and
  the polar gradient form are not built)
  the relaxed cases of GenericNonMaxTests: testNotStrictRule, checkBorderMaximum, checkCanDetectAlongImageBorder, compareToNaive (radii 1..4)
and the order sensitivity of the gradient votes on the very inputs tests/test_gpu_hough.py uses: without it a kernel that sums a cell's
contributions in another order could pass the GPU test.  The host side of boofcv_amd/lines.py (tables, weights, transformToLine, merge) is
compared with the restatement here as well; it needs no GPU."""
import math

import numpy as np
import pytest

import hough_cases as HC
import hough_ref as R

F = np.float32


def test_binary_polar_obvious_line():
    width, height = 30, 40
    image = np.zeros((height, width), np.uint8)
    image[:, 5] = 1
    # ConfigExtract(4, -1, 0, false) -> relaxed radius 4; the transform sets the threshold from thresholdCounts = relative(0.001, 1)
    lines, _, _, transform = R.binary_transform_lines(image, R.Polar(0.5, 180), 4, (1.0, 0.001), 1)
    assert transform.shape == (180, 50) and transform.sum() == 40 * 180
    assert len(lines) > 0
    for px, py, sx, sy in lines:
        assert abs(float(px) - 5) <= 0.1
        assert abs(float(sx)) <= 1e-4
        assert abs(abs(float(sy)) - 1) <= 0.1


@pytest.mark.parametrize("dtype", (np.int16, np.float32))
def test_gradient_foot_obvious_line(dtype):
    width, height = 30, 40
    binary = np.zeros((height, width), np.uint8)
    dx, dy = np.zeros((height, width), dtype), np.zeros((height, width), dtype)
    binary[:, 5] = 1
    dx[:, 5] = 20
    # ConfigExtract(4, 5, 0, true), HoughParametersFootOfNorm(5), maxLines 0, the refinement at its default radius of 3
    lines, _, found, transform = R.gradient_transform_lines(dx, dy, binary, R.FootOfNorm(5), 4, 5, 0)
    assert transform[20, 5] == 40 and np.count_nonzero(transform) == 1
    assert len(lines) == 1 and found[0] == 40
    px, py, sx, sy = (float(v) for v in lines[0])
    assert abs(px - 5) <= 0.1
    norm = math.hypot(sx, sy)
    assert abs(sx / norm) <= 0.1 and abs(abs(sy / norm) - 1) <= 0.1


def test_foot_of_norm_validity_compares_y_with_origin_x():
    par = R.FootOfNorm(5)
    par.initialize(30, 40)   # origin (15, 20)
    assert not par.is_transform_valid(15, 19) and not par.is_transform_valid(12, 18)
    assert par.is_transform_valid(15, 20)        # |20 - originX| = 5: valid although it is the origin itself
    assert par.is_transform_valid(10, 15)


def test_truncation_toward_zero_gives_a_negative_weight():
    """a parameter in (-1, 0) gives x0 = 0 and a negative weight for the second cell"""
    par = R.FootOfNorm(5)
    binary = np.zeros((9, 9), np.uint8)
    dx, dy = np.zeros((9, 9), F), np.zeros((9, 9), F)
    binary[0, 0] = 1                      # origin (4, 4): the pixel is at (-4, -4)
    dx[0, 0], dy[0, 0] = F(1.0), F(0.1)   # v = -4.4 / 1.01: the foot is at about (-0.356, 3.564)
    cell, weight = R.gradient_votes(dx, dy, binary, par)
    px, py = par.parameterize(np.array([0]), np.array([0]), dx[0, 0:1], dy[0, 0:1])
    assert -1 < float(px[0]) < 0 and 3 < float(py[0]) < 4
    assert cell.tolist() == [3 * 9 + 0, 3 * 9 + 1, 4 * 9 + 0, 4 * 9 + 1]
    assert weight[0] > 0 and weight[1] < 0 and weight[2] > 0 and weight[3] < 0
    t = R.sum_votes(cell, weight, (9, 9))
    assert t[3, 1] < 0 and t[4, 1] < 0


# ---- GenericNonMaxTests, relaxed rule, maxima ----
def test_relaxed_rule_reports_equal_neighbours():
    img = np.zeros((40, 30), F)
    img[5, 3] = img[6, 3] = img[5, 4] = 30
    img[5, 2] = img[7, 4] = img[7, 6] = -30
    found = R.nonmax_relaxed(img, 2, 5, 0)
    assert sorted(map(tuple, found.tolist())) == [(3, 5), (3, 6), (4, 5)]


def test_relaxed_border_defines_only_where_a_peak_may_lie():
    img = np.zeros((40, 30), F)
    img[1, 0], img[1, 1] = 90, 30
    assert R.nonmax_relaxed(img, 1, 5, 0).tolist() == [[0, 1]]
    assert len(R.nonmax_relaxed(img, 1, 5, 1)) == 0


def test_relaxed_detects_along_the_image_border():
    w, h = 30, 40
    img = np.zeros((h, w), F)
    img[0, w // 2] = img[h - 1, w // 2] = img[h // 2, 0] = img[h // 2, w - 1] = 90
    assert len(R.nonmax_relaxed(img, 2, 5, 0)) == 4


@pytest.mark.parametrize("radius", (1, 2, 3, 4))
def test_relaxed_block_search_equals_the_naive_rule(radius):
    rng = np.random.RandomState(2134 + radius)
    for _ in range(10):
        img = np.clip(rng.normal(0, 3, (40, 30)), -100, 100).astype(F)
        found = R.nonmax_relaxed(img, radius, 0.6, 0)
        naive = R.nonmax_relaxed_naive(img, radius, 0.6, 0)
        assert len(found) > 0 and len(found) == len(naive)
        assert set(map(tuple, found.tolist())) == naive


def test_relaxed_quirks():
    img = np.full((5, 7), F(3))
    every = R.nonmax_relaxed(img, 1, 3, 0)            # a plateau equal to the threshold: every cell, block by block
    assert len(every) == 35 and every[:4].tolist() == [[0, 0], [1, 0], [0, 1], [1, 1]]
    img[2, 2] = R.FLOAT_MAX                           # a block whose peak is Float.MAX_VALUE reports nothing, and it beats its neighbours
    found = set(map(tuple, R.nonmax_relaxed(img, 1, 3, 0).tolist()))
    assert (2, 2) not in found and (3, 3) not in found and (0, 0) in found and (6, 4) in found


# ---- the order of the gradient sum matters on the GPU test's inputs ----
@pytest.mark.parametrize("case", ("noise100", "noise10", "column47", "s16"))
@pytest.mark.parametrize("size", HC.LARGE)
def test_reverse_order_changes_bits_on_the_gpu_test_inputs(case, size):
    w, h = size
    dx, dy, binary = HC.gradient_case(case, w, h)
    changed = 0
    for b in range(3):
        cell, weight = R.gradient_votes(dx[b], dy[b], binary[b], R.FootOfNorm(5))
        fwd = R.sum_votes(cell, weight, (h, w))
        rev = R.sum_votes(cell, weight, (h, w), reverse=True)
        changed += int(np.count_nonzero(fwd.view(np.int32) != rev.view(np.int32)))
    assert changed > 0, "summing in reverse raster order gives the same bits: these inputs cannot tell the orders apart"


def test_extreme_gradients_cover_nan_and_saturation():
    dx, dy, binary = HC.gradient_case("extremes", 61, 47)
    par = R.FootOfNorm(5)
    par.initialize(61, 47)
    ys, xs = np.nonzero(binary[0])
    px, py = par.parameterize(xs, ys, dx[0][ys, xs], dy[0][ys, xs])
    assert np.isnan(px).any() and np.isinf(px).any()
    x0 = R.java_f2i(px)
    assert (x0 == R.INT_MAX).any() and (R.wrap_i32(x0.astype(np.int64) + 1) == R.INT_MIN).any()
    t = R.hough_gradient(dx[0], dy[0], binary[0], par)
    assert np.isnan(t[0, 0]) and np.isnan(t[1, 1])       # (int) NaN = 0: the four cells around (0, 0) take NaN weights
    assert np.isfinite(t[5:, 5:]).all()


# ---- the host side of boofcv_amd/lines.py equals the restatement ----
def test_mirror_tables_and_weights():
    from boofcv_amd import lines
    for n in (180, 7, 2):
        t = lines.CachedSineCosine_F32(0.0, F(math.pi), n)
        c, s = R.cached_sine_cosine(0.0, F(math.pi), n)
        assert t.c.tobytes() == c.tobytes() and t.s.tobytes() == s.tobytes()
    c, s = R.cached_sine_cosine(0.0, F(math.pi), 180)
    assert c[0] == 1 and s[0] == 0 and c[179] == -1 and abs(float(c[90])) < 0.01
    for r in (1, 3, 5):
        wgt = lines.weightPixelGaussian(r)
        assert wgt.tobytes() == R.weight_gaussian(r).tobytes() and abs(float(wgt.sum()) - 1) < 1e-5 and wgt.argmax() == (2 * r + 1) ** 2 // 2


def test_mirror_merge_equals_the_restatement():
    from boofcv_amd import lines
    rng = np.random.RandomState(5)
    w, h = 120, 90
    for trial in range(6):
        n = 25
        ang = rng.rand(n) * math.pi
        if trial % 2:
            ang = np.round(ang * 4) / 4 + rng.rand(n) * 0.05      # near-parallel groups, so that pairs merge
        raw = [(F(rng.rand() * w), F(rng.rand() * h), F(math.cos(a)), F(math.sin(a))) for a in ang]
        inten = (rng.randint(1, 6, n) * 10).astype(F)           # ties: the comparator's position rules decide
        for max_lines in (10, 3):
            want = R.merge_lines(raw, inten, math.pi * 0.05, 10.0, max_lines, w, h)
            post = lines.ImageLinePruneMerge()
            for l, v in zip(raw, inten):
                post.add(lines.LineParametric2D_F32(*l), v)
            post.pruneSimilar(F(math.pi * 0.05), F(10.0), w, h)
            post.pruneNBest(max_lines)
            got = [(l.p.x, l.p.y, l.slope.x, l.slope.y) for l in post.createList()]
            assert got == want and 0 < len(got) <= max_lines
        assert len(R.merge_lines(raw, inten, math.pi * 0.05, 10.0, n, w, h)) < n   # something merged


def test_mirror_defaults_and_refusals():
    from boofcv_amd import lines
    from boofcv_amd.api import GrayF32, GrayS32, GrayU8, IllegalArgumentException
    b, g, p, f = lines.ConfigHoughBinary(), lines.ConfigHoughGradient(), lines.ConfigParamPolar(), lines.ConfigParamFoot()
    assert (b.localMaxRadius, b.maxLines, b.mergeDistance, b.minCounts.length, b.minCounts.fraction) == (1, 10, 10.0, 1.0, 0.001)
    assert (g.localMaxRadius, g.minCounts, g.minDistanceFromOrigin, g.thresholdEdge, g.maxLines, g.refineRadius) == (2, 5, 5, 30.0, 0, 3)
    assert (p.resolutionRange, p.numBinsAngle, f.minDistanceFromOrigin) == (2.0, 180, 5)
    assert b.mergeAngle == g.mergeAngle == math.pi * 0.05
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.houghLinePolar(lines.ConfigHoughGradient(), None, GrayU8)
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.houghLineFootSub(None, GrayU8)
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.lineRansac(None, GrayF32)
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.houghLineFoot(None, None, GrayS32)
    with pytest.raises(IllegalArgumentException):
        lines.HoughTransformGradient(2, 5, lines.HoughParametersFootOfNorm(5), GrayS32)
    with pytest.raises(IllegalArgumentException):
        lines.HoughTransformGradient(2, 5, lines.HoughParametersPolar(2.0, 180))
    det = lines.FactoryDetectLine.houghLineFoot(None, None, GrayU8)
    assert det.getInputType() is GrayU8 and det.getThresholdEdge() == 30 and det.getHough().getRefineRadius() == 3
    det = lines.FactoryDetectLine.houghLinePolar(None, None, None, GrayU8)
    assert det.getHough().getMaxLines() == 10 and det.getThresholder().config.type.name == "GLOBAL_OTSU"
    with pytest.raises(IllegalArgumentException):   # what the threshold kernels refuse stays refused
        lines.FactoryDetectLine.houghLinePolar(None, None, None, GrayF32)
