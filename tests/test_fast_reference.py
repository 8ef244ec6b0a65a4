"""CPU checks of the FAST / min-max NMS reference (tests/fast_ref.py) against the reference implementation's own known answers, and of the
public surface the GPU path is reached through (header, ctypes table, Python mirror).  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fast_ref as fr   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("bhip_fast_u8", "bhip_fast_f32", "bhip_fast_dev_u8", "bhip_fast_dev_f32", "bhip_nonmax_block_minmax_f32", "bhip_nonmax_block_minmax_dev_f32")


# ---- the reference's known answers ----
def test_circle_is_the_sixteen_offsets_of_discretized_circle():
    assert fr.CIRCLE == [(3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3), (0, -3), (1, -3), (2, -2),
                         (3, -1)]


@pytest.mark.parametrize("n", [9, 10, 11, 12])
@pytest.mark.parametrize("high", [True, False])
def test_perfect_circle(n, high):
    """GenericFastCorner.perfectCircle: 12x14, fill 99, centre 100, n contiguous ring pixels 255 / 0, all 16 rotations (tol 20)"""
    w, h = 12, 14
    for i in range(16):
        img = np.full((h, w), 99, np.uint8)
        for j in range(n):
            dx, dy = fr.CIRCLE[(i + j) % 16]
            img[h // 2 + dy, w // 2 + dx] = 255 if high else 0
        img[h // 2, w // 2] = 100
        inten, low, hi, _ = fr.fast(img, 20, n, 1.0)
        assert np.array_equal(hi if high else low, [[w // 2, h // 2]])
        if n == 9 and high:
            assert inten[h // 2, w // 2] == 1395.0   # 9 * 255 - 100 * 9


@pytest.mark.parametrize("n", [9, 12])
def test_check_intensity(n):
    """GenericFastCorner.checkIntensity: the circle at (4,5) is weaker than the circle at (12,20)"""
    img = np.zeros((50, 40), np.uint8)
    for (x, y), b in (((4, 5), 21), ((12, 20), 30)):
        for dx, dy in fr.CIRCLE[:n]:
            img[y + dy, x + dx] = b
    inten = fr.fast(img, 20, n, 1.0)[0]
    assert 0 < inten[5, 4] < inten[20, 12]


def _ring_image(centre, values, dtype):
    img = np.full((7, 7), centre, dtype)
    for (dx, dy), v in zip(fr.CIRCLE, values):
        img[3 + dy, 3 + dx] = v
    return img


def test_f32_total_truncates_toward_zero_after_every_addition():
    # nine ring pixels of 0.4 around 0.1, tol 0.2: a bright corner whose int total stays 0 -> 0 - 0.1f * 9 (negative)
    img = _ring_image(0.1, [0.4] * 9 + [0.1] * 7, np.float32)
    inten, low, high, _ = fr.fast(img, 0.2, 9, 1.0)
    assert len(low) == 0 and np.array_equal(high, [[3, 3]])
    assert inten[3, 3] == np.float32(0) - np.float32(0.1) * np.float32(9) and inten[3, 3] < 0
    # negative pixels: -2.5 nine times.  (int) truncates toward zero: 0 -> -2 -> -4 (-4.5) -> -6 -> -8 (-8.5) ... ; floor would give -3, -6, ...
    img = _ring_image(10.0, [-2.5] * 9 + [10.0] * 7, np.float32)
    inten, low, high, _ = fr.fast(img, 1.0, 9, 1.0)
    total = 0
    for _ in range(9):
        total = int(np.float32(total) + np.float32(-2.5))   # Python's int() truncates toward zero, like Java's (int)
    assert total == -18 and np.array_equal(low, [[3, 3]]) and len(high) == 0
    assert inten[3, 3] == np.float32(total) - np.float32(10.0) * np.float32(9)
    # saturation and NaN of Java's (int)
    assert list(fr.java_f2i(np.array([np.nan, 3e9, -3e9, -1.9, 1.9], np.float32))) == [0, 2147483647, -2147483648, -1, 1]


def test_early_stop_keeps_the_crossing_row_and_zeroes_the_rest():
    h, w = 16, 24
    flat = fr.fast(np.full((h, w), 50, np.uint8), 5, 9, 0.05)   # no corners: the limit is never reached, every row is processed
    assert len(flat[1]) == 0 and len(flat[2]) == 0 and flat[3] == h - 4
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    inten_all, low_all, high_all, stop_all = fr.fast(img, 20, 9, 1.0)
    assert stop_all == h - 4
    per_row = np.bincount(np.concatenate([low_all[:, 1], high_all[:, 1]]), minlength=h)
    limit = fr.max_features(0.05, w, h)
    assert limit == 19   # rows 3 .. 7 hold 3 + 3 + 4 + 5 + 5 = 20 corners: row 7 crosses the limit
    running = np.cumsum(per_row)
    expect = int(np.nonzero((running >= limit) & (np.arange(h) >= 3))[0][0])
    inten, low, high, stop = fr.fast(img, 20, 9, 0.05)
    assert stop == expect == 7 and len(low) + len(high) == 20
    assert np.array_equal(low, low_all[low_all[:, 1] <= stop]) and np.array_equal(high, high_all[high_all[:, 1] <= stop])
    assert len(low) + len(high) >= limit > running[stop - 1]   # the row that crossed the limit is kept whole
    assert np.array_equal(inten[:stop + 1], inten_all[:stop + 1]) and not inten[stop + 1:].any() and inten_all[stop + 1:].any()
    # a limit of 0: row 3 is still processed
    assert fr.fast(img, 20, 9, 1e-9)[3] == 3


@pytest.mark.parametrize("radius,border,threshold", [(1, 0, 0.0), (2, 3, 0.0), (3, 5, 50.0), (4, 0, 50.0)])
def test_block_nms_equals_the_brute_force_strict_rule(radius, border, threshold):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (37, 45), dtype=np.uint8)
    inten = fr.fast(img, 20, 9, 1.0)[0]
    assert (inten < 0).any() and (inten > 0).any()
    inten[10, 12] = fr.FLOAT_MAX     # exclusion markers
    inten[20, 30] = -fr.FLOAT_MAX
    bmin, bmax = fr.nonmax_brute(inten, radius, -threshold, border, True), fr.nonmax_brute(inten, radius, threshold, border, False)
    assert len(bmin) > 0 and len(bmax) > 0
    for dmin, dmax in ((True, False), (False, True), (True, True)):
        mins, maxs = fr.nonmax_block(inten, radius, -threshold, threshold, border, dmin, dmax)
        assert np.array_equal(mins, bmin if dmin else bmin[:0])
        assert np.array_equal(maxs, bmax if dmax else bmax[:0])


# ---- the surface ----
def test_header_and_ctypes_table_declare_the_new_exports():
    from boofcv_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "boofhip.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name


def test_config_fast_corner_defaults_and_validity():
    from boofcv_amd import api
    c = api.ConfigFastCorner()
    assert (c.pixelTol, c.minContinuous, c.maxFeatures) == (20, 9, 0.1)
    c.checkValidity()
    for bad in (dict(minContinuous=8), dict(minContinuous=13), dict(maxFeatures=-0.1), dict(maxFeatures=1.5)):
        with pytest.raises(api.IllegalArgumentException):
            api.ConfigFastCorner(**bad).checkValidity()
    api.ConfigFastCorner(maxFeatures=0.0).checkValidity()   # the config allows 0; FastCornerDetector.setMaxFeaturesFraction refuses it
    assert callable(api.FactoryDetectPoint.createFast) and callable(api.FactoryIntensityPointAlg.fast)


def test_min_and_max_extractor_configs_pass_the_config_check():
    """FactoryFeatureExtractor.nonmax no longer refuses strict detectMinimums configs (creating the extractor itself needs a GPU context, so
    only the config check is exercised here: with a GPU-less context stub)"""
    from boofcv_amd import api

    class NoGpu:
        _h = None
    for dmin, dmax in ((True, True), (True, False), (False, True), (False, False)):
        e = api.FactoryFeatureExtractor.nonmax(api.ConfigExtract(2, 5.0, 1, True, dmin, dmax), ctx=NoGpu())
        assert e.canDetectMaximums() == dmax and e.canDetectMinimums() == (dmin or not dmax)
        assert (e.getThresholdMinimum(), e.getThresholdMaximum()) == (-5.0, 5.0)
        e.setThresholdMinimum(-1.0)
        assert e.getThresholdMinimum() == -1.0 and e.getThresholdMaximum() == 5.0
    with pytest.raises(RuntimeError):
        api.FactoryFeatureExtractor.nonmax(api.ConfigExtract(2, 5.0, 1, False, True, True), ctx=NoGpu())   # the relaxed rule is still refused
