"""The CPU model of the fp16 association filter (tests/assoc_filter_model.py) against hand-computed literals, and the conditions under
which the problems of tests/test_gpu_assoc_filter.py test the filter's band: for every planted pair, in the row and in the column
direction, the exact order and the filter's order are opposite by at least 0.35 of the band, while the documented error bound holds."""
import numpy as np
import pytest

import assoc_filter_model as fm

F32_BELOW_1 = np.nextafter(np.float32(1.0), np.float32(0))


def test_scale_exp_literals():
    # frexp(1.0) = (0.5, 1): q = 1 and the scaled maximum is 1/4;  just below 1.0 the exponent is 0: q = 0
    assert fm.scale_exp(1.0) == 1
    assert fm.scale_exp(F32_BELOW_1) == 0
    # 2^-3 = 0.5 * 2^-2 -> (-2 + 1) >> 1 = -1 (scaled 2^-3 * 2^2 = 1/2);  2^-4 = 0.5 * 2^-3 -> -2 >> 1 = -1 (scaled 1/4);
    # 2^-5 = 0.5 * 2^-4 -> -3 >> 1 = -2 (scaled 2^-5 * 2^4 = 1/2)
    assert fm.scale_exp(2.0 ** -3) == -1
    assert fm.scale_exp(2.0 ** -4) == -1
    assert fm.scale_exp(2.0 ** -5) == -2
    assert fm.scale_exp(4.0) == 2 and fm.scale_exp(2.0) == 1 and fm.scale_exp(0.25) == 0 and fm.scale_exp(0.5) == 0
    assert fm.scale_exp(0.0) == 0 and fm.scale_exp(np.float32("nan")) == 0
    for n, scaled in [(1.0, 0.25), (2.0 ** -3, 0.5), (2.0 ** -4, 0.25), (2.0 ** -5, 0.5), (float(F32_BELOW_1), float(F32_BELOW_1))]:
        assert np.ldexp(np.float32(n), -2 * fm.scale_exp(n)) == np.float32(scaled)


def test_norms_split_and_band_literals():
    # one row (0.5, 0, ...): sum 0.25, rounded up 0.25 (1 + 2^-22); alone it is the maximum: q = 0
    row = np.zeros((1, 64)); row[0, 0] = 0.5
    assert fm.raw_norms(row)[0] == np.float32(0.25 * (1 + 2.0 ** -22))
    m = fm.FilterModel(row, row)
    assert m.q == 0 and m.S.h[0, 0] == 0.5
    # hi = fl16(0.25 (1 + 2^-22)) = 0.25, lo = 2^-24 exactly (an fp16 subnormal)
    assert m.S.hl[0] == 0.25 + 2.0 ** -24
    assert m.d_tilde(0, 0) == 1.0 + 2 * (0.25 + 2.0 ** -24) - 2 * 0.25
    n = np.float32(0.25 * (1 + 2.0 ** -22))
    assert m.band_row(0) == float(np.float32(2) * (np.float32(1.03e-3) * (n + n) + np.float32(2e-5)))
    assert abs(m.band_row(0) - 2 * (1.03e-3 * 0.5 + 2e-5)) < 1e-9
    # fl16(fl32(x)): 2^-3 (1 + 2^-10) + 0.49 ulp rounds down, + 0.51 ulp rounds up
    x = 2.0 ** -3 * (1 + 2.0 ** -10)
    row2 = np.zeros((2, 64)); row2[0, 0] = x + 0.49 * fm.U; row2[1, 0] = x + 0.51 * fm.U
    m = fm.FilterModel(np.concatenate([row2, 0.9 * np.eye(64)[:1]]), row2)     # the 0.81 row keeps q = 0
    assert m.q == 0 and m.S.h[0, 0] == x and m.S.h[1, 0] == x + fm.U
    assert fm.degenerate(np.full((1, 64), 2.0 ** 47)) and not fm.degenerate(np.full((1, 64), 2.0 ** 46))
    assert fm.degenerate(np.full((1, 64), np.nan))


@pytest.mark.parametrize("k", fm.SCALES)
def test_scaled_maximum_in_range(k):
    (src, dst), _ = fm.row_problem(417)
    m = fm.FilterModel(np.ldexp(src, k), np.ldexp(dst, k))
    assert 0.25 <= float(m.maxN) < 1.0
    assert m.q == fm.FilterModel(src, dst).q + k
    assert not fm.degenerate(np.ldexp(src, k), np.ldexp(dst, k))


def test_scale_past_the_norm_limit_is_degenerate():
    (src, dst), _ = fm.row_problem(417)
    assert fm.degenerate(np.ldexp(src, fm.SCALE_FALLBACK), np.ldexp(dst, fm.SCALE_FALLBACK))


def _check_all(src, dst, plants, label):
    m = fm.FilterModel(src, dst)
    dt = m.d_tilde_all()
    ratios = []
    for i, i2, js, jp in plants:
        ratios += fm.check_planted(m, i, i2, js, jp)
        # the competitors are the filter's minima of row i and of column j*: nothing unplanted comes near
        assert np.argmin(dt[i]) == jp and np.argmin(dt[:, js]) == i2
    print("%s: q = %d, inversion / band %.3f .. %.3f" % (label, m.q, min(ratios), max(ratios)))   # shown with pytest -s
    return m


@pytest.mark.parametrize("nd", sorted(fm.COLUMNS))
def test_row_problems_reach_the_band(nd):
    (src, dst), plants = fm.row_problem(nd)
    assert [p[0] for p in plants] == [0, 31, 32, 63, 64, 255, 256, len(src) - 1]
    _check_all(src, dst, plants, "rows, nd = %d" % nd)


def test_column_problem_reaches_the_band():
    (src, dst), plants = fm.col_problem()
    assert any(i // 64 != i2 // 64 and i // 256 == i2 // 256 for i, i2, _, _ in plants)   # other wave tile, same row chunk
    assert sum(i // 256 != i2 // 256 for i, i2, _, _ in plants) >= 3                       # different row chunks
    _check_all(src, dst, plants, "columns")


@pytest.mark.parametrize("k", fm.SCALES)
def test_scaled_problems_reach_the_band(k):
    (src, dst), plants = fm.row_problem(417)
    _check_all(np.ldexp(src, k), np.ldexp(dst, k), plants, "scale 2^%d" % k)


@pytest.mark.parametrize("below", [False, True])
def test_q_boundary_problems(below):
    (src, dst), plants = fm.q_boundary_problem(below)
    m = _check_all(src, dst, plants, "q boundary, %s" % ("one ulp below 1" if below else "exactly 1"))
    assert m.maxRaw == (F32_BELOW_1 if below else np.float32(1.0))
    assert m.q == (0 if below else 1)
    assert m.maxN == (F32_BELOW_1 if below else np.float32(0.25))


def test_batched_problem_reaches_the_band():
    rows, src_off, dst_off = fm.batched_problem()
    s, d = rows[src_off[0]:src_off[0] + fm.BATCH_NS[0]], rows[dst_off[0]:dst_off[0] + fm.BATCH_ND[0]]
    m = fm.FilterModel(s, d, buffer=rows)      # q and the bands' maximum come from the whole buffer, gap rows included
    ratios = fm.check_planted(m, *fm.BATCH_PLANTS[0])
    print("batched: q = %d, inversion / band %.3f .. %.3f" % (m.q, min(ratios), max(ratios)))
    # segments and gaps tile the buffer without overlap
    segs = sorted([(o, n) for o, n in zip(src_off, fm.BATCH_NS)] + [(o, n) for o, n in zip(dst_off, fm.BATCH_ND)])
    assert segs[0][0] == 0 and all(a + n + fm.BATCH_GAP == b for (a, n), (b, _) in zip(segs, segs[1:]))
    assert segs[-1][0] + segs[-1][1] + fm.BATCH_GAP == len(rows)


@pytest.mark.parametrize("nd", sorted(fm.COLUMNS))
def test_model_filter_with_a_quarter_of_the_band_loses_the_planted_pairs(orc, nd):
    """The model's candidate list with the full band gives the oracle's forward pairs; with a quarter of the band (2.0 -> 0.5 in
    k_assoc_thresholds) every planted source row is matched with its competitor: the GPU tests would notice such a filter."""
    (src, dst), plants = fm.row_problem(nd)
    m = fm.FilterModel(src, dst)
    ep, _ = orc.associate_l2(src, dst, orc.MAX_VALUE_F64, False)
    assert np.array_equal(fm.emulate_forward(m), ep)
    quarter = fm.emulate_forward(m, 0.25)
    for i, _, js, jp in plants:
        assert ep[i] == js and quarter[i] == jp
    assert (quarter != ep).sum() == len(plants)
