"""CPU: tests/assoc_ref.py, the NumPy model of the greedy association, against what the reference's own test pins (TestAssociateGreedy), against
hand-made matrices with one rule each, and against the compiled oracle on the tie-dense problems of tests/test_gpu_assoc_hamming.py; and the
non-vacuity of those problems: the shares of tied rows, tied columns, surviving and removed matches are asserted here.  No GPU."""
import numpy as np
import pytest

import assoc_ref as ar

MAX = ar.MAX_VALUE


def _abs(src, dst):
    """ScoreAssociateEuclidean_F64 on one-element descriptors"""
    return np.abs(np.asarray(src, float)[:, None] - np.asarray(dst, float)[None, :])


# ---- TestAssociateGreedy ----
def test_reference_basic():
    p, f = ar.greedy(_abs([1, 2, 3, 4], [3, 4, 1, 40]), 0.5, False)
    assert p.tolist() == [2, -1, 0, 1] and p.dtype == np.int32 and f.dtype == np.float64
    assert f[0] == 0 and f[2] == 0 and f[3] == 0 and f[1] == 0.5          # an unmatched row keeps maxFitError


def test_reference_max_error():
    W = _abs([1, 2, 3, 4], [3, 4, 1.1, 40])
    assert ar.greedy(W, 10, False)[0][1] == 2
    assert ar.greedy(W, 0.1, False)[0][1] == -1


def test_reference_backwards():
    p, f = ar.greedy(_abs([1, 2, 3, 8], [3, 4, 1, 10]), 10, True)
    assert p.tolist() == [2, -1, 0, 3]
    assert f[0] == 0 and f[2] == 0 and f[3] == 2 and f[1] == MAX          # a match the backward check removes gets Double.MAX_VALUE
    # without the check row 1 (equally far from 1 and 3) takes the later of the two
    assert ar.greedy(_abs([1, 2, 3, 8], [3, 4, 1, 10]), 10, False)[0].tolist() == [2, 2, 0, 3]


# ---- one rule per matrix ----
def test_row_tie_takes_the_last_index():
    W = np.array([[4, 9, 4], [7, 7, 7], [1, 5, 2]])
    p, f = ar.greedy(W, MAX, False)
    assert p.tolist() == [2, 2, 0] and f.tolist() == [4.0, 7.0, 1.0]


def test_column_tie_kills_the_match():
    W = np.array([[3, 9, 9], [3, 9, 9], [9, 9, 1]])
    p, f = ar.greedy(W, MAX, True)
    assert p.tolist() == [-1, -1, 2] and f.tolist() == [MAX, MAX, 1.0]     # rows 0 and 1 tie in column 0: neither keeps it
    # a lower entry elsewhere in the column kills as well, an equal one in another column does not
    W = np.array([[3, 9, 9], [2, 1, 9], [9, 9, 3]])
    p, f = ar.greedy(W, MAX, True)
    assert p.tolist() == [-1, 1, 2] and f.tolist() == [MAX, 1.0, 3.0]


def test_threshold_is_inclusive():
    W = np.array([[5, 8, 9], [8, 6, 9], [9, 9, 7]])
    p, f = ar.greedy(W, 6.0, True)
    assert p.tolist() == [0, 1, -1] and f.tolist() == [5.0, 6.0, 6.0]      # score == maxFitError is a match
    p, f = ar.greedy(W, 5.5, True)
    assert p.tolist() == [0, -1, -1] and f.tolist() == [5.0, 5.5, 5.5]     # maxFitError = score - 0.5 is not


def test_negative_threshold_matches_nothing():
    W = np.array([[0, 1, 2], [1, 0, 2], [2, 1, 0]])
    for backwards in (False, True):
        p, f = ar.greedy(W, -1.0, backwards)
        assert p.tolist() == [-1, -1, -1] and f.tolist() == [-1.0, -1.0, -1.0]
    assert ar.greedy(W, 0.0, True)[0].tolist() == [0, 1, 2]


def test_empty_sets():
    p, f = ar.greedy(np.zeros((3, 0)), 2.5, True)
    assert p.tolist() == [-1, -1, -1] and f.tolist() == [2.5, 2.5, 2.5]
    p, f = ar.greedy(np.zeros((0, 3)), 2.5, True)
    assert len(p) == 0 and len(f) == 0
    assert ar.hamming_scores(np.zeros((0, 16), np.int32), np.zeros((4, 16), np.int32)).shape == (0, 4)


def test_hamming_scores_by_hand():
    src = np.array([[0, -1], [1, 0], [-2**31, 5]], np.int32)
    dst = np.array([[0, 0], [-1, -1]], np.int32)
    W = ar.hamming_scores(src, dst)
    assert W.dtype == np.int32 and W.tolist() == [[32, 32], [1, 63], [3, 61]]     # the sign bit is one bit like any other


# ---- against the oracle, on every problem the GPU tests run ----
@pytest.mark.parametrize("ns,nd,words", [(ns, nd, 16) for ns, nd in ar.SHAPES_16 + ar.SHAPES_SHARDED] + ar.SHAPES_OTHER)
def test_model_equals_oracle(orc, ns, nd, words):
    src, dst, W = ar.case(ns, nd, words)
    for maxErr in ar.thresholds(W):
        for backwards in (False, True):
            p, f = ar.greedy(W, maxErr, backwards)
            ep, ef = orc.associate_hamming(src, dst, maxErr, backwards)
            assert np.array_equal(p, ep) and np.array_equal(f, ef), (maxErr, backwards)


# ---- column records ----
def _top2_loop(W, src_begin):
    out = []
    for j in range(W.shape[1]):
        min1 = min2 = np.inf
        idx = -1
        for i in range(W.shape[0]):
            v = float(W[i, j])
            if v < min1:
                min1, min2, idx = v, min1, src_begin + i
            elif v < min2:
                min2 = v
        out.append((min1, min2, idx))
    return out


@pytest.mark.parametrize("begin,count", [(0, 65), (0, 1), (7, 2), (20, 45), (64, 1), (30, 0)])
def test_column_top2_against_a_loop(begin, count):
    _, _, W = ar.case(65, 129, 17)
    part = W[begin:begin + count]
    min1, min2, idx1 = ar.column_top2(part, src_begin=begin)
    assert min1.dtype == np.float64 and min2.dtype == np.float64 and idx1.dtype == np.int32
    assert list(zip(min1.tolist(), min2.tolist(), idx1.tolist())) == _top2_loop(part, begin)
    if count == 0:
        assert np.isinf(min1).all() and np.isinf(min2).all() and (idx1 == -1).all()
    if count == 1:
        assert np.isinf(min2).all() and (idx1 == begin).all()
    if count == 65:
        assert (min1 == min2).mean() > 0.2                    # the case has column ties to get right


# ---- the GPU tests' inputs are what they claim to be ----
@pytest.mark.parametrize("ns,nd", ar.LARGE_16)
def test_large_cases_are_tie_dense(ns, nd):
    _, _, W = ar.case(ns, nd)
    st = ar.tie_stats(W)
    print(ns, nd, st)
    assert st["tied_rows"] >= 0.40
    assert st["tied_cols"] >= 0.40
    assert st["median_span"] >= nd / 4
    assert st["survivors"] >= 0.25 * min(ns, nd)
    assert st["killed"] >= 0.25 * ns


def test_tie_stats_by_hand():
    W = np.array([[1, 5, 1, 5],      # tied row, span 2; takes column 2; row 2 is lower there: removed
                  [5, 2, 5, 3],      # unique minimum in column 1, unique in that column: survives
                  [4, 4, 0, 3]])     # takes column 2, the strict column minimum: survives
    st = ar.tie_stats(W)
    assert st == dict(tied_rows=1 / 3, tied_cols=1 / 4, median_span=2.0, survivors=2, killed=1)


def test_thresholds_and_generator_are_fixed():
    src, dst, W = ar.case(129, 97)
    s2, d2 = ar.tie_dense(np.random.default_rng(1000003 * 129 + 1009 * 97 + 16), 129, 97, 16)
    assert np.array_equal(src, s2) and np.array_equal(dst, d2) and src.dtype == np.int32 and src.shape == (129, 16)
    t = ar.thresholds(W)
    m = t[1]
    assert t == [MAX, m, m - 0.5, 0.0, -1.0, m + 1.0] and (W.min(axis=1) == m).any()
    with pytest.raises(ValueError):
        W[0, 0] = 0                                           # shared between tests: read-only
