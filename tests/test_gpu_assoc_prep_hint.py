"""The one-pass prep of the fp16 association filter (boofcv_amd/csrc/assoc_mfma.hip): descriptors are converted with the scale exponent the
previous call on the context measured (the hint q_h, 1 on a fresh context), and the call is repeated with the measured exponent when
the norms do not fit it.  Pass 2 forms its thresholds itself, and the result kernel is launched before the host has read the flags.

Every result is compared with the oracle's greedy association, pairs and fit quality bit for bit: the same standard as
tests/test_gpu_assoc_filter.py.  A result must not depend on the hint, so the history tests also compare with the same call on a fresh
context.  Which way a call went is read from the profile report: k_assoc_prep is bracketed once per run of the filter, so one launch
means the hint held and two mean the call was repeated; the exact scan kernels mean the fallback.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import assoc_filter_model as fm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()
    return a


@pytest.fixture
def ctx(api):
    c = api.Context(0)
    c.profile(True)
    yield c
    c.close()


def _run(api, ctx, src, dst, maxErr, backwards):
    """-> pairs, fit, runs of the filter (0: the exact fallback answered without it), whether the exact scan kernels ran"""
    ctx.profileReset()
    a = api.FactoryAssociation.greedy(api.ScoreAssociateEuclideanSq_F64(), maxErr, backwards, ctx=ctx)
    a.setSource(src); a.setDestination(dst); a.associate()
    p, f = np.array(a.getPairs()), np.array(a.getFitQuality())
    rep = ctx.profileReport()
    return p, f, rep.get("k_assoc_prep", {}).get("launches", 0), ("k_assoc_scan_rows" in rep or "k_assoc_scan_cols" in rep)


def _check(api, orc, ctx, src, dst, backwards=True, runs=None, fallback=False, maxErr=None):
    maxErr = api.Double_MAX_VALUE if maxErr is None else maxErr
    p, f, took, fell = _run(api, ctx, src, dst, maxErr, backwards)
    ep, ef = orc.associate_l2(src, dst, maxErr, backwards)
    assert np.array_equal(p, ep), "rows with wrong pairs: %s" % np.nonzero(p != ep)[0].tolist()
    assert np.array_equal(f, ef)
    assert fallback is None or fell == fallback      # None: either path may answer
    assert runs is None or took == runs, (took, runs)
    return p, f


def _fresh(api, orc, src, dst, backwards=True):
    """the same call on a context that has no history"""
    c = api.Context(0)
    c.profile(True)
    try:
        return _check(api, orc, c, src, dst, backwards)
    finally:
        c.close()


def _unit_rows(ns, nd, seed):
    """unit vectors; the first half of the destination rows are noisy copies of source rows, so that most rows have a match that survives
    the backward check, the rest are unrelated"""
    rng = np.random.default_rng(seed)
    src, dst = fm.filler(rng, ns), fm.filler(rng, nd)
    k = min(ns, nd) // 2
    dst[:k] = src[:k] + rng.normal(scale=0.02, size=(k, fm.DOF))
    dst[:k] /= np.linalg.norm(dst[:k], axis=1, keepdims=True)
    return src, dst


# ------------------------------------------------------------------------------------------------------------------ 1. history
def test_hint_history(api, orc, ctx):
    """unit rows, the same rows times 2^12 and 2^-12, unit rows again, on one context: the first call meets the initial hint, each of the
    others a hint that is off by 12 and is repeated once; all four give the oracle's result and that of a fresh context"""
    src, dst = _unit_rows(70, 100, 1)
    p0 = None
    for k, runs in ((0, 1), (12, 2), (-12, 2), (0, 2)):
        s, d = np.ldexp(src, k), np.ldexp(dst, k)
        p, f = _check(api, orc, ctx, s, d, runs=runs)
        pf, ff = _fresh(api, orc, s, d)
        assert np.array_equal(p, pf) and np.array_equal(f, ff), k
        p0 = p if p0 is None else p0
        assert np.array_equal(p, p0), k          # a power of two changes no decision
    assert (p0 >= 0).sum() >= 30
    # and once the hint has settled, the call is not repeated
    _check(api, orc, ctx, src, dst, runs=1)


# ------------------------------------------------------------------------------------------------------------------ 2. window edges
FOUR, QUARTER = np.float32(4.0), np.float32(0.25)
EDGES = {
    "4.0": (FOUR, 2),                                         # 4^q_h itself: outside, repeated
    "below_4.0": (np.nextafter(FOUR, np.float32(0)), 1),      # the largest norm the hint 1 still covers
    "0.25": (QUARTER, 1),                                     # 4^(q_h - 2): the smallest maximum it covers
    "below_0.25": (np.nextafter(QUARTER, np.float32(0)), 2),
}


@pytest.mark.parametrize("backwards", [False, True])
@pytest.mark.parametrize("edge", list(EDGES))
def test_window_edges(api, orc, ctx, edge, backwards):
    """After a unit-norm call the hint is 1 and holds for a largest raw norm (fp32, rounded up, what the kernel compares) in [1/4, 4).  One
    source row carries exactly the edge value; every other row stays below it."""
    target, runs = EDGES[edge]
    src, dst = _unit_rows(70, 100, 2)
    _check(api, orc, ctx, src, dst, backwards, runs=1)
    if target < 1:
        src, dst = 0.45 * src, 0.45 * dst            # squared norms of 0.2025, under both small edges
    lead = fm.with_norm_leader(src, target)
    assert fm.raw_norms(lead).max() == target and fm.raw_norms(dst).max() < target
    _check(api, orc, ctx, lead, dst, backwards, runs=runs)


# ------------------------------------------------------------------------------------------------------------------ 3. two arrays
@pytest.mark.parametrize("large", ["src", "dst"])
def test_source_and_destination_scales_differ(api, orc, ctx, large):
    """source and destination are different arrays 2^6 apart in scale: one exponent serves both, taken from the larger of the two.  The
    first call finds the hint 1 too small for squared norms of 2^12 and is repeated; the second call holds."""
    src, dst = _unit_rows(70, 100, 3)
    if large == "src":
        src = np.ldexp(src, 6)
    else:
        dst = np.ldexp(dst, 6)
    p, f = _check(api, orc, ctx, src, dst, runs=2)
    _check(api, orc, ctx, src, dst, runs=1)
    pf, ff = _fresh(api, orc, src, dst)
    assert np.array_equal(p, pf) and np.array_equal(f, ff)


# ------------------------------------------------------------------------------------------------------------------ 4. non-finite
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_row_does_not_poison_the_hint(api, orc, ctx, bad):
    """a NaN / Inf component sends the call to the exact kernels (nothing of the filter's run is kept: the result kernel was launched before
    the host saw the flag and must have written nothing); the next, clean call on the context goes through the filter in one run"""
    src, dst = _unit_rows(70, 100, 4)
    _check(api, orc, ctx, src, dst, runs=1)
    dirty = src.copy()
    dirty[17, 5] = bad
    _check(api, orc, ctx, dirty, dst, fallback=True)
    _check(api, orc, ctx, src, dst, runs=1)


# ------------------------------------------------------------------------------------------------------------------ 5. zeros
@pytest.mark.parametrize("backwards", [False, True])
def test_all_zero_descriptors(api, orc, ctx, backwards):
    """no positive norm: any exponent holds; every score is 0 and every column ties.  Whichever path answers (the candidate list of an
    all-tie problem can overflow), the result is the oracle's, and the next call is not disturbed"""
    z = np.zeros((70, fm.DOF)), np.zeros((100, fm.DOF))
    _check(api, orc, ctx, z[0], z[1], backwards, fallback=None)
    src, dst = _unit_rows(70, 100, 5)
    _check(api, orc, ctx, src, dst, backwards, runs=1)
    # zero rows against real ones: the maximum is the destination's and the hint holds (every column is nearly as good for every row, so
    # the exact kernels may have to finish the call)
    _check(api, orc, ctx, z[0], dst, backwards, runs=1, fallback=None)


# ------------------------------------------------------------------------------------------------------------------ 6. thresholds
EDGE_NS, EDGE_ND = (1, 63, 65, 257), (1, 33, 383, 385)


@pytest.fixture(scope="module")
def edge_table(orc):
    """all 16 (ns, nd) problems in one buffer, segment order src 0, dst 0, src 1, ... with gap rows, and the oracle's answer to each"""
    rng = np.random.default_rng(6)
    parts, src_off, dst_off, ns_l, nd_l, at = [], [], [], [], [], 0
    for ns in EDGE_NS:
        for nd in EDGE_ND:
            s, d = _unit_rows(ns, nd, 600 + 16 * ns + nd)
            for seg, offs in ((s, src_off), (d, dst_off)):
                offs.append(at)
                parts += [seg, fm.filler(rng, 2)]
                at += len(seg) + 2
            ns_l.append(ns); nd_l.append(nd)
    rows = np.concatenate(parts)
    want = [orc.associate_l2(rows[so:so + a], rows[do:do + b], orc.MAX_VALUE_F64, True) for so, do, a, b in zip(src_off, dst_off, ns_l, nd_l)]
    return rows, np.array(src_off, np.int64), np.array(dst_off, np.int64), np.array(ns_l, np.int32), np.array(nd_l, np.int32), want


@pytest.mark.parametrize("rowsplit", [None, "1", "3"])
def test_thresholds_in_pass2_at_every_edge(api, orc, edge_table, monkeypatch, rowsplit):
    """ns in {1, 63, 65, 257} x nd in {1, 33, 383, 385} as one batched table (16 problems: dealt to the XCD queues with padding entries),
    with the default row chunks, whole-problem sweeps and three chunks: pass 2 computes the threshold of every row tile (a wave's last tile
    of 1 or 63 rows, a second turn of one row) and of every strip column (strips of 1, 33, 383 and 384 + 1 columns) in place, with
    -inf for the rows and columns that do not exist"""
    import torch
    from boofcv_amd import _lib
    if rowsplit is None:
        monkeypatch.delenv("BHIP_ASSOC_ROWSPLIT", raising=False)
    else:
        monkeypatch.setenv("BHIP_ASSOC_ROWSPLIT", rowsplit)
    L = _lib.load()
    rows, src_off, dst_off, ns, nd, want = edge_table
    n = len(ns)
    dev = torch.from_numpy(rows).cuda()
    pairs = torch.full((len(rows),), -7, dtype=torch.int32, device="cuda"); fit = torch.full((len(rows),), -3.0, dtype=torch.float64, device="cuda")
    ctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.profile(True); ctx.profileReset()
    LL, I = C.POINTER(C.c_longlong), C.POINTER(C.c_int)
    st = L.bhip_assoc_l2_dev_batched(ctx._h, C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr()), 64, n, src_off.ctypes.data_as(LL), ns.ctypes.data_as(I),
                                     dst_off.ctypes.data_as(LL), nd.ctypes.data_as(I), api.Double_MAX_VALUE, 1, C.c_void_p(pairs.data_ptr()),
                                     C.c_void_p(fit.data_ptr()))
    assert st == 0, L.bhip_last_error(ctx._h)
    torch.cuda.synchronize()
    rep = ctx.profileReport()
    ctx.close()
    assert "k_assoc_scan_rows" not in rep and "k_assoc_scan_cols" not in rep and rep["k_assoc_prep"]["launches"] == 1, sorted(rep)
    pairs, fit = pairs.cpu().numpy(), fit.cpu().numpy()
    written = np.zeros(len(rows), bool)
    for k in range(n):
        s = slice(src_off[k], src_off[k] + ns[k])
        assert np.array_equal(pairs[s], want[k][0]) and np.array_equal(fit[s], want[k][1]), (int(ns[k]), int(nd[k]))
        written[s] = True
    assert (pairs[~written] == -7).all() and (fit[~written] == -3.0).all()
