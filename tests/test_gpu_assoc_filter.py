"""The fp16 filter of the greedy L2 association (boofcv_amd/csrc/assoc_mfma.hip) at its error bound and at the edges of its tiling.

Every result is compared with the oracle's greedy association, pairs and fit quality bit for bit.  The inputs come from
tests/assoc_filter_model.py: pairs whose order the filter sees reversed by about 0.44 of its band (tests/test_assoc_filter_model.py proves
that for each of them without a GPU), placed on the edges of the wave tiles, column tiles, steps, strips and row chunks.  Each test runs on
its own context and reads from the profile report which path gave the result: the matrix-core filter, or the exact scan kernels that a
degenerate input falls back to.  Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import functools

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


def _path(ctx):
    """'mfma': the filter's result was used; 'fallback': the exact scan kernels ran (after the filter gave up, or instead of it)"""
    rep = ctx.profileReport()
    if "k_assoc_scan_rows" in rep or "k_assoc_scan_cols" in rep:
        return "fallback"
    assert "k_assoc_mfma_pass2" in rep, sorted(rep)
    return "mfma"


def _gpu(api, ctx, src, dst, maxErr, backwards):
    ctx.profileReset()
    a = api.FactoryAssociation.greedy(api.ScoreAssociateEuclideanSq_F64(), maxErr, backwards, ctx=ctx)
    a.setSource(src); a.setDestination(dst); a.associate()
    return np.array(a.getPairs()), np.array(a.getFitQuality()), _path(ctx)


def _check(api, orc, ctx, src, dst, maxErr, backwards, path="mfma"):
    p, f, took = _gpu(api, ctx, src, dst, maxErr, backwards)
    ep, ef = orc.associate_l2(src, dst, maxErr, backwards)
    assert np.array_equal(p, ep), "rows with wrong pairs: %s" % np.nonzero(p != ep)[0].tolist()
    assert np.array_equal(f, ef)
    assert path is None or took == path
    return p, f, took


@functools.lru_cache(maxsize=None)
def _row_problem(nd):
    return fm.row_problem(nd)


def _between(src, dst, plants):
    """a maxFitError between the exact distances of every planted (i, j*) and every planted (i, j')"""
    lo = max(fm.exact_l2(src[i], dst[js]) for i, _, js, _ in plants)
    hi = min(fm.exact_l2(src[i], dst[jp]) for i, _, _, jp in plants)
    assert lo < hi
    return np.sqrt(lo * hi)


# ------------------------------------------------------------------------------------------------------------------ (a) rows
@pytest.mark.parametrize("backwards", [False, True])
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("nd", sorted(fm.COLUMNS))
def test_planted_row_inversions(api, orc, ctx, nd, cut, backwards):
    """Source rows 0, 31, 32, 63, 64, 255, 256, ns - 1 each prefer j* exactly and j' in fp16; (j*, j') share a tile, a step, straddle a
    step, the strip boundary, and lie in a last strip of 33 columns (two tiles), of 1 column and of 65 columns (an odd tile count)."""
    (src, dst), plants = _row_problem(nd)
    maxErr = _between(src, dst, plants) if cut else api.Double_MAX_VALUE
    p, f, _ = _check(api, orc, ctx, src, dst, maxErr, backwards)
    for i, i2, js, jp in plants:
        assert p[i] == js and f[i] == fm.exact_l2(src[i], dst[js])
        assert p[i2] == (-1 if cut else jp)


# ------------------------------------------------------------------------------------------------------------------ (b) columns
def test_planted_column_inversions(api, orc, ctx):
    """Column j* prefers source i exactly and i2 in fp16; (i, i2) in different wave tiles of a block, and in different 256-row chunks of
    the single problem, whose column minima meet in the global atomics."""
    (src, dst), plants = fm.col_problem()
    p, f, _ = _check(api, orc, ctx, src, dst, api.Double_MAX_VALUE, True)
    for i, i2, js, jp in plants:
        assert p[i] == js and p[i2] == jp


# ------------------------------------------------------------------------------------------------------------------ (c) scales
def test_scale_sweep(api, orc, ctx):
    """The problem of (a) times 2^k: same pairs, fit times 4^k bit for bit, the filter used for every k (q follows k)."""
    (src, dst), plants = _row_problem(417)
    p0, f0, _ = _check(api, orc, ctx, src, dst, api.Double_MAX_VALUE, True)
    assert (p0 >= 0).sum() >= 2 * len(plants)
    for k in fm.SCALES + (fm.SCALE_FALLBACK,):
        p, f, _ = _check(api, orc, ctx, np.ldexp(src, k), np.ldexp(dst, k), api.Double_MAX_VALUE, True,
                         "fallback" if k == fm.SCALE_FALLBACK else "mfma")
        assert np.array_equal(p, p0), k
        with np.errstate(over="ignore"):
            assert np.array_equal(f, np.where(p0 >= 0, np.ldexp(f0, 2 * k), f0)), k     # unmatched rows keep Double.MAX_VALUE


@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("backwards", [False, True])
def test_q_boundary(api, orc, ctx, below, backwards):
    """q is taken from a norm of exactly 1 = 4^0, and from one fp32 ulp below it (the scaled quads differ by a factor of 4)."""
    (src, dst), plants = fm.q_boundary_problem(below)
    p, _, _ = _check(api, orc, ctx, src, dst, api.Double_MAX_VALUE, backwards)
    for i, _, js, _ in plants:
        assert p[i] == js


# ------------------------------------------------------------------------------------------------------------------ (d) subnormals
@pytest.mark.parametrize("shift", [12, 20])
def test_subnormal_rows(api, orc, ctx, shift):
    """Rows at 2^-12 and 2^-20 of the largest norm are fp16 subnormals (or one unit of them) after scaling: every pair of them is inside
    the band.  Whichever path answers, the result is the oracle's."""
    (src, dst), _ = fm.subnormal_problem(shift)
    for backwards in (False, True):
        _, _, took = _check(api, orc, ctx, src, dst, api.Double_MAX_VALUE, backwards, path=None)
        print("subnormal rows, 2^-%d, backwards=%s: %s" % (shift, backwards, took))


# ------------------------------------------------------------------------------------------------------------------ (e) staging
def _distinct_rows(n, seed):
    return fm.filler(np.random.default_rng(seed), n)


def test_candidate_staging_overflow(api, orc, ctx):
    """64 source rows, each 6 times in a destination of 384 columns: one block, one wave tile, 384 listed pairs for 256 staging slots --
    128 of them take the direct path to the global list; the list cap (8 * 448 + 4096) is far away."""
    src = _distinct_rows(64, 5)
    dst = np.tile(src, (6, 1))
    p, f, _ = _check(api, orc, ctx, src, dst, api.Double_MAX_VALUE, False)
    assert np.array_equal(p, np.arange(64) + 320) and not f.any()        # forward: the largest index among the exact ties
    # backward: the six columns of a row tie, its match (the last copy) is the only row at that column's minimum and survives
    p, f, _ = _check(api, orc, ctx, src, dst, api.Double_MAX_VALUE, True)
    assert np.array_equal(p, np.arange(64) + 320) and not f.any()
    # the same with the copies as sources: six rows tie in every column, no match survives the backward check
    p, _, _ = _check(api, orc, ctx, dst, src, api.Double_MAX_VALUE, True)
    assert (p == -1).all()


def test_candidate_staging_flush_between_row_tiles(api, orc, ctx, monkeypatch):
    """ns = 320, three copies of every row.  With one row chunk per strip (BHIP_ASSOC_ROWSPLIT, read at every call) wave 0 sweeps rows
    0..63 and then 256..319.  The first strip holds the copies of exactly those rows: 192 pairs after the first tile (more than half of
    the staging area: flushed, counter reset), 192 more after the second."""
    monkeypatch.setenv("BHIP_ASSOC_ROWSPLIT", "1")
    src = _distinct_rows(320, 6)
    order = np.concatenate([np.arange(0, 64), np.arange(256, 320), np.arange(64, 256)])
    owner = np.repeat(order, 3)                       # column -> source row
    dst = src[owner]
    assert len(dst) == 960 and set(owner[:384]) == set(range(0, 64)) | set(range(256, 320))
    last = np.array([np.nonzero(owner == i)[0].max() for i in range(320)])
    for backwards in (False, True):
        p, f, _ = _check(api, orc, ctx, src, dst, api.Double_MAX_VALUE, backwards)
        assert np.array_equal(p, last) and not f.any()


# ------------------------------------------------------------------------------------------------------------------ (f) batched
def test_batched_table_19_problems(api, orc):
    """bhip_assoc_l2_dev_batched with 19 problems in one device buffer: from 16 problems on the block table is dealt to the XCDs by
    problem index and padded with empty entries.  Gap rows and destination rows keep the sentinels of the output arrays."""
    import torch
    from boofcv_amd import _lib
    L = _lib.load()
    rows, src_off, dst_off = fm.batched_problem()
    ns, nd = np.array(fm.BATCH_NS, np.int32), np.array(fm.BATCH_ND, np.int32)
    n = len(ns)
    assert n >= 16 and {1, 385, 800} <= set(nd.tolist())
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
    took = _path(ctx)
    ctx.close()
    pairs, fit = pairs.cpu().numpy(), fit.cpu().numpy()
    written = np.zeros(len(rows), bool)
    for k in range(n):
        s, d = slice(src_off[k], src_off[k] + ns[k]), slice(dst_off[k], dst_off[k] + nd[k])
        p, f = orc.associate_l2(rows[s], rows[d], api.Double_MAX_VALUE, True)
        assert np.array_equal(pairs[s], p) and np.array_equal(fit[s], f), k
        written[s] = True
    i, i2, js, jp = fm.BATCH_PLANTS[0]
    assert pairs[src_off[0] + i] == js and pairs[src_off[0] + i2] == jp
    assert (~written).sum() == nd.sum() + 2 * n * fm.BATCH_GAP
    assert (pairs[~written] == -7).all() and (fit[~written] == -3.0).all()
    assert took == "mfma"
