"""Greedy Hamming association under dense ties, on every kernel path that feeds the shared merge kernels:
  the int8 matrix-core scan (boofcv_amd/csrc/assoc_ham_mfma.hip: k_ham_expand, k_ham_mfma<16, rows / cols>), 16-word descriptors, the default;
  the VALU popcount scan (associate.hip: k_assoc_scan<HamScorer<16>>, <HamScorerDyn>), any other length or BHIP_HAM_VALU=1 (read at every call);
  both through k_merge_rows / k_merge_cols / k_assoc_finish, unsharded and as phase 1 / phase 2 of the sharded form.

Every result is compared bit for bit, pairs and fit quality, with tests/assoc_ref.py (NumPy) and with the oracle.  The inputs are
assoc_ref.tie_dense: most rows and columns attain their minimum several times, far apart in index (tests/test_assoc_reference.py asserts the
shares on the CPU), so the rules that random descriptors never exercise decide nearly every row: the LAST destination among equal minima,
the inclusive threshold, and `min2 == min1` removing a match.  Each test runs on its own context and reads the path from the profile report.

Geometry of the matrix-core scan (bhip_ham_mfma_splits / bhip_ham_mfma_scan): a wave owns 32 rows of U, a block 128; the swept set V is cut
into splits = clamp(ceil(2048 / ceil(nU / 32)), ceil(nV / 65536), ceil(nV / 32)) pieces of per = ceil(nV / splits) rounded up to 32 columns.
  1x1, 1x33, 33x1     nU = 1: every fragment row clamps to row 0; a one-column tile; the min2 sentinel on columns with a single source
  31x32, 32x33, 129x97  tails of the wave tile and of the column tile, dead waves in the last block, splits of one tile
  4096x1100           rows: 16 splits of 96 = three tiles each (the double buffer is live), split 11 a full tile and a 12-column tail,
                      splits 12..15 empty; columns: 59 splits of 96, a partly filled last wave (rows 1088..1099), a dead fourth wave,
                      empty splits from 43 on
  1100x4096           the transpose: 59 row splits, 16 column splits
Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import assoc_ref as ar

pytestmark = pytest.mark.gpu

COLTOP = np.dtype([("min1", "<f8"), ("min2", "<f8"), ("idx1", "<i4"), ("pad", "<i4")])


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


@pytest.fixture
def torch_ctx(api):
    """a context on torch's current stream, for the entry points that take device tensors"""
    import torch
    c = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    c.profile(True)
    yield c
    torch.cuda.synchronize()
    c.close()


def _path(ctx, cols):
    """'mfma': the matrix-core scan gave the row (and, when `cols`, the column) records and the popcount scan did not run; 'scan': the reverse"""
    rep = ctx.profileReport()
    ran = {k for k in ("k_ham_mfma_rows", "k_ham_mfma_cols", "k_assoc_scan_rows", "k_assoc_scan_cols") if k in rep}
    for name, fam in (("mfma", "k_ham_mfma"), ("scan", "k_assoc_scan")):
        if ran == {fam + "_rows"} | ({fam + "_cols"} if cols else set()):
            assert ("k_ham_expand" in rep) == (name == "mfma")
            return name
    raise AssertionError("unexpected kernels for cols=%s: %s" % (cols, sorted(rep)))


_expected = {}


def _expect(orc, ns, nd, words, maxErr, backwards):
    """(pairs, fit) of the NumPy model and of the oracle for one case: computed once, shared by the tests, read-only"""
    key = (ns, nd, words, maxErr, backwards)
    if key not in _expected:
        src, dst, W = ar.case(ns, nd, words)
        out = ar.greedy(W, maxErr, backwards) + orc.associate_hamming(src, dst, maxErr, backwards)
        for a in out:
            a.setflags(write=False)
        _expected[key] = out
    return _expected[key]


def _gpu(api, ctx, src, dst, maxErr, backwards):
    ctx.profileReset()
    a = api.FactoryAssociation.greedy(api.ScoreAssociateHamming_B(), maxErr, backwards, ctx=ctx)
    a.setSource(src); a.setDestination(dst); a.associate()
    return np.array(a.getPairs()), np.array(a.getFitQuality()), _path(ctx, backwards)


def _same(p, f, ep, ef, what):
    assert p.dtype == ep.dtype and f.dtype == ef.dtype
    assert np.array_equal(p, ep), "%s: rows with wrong pairs %s" % (what, np.nonzero(p != ep)[0][:20].tolist())
    assert np.array_equal(f, ef), "%s: rows with wrong fit %s" % (what, np.nonzero(f != ef)[0][:20].tolist())


def _check(api, orc, ctx, ns, nd, words, maxErr, backwards, path):
    src, dst, _ = ar.case(ns, nd, words)
    p, f, took = _gpu(api, ctx, src, dst, maxErr, backwards)
    mp, mf, op, of = _expect(orc, ns, nd, words, maxErr, backwards)
    what = "%dx%dx%d maxErr=%r backwards=%s" % (ns, nd, words, maxErr, backwards)
    assert took == path, what
    _same(p, f, mp, mf, what + " vs model")
    _same(p, f, op, of, what + " vs oracle")
    return p, f


# ------------------------------------------------------------------------------------------------------------------ 1. matrix cores
@pytest.mark.parametrize("backwards", [False, True])
@pytest.mark.parametrize("ns,nd", ar.SHAPES_16)
def test_matrix_core_path(api, orc, ctx, monkeypatch, ns, nd, backwards):
    monkeypatch.delenv("BHIP_HAM_VALU", raising=False)
    _, _, W = ar.case(ns, nd)
    for maxErr in ar.thresholds(W):
        _check(api, orc, ctx, ns, nd, 16, maxErr, backwards, "mfma")


# ------------------------------------------------------------------------------------------------------------------ 2. popcount scan, 16 words
@pytest.mark.parametrize("backwards", [False, True])
@pytest.mark.parametrize("ns,nd", ar.SHAPES_16)
def test_scan_path_16_words_equals_matrix_core_path(api, orc, ctx, monkeypatch, ns, nd, backwards):
    """k_assoc_scan<HamScorer<16>> under BHIP_HAM_VALU=1: the reference's results, and bit for bit what the matrix cores give"""
    _, _, W = ar.case(ns, nd)
    for maxErr in ar.thresholds(W):
        monkeypatch.delenv("BHIP_HAM_VALU", raising=False)
        mp, mf = _check(api, orc, ctx, ns, nd, 16, maxErr, backwards, "mfma")
        monkeypatch.setenv("BHIP_HAM_VALU", "1")
        sp, sf = _check(api, orc, ctx, ns, nd, 16, maxErr, backwards, "scan")
        _same(sp, sf, mp, mf, "scan vs matrix cores, maxErr=%r" % maxErr)


# ------------------------------------------------------------------------------------------------------------------ 3. popcount scan, other lengths
@pytest.mark.parametrize("backwards", [False, True])
@pytest.mark.parametrize("ns,nd,words", ar.SHAPES_OTHER)
def test_scan_path_other_lengths(api, orc, ctx, monkeypatch, ns, nd, words, backwards):
    """k_assoc_scan<HamScorerDyn>: 1, 5 and 17 words never take the matrix cores"""
    monkeypatch.delenv("BHIP_HAM_VALU", raising=False)
    _, _, W = ar.case(ns, nd, words)
    for maxErr in ar.thresholds(W):
        _check(api, orc, ctx, ns, nd, words, maxErr, backwards, "scan")


# ------------------------------------------------------------------------------------------------------------------ 4. sharded phases
@pytest.mark.parametrize("valu", [False, True])
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("ns,nd", ar.SHAPES_SHARDED)
def test_sharded_phases(api, orc, torch_ctx, monkeypatch, ns, nd, R, valu):
    """R ranks on one GPU.  The column records of phase 1 are read back and compared with the model rank by rank, then concatenated as the
    all-gather would and given to phase 2, whose pairs must be the slices of the unsharded result.  5 x 40 over 8 ranks leaves three ranks
    without rows."""
    import torch
    from boofcv_amd import _lib, sharded
    assert _lib.load().bhip_assoc_coltop_bytes() == 24 == COLTOP.itemsize
    if valu:
        monkeypatch.setenv("BHIP_HAM_VALU", "1")
    else:
        monkeypatch.delenv("BHIP_HAM_VALU", raising=False)
    src, dst, W = ar.case(ns, nd)
    eng = sharded.GpuEngine(ctx=torch_ctx)
    ts, td = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dst.copy()).cuda()      # the shared arrays are read-only
    part = sharded.row_partition(ns, R)
    assert sum(c for _, c in part) == ns and (min(c for _, c in part) == 0) == (R > ns)
    for maxErr in (api.Double_MAX_VALUE, ar.thresholds(W)[-1]):
        locals_ = []
        for b, c in part:
            torch_ctx.profileReset()
            locals_.append(eng.phase1("hamming", ts[b:b + c].contiguous(), b, td, maxErr))
            if c:
                assert _path(torch_ctx, True) == ("scan" if valu else "mfma")
        for (b, c), (p, f, col) in zip(part, locals_):
            rec = col.cpu().numpy().view(COLTOP)
            assert rec.shape == (nd,)
            min1, min2, idx1 = ar.column_top2(W[b:b + c], src_begin=b)
            assert np.array_equal(rec["min1"], min1) and np.array_equal(rec["min2"], min2), (R, b, c)
            if c == 0:
                assert np.isinf(rec["min1"]).all() and np.isinf(rec["min2"]).all() and (rec["idx1"] == -1).all()
                continue
            strict = min2 > min1
            assert np.array_equal(rec["idx1"][strict], idx1[strict]), (R, b, c)
            tied = rec["idx1"][~strict]
            assert ((tied >= b) & (tied < b + c)).all()
            assert np.array_equal(W[tied, np.nonzero(~strict)[0]], min1[~strict])      # some source of this rank that attains min1
            # before phase 2 a rank holds its forward matches
            fp, ff = ar.greedy(W[b:b + c], maxErr, False)
            _same(p.cpu().numpy(), f.cpu().numpy(), fp, ff, "phase 1 of rank at %d" % b)
        col_all = torch.cat([l[2] for l in locals_])
        mp, mf, op, of = _expect(orc, ns, nd, 16, maxErr, True)
        for (b, c), (p, f, _) in zip(part, locals_):
            p2, f2 = eng.phase2(col_all, R, nd, p.clone(), f.clone(), b)
            torch.cuda.synchronize()
            _same(p2.cpu().numpy(), f2.cpu().numpy(), mp[b:b + c], mf[b:b + c], "R=%d rank at %d vs model" % (R, b))
            _same(p2.cpu().numpy(), f2.cpu().numpy(), op[b:b + c], of[b:b + c], "R=%d rank at %d vs oracle" % (R, b))


# ------------------------------------------------------------------------------------------------------------------ 5. device entry point
@pytest.mark.parametrize("valu", [False, True])
def test_device_entry_point(api, orc, torch_ctx, monkeypatch, valu):
    """bhip_assoc_hamming_dev on device tensors: it writes rows [0, ns) of the outputs and nothing else; nd == 0 leaves every row unmatched at
    maxFitError, ns == 0 writes nothing."""
    import torch
    from boofcv_amd import _lib
    L = _lib.load()
    if valu:
        monkeypatch.setenv("BHIP_HAM_VALU", "1")
    else:
        monkeypatch.delenv("BHIP_HAM_VALU", raising=False)
    ns, nd, GUARD = 129, 97, 64
    src, dst, W = ar.case(ns, nd)
    ts, td = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dst.copy()).cuda()      # the shared arrays are read-only
    P = lambda t: C.c_void_p(t.data_ptr())

    def run(n_src, n_dst, maxErr, backwards):
        pairs = torch.full((ns + GUARD,), -7, dtype=torch.int32, device="cuda")
        fit = torch.full((ns + GUARD,), -3.0, dtype=torch.float64, device="cuda")
        torch_ctx.profileReset()
        st = L.bhip_assoc_hamming_dev(torch_ctx._h, P(ts), n_src, P(td), n_dst, 16, maxErr, int(backwards), P(pairs), P(fit))
        assert st == 0, L.bhip_last_error(torch_ctx._h)
        torch.cuda.synchronize()
        pairs, fit = pairs.cpu().numpy(), fit.cpu().numpy()
        assert (pairs[n_src:] == -7).all() and (fit[n_src:] == -3.0).all()
        return pairs[:n_src], fit[:n_src]

    for backwards in (False, True):
        for maxErr in ar.thresholds(W):
            p, f = run(ns, nd, maxErr, backwards)
            assert _path(torch_ctx, backwards) == ("scan" if valu else "mfma")
            mp, mf, op, of = _expect(orc, ns, nd, 16, maxErr, backwards)
            _same(p, f, mp, mf, "dev vs model")
            _same(p, f, op, of, "dev vs oracle")
        p, f = run(ns, 0, 3.0, backwards)
        assert (p == -1).all() and (f == 3.0).all()
        _same(p, f, *ar.greedy(W[:, :0], 3.0, backwards), "nd == 0")
        p, f = run(0, nd, 3.0, backwards)
        assert len(p) == 0
        assert not any(k.startswith(("k_ham_mfma", "k_assoc_scan")) for k in torch_ctx.profileReport())
