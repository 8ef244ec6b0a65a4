"""GPU: the key-point list of the Fast-Hessian detector regrows (FhDetector::run in csrc/cabi.hip) inside a detect+describe object, with state
around it: a batch in which one frame overflows BHIP_SURF_INITIAL_CAPACITY and its neighbours do not, describe / BRIEF / fetchAll /
associateImages reading the list at the new pitch, the chunked host path falling back (or appending between two pitches) and the N-best
listing.  Everything is compared with the CPU oracle at the project's usual bars: key points bit-exact and in reference order, Laplacian
sign exact, every descriptor within 1e-5, every orientation within 1e-12 rad, no exception list.

Frames are 720x540, ConfigFastHessian(detectThreshold=0, extractRadius=1).  Oracle counts next to the capacity (8192), GrayF32 / GrayU8:
A (noise everywhere) 10863 / 10869; C, C2, C3 (constant 50, noise in the top-left 360x270) 3641, 3630, 3706 / 2881, 2825, 2938; Z (zeros) 0;
the 240x180 noise frame of the last step 1003 / 1002; with maxFeaturesPerScale=300 A keeps 745 and C 647 of those.  A regrow takes the
capacity to 10863 + 10863 / 4 + 64 = 13642.  Every test asserts its preconditions from the oracle's own counts before it compares, so a
case that no longer crosses the capacity fails instead of passing vacuously; the chunked cases also check, through the number of
k_describe launches, that each call took the path it is there for."""
import os

import numpy as np
import pytest

from boofcv_amd import _lib

pytestmark = pytest.mark.gpu

DESC_TOL = 1e-5
W, H = 720, 540
CAP = _lib.BHIP_SURF_INITIAL_CAPACITY
FH = dict(detectThreshold=0, extractRadius=1)
THREADS = min(os.cpu_count() or 1, 8)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()
    return a


# ---------------------------------------------------------------------------------------------------------------- frames and references
_frame_cache, _ref_cache = {}, {}


def _frame(orc, name, u8):
    """A: noise everywhere; C, C2, C3: constant 50 with noise in the top-left quarter; Z: zeros; S: the small frame of another shape.
    GrayF32 frames hold 0..100 noise, GrayU8 frames the floor of 0..255 noise."""
    key = (name, u8)
    if key not in _frame_cache:
        hi = 255.0 if u8 else 100.0
        if name == "A":
            a = orc.noise_image(W, H, 5, 0.0, hi).array().copy()
        elif name == "S":
            a = orc.noise_image(240, 180, 7, 0.0, hi).array().copy()
        elif name == "Z":
            a = np.zeros((H, W), np.float32)
        else:
            a = np.full((H, W), 50.0, np.float32)
            a[:270, :360] = orc.noise_image(360, 270, {"C": 11, "C2": 12, "C3": 13}[name], 0.0, hi).array()
        _frame_cache[key] = np.floor(a).astype(np.uint8) if u8 else np.ascontiguousarray(a, np.float32)
    return _frame_cache[key]


def _image(api, orc, name, u8):
    return (api.GrayU8 if u8 else api.GrayF32).wrap(_frame(orc, name, u8))


def _surf_ref(orc, name, u8=False, stable=True):
    """(xy_scale, angle, white, desc) of the oracle's detect + describe, computed once per frame and shared"""
    key = ("surf", name, u8, stable)
    if key not in _ref_cache:
        ref = orc.Surf(stable, fh=orc.FhCfg(**FH))
        if u8:
            ref.detect_u8(_frame(orc, name, True), threads=THREADS)
        else:
            ref.detect(orc.Gray.from_array(_frame(orc, name, False)), threads=THREADS)
        _ref_cache[key] = ref.fetch()
    return _ref_cache[key]


def _points_ref(orc, name, **cfg):
    """the oracle's Fast-Hessian points of a GrayF32 frame"""
    key = ("fh", name, tuple(sorted(cfg.items())))
    if key not in _ref_cache:
        ii = orc.integral(orc.Gray.from_array(_frame(orc, name, False)))
        _ref_cache[key] = orc.fh_detect(ii, orc.FhCfg(**dict(FH, **cfg)), threads=THREADS)
    return _ref_cache[key]


def _preconditions(counts):
    """counts: frame name -> the oracle's number of key points.  Frame A crosses the initial capacity, the quarter-noise frames stay well
    under it, the blank frame has nothing."""
    assert "A" in counts
    for name, n in counts.items():
        if name == "A":
            assert n > CAP, (name, n, CAP)
        elif name == "Z":
            assert n == 0, (name, n)
        elif name != "S":
            assert 1000 <= n <= CAP // 2, (name, n, CAP)


def _surf_preconditions(orc, names, u8=False, stable=True):
    _preconditions({n: len(_surf_ref(orc, n, u8, stable)[0]) for n in names})


def _compare(got, want):
    """one image's (xy_scale, angle, white, desc) against the oracle's: the bars of test_gpu_parity._compare_surf"""
    xys, ang, white, desc = want
    assert len(got[0]) == len(xys)
    assert np.array_equal(got[0], xys)          # location + scale: bit exact, reference order
    assert np.array_equal(got[2], white)        # Laplacian sign
    if len(xys):
        dang = np.abs(np.angle(np.exp(1j * (got[1] - ang))))
        derr = np.max(np.abs(got[3] - desc), axis=1)
        nout = int((derr > DESC_TOL).sum())
        assert nout == 0, "descriptors outside 1e-5: %d of %d, max err %.3g" % (nout, len(xys), derr.max())
        assert dang.max() < 1e-12, "orientation max err %.3g rad at key point %d" % (dang.max(), int(dang.argmax()))
        assert np.allclose(np.linalg.norm(got[3], axis=1), 1, atol=1e-12)


def _compare_batch(orc, dd, names, u8=False, stable=True):
    """every frame of the last batch against the oracle; fetchAll slices against the per-image fetches; totalFeatures against the counts"""
    per_image = [tuple(np.array(x) for x in dd._results(i)) for i in range(len(names))]
    for name, got in zip(names, per_image):
        _compare(got, _surf_ref(orc, name, u8, stable))
    xys, ang, white, desc, starts = dd.fetchAll()
    assert [int(s) for s in np.diff(starts)] == [len(p[0]) for p in per_image]
    assert dd.totalFeatures() == sum(len(p[0]) for p in per_image) == int(starts[-1])
    for i, one in enumerate(per_image):
        sl = slice(int(starts[i]), int(starts[i + 1]))
        assert np.array_equal(xys[sl], one[0]) and np.array_equal(ang[sl], one[1]) and np.array_equal(white[sl], one[2]) and np.array_equal(desc[sl], one[3]), i


def _copy(arrays):
    return tuple(np.array(a) for a in arrays)


def _same_arrays(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), (what, k)


def _make(api, stable=True, u8=False, ctx=None, **cfg):
    fac = api.FactoryDetectDescribe.surfStable if stable else api.FactoryDetectDescribe.surfFast
    return fac(api.ConfigFastHessian(**dict(FH, **cfg)), None, None, api.GrayU8 if u8 else api.GrayF32, ctx=ctx)


# ---------------------------------------------------------------------------------------------------------------- orientation ties
def test_orientation_ties_in_the_flat_part_of_a_float_frame(api, orc):
    """(no regrow: one frame per call.)  With detectThreshold = 0 the flat three quarters of a GrayF32 quarter-noise frame yield key points too:
    their gradients are the integral image's quantized round-off, sample sets come out mirror-symmetric, and candidate windows of the sliding
    orientation tie exactly.  The winner then depends on how the window sums round, so such key points must go through the reference's
    serial sweep (describe.hip, slidingWindowFast): before that, key point 21 of C2 and key point 2308 of C3 came out 0.37 and 0.54 rad
    off, their descriptors 0.22 and 0.39."""
    dd = _make(api)
    for name in ("C", "C2", "C3"):
        want = _surf_ref(orc, name)
        flat = (want[0][:, 0] >= 380) | (want[0][:, 1] >= 290)
        assert flat.sum() >= 500, (name, int(flat.sum()))     # key points well inside the constant part
        dd.detect(_image(api, orc, name, False))
        _compare(_copy(dd._results(0)), want)
    dd.close()


# ---------------------------------------------------------------------------------------------------------------- the plain path
@pytest.mark.parametrize("stable", [True, False], ids=["surfStable", "surfFast"])
@pytest.mark.parametrize("u8", [False, True], ids=["GrayF32", "GrayU8"])
def test_batch_with_one_overflowing_frame(api, orc, u8, stable):
    """[C, A, Z, C2] on a fresh object: the detector reruns the whole batch at a wider [image][cap] pitch because of frame A alone.  Then a
    smaller batch on the grown object, then one frame of another shape (plan rebuilt, capacity kept)."""
    _surf_preconditions(orc, ["C", "A", "Z", "C2", "C3", "S"], u8, stable)
    assert len(_surf_ref(orc, "S", u8, stable)[0]) > 500
    dd = _make(api, stable, u8)
    for names in (["C", "A", "Z", "C2"], ["C3", "C"], ["S"]):
        dd.detectBatch([_image(api, orc, n, u8) for n in names])
        _compare_batch(orc, dd, names, u8, stable)
    dd.close()


def test_device_batch_with_one_overflowing_frame(api, orc):
    """the same four frames device-resident with padded rows (row stride 736, image stride 736 * 545, every padding element 1e6): array for
    array what the dense host batch gives, which in turn is the oracle's"""
    torch = pytest.importorskip("torch")
    names = ["C", "A", "Z", "C2"]
    _surf_preconditions(orc, names)
    stride, rows = 736, 545
    host = _make(api)
    host.detectBatch([_image(api, orc, n, False) for n in names])
    want = _copy(host.fetchAll())
    assert [int(c) for c in np.diff(want[4])] == [len(_surf_ref(orc, n)[0]) for n in names]
    padded = np.full((len(names), rows, stride), 1e6, dtype=np.float32)
    for b, n in enumerate(names):
        padded[b, :H, :W] = _frame(orc, n, False)
    frames = torch.from_numpy(padded).cuda()
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    dev = _make(api, ctx=ctx)
    dev.detectDevice(frames.data_ptr(), stride * rows, stride, W, H, len(names))
    _same_arrays(_copy(dev.fetchAll()), want, "device batch")
    _compare(_copy(dev._results(1)), _surf_ref(orc, "A"))
    dev.close(); ctx.close(); host.close()


def test_overflow_in_front_of_association(api, orc):
    """associateImages on the descriptors left resident by a batch that regrew: source / destination pairs that read frame A's descriptors
    from both sides, against the oracle's greedy association of the fetched descriptors -- pairs and scores identical"""
    names = ["C", "A", "Z", "C2"]
    _surf_preconditions(orc, names)
    dd = _make(api)
    dd.detectBatch([_image(api, orc, n, False) for n in names])
    xys, ang, white, desc, starts = _copy(dd.fetchAll())
    assert [int(c) for c in np.diff(starts)] == [len(_surf_ref(orc, n)[0]) for n in names]
    src, dst = [0, 1, 3], [1, 3, 0]
    pairs, fit = dd.associateImages(src, dst)
    matched = 0
    for a, b in zip(src, dst):
        sa = slice(int(starts[a]), int(starts[a + 1]))
        ep, ef = orc.associate_l2(desc[sa], desc[int(starts[b]):int(starts[b + 1])], orc.MAX_VALUE_F64, True, threads=THREADS)
        assert np.array_equal(pairs[sa], ep) and np.array_equal(fit[sa], ef), (a, b)
        matched += int((ep >= 0).sum())
    assert matched > 1000
    sz = slice(int(starts[2]), int(starts[3]))
    assert np.all(pairs[sz] == -1) and np.all(fit[sz] == 0.0)
    dd.close()


# ---------------------------------------------------------------------------------------------------------------- the chunked host path
ORDERS = {"overflow_in_second_chunk": ["C", "C2", "A", "Z", "C3"], "overflow_in_first_chunk": ["A", "C", "C2", "Z", "C3"]}


def _plain_result(api, orc, names, monkeypatch):
    """fetchAll of an unchunked object on these frames, once per order"""
    key = ("plain",) + tuple(names)
    if key not in _ref_cache:
        monkeypatch.delenv("BHIP_SURF_CHUNK", raising=False)
        dd = _make(api)
        dd.detectBatch([_image(api, orc, n, False) for n in names])
        _ref_cache[key] = _copy(dd.fetchAll())
        dd.close()
    return _ref_cache[key]


def _describe_launches(dd, images):
    """detectBatch under the per-kernel profile -> how often k_describe was launched: once for a plain batch, once per chunk on the chunked
    path.  This is how the cases below know which path a call took."""
    ctx = dd.ctx
    ctx.profile(True)
    ctx.profileReset()
    try:
        dd.detectBatch(images)
        return ctx.profileReport().get("k_describe", {}).get("launches", 0)
    finally:
        ctx.profile(False)


def _slice_of(result, i):
    xys, ang, white, desc, starts = result
    sl = slice(int(starts[i]), int(starts[i + 1]))
    return xys[sl], ang[sl], white[sl], desc[sl]


@pytest.mark.parametrize("order", list(ORDERS))
def test_chunked_batch_falls_back_when_a_frame_overflows(api, orc, monkeypatch, order):
    """BHIP_SURF_CHUNK=2, five frames (chunks 2, 2, 1).  The worker's list regrows inside the chunk that holds frame A, the owner's [image][cap]
    array is then too narrow for it and the whole batch goes the plain way -- after chunk 0 has been appended (second chunk) or before anything
    has (first chunk).  The second batch on the same object finds owner and worker both grown and stays chunked."""
    names, again = ORDERS[order], ORDERS["overflow_in_second_chunk"]
    _surf_preconditions(orc, names)
    plain, plain_again = _plain_result(api, orc, names, monkeypatch), _plain_result(api, orc, again, monkeypatch)
    _compare(_slice_of(plain, names.index("A")), _surf_ref(orc, "A"))
    monkeypatch.setenv("BHIP_SURF_CHUNK", "2")
    dd = _make(api)
    # the chunks up to and including the one with frame A are described by the worker, then the whole batch once more the plain way
    assert _describe_launches(dd, [_image(api, orc, n, False) for n in names]) == names.index("A") // 2 + 2
    _same_arrays(_copy(dd.fetchAll()), plain, order)
    _compare(_copy(dd._results(names.index("A"))), _surf_ref(orc, "A"))
    assert _describe_launches(dd, [_image(api, orc, n, False) for n in again]) == 3     # three chunks, no fallback
    _same_arrays(_copy(dd.fetchAll()), plain_again, order + ", second batch")
    _compare(_copy(dd._results(again.index("A"))), _surf_ref(orc, "A"))
    dd.close()


def test_chunked_append_between_two_pitches(api, orc, monkeypatch):
    """The owner's list grows in a batch too small to be chunked (three frames, BHIP_SURF_CHUNK=2), so no worker exists yet.  The next batch
    is chunked: the new worker starts at the initial capacity, chunk 0 [C, C2] is copied from its pitch into the owner's wider one, and the
    worker regrows in chunk 1 [A, Z] without the batch leaving the chunked path."""
    names = ORDERS["overflow_in_second_chunk"]
    _surf_preconditions(orc, names)
    plain = _plain_result(api, orc, names, monkeypatch)
    monkeypatch.setenv("BHIP_SURF_CHUNK", "2")
    dd = _make(api)
    assert _describe_launches(dd, [_image(api, orc, n, False) for n in ["C", "A", "Z"]]) == 1      # below two chunks: the plain path
    _compare_batch(orc, dd, ["C", "A", "Z"])
    assert _describe_launches(dd, [_image(api, orc, n, False) for n in names]) == 3                # three chunks, no fallback
    _same_arrays(_copy(dd.fetchAll()), plain, "chunked after a plain regrow")
    for i, n in enumerate(names):
        _compare(_copy(dd._results(i)), _surf_ref(orc, n))
    dd.close()


# ---------------------------------------------------------------------------------------------------------------- BRIEF, N-best
def _brief_ref(orc, name):
    key = ("brief", name)
    if key not in _ref_cache:
        sp, cp = orc.brief_definition()
        pts = _points_ref(orc, name)
        _ref_cache[key] = pts, orc.brief_describe(orc.Gray.from_array(_frame(orc, name, False)), pts[:, :2].copy(), 16, sp, cp)
    return _ref_cache[key]


def _compare_brief_batch(orc, dd, names):
    refs = [_brief_ref(orc, n) for n in names]
    for i, (pts, words) in enumerate(refs):
        r = dd._results(i)
        assert np.array_equal(r[0], pts), (names, i)
        assert np.array_equal(r[3], words), (names, i)
    xys, words_all, starts = dd.fetchAll()
    assert np.array_equal(xys, np.concatenate([r[0] for r in refs])) and np.array_equal(words_all, np.concatenate([r[1] for r in refs]))


def test_brief_fusion_with_an_overflowing_frame(api, orc, monkeypatch):
    """Fast-Hessian + BRIEF reads the key points at the list's pitch too (bhip_launch_brief): points and words bit-exact against the oracle.
    Plain path; then BHIP_SURF_CHUNK=2, where [C, A, Z] is below two chunks and grows the owner, [C, C2, A, Z] stays chunked with a fresh worker
    (append between two pitches, worker regrow) and, on a fresh object, [C, A, Z, C2] falls back from the first chunk."""
    def fuse():
        brief = api.FactoryDescribeRegionPoint.brief(None, api.GrayF32)
        return api.FactoryDetectDescribe.fuseTogether(api.FactoryInterestPoint.fastHessian(api.ConfigFastHessian(**FH)), None, brief)

    _preconditions({n: len(_points_ref(orc, n)) for n in ["C", "A", "Z", "C2"]})
    monkeypatch.delenv("BHIP_SURF_CHUNK", raising=False)
    dd = fuse()
    dd.detectBatch([_image(api, orc, n, False) for n in ["C", "A", "Z"]])
    _compare_brief_batch(orc, dd, ["C", "A", "Z"])
    dd.close()
    monkeypatch.setenv("BHIP_SURF_CHUNK", "2")
    dd = fuse()
    for names in (["C", "A", "Z"], ["C", "C2", "A", "Z"]):
        dd.detectBatch([_image(api, orc, n, False) for n in names])
        _compare_brief_batch(orc, dd, names)
    dd.close()
    dd = fuse()
    dd.detectBatch([_image(api, orc, n, False) for n in ["C", "A", "Z", "C2"]])
    _compare_brief_batch(orc, dd, ["C", "A", "Z", "C2"])
    dd.close()


def test_nbest_listing_overflows_in_a_batch(api, orc):
    """maxFeaturesPerScale=300: the list holds every level's NMS maxima before the selection -- at least the key points of the unlimited
    detector, which is what the precondition is stated on -- and the selection reads it at the regrown pitch"""
    names = ["C", "A", "Z"]
    _preconditions({n: len(_points_ref(orc, n)) for n in names})
    dd = _make(api, maxFeaturesPerScale=300)
    dd.detectBatch([_image(api, orc, n, False) for n in names])
    for i, n in enumerate(names):
        want = _points_ref(orc, n, maxFeaturesPerScale=300)
        assert len(want) > 300 or n == "Z"
        assert len(want) < len(_points_ref(orc, n)) or n == "Z"     # the limit prunes
        assert np.array_equal(dd._results(i)[0], want), n
    dd.close()
