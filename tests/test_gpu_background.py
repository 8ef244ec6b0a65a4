"""GPU: the stationary background models (Basic, Gaussian, GMM on GrayU8 / GrayF32 / Planar of 1..4 bands), bit for bit against
tests/background_ref.py, through the device-batched API (device.DeviceBackgroundModel), the host classes (api.BackgroundStationary*) and the C
ABI.  Every comparison is exact: masks as bytes, the whole model state as fp32 bit patterns, after the last frame and after a prefix.

The kernel's tile is 64 * PX columns x 4 rows of one stream per workgroup, PX = 4, 2 or 1 consecutive pixels per lane for models of <= 16,
<= 32 or more float components, the lanes' groups aligned to the address of the mask row (boofcv_amd/csrc/background.hip).  1030 x 5 spans
five workgroups in x at PX = 4 (seventeen at PX = 1) and two in y, 130 x 70 spans three at PX = 1 and eighteen in y; 67, 1030 and 130 are no
multiples of 4 and 1 x 7 is narrower than a lane's group (and the width at which BackgroundStationaryGaussian never initialises)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import background_ref as bref
import view_layouts as vl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = np.array([40, 120, 210], np.float32)

# name -> (algorithm, config fields)
CONFIGS = {
    "basic": ("basic", dict(threshold=5.0, learnRate=0.25)),
    "gaussian": ("gaussian", dict(threshold=12.0, learnRate=0.05)),
    "gaussian_half": ("gaussian", dict(threshold=12.0, learnRate=0.5)),
    "gaussian_min5": ("gaussian", dict(threshold=12.0, learnRate=0.5, minimumDifference=5.0)),
    "gaussian_var100": ("gaussian", dict(threshold=12.0, learnRate=0.05, initialVariance=100.0, minimumDifference=5.0, unknownValue=7)),
    "gmm2": ("gmm", dict(learningPeriod=4.0, decayCoefient=0.5, numberOfGaussian=2, significantWeight=0.5, unknownValue=3)),
    "gmm3": ("gmm", dict(learningPeriod=4.0, decayCoefient=0.5, numberOfGaussian=3, significantWeight=0.5, unknownValue=3)),
    "gmm_default": ("gmm", dict()),
}
KINDS = {"u8": (np.uint8, 0), "f32": (np.float32, 0), "pl1_u8": (np.uint8, 1), "pl2_f32": (np.float32, 2), "pl3_u8": (np.uint8, 3), "pl3_f32": (np.float32, 3),
         "pl4_u8": (np.uint8, 4)}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    if bad.any():
        first = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError("%s: %d elements differ; first at %s: got %r want %r" % (what, int(bad.sum()), first, got[bad][0], want[bad][0]))


@functools.lru_cache(maxsize=None)
def _frames(kind, S, T, H, W, seed=1, constant=False):
    """[S][T][(B)][H][W]: every pixel jumps between three levels with small noise (the same level in every band, the bands 7 apart); with
    `constant` the left third of every frame keeps its first value"""
    dtype, bands = KINDS[kind]
    rng = np.random.default_rng(seed)
    nb = max(bands, 1)
    level = LEVELS[rng.integers(0, 3, (S, T, 1, H, W))]
    noise = rng.integers(-2, 3, (S, T, nb, H, W)).astype(np.float32)
    if dtype == np.float32:
        noise = noise + rng.integers(0, 4, (S, T, nb, H, W)).astype(np.float32) * np.float32(0.25)
    a = level + noise + np.arange(nb, dtype=np.float32).reshape(1, 1, nb, 1, 1) * 7
    if constant:
        a[:, :, :, :, :(W + 2) // 3] = a[:, :1, :, :, :(W + 2) // 3]
    a = a.astype(dtype)
    if bands == 0:
        a = a[:, :, 0]
    a.setflags(write=False)
    return a


def _segframes(kind, S, H, W, seed, constant):
    """the frames segment() is asked about: other levels and noise than any frame of the sequence, so that pixels of the constant region differ
    from their model (x/0) or, now and then, equal it (0/0)"""
    return _frames(kind, S, 1, H, W, seed + 100, False)[:, 0]


def _ref_model(cfgname, bands):
    alg, kw = CONFIGS[cfgname]
    if alg == "basic":
        return bref.stationaryBasic(kw["learnRate"], kw["threshold"], bands)
    if alg == "gaussian":
        return bref.stationaryGaussian(bands=bands, **kw)
    return bref.stationaryGmm(bands, **kw)


@functools.lru_cache(maxsize=None)
def _want(cfgname, kind, S, T, H, W, seed=1, constant=False, prefix=1):
    """per stream: masks [T][H][W], the state after `prefix` frames and after the last, the segmentation of _segframes afterwards, the counters"""
    fr = _frames(kind, S, T, H, W, seed, constant)
    sf = _segframes(kind, S, H, W, seed, constant)
    out = []
    for s in range(S):
        m = _ref_model(cfgname, KINDS[kind][1])
        masks = []
        mid = None
        for t in range(T):
            masks.append(m.updateBackground(fr[s, t], True))
            if t + 1 == prefix:
                mid = np.array(m.state())
        seg = m.segment(sf[s])
        out.append((np.stack(masks), mid, np.array(m.state()), seg, dict(m.counts)))
    return out


def _api_config(cfgname):
    from boofcv_amd import api
    alg, kw = CONFIGS[cfgname]
    if alg == "basic":
        c = api.ConfigBackgroundBasic(kw["threshold"], kw["learnRate"])
    elif alg == "gaussian":
        c = api.ConfigBackgroundGaussian(kw["threshold"], kw["learnRate"])
    else:
        c = api.ConfigBackgroundGmm()
    for k, v in kw.items():
        setattr(c, k, v)
    return alg, c


@functools.lru_cache(maxsize=None)
def _torch_ctx():
    import torch
    from boofcv_amd import api
    return api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)


def _device_model(torch, cfgname, kind):
    from boofcv_amd.device import DeviceBackgroundModel
    alg, c = _api_config(cfgname)
    dtype, bands = KINDS[kind]
    return DeviceBackgroundModel(alg, c, torch.uint8 if dtype == np.uint8 else torch.float32, bands, ctx=_torch_ctx())


def _check_against(torch, cfgname, kind, S, T, H, W, with_masks=True, constant=False, calls=None, seed=1):
    """the frames in the given split (`calls`: frames per update() call; default one call), compared after the first call and at the end"""
    calls = calls or [T]
    prefix = calls[0]
    want = _want(cfgname, kind, S, T, H, W, seed, constant, prefix)
    fr = torch.as_tensor(np.array(_frames(kind, S, T, H, W, seed, constant)), device="cuda:0")
    bg = _device_model(torch, cfgname, kind)
    try:
        t0 = 0
        for i, n in enumerate(calls):
            sentinel = torch.full((S, n, H, W), 0xA5, dtype=torch.uint8, device="cuda:0")
            got = bg.update(fr[:, t0:t0 + n], sentinel if with_masks else None)
            bg.ctx.synchronize()
            if with_masks:
                for s in range(S):
                    _same(got[s], want[s][0][t0:t0 + n], "%s %s masks of stream %d, frames %d..%d" % (cfgname, kind, s, t0, t0 + n - 1))
            t0 += n
            if i == 0 and want[0][1] is not None:
                for s in range(S):
                    _same(bg.model(s).reshape(want[s][1].shape), want[s][1], "%s %s model of stream %d after %d frames" % (cfgname, kind, s, prefix))
        for s in range(S):
            _same(bg.model(s).reshape(want[s][2].shape), want[s][2], "%s %s model of stream %d after all frames" % (cfgname, kind, s))
        seg = bg.segment(torch.as_tensor(np.array(_segframes(kind, S, H, W, seed, constant)), device="cuda:0"))
        bg.ctx.synchronize()
        for s in range(S):
            _same(seg[s], want[s][3], "%s %s segment of stream %d" % (cfgname, kind, s))
        for s in range(S):   # segment() changes no model
            _same(bg.model(s).reshape(want[s][2].shape), want[s][2], "%s %s model of stream %d after segment" % (cfgname, kind, s))
    finally:
        bg.close()
    return want


# ---- sequences built to hit every branch: asserted on the CPU first ----
GMM_BRANCHES = ("match", "new_gaussian", "first_gaussian", "full", "prune", "prune_moves_best", "match_insignificant")


@pytest.mark.parametrize("kind", ["u8", "pl3_u8", "pl2_f32"])
def test_gmm_every_branch(torch, kind):
    """maxGaussians 2 and 3, learningPeriod 4, decayCoefient 0.5: match, new Gaussian with room, first Gaussian (returns the unknown value of
    `common`, 0 here although the model's is 3), full mixture, a prune, a prune that moves the best Gaussian, a match below significantWeight"""
    total = {}
    for cfgname in ("gmm2", "gmm3"):
        for w in _want(cfgname, kind, 1, 7, 9, 40):
            for k, v in w[4].items():
                total[k] = total.get(k, 0) + v
    for b in GMM_BRANCHES:
        assert total.get(b, 0) > 0, "the sequence does not reach branch %r: %s" % (b, total)
    for cfgname in ("gmm2", "gmm3"):
        want = _check_against(torch, cfgname, kind, 1, 7, 9, 40, calls=[1, 6])
        assert set(np.unique(want[0][0][0])) == {0}       # first frame: common.unknownValue, still 0
        assert 3 not in np.unique(want[0][0])


@pytest.mark.parametrize("kind", ["u8", "f32", "pl3_u8", "pl1_u8", "pl4_u8"])
def test_gmm_default_config(torch, kind):
    _check_against(torch, "gmm_default", kind, 1, 12, 9, 40, calls=[1, 11])


@pytest.mark.parametrize("kind", ["u8", "f32", "pl3_u8", "pl2_f32"])
@pytest.mark.parametrize("cfgname", ["gaussian", "gaussian_half", "gaussian_min5", "gaussian_var100"])
def test_gaussian_denormal_variance(torch, cfgname, kind):
    """initialVariance = Float.MIN_VALUE on frames whose left third is constant: with learnRate 0.05 the variance stays the denormal, with 0.5
    it rounds to zero, and segment() divides by both: 0/0 = NaN (falls into the minimumDifference branch), x/0 = +Inf"""
    want = _want(cfgname, kind, 1, 4, 9, 40, 2, True, 1)
    c = want[0][4]
    if cfgname == "gaussian":
        assert c.get("denormal_variance", 0) > 0 and c.get("inf", 0) > 0, c
    if cfgname in ("gaussian_half", "gaussian_min5"):
        assert c.get("zero_variance", 0) > 0 and c.get("nan", 0) > 0 and c.get("inf", 0) > 0, c
    if cfgname == "gaussian_min5":
        assert c.get("beyond_close", 0) > 0 and c.get("beyond_far", 0) > 0, c
    _check_against(torch, cfgname, kind, 1, 4, 9, 40, constant=True, calls=[1, 3], seed=2)


@pytest.mark.parametrize("kind", ["u8", "pl3_u8", "f32", "pl3_f32"])
def test_basic_threshold_equality(torch, kind):
    """integer pixels and threshold 5: diff*diff == thresholdSq occurs (SB in float, PL as a double sum against numBands*threshold*threshold)"""
    from boofcv_amd.device import DeviceBackgroundModel
    dtype, bands = KINDS[kind]
    H, W = 9, 40
    rng = np.random.default_rng(5)
    shape = (1, 2, H, W) if bands == 0 else (1, 2, bands, H, W)
    fr = np.zeros(shape, np.float32)
    fr[:, 0] = rng.integers(20, 200, shape[2:])
    delta = rng.choice(np.array([-6, -5, -4, 0, 4, 5, 6], np.float32), (H, W))
    fr[:, 1] = fr[:, 0] + delta          # the same difference in every band
    fr = fr.astype(dtype)
    ref = bref.stationaryBasic(0.25, 5.0, bands)
    ref.updateBackground(fr[0, 0])
    want = ref.segment(fr[0, 1])
    assert ref.counts["equal"] > 0 and ref.counts["below"] > 0 and ref.counts["above"] > 0, ref.counts
    _, c = _api_config("basic")
    bg = DeviceBackgroundModel("basic", c, torch.uint8 if dtype == np.uint8 else torch.float32, bands, ctx=_torch_ctx())
    try:
        t = torch.as_tensor(fr, device="cuda:0")
        bg.update(t[:, :1])
        _same(bg.segment(t[:, 1])[0], want, "basic segment at the threshold")
        _same(bg.model(0), ref.state(), "basic model")
    finally:
        bg.close()


# (W, H), streams, frames, kind per algorithm
SHAPE_CASES = [((67, 21), 3, 7, ("u8", "pl2_f32", "pl3_u8")), ((40, 9), 1, 2, ("f32", "pl3_u8", "u8")), ((1, 7), 3, 7, ("u8", "u8", "pl2_f32")),
               ((1030, 5), 1, 2, ("pl3_u8", "f32", "u8")), ((130, 70), 1, 2, ("f32", "pl1_u8", "pl3_f32")), ((67, 21), 1, 1, ("pl4_u8", "pl4_u8", "pl4_u8"))]


@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("case", range(len(SHAPE_CASES)))
@pytest.mark.parametrize("alg", [0, 1, 2], ids=["basic", "gaussian_var100", "gmm3"])
def test_shapes_and_batches(torch, alg, case, with_masks):
    (W, H), S, T, kinds = SHAPE_CASES[case]
    cfgname = ("basic", "gaussian_var100", "gmm3")[alg]
    _check_against(torch, cfgname, kinds[alg], S, T, H, W, with_masks=with_masks, calls=[1, T - 1] if T > 1 else [1])


@pytest.mark.parametrize("cfgname,kind", [("basic", "pl3_u8"), ("gaussian_var100", "u8"), ("gmm3", "u8"), ("gmm_default", "pl3_u8")])
def test_seven_frames_in_one_call_equal_seven_calls(torch, cfgname, kind):
    _check_against(torch, cfgname, kind, 3, 7, 21, 67, calls=[7])
    _check_against(torch, cfgname, kind, 3, 7, 21, 67, calls=[1] * 7)
    _check_against(torch, cfgname, kind, 3, 7, 21, 67, calls=[2, 5])


# ---- views ----
def _strided(torch, layout, lead, H, W, dtype, shift=0):
    """a [*lead, H, W] window of `layout` into a sentinel-filled parent: the images are consecutive images of the layout"""
    n = int(np.prod(lead))
    parent, v = vl.make_view(layout, n, H, W, dtype, "cuda:0", shift)
    img, pitch = (v.stride(0) if n > 1 else vl.geometry(layout, n, H, W)[1]), v.stride(1)
    strides = []
    for i in range(len(lead)):
        strides.append(img * int(np.prod(lead[i + 1:])))
    view = torch.as_strided(parent, tuple(lead) + (H, W), tuple(strides) + (pitch, 1), v.storage_offset())
    return parent, view, v


@pytest.mark.parametrize("layout", vl.LAYOUTS)
@pytest.mark.parametrize("cfgname,kind", [("basic", "pl3_u8"), ("gaussian_var100", "f32"), ("gmm3", "u8"), ("gmm3", "pl2_f32")])
def test_strided_views_and_guard_bands(torch, cfgname, kind, layout):
    """frames and masks as strided views (GrayU8 rows at odd byte addresses in pad4_x1 and odd) inside sentinel-filled parents: the masks equal
    the reference, nothing outside the mask view is written, the frames' parent is not written at all"""
    from boofcv_amd import device as dv
    S, T, H, W = 2, 3, 11, 37
    dtype, bands = KINDS[kind]
    tdt = torch.uint8 if dtype == np.uint8 else torch.float32
    want = _want(cfgname, kind, S, T, H, W, 3, False, 1)
    fr = np.array(_frames(kind, S, T, H, W, 3))
    lead = (S, T, bands) if bands else (S, T)
    fparent, fview, _ = _strided(torch, layout, lead, H, W, tdt, shift=1 if layout == "odd" else 0)
    fview.copy_(torch.as_tensor(fr, device="cuda:0"))
    mparent, mview, mflat = _strided(torch, layout, (S, T), H, W, torch.uint8)
    fbefore, mbefore = vl.snapshot(fparent), vl.snapshot(mparent)
    torch.cuda.synchronize()
    bg = _device_model(torch, cfgname, kind)
    try:
        bg.update(fview, mview)
        bg.ctx.synchronize()
        for s in range(S):
            _same(mview[s], want[s][0], "%s masks of stream %d" % (layout, s))
            _same(bg.model(s).reshape(want[s][2].shape), want[s][2], "%s model of stream %d" % (layout, s))
        vl.assert_only_view_written(mparent, mflat, mbefore, "update masks " + layout)
        assert bool((vl.bits(fparent) == fbefore).all()), "the frames were written"
        sparent, sview, sflat = _strided(torch, layout, (S,), H, W, torch.uint8, shift=-1 if layout == "odd" else 0)
        sbefore = vl.snapshot(sparent)
        torch.cuda.synchronize()
        fview[:, 0].copy_(torch.as_tensor(np.array(_segframes(kind, S, H, W, 3, False)), device="cuda:0"))
        torch.cuda.synchronize()
        bg.segment(fview[:, 0], sview)
        bg.ctx.synchronize()
        for s in range(S):
            _same(sview[s], want[s][3], "%s segment of stream %d" % (layout, s))
        vl.assert_only_view_written(sparent, sflat, sbefore, "segment " + layout)
    finally:
        bg.close()


# ---- C ABI: host entries, store / fetch, reset, refusals, lifetime ----
@pytest.fixture(scope="module")
def cabi():
    from boofcv_amd import _lib, api
    L = _lib.load()
    ctx = api.Context(0)
    yield L, _lib, ctx
    ctx.close()


def _create(cabi, cfgname, kind, W, H, S):
    L, _lib, ctx = cabi
    alg, kw = CONFIGS[cfgname]
    dtype, bands = KINDS[kind]
    family = _lib.BHIP_IMAGE_PLANAR if bands else _lib.BHIP_IMAGE_GRAY
    pixel = _lib.BHIP_PIXEL_U8 if dtype == np.uint8 else _lib.BHIP_PIXEL_F32
    h = C.c_void_p()
    if alg == "basic":
        cfg = _lib.BgBasicCfg()
        L.bhip_bg_basic_cfg_default(C.byref(cfg))
        fn = L.bhip_bg_create_basic
    elif alg == "gaussian":
        cfg = _lib.BgGaussianCfg()
        L.bhip_bg_gaussian_cfg_default(C.byref(cfg))
        fn = L.bhip_bg_create_gaussian
    else:
        cfg = _lib.BgGmmCfg()
        L.bhip_bg_gmm_cfg_default(C.byref(cfg))
        fn = L.bhip_bg_create_gmm
    for k, v in kw.items():
        setattr(cfg, k, v)
    assert fn(ctx._h, C.byref(cfg), family, pixel, bands, W, H, S, C.byref(h)) == 0, ctx.lastError()
    return h


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_float))


def _fetch(cabi, h, s):
    L, _lib, ctx = cabi
    n = C.c_longlong()
    assert L.bhip_bg_model_floats(h, C.byref(n)) == 0
    out = np.zeros(n.value, np.float32)
    st = L.bhip_bg_fetch_model(h, s, _ptr(out))
    return st, out


@pytest.mark.parametrize("cfgname,kind", [("basic", "u8"), ("gaussian_var100", "pl2_f32"), ("gmm3", "pl3_u8"), ("gmm2", "f32")])
def test_host_entries_equal_the_reference_and_store_fetch_is_the_identity(cabi, cfgname, kind):
    L, _lib, ctx = cabi
    S, T, H, W = 2, 3, 9, 40
    dtype, bands = KINDS[kind]
    nb = max(bands, 1)
    want = _want(cfgname, kind, S, T, H, W, 4, False, 1)
    fr = np.array(_frames(kind, S, T, H, W, 4))
    # host frames inside a padded parent: start 5, rows W + 3 apart
    pitch = W + 3
    parent = np.zeros(5 + S * T * nb * H * pitch + 8, dtype)
    win = np.lib.stride_tricks.as_strided(parent[5:], (S, T, nb, H, W), tuple(x * parent.itemsize for x in (T * nb * H * pitch, nb * H * pitch, H * pitch, pitch, 1)))
    win[...] = fr.reshape(S, T, nb, H, W)
    masks = np.full((S, T, H, W + 1), 0xA5, np.uint8)
    h = _create(cabi, cfgname, kind, W, H, S)
    try:
        upd = L.bhip_bg_update_u8 if dtype == np.uint8 else L.bhip_bg_update_f32
        assert upd(h, _ptr(parent), 5, T * nb * H * pitch, nb * H * pitch, H * pitch, pitch, T, _ptr(masks), 0, T * H * (W + 1), H * (W + 1), W + 1) == 0, ctx.lastError()
        for s in range(S):
            _same(masks[s, :, :, :W], want[s][0], "host update masks")
            st, m = _fetch(cabi, h, s)
            assert st == 0
            _same(m.reshape(want[s][2].shape), want[s][2], "host update model")
        assert (masks[:, :, :, W] == 0xA5).all()
        win[:, 0] = np.array(_segframes(kind, S, H, W, 4, False)).reshape(S, nb, H, W)
        seg = np.full((S, H, W), 0xA5, np.uint8)
        sfn = L.bhip_bg_segment_u8 if dtype == np.uint8 else L.bhip_bg_segment_f32
        assert sfn(h, _ptr(parent), 5, T * nb * H * pitch, H * pitch, pitch, _ptr(seg), 0, H * W, W) == 0, ctx.lastError()
        for s in range(S):
            _same(seg[s], want[s][3], "host segment")
        # store then fetch: the identity, on bit patterns that are no result of the algorithm (NaN payloads, negative zero, denormals)
        n = want[0][2].size
        pattern = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)).view(np.float32)
        assert L.bhip_bg_store_model(h, 1, _ptr(pattern)) == 0
        st, back = _fetch(cabi, h, 1)
        assert st == 0
        _same(back, pattern, "store then fetch")
        st, other = _fetch(cabi, h, 0)
        _same(other.reshape(want[0][2].shape), want[0][2], "the other stream after a store")
    finally:
        assert L.bhip_bg_destroy(h) == 0


@pytest.mark.parametrize("cfgname,kind", [("basic", "u8"), ("gaussian_var100", "u8"), ("gmm3", "pl2_f32")])
def test_reset_of_one_stream_leaves_the_others(torch, cfgname, kind):
    S, T, H, W = 3, 3, 9, 40
    want = _want(cfgname, kind, S, T, H, W, 6, False, 1)
    fr = torch.as_tensor(np.array(_frames(kind, S, T, H, W, 6)), device="cuda:0")
    bg = _device_model(torch, cfgname, kind)
    try:
        bg.update(fr)
        bg.reset(1)
        for s in (0, 2):
            _same(bg.model(s).reshape(want[s][2].shape), want[s][2], "model of stream %d after reset(1)" % s)
        with pytest.raises(ValueError):
            bg.model(1)                                   # BHIP_ERR_INVALID: no model
        seg = bg.segment(torch.as_tensor(np.array(_segframes(kind, S, H, W, 6, False)), device="cuda:0"))
        unknown = CONFIGS[cfgname][1].get("unknownValue", 0) if cfgname != "basic" else 0
        assert (seg[1].cpu().numpy() == unknown).all()
        for s in (0, 2):
            _same(seg[s], want[s][3], "segment of stream %d after reset(1)" % s)
        # the reset stream starts again: its masks and model equal those of a fresh model fed the same frames
        masks = bg.update(fr, True)
        _same(masks[1], want[1][0], "masks of the reset stream")
        _same(bg.model(1).reshape(want[1][2].shape), want[1][2], "model of the reset stream")
    finally:
        bg.close()


def test_refused_calls_write_nothing(cabi, torch):
    L, _lib, ctx = cabi
    INV, UNS = _lib.BHIP_ERR_INVALID, _lib.BHIP_ERR_UNSUPPORTED
    G, P, I = _lib.BHIP_IMAGE_GRAY, _lib.BHIP_IMAGE_PLANAR, _lib.BHIP_IMAGE_INTERLEAVED
    h = C.c_void_p()

    def gmm(**kw):
        cfg = _lib.BgGmmCfg()
        L.bhip_bg_gmm_cfg_default(C.byref(cfg))
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    def basic(**kw):
        cfg = _lib.BgBasicCfg()
        L.bhip_bg_basic_cfg_default(C.byref(cfg))
        cfg.threshold = 5
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    def gaussian(**kw):
        cfg = _lib.BgGaussianCfg()
        L.bhip_bg_gaussian_cfg_default(C.byref(cfg))
        cfg.threshold = 5
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    refused = [
        (L.bhip_bg_create_gmm, gmm(learningPeriod=0), G, 0, INV), (L.bhip_bg_create_gmm, gmm(learningPeriod=-1), G, 0, INV),
        (L.bhip_bg_create_gmm, gmm(numberOfGaussian=0), G, 0, INV), (L.bhip_bg_create_gmm, gmm(numberOfGaussian=256), G, 0, INV),
        (L.bhip_bg_create_gmm, gmm(decayCoefient=-0.1), G, 0, INV), (L.bhip_bg_create_gmm, gmm(initialVariance=0), G, 0, INV),
        (L.bhip_bg_create_gmm, gmm(numberOfGaussian=9), G, 0, UNS), (L.bhip_bg_create_gmm, gmm(numberOfGaussian=255), G, 0, UNS),
        (L.bhip_bg_create_gmm, gmm(), P, 5, UNS), (L.bhip_bg_create_gmm, gmm(), I, 3, UNS), (L.bhip_bg_create_gmm, gmm(), P, 0, INV),
        (L.bhip_bg_create_basic, basic(learnRate=-0.1), G, 0, INV), (L.bhip_bg_create_basic, basic(learnRate=1.5), G, 0, INV),
        (L.bhip_bg_create_basic, basic(threshold=0), G, 0, INV), (L.bhip_bg_create_basic, basic(), I, 3, UNS), (L.bhip_bg_create_basic, basic(), P, 5, UNS),
        (L.bhip_bg_create_gaussian, gaussian(initialVariance=0), G, 0, INV), (L.bhip_bg_create_gaussian, gaussian(initialVariance=-1), G, 0, INV),
        (L.bhip_bg_create_gaussian, gaussian(minimumDifference=-1), G, 0, INV), (L.bhip_bg_create_gaussian, gaussian(threshold=-1), G, 0, INV),
        (L.bhip_bg_create_gaussian, gaussian(learnRate=2), G, 0, INV), (L.bhip_bg_create_gaussian, gaussian(), I, 3, UNS),
    ]
    for fn, cfg, family, bands, code in refused:
        h.value = 12345
        assert fn(ctx._h, C.byref(cfg), family, _lib.BHIP_PIXEL_U8, bands, 40, 9, 1, C.byref(h)) == code, (fn.__name__, family, bands, ctx.lastError())
        assert not h.value
    assert L.bhip_bg_create_basic(ctx._h, None, G, _lib.BHIP_PIXEL_U8, 0, 40, 9, 1, C.byref(h)) == INV and not h.value
    assert L.bhip_bg_create_gmm(ctx._h, gmm(), G, _lib.BHIP_PIXEL_U8, 0, 0, 9, 1, C.byref(h)) == INV and not h.value
    assert L.bhip_bg_create_gmm(ctx._h, gmm(), G, 2, 0, 40, 9, 1, C.byref(h)) == UNS and not h.value

    # refused calls on a live model: shape / type mismatches.  Neither the mask nor the model changes
    W, H, S, T = 40, 9, 2, 2
    hh = _create(cabi, "gmm3", "u8", W, H, S)
    try:
        fr = torch.as_tensor(np.array(_frames("u8", S, T, H, W, 8)), device="cuda:0")
        masks = torch.full((S, T, H, W), 0xA5, dtype=torch.uint8, device="cuda:0")
        p, mp = C.c_void_p(fr.data_ptr()), C.c_void_p(masks.data_ptr())
        assert L.bhip_bg_update_dev_u8(hh, p, T * H * W, H * W, 0, W, T, mp, T * H * W, H * W, W) == 0
        ctx.synchronize()
        good = masks.clone()
        st, before = _fetch(cabi, hh, 0)
        assert st == 0
        masks.fill_(0xA5)
        torch.cuda.synchronize()
        ff = fr.to(torch.float32)
        assert L.bhip_bg_update_dev_f32(hh, C.c_void_p(ff.data_ptr()), T * H * W, H * W, 0, W, T, mp, T * H * W, H * W, W) == INV      # other pixel type
        assert L.bhip_bg_update_dev_u8(hh, p, T * H * W, H * W, 0, W - 1, T, mp, T * H * W, H * W, W) == INV                          # stride < width
        assert L.bhip_bg_update_dev_u8(hh, p, T * H * W, H * W, 0, W, T, mp, T * H * W, H * W, W - 1) == INV                          # mask stride < width
        assert L.bhip_bg_update_dev_u8(hh, p, T * H * W, H * W, 0, W, 0, mp, T * H * W, H * W, W) == INV                              # no frames
        assert L.bhip_bg_update_dev_u8(hh, None, T * H * W, H * W, 0, W, T, mp, T * H * W, H * W, W) == INV
        assert L.bhip_bg_segment_dev_u8(hh, p, T * H * W, 0, W, None, H * W, W) == INV                                               # segment needs a mask
        assert L.bhip_bg_segment_dev_f32(hh, C.c_void_p(ff.data_ptr()), T * H * W, 0, W, mp, H * W, W) == INV
        assert L.bhip_bg_set_threshold(hh, 3.0) == INV and L.bhip_bg_set_minimum_difference(hh, 3.0) == INV                          # not GMM's
        assert L.bhip_bg_set_unknown_value(hh, 256) == INV and L.bhip_bg_set_unknown_value(hh, -1) == INV
        assert L.bhip_bg_reset(hh, S) == INV
        assert _fetch(cabi, hh, S)[0] == INV and _fetch(cabi, hh, -1)[0] == INV
        ctx.synchronize()
        assert bool((masks == 0xA5).all()), "a refused call wrote into the mask"
        st, after = _fetch(cabi, hh, 0)
        _same(after, before, "model after refused calls")
        assert good.shape == masks.shape
    finally:
        assert L.bhip_bg_destroy(hh) == 0


def test_lifetime_context_first_and_double_destroy():
    """as tests/test_handle_lifetime.py for the other handles: the context destroyed before the model leaves an inert shell, a destroyed or
    unknown pointer is refused"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = """
import ctypes as C, numpy as np
from boofcv_amd import _lib
L = _lib.load()
c = C.c_void_p(); g = C.c_void_p()
assert L.bhip_ctx_create(0, C.byref(c)) == 0
assert L.bhip_bg_create_gmm(c, None, 0, 0, 0, 40, 9, 1, C.byref(g)) == 0
fr = np.full((9, 40), 7, np.uint8)
p = fr.ctypes.data_as(C.POINTER(C.c_uint8))
assert L.bhip_bg_update_u8(g, p, 0, 0, 0, 0, 40, 1, None, 0, 0, 0, 0) == 0
assert L.bhip_ctx_destroy(c) == 0
assert L.bhip_bg_update_u8(g, p, 0, 0, 0, 0, 40, 1, None, 0, 0, 0, 0) == _lib.BHIP_ERR_INVALID
assert L.bhip_bg_reset(g, -1) == _lib.BHIP_ERR_INVALID
assert L.bhip_bg_destroy(g) == 0
assert L.bhip_bg_destroy(g) == _lib.BHIP_ERR_INVALID
assert L.bhip_bg_destroy(None) == 0
junk = C.create_string_buffer(4096)
assert L.bhip_bg_destroy(C.c_void_p(C.addressof(junk))) == _lib.BHIP_ERR_INVALID
assert L.bhip_bg_create_gmm(c, None, 0, 0, 0, 40, 9, 1, C.byref(g)) == _lib.BHIP_ERR_INVALID and not g.value
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"


# ---- the host classes ----
def _img(api, a):
    a = np.asarray(a)
    cls = api.GrayU8 if a.dtype == np.uint8 else api.GrayF32
    if a.ndim == 2:
        return cls.wrap(a)
    return api.Planar.wrap([cls.wrap(b) for b in a])


@pytest.mark.parametrize("cfgname,kind", [("basic", "u8"), ("basic", "pl3_f32"), ("gaussian_var100", "f32"), ("gaussian_min5", "pl3_u8"), ("gmm3", "u8"),
                                          ("gmm2", "pl2_f32")])
def test_host_classes(cfgname, kind):
    """FactoryBackgroundModel.stationary*: update with and without a mask, segment before any update (unknown value 2), the stale unknown value
    of the GMM, reset, and a frame of another width"""
    from boofcv_amd import api
    alg, c = _api_config(cfgname)
    dtype, bands = KINDS[kind]
    band = api.GrayU8 if dtype == np.uint8 else api.GrayF32
    imageType = api.PlanarType(bands, band) if bands else band
    bg = getattr(api.FactoryBackgroundModel, {"basic": "stationaryBasic", "gaussian": "stationaryGaussian", "gmm": "stationaryGmm"}[alg])(c, imageType)
    ref = _ref_model(cfgname, bands)
    try:
        H, W, T = 9, 40, 4
        fr = _frames(kind, 1, T, H, W, 9)[0]
        bg.setUnknownValue(2)
        ref.setUnknownValue(2)
        out = api.GrayU8(W, H)
        bg.segment(_img(api, fr[0]), out)                 # segmentBeforeUpdateBackGround
        _same(out.array(), ref.segment(fr[0]), "segment before update")
        for t in range(T):
            if t % 2 == 0:
                m = api.GrayU8(W, H)
                m.array()[...] = 0xA5
                bg.updateBackground(_img(api, fr[t]), m)
                _same(m.array(), ref.updateBackground(fr[t], True), "host class mask of frame %d" % t)
            else:
                bg.updateBackground(_img(api, fr[t]))
                ref.updateBackground(fr[t])
            bg.segment(_img(api, fr[0]), out)
            _same(out.array(), ref.segment(fr[0]), "host class segment after frame %d" % t)
        if alg == "basic":
            b = bg.getBackground()
            got = b.array()[None] if bands == 0 else np.stack([x.array() for x in b.bands])
            _same(got, ref.state(), "getBackground")
        # a narrower frame re-initialises Basic and GMM (the GMM's first mask shows the unknown value that segment() installed); Gaussian, whose
        # "not initialised" is width 1, throws
        fr2 = _frames(kind, 1, 2, H, W - 7, 10)[0]
        m = api.GrayU8(W - 7, H)
        if alg == "gaussian":
            with pytest.raises(ValueError):
                ref.updateBackground(fr2[0], True)
            with pytest.raises(api.IllegalArgumentException):
                bg.updateBackground(_img(api, fr2[0]), m)
        else:
            bg.updateBackground(_img(api, fr2[0]), m)
            _same(m.array(), ref.updateBackground(fr2[0], True), "mask after a change of width")
            if alg == "gmm":
                assert (m.array() == 2).all()
        bg.reset()
        ref.reset()
        out2 = api.GrayU8(W - 7, H)
        bg.segment(_img(api, fr2[1]), out2)
        _same(out2.array(), ref.segment(fr2[1]), "segment after reset")
        bg.updateBackground(_img(api, fr2[1]))
        ref.updateBackground(fr2[1])
        bg.segment(_img(api, fr2[0]), out2)
        _same(out2.array(), ref.segment(fr2[0]), "segment after reset and update")
    finally:
        bg.close()
