"""GPU: Horn-Schunck dense optical flow (FactoryDenseOpticalFlow.hornSchunck), bit for bit against tests/hornschunck_ref.py, through the
device-batched API (device.py), the host mirror (boofcv_amd/hornschunck.py) and the C ABI.  Flows and derivatives are compared as bit patterns,
NaN as NaN.

The iteration kernel gives a workgroup a TW x TH = 112 x 48 tile and fuses up to K = BHIP_FLOW_HS_MAX_FUSED = 8 iterations on it, with a halo of
as many pixels as it fuses; a call of N iterations is N // depth full launches and a remainder, alternating between two scratch flows.
  130 x 61    the main case: two tiles each way, the second partial on both axes; N = 2K+3 = 19 is two full launches and a remainder of 3 at depth
              K, and a remainder at depth 2 as well; the scene is a texture under sub-pixel motion with a flat patch (dx = dy = dt = 0 there)
  112 x 48    exactly one tile: no halo on any side       224 x 96    exactly 2 x 2 tiles: every tile has a halo on two sides only
  1x1 .. 2x2  every neighbour is a clamped one            5 x 60, 120 x 5   narrower / lower than K and more than one tile the other way: the
              halo exceeds the image on both sides and clamping does all the work
  N = 0, 1, K, K+1   no iteration at all (the zero flow is still written), one launch below / at the depth, a launch of one iteration after a full one
  20 x 30     the reference's known-answer rectangle at alpha = 0.2, one iteration
  alpha = 0   0/0 on the flat patch: the NaNs spread one pixel per iteration, across launches at depth 1 and inside one launch at depth K"""
import ctypes as C
import functools

import numpy as np
import pytest

import flow_ref as fr
import hornschunck_ref as hs
import view_layouts as vl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from boofcv_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


@pytest.fixture(scope="module")
def geometry(lib):
    TW, TH, K = lib.BHIP_FLOW_HS_TILE_WIDTH, lib.BHIP_FLOW_HS_TILE_HEIGHT, lib.BHIP_FLOW_HS_MAX_FUSED
    assert (TW, TH, K) == (112, 48, 8), "the shapes of this file were chosen for a 112 x 48 tile and K = 8"
    return TW, TH, K


@functools.lru_cache(maxsize=None)
def _scene(W, H, u8, seed=5):
    """a smooth texture moved by a sub-pixel shift and a small rotation, with a flat patch where the image is large enough for one"""
    flat = (W // 4, H // 4, max(W // 5, 3), max(H // 5, 3)) if W >= 12 and H >= 12 else None
    src, dst = fr.scene(W, H, seed, flat=flat)
    if u8:
        src, dst = np.rint(src).astype(np.uint8), np.rint(dst).astype(np.uint8)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


@functools.lru_cache(maxsize=None)
def _reference(W, H, u8, alpha, n, seed=5):
    """(flow [H, W, 2], derivatives [3, H, W] float32) of hornschunck_ref, computed once per case and shared by the tests that need it"""
    src, dst = _scene(W, H, u8, seed)
    flow, d = hs.horn_schunck(src, dst, alpha, n, u8)
    d = np.stack([np.asarray(p, np.float32) for p in d])
    flow.setflags(write=False)
    d.setflags(write=False)
    return flow, d


def _gpu(dev, src, dst, alpha, n, depth, derivs=None):
    ops, torch = dev
    return ops.denseFlowHornSchunck(torch.from_numpy(src.copy())[None].cuda(), torch.from_numpy(dst.copy())[None].cuda(), alpha, n, derivs=derivs, itersPerLaunch=depth)


MAIN = (130, 61)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_main_case_at_every_depth(dev, geometry, u8):
    """depth 0 (the library's choice) and forced 1, 2 and K all equal the reference, and so each other"""
    TW, TH, K = geometry
    W, H = MAIN
    assert TW < W < 2 * TW and TH < H < 2 * TH
    n = 2 * K + 3
    src, dst = _scene(W, H, u8)
    want, wantD = _reference(W, H, u8, 20.0, n)
    assert np.isfinite(want).all() and (np.abs(want) > 1e-3).mean() > 0.9   # a property of the scene: there is a flow to get wrong
    assert ((wantD[0] == 0) & (wantD[1] == 0) & (wantD[2] == 0)).sum() >= 20   # ... and a flat patch
    for depth in (0, 1, 2, K):
        flow, d = _gpu(dev, src, dst, 20.0, n, depth, derivs=True)
        assert fr.same_bits(flow[0].cpu().numpy(), want), "depth %d" % depth
        assert fr.same_bits(d[0].cpu().numpy(), wantD), "depth %d" % depth


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_iteration_counts_around_the_fusion_depth(dev, geometry, u8):
    TW, TH, K = geometry
    W, H = MAIN
    src, dst = _scene(W, H, u8)
    for n in (0, 1, K, K + 1):
        want, _ = _reference(W, H, u8, 20.0, n)
        for depth in (0, K):
            assert fr.same_bits(_gpu(dev, src, dst, 20.0, n, depth)[0].cpu().numpy(), want), (n, depth)
    assert not _reference(W, H, u8, 20.0, 0)[0].any()
    zero = _gpu(dev, src, dst, 20.0, -5, 0)[0].cpu().numpy()   # as the Java loop: no iteration, the flow is reset all the same
    assert zero.shape == (H, W, 2) and not zero.view(np.uint32).any()


def _shapes(TW, TH, K):
    return [(TW, TH), (2 * TW, 2 * TH), (1, 1), (1, 9), (9, 1), (2, 2), (K - 3, TH + 12), (TW + 8, K - 3)]


@pytest.mark.parametrize("index", range(8), ids=["one-tile", "2x2-tiles", "1x1", "1x9", "9x1", "2x2", "narrow", "low"])
def test_exact_tiles_and_degenerate_shapes(dev, geometry, index):
    TW, TH, K = geometry
    W, H = _shapes(TW, TH, K)[index]
    n = K + 3
    for u8 in (False, True):
        src, dst = _scene(W, H, u8)
        want, wantD = _reference(W, H, u8, 20.0, n)
        for depth in (1, K):
            flow, d = _gpu(dev, src, dst, 20.0, n, depth, derivs=True)
            assert fr.same_bits(flow[0].cpu().numpy(), want), (W, H, u8, depth)
            assert fr.same_bits(d[0].cpu().numpy(), wantD), (W, H, u8, depth)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_known_answer_rectangle(dev, u8):   # ChecksHornSchunck.process: alpha = 0.2f, one iteration
    dt = np.uint8 if u8 else np.float32
    image1, image2 = np.zeros((30, 20), dt), np.zeros((30, 20), dt)
    image1[:, 10:] = 100
    image2[:, 11:] = 100
    want, _ = hs.horn_schunck(image1, image2, 0.2, 1, u8)
    flow = _gpu(dev, image1, image2, 0.2, 1, 0)[0].cpu().numpy()
    assert fr.same_bits(flow, want)
    for y in range(29):
        assert flow[y, 9, 0] > 0.9 and flow[y, 10, 0] > 0.9 and abs(flow[y, 10, 1]) < 0.1 and abs(flow[y, 11, 1]) < 0.1


def test_alpha_zero_spreads_nan_as_the_reference_does(dev, geometry):
    TW, TH, K = geometry
    W, H = MAIN
    src, dst = _scene(W, H, False)
    want, _ = _reference(W, H, False, 0.0, 3)
    nan = np.isnan(want[:, :, 0])
    assert 30 < nan.sum() < W * H // 2
    for depth in (1, K):
        flow = _gpu(dev, src, dst, 0.0, 3, depth)[0].cpu().numpy()
        assert np.array_equal(np.isnan(flow), np.isnan(want)) and fr.same_bits(flow, want), depth


# ---------------------------------------------------------------------------------------------------------------- batches and views
@pytest.fixture(scope="module")
def batch(geometry):
    TW, TH, K = geometry
    W, H = MAIN
    pairs = [_scene(W, H, False, seed) for seed in (5, 6, 7)]
    refs = [_reference(W, H, False, 20.0, K + 2, seed) for seed in (5, 6, 7)]
    assert not fr.same_bits(refs[0][0], refs[1][0])
    return pairs, refs, K + 2


@pytest.mark.parametrize("layout", vl.LAYOUTS)
def test_batch_of_three_pairs_on_strided_views(dev, batch, layout):
    """inputs as views with different strides for source and destination, the flow in every layout of view_layouts with its guard bands intact"""
    ops, torch = dev
    W, H = MAIN
    pairs, refs, n = batch
    _, prev = vl.make_view("odd", 3, H, W, torch.float32, "cuda")
    _, curr = vl.make_view("pad4_x1", 3, H, W, torch.float32, "cuda", shift=3)
    assert prev.stride(1) != curr.stride(1)
    prev.copy_(torch.from_numpy(np.stack([p[0] for p in pairs])))
    curr.copy_(torch.from_numpy(np.stack([p[1] for p in pairs])))
    parent, rows = vl.make_view(layout, 3, H, 2 * W, torch.float32, "cuda")   # a row of the flow is 2 W floats
    out = torch.as_strided(parent, (3, H, W, 2), (rows.stride(0), rows.stride(1), 2, 1), rows.storage_offset())
    before = vl.snapshot(parent)
    got, d = ops.denseFlowHornSchunck(prev, curr, 20.0, n, out=out, derivs=True)
    assert got is out
    vl.assert_only_view_written(parent, rows, before, layout)
    for b in range(3):
        assert fr.same_bits(out[b].cpu().numpy(), refs[b][0]), "%s pair %d" % (layout, b)
        assert fr.same_bits(d[b].cpu().numpy(), refs[b][1]), "%s pair %d" % (layout, b)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_derivatives_output(dev, u8):
    """derivX, derivY, derivT exactly, the GrayS16 values of GrayU8 pairs as floats; derivY(w, h), which the reference never writes, is 0"""
    ops, torch = dev
    W, H = 37, 21
    src, dst = _scene(W, H, u8)
    _, wantD = _reference(W, H, u8, 20.0, 1)
    d = vl.sentinel_buffer(3 * H * W, torch.float32, "cuda").view(1, 3, H, W)
    flow, got = _gpu(dev, src, dst, 20.0, 1, 0, derivs=d)
    assert got is d
    got = got[0].cpu().numpy()
    assert fr.same_bits(got, wantD)
    assert got[1, H - 1, W - 1] == 0 and not got[0, :, W - 1].any() and not got[1, H - 1].any()
    assert np.abs(wantD).max() > 5
    if u8:
        assert np.array_equal(got, np.trunc(got))


# ---------------------------------------------------------------------------------------------------------------- the host mirror and the C ABI
def _sub(api, a, u8, lead, pad):
    """the array as a sub-image: odd startIndex, stride > width"""
    H, W = a.shape
    stride = W + pad
    data = np.full(lead + stride * H + 5, 99, a.dtype)
    data[lead:lead + stride * H].reshape(H, stride)[:, :W] = a
    return (api.GrayU8 if u8 else api.GrayF32)(W, H, data, lead, stride)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_host_mirror_on_sub_images_and_a_second_size_on_the_same_object(geometry, u8):
    """DenseOpticalFlowHornSchunck.process == the reference; what the caller's flow held is reset, as resetOutput says"""
    from boofcv_amd import api, hornschunck as m
    TW, TH, K = geometry
    it = api.GrayU8 if u8 else api.GrayF32
    n = K + 2
    alg = m.FactoryDenseOpticalFlowHornSchunck.hornSchunck(m.ConfigHornSchunck(20.0, n), it)
    for W, H in (MAIN, (37, 21)):
        src, dst = _scene(W, H, u8)
        want, _ = _reference(W, H, u8, 20.0, n)
        flow = api.ImageFlow(W, H)
        flow.data[...] = 7.5
        alg.process(_sub(api, src, u8, 3, 5), _sub(api, dst, u8, 7, 1), flow)
        assert fr.same_bits(flow.data, want), (W, H)
    alg.setNumIterations(1)
    flow = api.ImageFlow(37, 21)
    alg.process(it.wrap(_scene(37, 21, u8)[0]), it.wrap(_scene(37, 21, u8)[1]), flow)
    assert fr.same_bits(flow.data, _reference(37, 21, u8, 20.0, 1)[0])


def test_dev_entry_points_refuse_and_write_nothing(dev, lib, geometry):
    ops, torch = dev
    TW, TH, K = geometry
    L = lib.load()
    W, H = 37, 21
    src, dst = _scene(W, H, False)
    s, d = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dst.copy()).cuda()
    s8, d8 = torch.from_numpy(_scene(W, H, True)[0].copy()).cuda(), torch.from_numpy(_scene(W, H, True)[1].copy()).cuda()
    parent, rows = vl.make_view("odd", 1, H, 2 * W, torch.float32, "cuda")
    out = torch.as_strided(parent, (1, H, W, 2), (rows.stride(0), rows.stride(1), 2, 1), rows.storage_offset())
    deriv = vl.sentinel_buffer(3 * H * W, torch.float32, "cuda")
    before, beforeD = vl.snapshot(parent), vl.bits(deriv).clone()
    P = lambda t: C.c_void_p(t.data_ptr())
    fs = rows.stride(1)

    def call(fn=L.bhip_flow_hs_dev_f32, a=s, b=d, n=3, ss=W, ds=W, w=W, h=H, batch=1, flow=out, f=fs, depth=0):
        return fn(ops.ctx._h, 20.0, n, P(a), W * H, ss, P(b), W * H, ds, w, h, batch, P(flow) if flow is not None else None, rows.stride(0), f, P(deriv), depth)

    invalid = [dict(w=0), dict(h=-1), dict(batch=0), dict(f=2 * W - 1), dict(ss=W - 1), dict(ds=W - 1), dict(depth=-1), dict(depth=K + 1), dict(flow=None)]
    for kw in invalid:
        assert call(**kw) == lib.BHIP_ERR_INVALID, kw
        assert call(L.bhip_flow_hs_dev_u8, s8, d8, **kw) == lib.BHIP_ERR_INVALID, kw
    # limits: refused from the sizes alone, before any memory is touched or reserved
    for kw in (dict(batch=65536), dict(w=(1 << 20) + 1, h=1, ss=(1 << 20) + 1, ds=(1 << 20) + 1, f=(1 << 22)), dict(w=1 << 15, h=1 << 15, ss=1 << 15, ds=1 << 15, f=1 << 16)):
        assert call(**kw) == lib.BHIP_ERR_UNSUPPORTED, kw
        assert call(L.bhip_flow_hs_dev_u8, s8, d8, **kw) == lib.BHIP_ERR_UNSUPPORTED, kw
    # the host forms
    flow = np.full((H, 2 * W + 3), -77.25, np.float32)
    fp = flow.ctypes.data_as(lib._fp)
    sp, dp = src.ctypes.data_as(lib._fp), dst.ctypes.data_as(lib._fp)
    for args in ((sp, 0, W, dp, 0, W, 0, H, fp, 1, 2 * W + 3), (sp, 0, W, dp, 0, W, W, 0, fp, 1, 2 * W + 3), (sp, 0, W - 1, dp, 0, W, W, H, fp, 1, 2 * W + 3),
                 (sp, 0, W, dp, 0, W, W, H, fp, 1, 2 * W - 1), (sp, 0, W, dp, 0, W, W, H, None, 1, 2 * W + 3), (None, 0, W, dp, 0, W, W, H, fp, 1, 2 * W + 3)):
        assert L.bhip_flow_hs_f32(ops.ctx._h, 20.0, 3, *args) == lib.BHIP_ERR_INVALID, args[6:]
    assert L.bhip_flow_hs_f32(ops.ctx._h, 20.0, 3, sp, 0, 1 << 15, dp, 0, 1 << 15, 1 << 15, 1 << 15, fp, 1, 1 << 16) == lib.BHIP_ERR_UNSUPPORTED
    assert (flow == -77.25).all(), "a refused call wrote to its output"
    # the device mirror turns the two statuses into its two exceptions
    from boofcv_amd import api
    with pytest.raises(api.IllegalArgumentException):
        ops.denseFlowHornSchunck(s[None], d[None], out=out, itersPerLaunch=K + 1)
    with pytest.raises(api.IllegalArgumentException):
        ops.denseFlowHornSchunck(s[None], d[None, :, :-1])
    ops.ctx.synchronize()
    assert bool((vl.bits(parent) == before).all()) and bool((vl.bits(deriv) == beforeD).all()), "a refused call wrote to its output"
    # and the same arguments, valid, through the C entry directly: the strided flow and the derivatives of the reference
    assert call(n=K + 2, depth=2) == lib.BHIP_OK
    ops.ctx.synchronize()
    want, wantD = _reference(W, H, False, 20.0, K + 2)
    assert fr.same_bits(out[0].cpu().numpy(), want) and fr.same_bits(deriv.view(3, H, W).cpu().numpy(), wantD)
    vl.assert_only_view_written(parent, rows, before, "odd")
