"""GPU: dense KLT optical flow (FactoryDenseOpticalFlow.flowKlt), bit for bit against tests/flow_ref.py, through the device-batched API
(device.py), the host-buffer API (api.py) and the C ABI.  Flows are compared as bit patterns, NaN as NaN; the per-pixel track records field
by field.

The lane-per-pixel track kernel (radius 1..3) gives a wave 64 consecutive pixels of a row: 70 x 23 is a full and a partial group, 129 x 9 three
groups, 64 x 16 exactly one; radius 4 and 6 run the wave-per-pixel kernel, which the main case also runs at radius 3 (form = WAVE).  The
reduce kernel's tile is 32 x 8 slots: every shape here has more than one tile, none a whole number of them but 64 x 16."""
import ctypes as C
import functools

import numpy as np
import pytest

import flow_ref as fr
import klt_ref as kr
import view_layouts as vl

pytestmark = pytest.mark.gpu

AUTO, LANE, WAVE = 0, 1, 2


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


@functools.lru_cache(maxsize=None)
def _scene(W, H, u8, seed=5):
    """a smooth texture moved by a sub-pixel shift and a small rotation; a flat patch (tracks fail to start) and a patch only the second frame has"""
    src, dst = fr.scene(W, H, seed, flat=(6, 3, min(16, W // 3), min(14, H - 6)), occluder=(W // 2, H // 3, min(12, W // 4), min(8, H // 3)))
    if u8:
        src, dst = np.rint(src).astype(np.uint8), np.rint(dst).astype(np.uint8)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


@functools.lru_cache(maxsize=None)
def _reference(orc, W, H, scales, radius, u8, cfg_items, seed=5):
    """(flow [H, W, 2], records) of flow_ref, computed once per case and shared by the tests that need it"""
    src, dst = _scene(W, H, u8, seed)
    flow, rec = fr.dense_flow_klt(orc, src, dst, scales, radius, kr.KltConfig(**dict(cfg_items)), u8)
    flow.setflags(write=False)
    return flow, rec


def _pklt(api, scales, cfg_items):
    cfg = api.PkltConfig(pyramidScaling=scales)
    for k, v in cfg_items:
        setattr(cfg.config, k, v)
    return cfg


def _tracks(t):
    """the int32 [.., 4] records as (fault, error, dx, dy)"""
    a = t.cpu().numpy()
    return a[..., 0], a[..., 1].view(np.float32), a[..., 2].view(np.float32), a[..., 3].view(np.float32)


def _check(flow, tracks, want_flow, rec, what):
    assert fr.same_bits(flow, want_flow), what
    invalid = np.isnan(want_flow[:, :, 0])
    assert not flow[invalid, 1].any(), what + ": y of an invalid pixel is 0"
    if tracks is not None:
        fault, error, dx, dy = tracks
        assert np.array_equal(fault, rec["fault"]), what
        for name, got in (("error", error), ("dx", dx), ("dy", dy)):
            assert fr.same_bits(got, rec[name]), what + ": " + name


# W, H, scales, radius, u8, KltConfig fields that differ from the defaults, form
CASES = [
    (70, 23, (1, 2), 3, False, (), AUTO),                                  # the main case: a full and a partial 64-lane group
    (70, 23, (1, 2), 3, False, (), WAVE),                                  # the same through the wave-per-pixel kernel
    (70, 23, (1, 2), 2, True, (), AUTO),
    (129, 9, (1, 2), 3, False, (), AUTO),                                  # three groups; the top layer has no pixel whose template is inside
    (33, 17, (1, 2, 4), 1, False, (), AUTO),
    (33, 17, (1, 2), 3, True, (), AUTO),
    (64, 16, (1,), 2, False, (), AUTO),                                    # exactly one group per row, one layer
    (64, 16, (1,), 1, True, (), AUTO),
    (20, 25, (1, 2, 4), 3, False, (), AUTO),                               # the top layer is smaller than a radius-3 template
    (33, 17, (1, 2), 4, False, (), AUTO),                                  # generic form
    (33, 17, (1, 2), 6, True, (), AUTO),
    (33, 17, (1, 2, 4), 2, False, (), WAVE),
    (70, 23, (1, 2), 2, False, (("maxIterations", 1),), AUTO),
    (70, 23, (1, 2), 3, False, (("maxPerPixelError", 4.0),), AUTO),        # LARGE_ERROR everywhere the match is not close
    (70, 23, (1, 2), 2, True, (("maxIterations", 1), ("maxPerPixelError", 6.0)), WAVE),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-s%s-r%d-%s-%s-%s" % (c[0], c[1], "".join(map(str, c[2])), c[3], "u8" if c[4] else "f32",
                                                                                 "_".join("%s%s" % kv for kv in c[5]) or "default", ("auto", "lane", "wave")[c[6]]))
def test_flow_and_tracks_match_the_reference(dev, api, orc, case):
    ops, torch = dev
    W, H, scales, radius, u8, cfg_items, form = case
    src, dst = _scene(W, H, u8)
    want, rec = _reference(orc, W, H, scales, radius, u8, cfg_items)
    if case == CASES[0]:
        # the class condition of the main case: every way a slot can get its value occurs often enough to be tested
        seen = np.bincount(fr.classify(rec, radius).reshape(-1), minlength=5)
        assert (seen[[fr.OWN, fr.LATER, fr.EARLIER, fr.INVALID]] >= 20).all(), dict(zip(fr.CLASS_NAMES, seen))
    if cfg_items and cfg_items[-1][0] == "maxPerPixelError":
        assert (rec["fault"] == fr.LARGE_ERROR).sum() >= 20
    flow, tracks = ops.denseFlowKlt(torch.from_numpy(src.copy())[None].cuda(), torch.from_numpy(dst.copy())[None].cuda(), _pklt(api, scales, cfg_items), radius,
                                    tracks=True, form=form)
    _check(flow[0].cpu().numpy(), [t[0] for t in _tracks(tracks)], want, rec, str(case))
    pixels, iterations = ops.denseFlowStats()
    assert pixels == W * H and iterations == int(rec["iterations"].sum())


BATCH = (70, 23, (1, 2), 2, ())


@pytest.fixture(scope="module")
def batch(orc):
    W, H, scales, radius, cfg_items = BATCH
    pairs = [_scene(W, H, False, seed) for seed in (5, 6, 7)]
    refs = [_reference(orc, W, H, scales, radius, False, cfg_items, seed) for seed in (5, 6, 7)]
    assert not fr.same_bits(refs[0][0], refs[1][0])
    return pairs, refs


@pytest.mark.parametrize("layout", vl.LAYOUTS)
def test_batch_of_three_pairs_on_strided_views(dev, api, batch, layout):
    """inputs as views at odd element offsets, the output in every layout of view_layouts with its guard bands intact"""
    ops, torch = dev
    W, H, scales, radius, cfg_items = BATCH
    pairs, refs = batch
    _, prev = vl.make_view("odd", 3, H, W, torch.float32, "cuda")
    _, curr = vl.make_view("pad4_x1", 3, H, W, torch.float32, "cuda", shift=3)
    prev.copy_(torch.from_numpy(np.stack([p[0] for p in pairs])))
    curr.copy_(torch.from_numpy(np.stack([p[1] for p in pairs])))
    parent, rows = vl.make_view(layout, 3, H, 2 * W, torch.float32, "cuda")   # a row of the flow is 2 W floats
    out = torch.as_strided(parent, (3, H, W, 2), (rows.stride(0), rows.stride(1), 2, 1), rows.storage_offset())
    before = vl.snapshot(parent)
    got = ops.denseFlowKlt(prev, curr, _pklt(api, scales, cfg_items), radius, out=out)
    assert got is out
    vl.assert_only_view_written(parent, rows, before, layout)
    for b in range(3):
        _check(out[b].cpu().numpy(), None, refs[b][0], refs[b][1], "%s pair %d" % (layout, b))


def _sub(api, a, u8, lead, pad):
    """the array as a sub-image: odd startIndex, stride > width"""
    H, W = a.shape
    stride = W + pad
    data = np.full(lead + stride * H + 5, 99, a.dtype)
    data[lead:lead + stride * H].reshape(H, stride)[:, :W] = a
    return (api.GrayU8 if u8 else api.GrayF32)(W, H, data, lead, stride)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_host_entry_on_sub_images_and_a_second_size_on_the_same_object(api, orc, u8):
    """DenseOpticalFlow.process == the device entry == the reference; y of invalid pixels keeps what the caller's flow held"""
    it = api.GrayU8 if u8 else api.GrayF32
    alg = api.FactoryDenseOpticalFlow.flowKlt(api.PkltConfig(pyramidScaling=(1, 2)), 2, it, None)
    for W, H in ((70, 23), (33, 17)):
        src, dst = _scene(W, H, u8)
        want, rec = _reference(orc, W, H, (1, 2), 2, u8, ())
        flow = api.ImageFlow(W, H)
        flow.data[:, :, 1] = 7.5
        alg.process(_sub(api, src, u8, 3, 5), _sub(api, dst, u8, 7, 1), flow)
        kept = want.copy()
        kept[np.isnan(want[:, :, 0]), 1] = 7.5
        assert fr.same_bits(flow.data, kept), (W, H)
        assert np.isnan(want[:, :, 0]).sum() >= 10   # a property of the scene, not of the library: the kept-y rule has pixels to apply to
        fresh = api.ImageFlow(W, H)
        alg.process(it.wrap(src), it.wrap(dst), fresh)
        assert fr.same_bits(fresh.data, want), (W, H)


# what is refused: (status class, radius, scales, KltConfig fields, form)
REFUSED = [
    ("invalid", 0, (1, 2), (), AUTO),
    ("invalid", -1, (1, 2), (), AUTO),
    ("invalid", 2, (), (), AUTO),
    ("invalid", 2, (2, 4), (), AUTO),
    ("invalid", 2, (1, 4, 2), (), AUTO),
    ("invalid", 2, (1, 2, 3), (), AUTO),
    ("invalid", 2, (1, 2), (), 3),
    ("unsupported", 8, (1, 2), (), AUTO),
    ("unsupported", 2, (1,) * 9, (), AUTO),
    ("unsupported", 2, (1, 2), (("maxIterations", 0),), AUTO),
    ("unsupported", 4, (1, 2), (), LANE),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "%s-r%d-s%s-%s-form%d" % (c[0], c[1], "".join(map(str, c[2])) or "none", "_".join("%s%s" % kv for kv in c[3]) or "default", c[4]))
def test_refused_calls_write_nothing(dev, api, case):
    from boofcv_amd import _lib
    ops, torch = dev
    kind, radius, scales, cfg_items, form = case
    W, H = 33, 17
    src, dst = _scene(W, H, False)
    err = api.IllegalArgumentException if kind == "invalid" else RuntimeError
    status = _lib.BHIP_ERR_INVALID if kind == "invalid" else _lib.BHIP_ERR_UNSUPPORTED
    cfg = _pklt(api, scales, cfg_items)
    # the device entry
    parent, rows = vl.make_view("odd", 1, H, 2 * W, torch.float32, "cuda")
    out = torch.as_strided(parent, (1, H, W, 2), (rows.stride(0), rows.stride(1), 2, 1), rows.storage_offset())
    tracks = torch.full((1, H, W, 4), vl.SENTINEL[torch.int32], dtype=torch.int32, device="cuda")
    before = vl.snapshot(parent)
    with pytest.raises(err) as e:
        ops.denseFlowKlt(torch.from_numpy(src.copy())[None].cuda(), torch.from_numpy(dst.copy())[None].cuda(), cfg, radius, out=out, tracks=tracks, form=form)
    assert (kind == "invalid") == isinstance(e.value, api.IllegalArgumentException)
    ops.ctx.synchronize()
    assert bool((vl.bits(parent) == before).all()) and bool((tracks == vl.SENTINEL[torch.int32]).all()), "a refused call wrote to its output"
    # the host entry (it has no form argument)
    if form == AUTO:
        flow = np.full((H, 2 * W + 3), -77.25, np.float32)
        sc = (C.c_int * max(len(scales), 1))(*scales)
        st = _lib.load().bhip_flow_klt_f32(ops.ctx._h, C.byref(cfg.config._c()), radius, sc, len(scales), src.ctypes.data_as(_lib._fp), 0, W,
                                           dst.ctypes.data_as(_lib._fp), 0, W, W, H, flow.ctypes.data_as(_lib._fp), 1, 2 * W + 3)
        assert st == status
        assert (flow == -77.25).all(), "a refused call wrote to its output"
    # sizes and strides
    for w, h, b, fs in ((0, H, 1, 2 * W), (W, -1, 1, 2 * W), (W, H, 0, 2 * W), (W, H, 1, 2 * W - 1)):
        st = _lib.load().bhip_flow_klt_dev_f32(ops.ctx._h, None, 2, (C.c_int * 2)(1, 2), 2, C.c_void_p(out.data_ptr()), W * H, W, C.c_void_p(out.data_ptr()), W * H, W,
                                               w, h, b, C.c_void_p(out.data_ptr()), rows.stride(0), fs, None, AUTO)
        assert st == _lib.BHIP_ERR_INVALID
    ops.ctx.synchronize()
    assert bool((vl.bits(parent) == before).all())
