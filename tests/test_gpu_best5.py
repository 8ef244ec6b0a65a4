"""GPU: five-region block-matching stereo on GrayU8 pairs (FactoryStereoDisparity.blockMatchBest5, errorType = SAD; GrayU8 or sub-pixel GrayF32
disparity), bit for bit against tests/best5_ref.py, through the device-batched API (device.py), the host-buffer mirror (best5.py) and the C ABI.
Every comparison is exact; GrayF32 disparities are compared as bit patterns.

The kernel's tile is TILE_W = 32 selector columns x TILE_H = 16 output rows per workgroup, and a range above RANGE_SPLIT = 128 runs the wide-slab
instantiation (DISP5_TW, DISP5_TH and RC in boofcv_amd/csrc/disparity.hip); tests/best5_cases.py holds the cases, those at the tile's edges among
them, and tests/test_best5_reference.py shows on the CPU that they tell the rule from its neighbours."""
import ctypes as C

import numpy as np
import pytest

import best5_cases as bc
import disparity_ref as dr
import view_layouts as vl

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = bc.TILE_W, bc.TILE_H


@pytest.fixture(scope="module")
def b():
    import boofcv_amd
    return boofcv_amd


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cfg(b, minD, rng, rx, ry, mpe, rtol, tex, subpixel=True):
    return b.ConfigDisparityBMBest5(minDisparity=minD, rangeDisparity=rng, regionRadiusX=rx, regionRadiusY=ry, maxPerPixelError=mpe, validateRtoL=rtol,
                                    texture=tex, subpixel=subpixel)


def _dev_run(dev, b, left, right, params, subpixel, out=None):
    ops, torch = dev
    lt = torch.as_tensor(np.array(left), device=ops.device)
    rt = torch.as_tensor(np.array(right), device=ops.device)
    if lt.dim() == 2:
        lt, rt = lt.unsqueeze(0), rt.unsqueeze(0)
    got = ops.disparityBM5(lt, rt, _cfg(b, *params), subpixel=subpixel, out=out)
    ops.ctx.synchronize()
    return got


def _same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = _bits(got) != _bits(want)
    if bad.any():
        ys, xs = np.nonzero(bad)[-2:]
        raise AssertionError("%s: %d pixels differ; first (x, y) %s: got %r want %r" % (what, int(bad.sum()), (int(xs[0]), int(ys[0])),
                                                                                  got[bad][0], want[bad][0]))


@pytest.mark.parametrize("case", bc.SAD_CASES, ids=bc.case_id)
def test_best5_cases(dev, b, case):
    W, H, minD, rng, rx, ry, mpe, rtol, tex, outputs, binary = case
    left, right = bc.scene(W, H, minD, rng, binary=binary)
    for output in outputs:
        sub = output == "f32"
        want, _ = bc.want(W, H, minD, rng, rx, ry, mpe, rtol, tex, sub, binary=binary)
        got = _dev_run(dev, b, left, right, (minD, rng, rx, ry, mpe, rtol, tex), sub)
        _same(got[0], want, "%s %s" % (bc.case_id(case), output))


def test_shapes_without_a_selected_pixel_are_filled(dev, b):
    """no selector column, and rh <= H < 4*ry + 1: BHIP_OK and the whole view holds rangeDisparity"""
    for W, H, minD, rng, rx, ry in ((20, 20, 5, 7, 4, 1), (40, 9, 0, 10, 1, 3)):
        left, right = bc.scene(W, H, minD, rng)
        for sub in (True, False):
            got = _dev_run(dev, b, left, right, (minD, rng, rx, ry, 0, 1, .15), sub)[0].cpu().numpy()
            assert (got == rng).all()


@pytest.mark.parametrize("off", ["maxPerPixelError", "validateRtoL", "texture", "all"])
@pytest.mark.parametrize("sub", [True, False], ids=["f32", "u8"])
def test_each_check_disabled_on_its_own(dev, b, off, sub):
    W, H, minD, rng, rx, ry = 131, 23, 0, 100, 3, 2
    mpe, rtol, tex = 20, 1, .15      # 20 per pixel of three regions: each of the three rejections holds at least 10 reference pixels
    if off in ("maxPerPixelError", "all"):
        mpe = 0
    if off in ("validateRtoL", "all"):
        rtol = -1
    if off in ("texture", "all"):
        tex = 0.0
    left, right = bc.scene(W, H, minD, rng)
    want, cls = bc.want(W, H, minD, rng, rx, ry, mpe, rtol, tex, sub)
    counts = dr.class_counts(cls)
    disabled = {"maxPerPixelError": [dr.REJECT_ERROR], "validateRtoL": [dr.REJECT_RTOL], "texture": [dr.REJECT_TEXTURE],
                "all": [dr.REJECT_ERROR, dr.REJECT_RTOL, dr.REJECT_TEXTURE]}[off]
    assert all(counts[k] == 0 for k in disabled)
    assert off == "all" or all(counts[k] >= 10 for k in (dr.REJECT_ERROR, dr.REJECT_RTOL, dr.REJECT_TEXTURE) if k not in disabled), counts
    _same(_dev_run(dev, b, left, right, (minD, rng, rx, ry, mpe, rtol, tex), sub)[0], want, off)


def test_batch_of_three_strided_pairs_at_odd_byte_offsets(dev, b):
    """three different pairs, rows W+3 bytes apart starting at byte offset 1, images a non-dense stride apart; the output dense"""
    ops, torch = dev
    W, H, minD, rng, rx, ry, mpe, rtol, tex = 131, 23, 0, 100, 3, 2, 30, 1, .15
    pitch, image = W + 3, (W + 3) * (H + 1) + 5
    parents = [torch.full((1 + 3 * image + 64,), 0xA5, dtype=torch.uint8, device=ops.device) for _ in range(2)]
    views = [torch.as_strided(p, (3, H, W), (image, pitch, 1), 1) for p in parents]
    assert views[0].data_ptr() % 2 == 1
    for k in range(3):
        left, right = bc.scene(W, H, minD, rng, seed=1 + k)
        views[0][k].copy_(torch.as_tensor(np.array(left), device=ops.device))
        views[1][k].copy_(torch.as_tensor(np.array(right), device=ops.device))
    torch.cuda.synchronize()
    for sub in (True, False):
        got = ops.disparityBM5(views[0], views[1], _cfg(b, minD, rng, rx, ry, mpe, rtol, tex), subpixel=sub)
        ops.ctx.synchronize()
        for k in range(3):
            _same(got[k], bc.want(W, H, minD, rng, rx, ry, mpe, rtol, tex, sub, seed=1 + k)[0], "pair %d" % k)


@pytest.mark.parametrize("layout", ["pad4", "pad4_x1", "odd"])
@pytest.mark.parametrize("sub", [True, False], ids=["f32", "u8"])
def test_output_windows_keep_their_guard_bands(dev, b, layout, sub):
    ops, torch = dev
    W, H, minD, rng, rx, ry, mpe, rtol, tex = 67, 25, 2, 30, 2, 1, 25, 1, .15
    B = 2
    lefts, rights = zip(*[bc.scene(W, H, minD, rng, seed=1 + k) for k in range(B)])
    parent, view = vl.make_view(layout, B, H, W, torch.float32 if sub else torch.uint8, ops.device)
    before = vl.snapshot(parent)
    torch.cuda.synchronize()
    _dev_run(dev, b, np.stack(lefts), np.stack(rights), (minD, rng, rx, ry, mpe, rtol, tex), sub, out=view)
    vl.assert_only_view_written(parent, view, before, layout)
    for k in range(B):
        _same(view[k], bc.want(W, H, minD, rng, rx, ry, mpe, rtol, tex, sub, seed=1 + k)[0], "%s pair %d" % (layout, k))


@pytest.mark.parametrize("sub", [True, False], ids=["f32", "u8"])
def test_host_mirror_equals_device_entry(dev, b, sub):
    """FactoryStereoDisparityBest5.blockMatchBest5(...).process on sub-images with an odd startIndex and stride > width"""
    W, H, minD, rng, rx, ry, mpe, rtol, tex = 131, 23, 0, 100, 3, 2, 30, 1, .15
    left, right = bc.scene(W, H, minD, rng)
    subs = []
    for img in (left, right):
        big = b.GrayU8(W + 5, H + 3)
        s = big.subimage(1, 2, 1 + W, 2 + H)
        s.array()[:, :] = img
        subs.append(s)
    alg = b.FactoryStereoDisparityBest5.blockMatchBest5(_cfg(b, minD, rng, rx, ry, mpe, rtol, tex, subpixel=sub), b.GrayU8, b.GrayF32 if sub else b.GrayU8)
    alg.process(*subs)
    host = alg.getDisparity().array().copy()
    _same(host, bc.want(W, H, minD, rng, rx, ry, mpe, rtol, tex, sub)[0], "host")
    _same(_dev_run(dev, b, left, right, (minD, rng, rx, ry, mpe, rtol, tex), sub)[0], host, "device")
    assert (alg.getBorderX(), alg.getBorderY(), alg.getMinDisparity(), alg.getRangeDisparity(), alg.getInvalidValue()) == (2 * rx, 2 * ry, minD, rng, rng)
    # a second pair on the same object: the whole image is written again
    left2, right2 = bc.scene(W, H, minD, rng, seed=2)
    alg.process(b.GrayU8.wrap(left2), b.GrayU8.wrap(right2))
    _same(alg.getDisparity().array().copy(), bc.want(W, H, minD, rng, rx, ry, mpe, rtol, tex, sub, seed=2)[0], "second pair")
    with pytest.raises(RuntimeError, match="The maximum disparity is too large for this image size: max size 34"):
        alg.process(b.GrayU8(40, H), b.GrayU8(40, H))


def test_c_abi_directly_with_a_null_config(dev, b):
    """bhip_disparity_bm5_dev_u8_f32 and the host entry bhip_disparity_bm5_u8_f32 through ctypes; cfg = NULL is the reference default"""
    ops, torch = dev
    from boofcv_amd import _lib
    W, H = 131, 29
    left, right = bc.scene(W, H, 0, 100)
    want = bc.want(W, H, 0, 100, 3, 3, 0, 1, .15, True)[0]
    lt = torch.as_tensor(np.array(left), device=ops.device)
    rt = torch.as_tensor(np.array(right), device=ops.device)
    out = torch.full((H, W), -7.0, dtype=torch.float32, device=ops.device)
    torch.cuda.synchronize()
    st = ops.L.bhip_disparity_bm5_dev_u8_f32(ops.ctx._h, None, C.c_void_p(lt.data_ptr()), H * W, W, C.c_void_p(rt.data_ptr()), H * W, W, W, H, 1,
                                             C.c_void_p(out.data_ptr()), H * W, W)
    ops.ctx.synchronize()
    assert st == 0
    _same(out, want, "device entry")
    hl, hr = np.ascontiguousarray(left).reshape(-1), np.ascontiguousarray(right).reshape(-1)
    hout = np.full(H * W, -7.0, np.float32)
    st = ops.L.bhip_disparity_bm5_u8_f32(ops.ctx._h, None, hl.ctypes.data_as(_lib._u8p), 0, W, hr.ctypes.data_as(_lib._u8p), 0, W, W, H,
                                         hout.ctypes.data_as(_lib._fp), 0, W)
    assert st == 0
    _same(hout.reshape(H, W), want, "host entry")


# (W, H, minD, range, rx, ry, subpixel, status): BHIP_ERR_INVALID = -1, BHIP_ERR_UNSUPPORTED = -2
REFUSED = [
    (60, 20, -1, 10, 2, 2, True, -1),
    (60, 20, 0, 0, 2, 2, True, -1),
    (60, 20, 0, 10, -1, 2, True, -1),
    (60, 20, 0, 10, 2, -1, True, -1),
    (60, 20, 0, 57, 2, 2, True, -1),       # maxD > W - 2*rx = 56
    (60, 20, 50, 7, 2, 2, True, -1),
    (60, 4, 0, 10, 2, 2, True, -1),        # H < rh
    (300, 9, 0, 254, 2, 1, False, -1),     # inv = 255 > 254 in a GrayU8 disparity
    (300, 20, 0, 10, 8, 2, True, -2),
    (300, 20, 0, 10, 2, 8, True, -2),
    (300, 9, 0, 257, 2, 1, True, -2),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "%dx%d_min%d_range%d_r%dx%d_%s_%d" % c)
def test_refused_calls_write_nothing(dev, b, case):
    ops, torch = dev
    from boofcv_amd import _lib
    W, H, minD, rng, rx, ry, sub, status = case
    dt = torch.float32 if sub else torch.uint8
    left = torch.zeros((1, H, W), dtype=torch.uint8, device=ops.device)
    right = torch.zeros((1, H, W), dtype=torch.uint8, device=ops.device)
    parent, view = vl.make_view("dense", 1, H, W, dt, ops.device)
    before = vl.snapshot(parent)
    torch.cuda.synchronize()
    cfg = _lib.DisparityBmCfg(minD, rng, rx, ry, 0.0, 1, 0.15)
    fn = ops.L.bhip_disparity_bm5_dev_u8_f32 if sub else ops.L.bhip_disparity_bm5_dev_u8_u8
    st = fn(ops.ctx._h, C.byref(cfg), C.c_void_p(left.data_ptr()), H * W, W, C.c_void_p(right.data_ptr()), H * W, W, W, H, 1,
            C.c_void_p(view.data_ptr()), H * W, W)
    ops.ctx.synchronize()
    assert st == status
    assert bool((vl.bits(parent) == before).all()), "a refused call wrote to its output"
    # the host entry answers the same and leaves the caller's array alone
    hl, hr = np.zeros(H * W, np.uint8), np.zeros(H * W, np.uint8)
    out = np.full(H * W, 7, np.float32 if sub else np.uint8)
    hfn = ops.L.bhip_disparity_bm5_u8_f32 if sub else ops.L.bhip_disparity_bm5_u8_u8
    st = hfn(ops.ctx._h, C.byref(cfg), hl.ctypes.data_as(_lib._u8p), 0, W, hr.ctypes.data_as(_lib._u8p), 0, W, W, H,
             out.ctypes.data_as(_lib._fp if sub else _lib._u8p), 0, W)
    assert st == status and (out == 7).all()
