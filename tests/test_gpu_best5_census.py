"""GPU: five-region block matching on census images (FactoryStereoDisparity.blockMatchBest5, errorType = CENSUS), bit for bit against
tests/best5_ref.py with census_ref's row score, for one variant per census word size (GrayU8, GrayS32, GrayS64) and the circle.  Every comparison
is exact; GrayF32 disparities are compared as bit patterns.

The 4-byte census words have their own band: ROWS_W32 - 4*regionRadiusY = 32 - 4*ry output rows per workgroup (DISP5_ROWS_W32 in
boofcv_amd/csrc/disparity.hip), four at ry = 7; BLOCK_3_3 runs the 1-byte geometry of SAD."""
import ctypes as C

import numpy as np
import pytest

import best5_cases as bc
import census_cases as cc
import disparity_ref as dr
import view_layouts as vl

pytestmark = pytest.mark.gpu

ROWS_W32 = bc.ROWS_W32


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


def _same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = _bits(got) != _bits(want)
    if bad.any():
        ys, xs = np.nonzero(bad)[-2:]
        raise AssertionError("%s: %d pixels differ; first (x, y) %s: got %r want %r" % (what, int(bad.sum()), (int(xs[0]), int(ys[0])),
                                                                                  got[bad][0], want[bad][0]))


def _cfg(b, params, subpixel=True):
    minD, rng, rx, ry, mpe, rtol, tex = params
    return b.ConfigDisparityBMBest5(minDisparity=minD, rangeDisparity=rng, regionRadiusX=rx, regionRadiusY=ry, maxPerPixelError=mpe, validateRtoL=rtol,
                                    texture=tex, subpixel=subpixel, errorType=b.DisparityError.CENSUS)


def _dev_run(dev, b, left, right, params, variant, subpixel, out=None):
    ops, torch = dev
    lt = torch.as_tensor(np.array(left), device=ops.device)
    rt = torch.as_tensor(np.array(right), device=ops.device)
    if lt.dim() == 2:
        lt, rt = lt.unsqueeze(0), rt.unsqueeze(0)
    got = ops.disparityBM5(lt, rt, _cfg(b, params), variant=b.CensusVariants[variant], subpixel=subpixel, out=out)
    ops.ctx.synchronize()
    return got


@pytest.mark.parametrize("variant", bc.CENSUS_VARIANTS)
@pytest.mark.parametrize("case", bc.CENSUS_CASES, ids=lambda c: c[0])
def test_best5_census_cases(dev, b, case, variant):
    name, W, H = case[:3]
    params = bc.census_params(case, variant)
    left, right = bc.scene(W, H, params[0], params[1])
    for sub in (True, False):
        want, cls = bc.want(W, H, *params, sub, variant=variant)
        assert (cls != dr.BORDER).sum() >= 100
        _same(_dev_run(dev, b, left, right, params, variant, sub)[0], want, "%s %s %s" % (name, variant, "f32" if sub else "u8"))


@pytest.mark.parametrize("variant", ["BLOCK_3_3", "BLOCK_5_5"])
def test_batch_of_strided_pairs_into_an_output_window(dev, b, variant):
    """three different pairs in strided input views at an odd byte offset, the output a window of a sentinel-filled parent"""
    ops, torch = dev
    case = bc.CENSUS_CASES[2]
    W, H = case[1:3]
    params = bc.census_params(case, variant)
    pitch, image = W + 3, (W + 3) * (H + 1) + 5
    parents = [torch.full((1 + 3 * image + 64,), 0xA5, dtype=torch.uint8, device=ops.device) for _ in range(2)]
    views = [torch.as_strided(p, (3, H, W), (image, pitch, 1), 1) for p in parents]
    for k in range(3):
        left, right = bc.scene(W, H, params[0], params[1], seed=1 + k)
        views[0][k].copy_(torch.as_tensor(np.array(left), device=ops.device))
        views[1][k].copy_(torch.as_tensor(np.array(right), device=ops.device))
    parent, view = vl.make_view("pad4_x1", 3, H, W, torch.float32, ops.device)
    before = vl.snapshot(parent)
    torch.cuda.synchronize()
    ops.disparityBM5(views[0], views[1], _cfg(b, params), variant=b.CensusVariants[variant], subpixel=True, out=view)
    ops.ctx.synchronize()
    vl.assert_only_view_written(parent, view, before, "pad4_x1")
    for k in range(3):
        _same(view[k], bc.want(W, H, *params, True, seed=1 + k, variant=variant)[0], "pair %d" % k)


@pytest.mark.parametrize("variant", ["BLOCK_5_5", "CIRCLE_9"])
def test_host_mirror_and_c_abi(dev, b, variant):
    ops, torch = dev
    from boofcv_amd import _lib
    case = bc.CENSUS_CASES[0]
    W, H = case[1:3]
    params = bc.census_params(case, variant)
    left, right = bc.scene(W, H, params[0], params[1])
    want = bc.want(W, H, *params, True, variant=variant)[0]
    config = _cfg(b, params)
    config.configCensus = b.ConfigDisparityError.Census(b.CensusVariants[variant])
    alg = b.FactoryStereoDisparityBest5.blockMatchBest5(config, b.GrayU8, b.GrayF32)
    alg.process(b.GrayU8.wrap(np.array(left)), b.GrayU8.wrap(np.array(right)))
    _same(alg.getDisparity().array().copy(), want, "host mirror")
    assert (alg.getBorderX(), alg.getBorderY()) == (2 * params[2], 2 * params[3])
    assert alg.getCLeft().width == W and alg.getCLeft().height == H
    # the C ABI directly: the host entry with the variant's ordinal
    cfg = _lib.DisparityBmCfg(*params[:4], float(params[4]), params[5], params[6])
    hl, hr = np.ascontiguousarray(left).reshape(-1), np.ascontiguousarray(right).reshape(-1)
    hout = np.full(H * W, -7.0, np.float32)
    st = ops.L.bhip_disparity_bm5_census_u8_f32(ops.ctx._h, C.byref(cfg), int(b.CensusVariants[variant]), hl.ctypes.data_as(_lib._u8p), 0, W,
                                                hr.ctypes.data_as(_lib._u8p), 0, W, W, H, hout.ctypes.data_as(_lib._fp), 0, W)
    assert st == 0
    _same(hout.reshape(H, W), want, "C ABI")


# (W, H, minD, range, rx, ry, variant ordinal, status)
REFUSED = [
    (60, 20, 0, 57, 2, 2, 1, -1),          # maxD > W - 2*rx
    (60, 4, 0, 10, 2, 2, 1, -1),           # H < rh
    (60, 20, 0, 10, 2, 2, 6, -1),          # no such variant
    (60, 20, 0, 10, 2, 2, -1, -1),
    (60, 3, 0, 10, 1, 1, 5, -1),           # CIRCLE_9 has radius 4: H < radius + 1
    (300, 20, 0, 10, 8, 2, 1, -2),
    (300, 9, 0, 257, 2, 1, 0, -2),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "%dx%d_min%d_range%d_r%dx%d_v%d_%d" % c)
def test_refused_calls_write_nothing(dev, b, case):
    ops, torch = dev
    from boofcv_amd import _lib
    W, H, minD, rng, rx, ry, variant, status = case
    left = torch.zeros((1, H, W), dtype=torch.uint8, device=ops.device)
    right = torch.zeros((1, H, W), dtype=torch.uint8, device=ops.device)
    parent, view = vl.make_view("dense", 1, H, W, torch.float32, ops.device)
    before = vl.snapshot(parent)
    torch.cuda.synchronize()
    cfg = _lib.DisparityBmCfg(minD, rng, rx, ry, 0.0, 1, 0.15)
    st = ops.L.bhip_disparity_bm5_census_dev_u8_f32(ops.ctx._h, C.byref(cfg), variant, C.c_void_p(left.data_ptr()), H * W, W, C.c_void_p(right.data_ptr()),
                                                    H * W, W, W, H, 1, C.c_void_p(view.data_ptr()), H * W, W)
    ops.ctx.synchronize()
    assert st == status
    assert bool((vl.bits(parent) == before).all()), "a refused call wrote to its output"
