"""GPU: dense stereo disparity by census block matching on GrayU8 pairs (FactoryStereoDisparity.blockMatch with errorType = CENSUS, GrayU8 or
sub-pixel GrayF32 disparity), bit for bit against tests/census_ref.py, through the device-batched API (device.py), the host-buffer API
(census.py) and the C ABI.  Every comparison is exact; GrayF32 disparities are compared as bit patterns.

Variants: BLOCK_3_3, BLOCK_5_5 and BLOCK_7_7, one per census word size (GrayU8, GrayS32, GrayS64), and CIRCLE_9.  The cases are
tests/census_cases.py's (the geometry of test_gpu_disparity.py's table); tests/test_census_reference.py asserts on the CPU that each holds at
least 10 reference pixels of every class it claims.  The matching kernel's tile is 64 block columns wide; it is 16 output rows high for the
1-byte words and 22 - 2*regionRadiusY rows for the 4-byte ones (boofcv_amd/csrc/disparity.hip): the 259-wide case spans five column tiles,
the 200 x 40 case four column tiles and three row bands."""
import ctypes as C

import numpy as np
import pytest

import census_cases as cc
import census_ref as cr
import disparity_ref as dr
import view_layouts as vl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _cfg(api, minD, rng, rx, ry, mpe, rtol, tex, subpixel=True):
    return api.ConfigDisparityBM(minDisparity=minD, rangeDisparity=rng, regionRadiusX=rx, regionRadiusY=ry, maxPerPixelError=mpe, validateRtoL=rtol,
                                 texture=tex, subpixel=subpixel, errorType=api.DisparityError.CENSUS)


def _dev_run(dev, api, variant, left, right, params, subpixel, out=None):
    ops, torch = dev
    lt = torch.as_tensor(np.array(left), device=ops.device)
    rt = torch.as_tensor(np.array(right), device=ops.device)
    if lt.dim() == 2:
        lt, rt = lt.unsqueeze(0), rt.unsqueeze(0)
    got = ops.disparityBMCensus(lt, rt, _cfg(api, *params), variant=cr.VARIANTS.index(variant), subpixel=subpixel, out=out)
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


@pytest.mark.parametrize("variant", cc.BM_VARIANTS)
@pytest.mark.parametrize("case", cc.BM_CASES, ids=lambda c: c[0])
def test_block_match_cases(dev, api, case, variant):
    name, W, H, minD, rng = case[:5]
    params = cc.params(case, variant)
    left, right = cc.scene(W, H, minD, rng)
    for output in case[10]:
        sub = output == "f32"
        want, _ = cc.want(variant, W, H, *params, sub)
        got = _dev_run(dev, api, variant, left, right, params, sub)
        _same(got[0], want, "%s %s %s" % (name, variant, output))


@pytest.mark.parametrize("off", ["maxPerPixelError", "validateRtoL", "texture", "all"])
@pytest.mark.parametrize("variant", cc.BM_VARIANTS)
def test_each_check_disabled_on_its_own(dev, api, variant, off):
    case = next(c for c in cc.BM_CASES if c[0] == "row_bands")
    name, W, H, minD, rng, rx, ry = case[:7]
    mpe, rtol, tex = cc.each_check_params(variant, off)
    left, right = cc.scene(W, H, minD, rng)
    for sub in (True, False):
        want, cls = cc.want(variant, W, H, minD, rng, rx, ry, mpe, rtol, tex, sub)
        counts = dr.class_counts(cls)
        disabled = {"maxPerPixelError": [dr.REJECT_ERROR], "validateRtoL": [dr.REJECT_RTOL], "texture": [dr.REJECT_TEXTURE],
                    "all": [dr.REJECT_ERROR, dr.REJECT_RTOL, dr.REJECT_TEXTURE]}[off]
        assert all(counts[k] == 0 for k in disabled)
        _same(_dev_run(dev, api, variant, left, right, (minD, rng, rx, ry, mpe, rtol, tex), sub)[0], want, "%s %s" % (variant, off))


@pytest.mark.parametrize("variant", cc.BM_VARIANTS)
def test_batch_of_three_strided_pairs_at_odd_byte_offsets(dev, api, variant):
    """three different pairs, rows W+3 bytes apart starting at byte offset 1, images a non-dense stride apart; the output dense"""
    ops, torch = dev
    case = next(c for c in cc.BM_CASES if c[0] == "min2_u8")
    W, H, minD, rng = case[1:5]
    params = cc.params(case, variant)
    pitch, image = W + 3, (W + 3) * (H + 1) + 5
    parents = [torch.full((1 + 3 * image + 64,), 0xA5, dtype=torch.uint8, device=ops.device) for _ in range(2)]
    views = [torch.as_strided(p, (3, H, W), (image, pitch, 1), 1) for p in parents]
    assert views[0].data_ptr() % 2 == 1
    for b in range(3):
        left, right = cc.scene(W, H, minD, rng, seed=1 + b)
        views[0][b].copy_(torch.as_tensor(np.array(left), device=ops.device))
        views[1][b].copy_(torch.as_tensor(np.array(right), device=ops.device))
    torch.cuda.synchronize()
    for sub in (True, False):
        got = ops.disparityBMCensus(views[0], views[1], _cfg(api, *params), variant=cr.VARIANTS.index(variant), subpixel=sub)
        ops.ctx.synchronize()
        for b in range(3):
            _same(got[b], cc.want(variant, W, H, *params, sub, seed=1 + b)[0], "%s pair %d" % (variant, b))


@pytest.mark.parametrize("layout", ["pad4", "pad4_x1", "odd"])
@pytest.mark.parametrize("sub", [True, False], ids=["f32", "u8"])
@pytest.mark.parametrize("variant", cc.BM_VARIANTS)
def test_output_windows_keep_their_guard_bands(dev, api, variant, sub, layout):
    ops, torch = dev
    case = next(c for c in cc.BM_CASES if c[0] == "min2_u8")
    W, H, minD, rng = case[1:5]
    params = cc.params(case, variant)
    B = 2
    lefts, rights = zip(*[cc.scene(W, H, minD, rng, seed=1 + b) for b in range(B)])
    parent, view = vl.make_view(layout, B, H, W, torch.float32 if sub else torch.uint8, ops.device)
    before = vl.snapshot(parent)
    torch.cuda.synchronize()
    _dev_run(dev, api, variant, np.stack(lefts), np.stack(rights), params, sub, out=view)
    vl.assert_only_view_written(parent, view, before, layout)
    for b in range(B):
        _same(view[b], cc.want(variant, W, H, *params, sub, seed=1 + b)[0], "%s %s pair %d" % (variant, layout, b))


@pytest.mark.parametrize("sub", [True, False], ids=["f32", "u8"])
@pytest.mark.parametrize("variant", cc.BM_VARIANTS)
def test_host_entry_equals_device_entry(dev, api, variant, sub):
    """FactoryStereoDisparityCensus.blockMatch(...).process on sub-images with an odd startIndex and stride > width; a second pair on the same
    object; the census images of the wrapper"""
    from boofcv_amd import census
    case = next(c for c in cc.BM_CASES if c[0] == "min2_u8")
    W, H, minD, rng, rx, ry = case[1:7]
    params = cc.params(case, variant)
    left, right = cc.scene(W, H, minD, rng)
    subs = []
    for img in (left, right):
        big = api.GrayU8(W + 5, H + 3)
        s = big.subimage(1, 2, 1 + W, 2 + H)
        s.array()[:, :] = img
        subs.append(s)
    alg = census.FactoryStereoDisparityCensus.blockMatch(_cfg(api, *params, subpixel=sub), api.GrayU8, api.GrayF32 if sub else api.GrayU8,
                                                         census.ConfigDisparityError.Census(census.CensusVariants[variant]))
    alg.process(*subs)
    host = alg.getDisparity().array().copy()
    _same(host, cc.want(variant, W, H, *params, sub)[0], "host")
    _same(_dev_run(dev, api, variant, left, right, params, sub)[0], host, "device")
    assert (alg.getBorderX(), alg.getBorderY(), alg.getMinDisparity(), alg.getRangeDisparity(), alg.getInvalidValue()) == (rx, ry, minD, rng, rng)
    for got, img in ((alg.getCLeft(), left), (alg.getCRight(), right)):
        want = cr.census_variant(img, variant)
        assert isinstance(got, alg.getCensusTran().getOutputType()) and got.array().dtype == want.dtype and (got.array() == want).all()
    # a second pair on the same object: the whole image is written again
    left2, right2 = cc.scene(W, H, minD, rng, seed=2)
    alg.process(api.GrayU8.wrap(left2), api.GrayU8.wrap(right2))
    _same(alg.getDisparity().array().copy(), cc.want(variant, W, H, *params, sub, seed=2)[0], "second pair")
    assert (alg.getCLeft().array() == cr.census_variant(left2, variant)).all()


# (W, H, minD, range, rx, ry, variant, subpixel, status): BHIP_ERR_INVALID = -1, BHIP_ERR_UNSUPPORTED = -2
REFUSED = [
    (60, 20, -1, 10, 2, 2, 1, True, -1),
    (60, 20, 0, 0, 2, 2, 1, True, -1),
    (60, 20, 0, 10, -1, 2, 0, True, -1),
    (60, 20, 0, 10, 2, -1, 2, True, -1),
    (60, 20, 0, 57, 2, 2, 1, True, -1),       # maxD > W - 2*rx = 56
    (60, 20, 50, 7, 2, 2, 5, True, -1),
    (60, 4, 0, 10, 2, 2, 0, True, -1),        # H < rh
    (300, 9, 0, 254, 2, 1, 1, False, -1),     # inv = 255 > 254 in a GrayU8 disparity
    (60, 20, 0, 10, 2, 2, -1, True, -1),      # no such variant
    (60, 20, 0, 10, 2, 2, 6, True, -1),
    (60, 3, 0, 10, 2, 1, 2, True, -1),        # H >= rh, but < radius + 1 of the 7x7 census
    (60, 5, 0, 10, 2, 1, 4, False, -1),       # BLOCK_13_5: radius 5
    (300, 20, 0, 10, 8, 2, 1, True, -2),
    (300, 20, 0, 10, 2, 8, 0, True, -2),
    (300, 9, 0, 257, 2, 1, 2, True, -2),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "%dx%d_min%d_range%d_r%dx%d_v%d_%s_%d" % c)
def test_refused_calls_write_nothing(dev, api, case):
    ops, torch = dev
    from boofcv_amd import _lib
    W, H, minD, rng, rx, ry, variant, sub, status = case
    dt = torch.float32 if sub else torch.uint8
    left = torch.zeros((1, H, W), dtype=torch.uint8, device=ops.device)
    right = torch.zeros((1, H, W), dtype=torch.uint8, device=ops.device)
    parent, view = vl.make_view("dense", 1, H, W, dt, ops.device)
    before = vl.snapshot(parent)
    torch.cuda.synchronize()
    cfg = _lib.DisparityBmCfg(minD, rng, rx, ry, 0.0, 1, 0.15)
    fn = ops.L.bhip_disparity_bm_census_dev_u8_f32 if sub else ops.L.bhip_disparity_bm_census_dev_u8_u8
    st = fn(ops.ctx._h, C.byref(cfg), variant, C.c_void_p(left.data_ptr()), H * W, W, C.c_void_p(right.data_ptr()), H * W, W, W, H, 1,
            C.c_void_p(view.data_ptr()), H * W, W)
    ops.ctx.synchronize()
    assert st == status
    assert bool((vl.bits(parent) == before).all()), "a refused call wrote to its output"
    # the host entry answers the same and leaves the caller's array alone
    hl, hr = np.zeros(H * W, np.uint8), np.zeros(H * W, np.uint8)
    out = np.full(H * W, 7, np.float32 if sub else np.uint8)
    hfn = ops.L.bhip_disparity_bm_census_u8_f32 if sub else ops.L.bhip_disparity_bm_census_u8_u8
    st = hfn(ops.ctx._h, C.byref(cfg), variant, hl.ctypes.data_as(_lib._u8p), 0, W, hr.ctypes.data_as(_lib._u8p), 0, W, W, H,
             out.ctypes.data_as(_lib._fp if sub else _lib._u8p), 0, W)
    assert st == status and (out == 7).all()


@pytest.mark.parametrize("variant", cc.BM_VARIANTS)
def test_null_config_is_the_reference_default(dev, api, variant):
    ops, torch = dev
    W, H = 131, 19
    left, right = cc.scene(W, H, 0, 100)
    lt = torch.as_tensor(np.array(left), device=ops.device).unsqueeze(0)
    rt = torch.as_tensor(np.array(right), device=ops.device).unsqueeze(0)
    got = ops.disparityBMCensus(lt, rt, None, variant=cr.VARIANTS.index(variant), subpixel=True)
    ops.ctx.synchronize()
    _same(got[0], cc.want(variant, W, H, 0, 100, 3, 3, 0, 1, .15, True)[0])


def test_sad_entry_is_unchanged_by_a_census_call_on_the_same_context(dev, api):
    """the two forms share the context's scratch buffer: a SAD pair after a census pair"""
    ops, torch = dev
    W, H, minD, rng = 131, 19, 0, 100
    left, right = cc.scene(W, H, minD, rng)
    lt = torch.as_tensor(np.array(left), device=ops.device).unsqueeze(0)
    rt = torch.as_tensor(np.array(right), device=ops.device).unsqueeze(0)
    ops.disparityBMCensus(lt, rt, None, variant=2)
    got = ops.disparityBM(lt, rt, None, subpixel=True)
    ops.ctx.synchronize()
    _same(got[0], dr.block_match(left, right)[0], "SAD after census")
