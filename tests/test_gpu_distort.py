"""GPU: the image remap (ImageDistort on GrayU8 / GrayF32, nearest-neighbour / bilinear, ZERO / EXTENDED), bit for bit against
tests/distort_ref.py, through the device-batched API (device.py), the host-buffer API (api.py) and the C ABI.  Every comparison is exact;
GrayF32 results are compared as bit patterns.

The kernel's tile is 64 columns x 16 rows of the crop per workgroup, four consecutive pixels per lane, the lanes' groups of four aligned to the
destination row's address (boofcv_amd/csrc/distort.hip): the 50- and 67-wide destinations are narrower / one pixel wider than a tile, the
259-wide one spans five; 37 rows span three bands; none of the widths is a multiple of 4."""
import ctypes as C
import functools

import numpy as np
import pytest

import disparity_ref as dr
import distort_ref as dref
import view_layouts as vl

pytestmark = pytest.mark.gpu

DTYPES = {"u8": np.uint8, "f32": np.float32}
INTERPS = {"nn": dref.NEAREST_NEIGHBOR, "bilinear": dref.BILINEAR}
BORDERS = {"zero": dref.ZERO, "extended": dref.EXTENDED}
SOURCES = [(67, 21), (131, 19)]
DESTS = [(50, 37), (67, 21), (259, 17)]


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


def _same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    if bad.any():
        ys, xs = np.nonzero(bad)[-2:]
        raise AssertionError("%s: %d pixels differ; first (x, y) %s: got %r want %r" % (what, int(bad.sum()), (int(xs[0]), int(ys[0])), got[bad][0], want[bad][0]))


def _sentinel_np(shape, dtype):
    """what view_layouts puts into a parent, as a NumPy image: the value every pixel of a destination holds before the call"""
    import torch
    if np.dtype(dtype) == np.float32:
        return np.full(shape, vl.SENTINEL[torch.float32], np.uint32).view(np.float32)
    return np.full(shape, vl.SENTINEL[torch.uint8], np.uint8)


@functools.lru_cache(maxsize=None)
def _src(sw, sh, tname, seed=1):
    a = dref.fill_uniform(sw, sh, DTYPES[tname], seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _rot_map(dw, dh, sw, sh, degrees=30):
    m = dref.rotation_map(dw, dh, sw, sh, degrees)
    m.setflags(write=False)
    return m


def _edge_values(n):
    f = np.float32
    return [f(-1000), f(-1), f(-0.1), f(-0.0), f(0), f(0.5), f(n - 2), np.nextafter(f(n - 2), f(np.inf)), f(n - 1.5), f(n - 1), np.nextafter(f(n - 1), f(np.inf)),
            f(n), f(1e6)]


@functools.lru_cache(maxsize=None)
def _edge_map(dw, dh, sw, sh):
    """the 30 degree rotation with, from row 1 column 2 on, the 13 branch boundaries of get / the inside test in x and y: the diagonal, each x
    value against an interior y and each y value against an interior x"""
    m = np.array(_rot_map(dw, dh, sw, sh))
    ex, ey = _edge_values(sw), _edge_values(sh)
    entries = list(zip(ex, ey)) + [(x, np.float32(7.25)) for x in ex] + [(np.float32(20.5), y) for y in ey]
    flat = m.reshape(-1, 2)
    flat[dw + 2:dw + 2 + len(entries)] = np.array(entries, np.float32)
    assert np.signbit(flat[dw + 2 + 3, 0]) and flat[dw + 2 + 3, 0] == 0     # -0.0 survived
    m.setflags(write=False)
    return m


MAPS = {"rot30": _rot_map, "edge": _edge_map}


@functools.lru_cache(maxsize=None)
def _want(mapname, sw, sh, dw, dh, tname, iname, bname, seed=1):
    """(rendered with renderAll = true, mask) of the reference; renderAll = false is derived by _expect"""
    out, mask, _ = dref.distort(_src(sw, sh, tname, seed), MAPS[mapname](dw, dh, sw, sh), INTERPS[iname], BORDERS[bname], True, np.zeros((dh, dw), DTYPES[tname]))
    out.setflags(write=False)
    mask.setflags(write=False)
    return out, mask


def _expect(all_px, mask, renderAll, before):
    """the destination after the call: renderAll = false assigns the same value, but only where the mask is 1 (ImageDistortCache_SB :171-185
    against :136-148: the same assigner.assign(interp.get(...)) behind the inside test)"""
    return np.array(all_px) if renderAll else np.where(mask == 1, all_px, before)


def _t(dev, a):
    ops, torch = dev
    return torch.as_tensor(np.array(a), device=ops.device)


def _run(dev, src, renderAll=True, interp=dref.BILINEAR, border=dref.EXTENDED, with_mask=True, **kw):
    """src [H,W] or [B,H,W] NumPy -> (out, mask) NumPy of a sentinel-filled destination / mask"""
    ops, torch = dev
    s = _t(dev, src)
    if s.dim() == 2:
        s = s.unsqueeze(0)
    m = kw.pop("map", None)
    if m is not None and not hasattr(m, "is_cuda"):
        m = _t(dev, m)
    if m is not None:
        dh, dw = m.shape[-3], m.shape[-2]
    else:
        dh, dw = kw.pop("shape")
    dt = s.dtype
    _, out = vl.make_view("dense", s.shape[0], dh, dw, dt, ops.device)
    _, mask = vl.make_view("dense", s.shape[0], dh, dw, torch.uint8, ops.device)
    torch.cuda.synchronize()
    ops.distort(s, map=m, interp=interp, border=border, renderAll=renderAll, out=out, mask=mask if with_mask else None, **kw)
    ops.ctx.synchronize()
    return out.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("dst", DESTS, ids=lambda d: "dst%dx%d" % d)
@pytest.mark.parametrize("src", SOURCES, ids=lambda s: "src%dx%d" % s)
@pytest.mark.parametrize("tname", DTYPES)
@pytest.mark.parametrize("iname", INTERPS)
def test_case_table(dev, src, dst, tname, iname):
    (sw, sh), (dw, dh) = src, dst
    for bname in BORDERS:
        all_px, wmask = _want("rot30", sw, sh, dw, dh, tname, iname, bname)
        assert 0 < int(wmask.sum()) < dw * dh
        for renderAll in (True, False):
            got, gmask = _run(dev, _src(sw, sh, tname), renderAll, INTERPS[iname], BORDERS[bname], map=_rot_map(dw, dh, sw, sh))
            _same(got[0], _expect(all_px, wmask, renderAll, _sentinel_np((dh, dw), DTYPES[tname])), "%s renderAll=%s" % (bname, renderAll))
            _same(gmask[0], wmask, "mask %s renderAll=%s" % (bname, renderAll))


@pytest.mark.parametrize("tname", DTYPES)
@pytest.mark.parametrize("iname", INTERPS)
@pytest.mark.parametrize("bname", BORDERS)
def test_edge_map(dev, tname, iname, bname):
    sw, sh, dw, dh = 67, 21, 50, 37
    all_px, wmask = _want("edge", sw, sh, dw, dh, tname, iname, bname)
    for renderAll in (True, False):
        got, gmask = _run(dev, _src(sw, sh, tname), renderAll, INTERPS[iname], BORDERS[bname], map=_edge_map(dw, dh, sw, sh))
        _same(got[0], _expect(all_px, wmask, renderAll, _sentinel_np((dh, dw), DTYPES[tname])), "renderAll=%s" % renderAll)
        _same(gmask[0], wmask, "mask")


@pytest.mark.parametrize("tname", DTYPES)
@pytest.mark.parametrize("iname", INTERPS)
def test_rotation_by_90_degrees_is_a_permutation(dev, tname, iname):
    """sx = y, sy = dw-1-x: every lane of a wave reads another source row"""
    dw, dh = 67, 21
    sw, sh = dh, dw
    ys, xs = np.mgrid[0:dh, 0:dw]
    m = np.ascontiguousarray(np.stack([ys, dw - 1 - xs], -1).astype(np.float32))
    src = _src(sw, sh, tname)
    for bname in BORDERS:
        got, gmask = _run(dev, src, True, INTERPS[iname], BORDERS[bname], map=m)
        _same(got[0], np.ascontiguousarray(np.rot90(src, -1)), bname)
        assert (gmask == 1).all()


AFFINE = (0.9, 0.25, -0.2, 0.85, 3.5, -2.25)
HOMOGRAPHY = (1.02, 0.04, -2.0, -0.03, 0.97, 1.5, 4e-4, -7e-4, 1.0)
HOMOGRAPHY_Z = (1.0, 0.1, 2.0, 0.05, 1.0, -1.0, 0.04, 0.013, -1.00471)   # z changes sign inside the 50 x 37 destination
MODELS = {"affine": (dref.AFFINE, AFFINE), "homography": (dref.HOMOGRAPHY, HOMOGRAPHY), "homography_z_sign": (dref.HOMOGRAPHY, HOMOGRAPHY_Z)}


@functools.lru_cache(maxsize=None)
def _model_map(name, dw, dh):
    m = dref.make_map(*MODELS[name], dw, dh)
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("name", MODELS)
def test_model_path_is_the_map_path_on_the_built_map(dev, name):
    ops, torch = dev
    sw, sh, dw, dh = 67, 21, 50, 37
    model, coeff = MODELS[name]
    want_map = _model_map(name, dw, dh)
    assert np.isfinite(want_map).all() and float(np.abs(want_map).max()) <= 2.0 ** 30       # inside the domain
    if name == "homography_z_sign":
        c = np.array(coeff, np.float32)
        ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float32)
        z = c[6] * xs + c[7] * ys + c[8]
        assert (z < 0).any() and (z > 0).any() and (z != 0).all()
    built = ops.distortBuildMap(model, coeff, dw, dh)
    ops.ctx.synchronize()
    _same(built, want_map, "bhip_distort_build_map")
    for tname in DTYPES:
        for iname in INTERPS:
            for renderAll in (True, False):
                src = _src(sw, sh, tname)
                by_map, mask_map = _run(dev, src, renderAll, INTERPS[iname], dref.EXTENDED, map=built)
                by_model, mask_model = _run(dev, src, renderAll, INTERPS[iname], dref.EXTENDED, model=model, coeff=coeff, shape=(dh, dw))
                _same(by_model, by_map, "%s %s renderAll=%s" % (tname, iname, renderAll))
                _same(mask_model, mask_map, "mask")
    # and against the reference, once per type
    for tname in DTYPES:
        want, wmask, _ = dref.distort(_src(sw, sh, tname), want_map, dref.BILINEAR, dref.ZERO, True, np.zeros((dh, dw), DTYPES[tname]))
        got, gmask = _run(dev, _src(sw, sh, tname), True, dref.BILINEAR, dref.ZERO, model=model, coeff=coeff, shape=(dh, dw))
        _same(got[0], want, tname)
        _same(gmask[0], wmask, "mask")


@pytest.mark.parametrize("tname", DTYPES)
def test_render_inside_only_keeps_the_sentinel(dev, tname):
    """renderAll = false, called on the reference directly: skipped pixels keep the sentinel, also inside a run of four that holds both kinds"""
    sw, sh, dw, dh = 67, 21, 67, 21
    m = _rot_map(dw, dh, sw, sh)
    before = _sentinel_np((dh, dw), DTYPES[tname])
    want, wmask, n = dref.distort(_src(sw, sh, tname), m, dref.BILINEAR, dref.EXTENDED, False, before)
    assert 0 < n < dw * dh
    # every alignment of a group of four consecutive pixels sees a group with both kinds
    for a in range(4):
        groups = wmask[:, a:a + 4 * ((dw - a) // 4)].reshape(dh, -1, 4).sum(-1)
        assert ((groups > 0) & (groups < 4)).any()
    got, gmask = _run(dev, _src(sw, sh, tname), False, dref.BILINEAR, dref.EXTENDED, map=m)
    _same(got[0], want)
    _same(gmask[0], wmask)
    assert (_bits(got[0])[wmask == 0] == _bits(before)[wmask == 0]).all()
    # without a mask the image is the same
    got2, untouched = _run(dev, _src(sw, sh, tname), False, dref.BILINEAR, dref.EXTENDED, with_mask=False, map=m)
    _same(got2[0], want)
    assert (untouched == 0xA5).all()


@pytest.mark.parametrize("tname", DTYPES)
@pytest.mark.parametrize("renderAll", [True, False])
def test_crop(dev, tname, renderAll):
    sw, sh, dw, dh = 67, 21, 50, 37
    crop = (3, 2, 41, 30)
    m = _rot_map(dw, dh, sw, sh)
    before = _sentinel_np((dh, dw), DTYPES[tname])
    want, wmask, _ = dref.distort(_src(sw, sh, tname), m, dref.BILINEAR, dref.ZERO, renderAll, before, crop=crop)
    got, gmask = _run(dev, _src(sw, sh, tname), renderAll, dref.BILINEAR, dref.ZERO, map=m, crop=crop)
    _same(got[0], want)                                   # outside the crop `want` is the sentinel
    _same(gmask[0], np.where(wmask == 255, np.uint8(0xA5), wmask))
    keep = np.ones((dh, dw), bool)
    keep[2:30, 3:41] = False
    assert (_bits(got[0])[keep] == _bits(before)[keep]).all() and (gmask[0][keep] == 0xA5).all()


@pytest.mark.parametrize("layout", ["pad4", "pad4_x1", "odd"])
@pytest.mark.parametrize("tname", DTYPES)
def test_strided_batch_into_output_windows(dev, layout, tname):
    """three different sources, rows sw+3 elements apart starting at element 1, images a non-dense stride apart; the destination and the mask
    windows of `layout`; one map shared by the batch against three maps"""
    ops, torch = dev
    sw, sh, dw, dh, B = 67, 21, 50, 37, 3
    tdt = torch.uint8 if tname == "u8" else torch.float32
    pitch, image = sw + 3, (sw + 3) * (sh + 1) + 5
    parent = vl.sentinel_buffer(1 + B * image + 64, tdt, ops.device)
    srcs = torch.as_strided(parent, (B, sh, sw), (image, pitch, 1), 1)
    if tname == "u8":
        assert srcs.data_ptr() % 2 == 1
    for b in range(B):
        srcs[b].copy_(_t(dev, _src(sw, sh, tname, seed=1 + b)))
    maps = [_rot_map(dw, dh, sw, sh, deg) for deg in (30, 75, 160)]
    shared, each = _t(dev, maps[0]), _t(dev, np.stack(maps))
    for renderAll in (True, False):
        for which, mt in (("shared", shared), ("each", each)):
            dparent, dview = vl.make_view(layout, B, dh, dw, tdt, ops.device)
            mparent, mview = vl.make_view(layout, B, dh, dw, torch.uint8, ops.device)
            dbefore, mbefore = vl.snapshot(dparent), vl.snapshot(mparent)
            torch.cuda.synchronize()
            ops.distort(srcs, map=mt, interp=dref.BILINEAR, border=dref.EXTENDED, renderAll=renderAll, out=dview, mask=mview)
            ops.ctx.synchronize()
            vl.assert_only_view_written(dparent, dview, dbefore, layout)
            vl.assert_only_view_written(mparent, mview, mbefore, layout + " mask")
            for b in range(B):
                want, wmask, _ = _batch_want(sw, sh, dw, dh, tname, 1 + b, (30, 75, 160)[0 if which == "shared" else b])
                _same(dview[b], _expect(want, wmask, renderAll, _sentinel_np((dh, dw), DTYPES[tname])), "%s image %d renderAll=%s" % (which, b, renderAll))
                _same(mview[b], wmask, "%s mask %d" % (which, b))


@functools.lru_cache(maxsize=None)
def _batch_want(sw, sh, dw, dh, tname, seed, degrees):
    return dref.distort(_src(sw, sh, tname, seed), _rot_map(dw, dh, sw, sh, degrees), dref.BILINEAR, dref.EXTENDED, True, np.zeros((dh, dw), DTYPES[tname]))


class _Wobble:
    """a transform of the caller's own: compute(x, y) in float32, evaluated on the host into a map"""

    def __new__(cls, api):
        class Wobble(api.PixelTransform):
            def compute(self, x, y):
                f = np.float32
                return f(x) * f(1.25) + f(y) * f(0.125) - f(3.5), f(y) * f(0.5) + f(x) * f(0.0625) - f(1.25)
        return Wobble()


@pytest.mark.parametrize("tname", DTYPES)
def test_host_entry_equals_device_entry(dev, api, tname):
    """FactoryDistort.distortSB(...).apply on sub-images with an odd startIndex and stride > width: a transform of the caller's (the map form), an
    affine model uncached (the model form) and cached (the map form again); then another destination size on the same object"""
    sw, sh, dw, dh = 67, 21, 50, 37
    G = api.GrayU8 if tname == "u8" else api.GrayF32
    src = _src(sw, sh, tname)

    def sub(w, h, fill=None, G=G):
        big = G(w + 5, h + 3)
        s = big.subimage(1, 2, 1 + w, 2 + h)
        assert s.startIndex % 2 == 1 and s.stride > w
        if fill is not None:
            s.array()[:, :] = fill
        return s

    interp = api.FactoryInterpolation.createPixelS(0, 255, api.InterpolationType.BILINEAR, api.BorderType.ZERO, G)
    wob = _Wobble(api)
    wmap = api._host_map(wob, dw, dh).reshape(dh, dw, 2)
    aff = api.PixelTransformAffine_F32(*AFFINE)
    amap = _model_map("affine", dw, dh)
    for cached, t, tmap in ((False, wob, wmap), (False, aff, amap), (True, aff, amap)):
        d = api.FactoryDistort.distortSB(cached, interp, G)
        d.setModel(t)
        for renderAll in (True, False):
            d.setRenderAll(renderAll)
            dst, mask = sub(dw, dh, 9), sub(dw, dh, 9, api.GrayU8)
            d.apply(sub(sw, sh, src), dst, mask)
            want, wmask, _ = dref.distort(src, np.ascontiguousarray(tmap), dref.BILINEAR, dref.ZERO, renderAll, np.full((dh, dw), 9, DTYPES[tname]))
            _same(dst.array().copy(), want, "host cached=%s renderAll=%s" % (cached, renderAll))
            _same(mask.array().copy(), wmask, "host mask")
            got, gmask = _run(dev, src, renderAll, dref.BILINEAR, dref.ZERO, map=np.ascontiguousarray(tmap))
            if renderAll:
                _same(got[0], dst.array().copy(), "device")
            _same(gmask[0], mask.array().copy(), "device mask")
        # the crop form, then a second destination size on the same object: the map is rebuilt
        dst = sub(dw, dh, 9)
        d.setRenderAll(True)
        d.apply(sub(sw, sh, src), dst, 3, 2, 41, 30)
        want, _, _ = dref.distort(src, np.ascontiguousarray(tmap), dref.BILINEAR, dref.ZERO, True, np.full((dh, dw), 9, DTYPES[tname]), crop=(3, 2, 41, 30))
        _same(dst.array().copy(), want, "host crop")
        dw2, dh2 = 23, 11
        dst2 = sub(dw2, dh2, 9)
        d.apply(sub(sw, sh, src), dst2)
        map2 = api._host_map(t, dw2, dh2).reshape(dh2, dw2, 2)
        want2, _, _ = dref.distort(src, np.ascontiguousarray(map2), dref.BILINEAR, dref.ZERO, True, np.full((dh2, dw2), 9, DTYPES[tname]))
        _same(dst2.array().copy(), want2, "second destination size")


def test_distort_single_skip_rule(dev, api):
    """DistortImageOps.distortSingle with BorderType.SKIP: EXTENDED and renderAll = false; DistortImageOps.affine inverts in float"""
    sw, sh = 67, 21
    src = _src(sw, sh, "u8")
    t = api.PixelTransformAffine_F32(*AFFINE)
    out = api.GrayU8(50, 37)
    out.data[:] = 9
    api.DistortImageOps.distortSingle(api.GrayU8.wrap(src), out, t, api.InterpolationType.BILINEAR, api.BorderType.SKIP)
    want, _, n = dref.distort(src, _model_map("affine", 50, 37), dref.BILINEAR, dref.EXTENDED, False, np.full((37, 50), 9, np.uint8))
    assert 0 < n < 50 * 37
    _same(out.array().copy(), want)
    out2 = api.GrayU8(sw, sh)
    api.DistortImageOps.affine(api.GrayU8.wrap(src), out2, api.BorderType.ZERO, api.InterpolationType.NEAREST_NEIGHBOR, 1, 0, 0, 1, 2, 3)   # a shift by (2, 3)
    assert (out2.array()[3:, 2:] == src[:-3, :-2]).all() and (out2.array()[:3] == 0).all() and (out2.array()[:, :2] == 0).all()


# (what, status, overrides): BHIP_ERR_INVALID = -1, BHIP_ERR_UNSUPPORTED = -2
REFUSED = [
    ("empty_source_w", -1, dict(sw=0)),
    ("empty_source_h", -1, dict(sh=0)),
    ("crop_right", -1, dict(crop=(0, 0, 51, 37))),
    ("crop_bottom", -1, dict(crop=(0, 0, 50, 38))),
    ("crop_negative", -1, dict(crop=(-1, 0, 50, 37))),
    ("crop_reversed", -1, dict(crop=(10, 0, 9, 37))),
    ("null_map_or_coeff", -1, dict(coords=None)),
    ("no_such_model", -1, dict(model=3)),
    ("bicubic", -2, dict(interp=2)),
    ("polynomial4", -2, dict(interp=3)),
    ("border_skip", -2, dict(border=0)),
    ("border_normalized", -2, dict(border=2)),
    ("border_reflect", -2, dict(border=3)),
    ("border_wrap", -2, dict(border=4)),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c[0])
@pytest.mark.parametrize("tname", DTYPES)
def test_refused_calls_write_nothing(dev, tname, case):
    ops, torch = dev
    from boofcv_amd import _lib
    what, status, o = case
    sw, sh, dw, dh = 67, 21, 50, 37
    tdt = torch.uint8 if tname == "u8" else torch.float32
    hp = _lib._u8p if tname == "u8" else _lib._fp
    src = torch.zeros((1, sh, sw), dtype=tdt, device=ops.device)
    dmap = _t(dev, _rot_map(dw, dh, sw, sh))
    coeff = np.array(AFFINE, np.float32)
    crop = o.get("crop", (0, 0, dw, dh))
    interp, border = o.get("interp", dref.BILINEAR), o.get("border", dref.EXTENDED)
    psw, psh = o.get("sw", sw), o.get("sh", sh)
    null = "coords" in o
    sfx = "u8" if tname == "u8" else "f32"
    forms = [("map", getattr(ops.L, "bhip_distort_map_dev_" + sfx), (None if null else C.c_void_p(dmap.data_ptr()), 0))]
    forms.append(("model", getattr(ops.L, "bhip_distort_model_dev_" + sfx), (o.get("model", dref.AFFINE), None if null else coeff.ctypes.data_as(_lib._fp))))
    for name, fn, coords in forms:
        if "model" in o and name == "map":
            continue
        parent, view = vl.make_view("dense", 1, dh, dw, tdt, ops.device)
        mparent, mview = vl.make_view("dense", 1, dh, dw, torch.uint8, ops.device)
        before, mbefore = vl.snapshot(parent), vl.snapshot(mparent)
        torch.cuda.synchronize()
        st = fn(ops.ctx._h, C.c_void_p(src.data_ptr()), sh * sw, sw, psw, psh, 1, *coords, dw, dh, *crop, interp, border, 1, C.c_void_p(view.data_ptr()), dh * dw, dw,
                C.c_void_p(mview.data_ptr()), dh * dw, dw)
        ops.ctx.synchronize()
        assert st == status, name
        assert bool((vl.bits(parent) == before).all()) and bool((vl.bits(mparent) == mbefore).all()), "a refused call wrote to its output"
    # the host entries answer the same and leave the caller's arrays alone
    hsrc = np.zeros(sh * sw, DTYPES[tname])
    hmap = np.array(_rot_map(dw, dh, sw, sh)).reshape(-1)
    forms = [("map", getattr(ops.L, "bhip_distort_map_" + sfx), (None if null else hmap.ctypes.data_as(_lib._fp),))]
    forms.append(("model", getattr(ops.L, "bhip_distort_model_" + sfx), (o.get("model", dref.AFFINE), None if null else coeff.ctypes.data_as(_lib._fp))))
    for name, fn, coords in forms:
        if "model" in o and name == "map":
            continue
        out, hmask = np.full(dh * dw, 7, DTYPES[tname]), np.full(dh * dw, 7, np.uint8)
        st = fn(ops.ctx._h, hsrc.ctypes.data_as(hp), 0, sw, psw, psh, *coords, dw, dh, *crop, interp, border, 1, out.ctypes.data_as(hp), 0, dw,
                hmask.ctypes.data_as(_lib._u8p), 0, dw)
        assert st == status and (out == 7).all() and (hmask == 7).all(), name


def test_build_map_refusals(dev):
    ops, torch = dev
    from boofcv_amd import _lib
    coeff = np.array(AFFINE, np.float32)
    parent = vl.sentinel_buffer(2 * 8 * 8 + 64, torch.float32, ops.device)
    before = vl.snapshot(parent)
    torch.cuda.synchronize()
    p = C.c_void_p(parent.data_ptr())
    for args in ((0, coeff.ctypes.data_as(_lib._fp), 8, 8, p), (3, coeff.ctypes.data_as(_lib._fp), 8, 8, p), (1, None, 8, 8, p), (1, coeff.ctypes.data_as(_lib._fp), 0, 8, p),
                 (1, coeff.ctypes.data_as(_lib._fp), 8, 8, None)):
        assert ops.L.bhip_distort_build_map(ops.ctx._h, *args) == -1
    ops.ctx.synchronize()
    assert bool((vl.bits(parent) == before).all())


def test_rectify_then_block_match_on_the_device(dev, api):
    """both frames of a stereo pair through a mild homography (the model form), the outputs straight into disparityBM"""
    ops, torch = dev
    W, H, minD, rng, rx, ry, mpe, rtol, tex = 67, 21, 2, 30, 2, 1, 25, 1, .15
    left, right = dr.stereo_scene(W, H, minD, rng, 1)
    hl = (1.0, 0.004, 0.25, -0.003, 1.0, 0.125, 1e-5, -2e-5, 1.0)
    hr = (1.0, -0.002, -0.5, 0.005, 1.0, 0.25, -1e-5, 1e-5, 1.0)
    rect, want_rect = [], []
    for img, h in ((left, hl), (right, hr)):
        out = ops.distort(_t(dev, img).unsqueeze(0), model=dref.HOMOGRAPHY, coeff=h, interp=dref.BILINEAR, border=dref.EXTENDED, shape=(H, W))
        rect.append(out)
        w, _, _ = dref.distort(img, dref.make_map(dref.HOMOGRAPHY, h, W, H), dref.BILINEAR, dref.EXTENDED, True, np.zeros((H, W), np.uint8))
        want_rect.append(w)
    cfg = api.ConfigDisparityBM(minDisparity=minD, rangeDisparity=rng, regionRadiusX=rx, regionRadiusY=ry, maxPerPixelError=mpe, validateRtoL=rtol, texture=tex)
    got = ops.disparityBM(rect[0], rect[1], cfg, subpixel=True)
    ops.ctx.synchronize()
    _same(rect[0][0], want_rect[0], "rectified left")
    _same(rect[1][0], want_rect[1], "rectified right")
    want, _ = dr.block_match(want_rect[0], want_rect[1], minD, rng, rx, ry, mpe, rtol, tex, True)
    assert len(np.unique(want)) > 3
    _same(got[0], want, "disparity")
