"""GPU: dense descriptors (FactoryDescribeImageDense.hog, both variants, and .sift) against tests/dense_ref.py, through the device-batched calls
(DeviceImageOps.denseHog / denseSift), the host-buffer C ABI (bhip_dense_*) and the mirror classes (boofcv_amd/dense.py).

Exact: counts, locations and their order; the fast variant's cell histograms as float bit patterns.  Every descriptor element of every descriptor of
every case is within 1e-12 absolute of the reference (the bound the project holds SIFT descriptors to): the only admitted difference is the last
ulps of atan / atan2 between the C library and the device library.  The largest difference and whether the descriptors were bit-identical are
printed for every case.

Preconditions, asserted on the reference alone before anything is compared (a failing one means the input is wrong, not the kernel):
  * every HOG case has all its atan values at least 64 double-ulps from a float rounding midpoint: a device atan a few ulps off narrows to the same
    float, after which every HOG operation is IEEE-specified;
  * the axis cases contain dx == 0 samples, with dy >= 0 (ramp-y, const) and with dy < 0 (down);
  * every noise case has at least one element clipped at 0.2;
  * the standard variant's noise cases visit pixels on both sides of the pixelsPerCell / 2 split.

Images: `noise` is numpy's default_rng(seed) in [0, 255) (float32, or floor of it as uint8); ramp-x / ramp-y are 2 * x / 2 * y; down is 250 - 3 * y (every
column strictly decreasing: dx == 0, dy < 0) with two squares; const is 37 everywhere (every gradient is 0: atanSafe(0, 0) gives the angle pi,
magnitudes are 0 and the descriptors stay all-zero)."""
import ctypes as C
import functools

import numpy as np
import pytest

import dense_ref as dr
import view_layouts as vl

pytestmark = pytest.mark.gpu

DESC_TOL = 1e-12
ATAN_MARGIN = 64.0
HOG_DEFAULT = (9, 8, 3, 3, 1)
SIFT_DEFAULT = (4, 4, 8, 0.5, 0.2, 6.0, 6.0)
# name -> (algorithm, W, H, image kind, seed, config): hog (bins, pixelsPerCell, cellsPerBlockX, cellsPerBlockY, stepBlock) + variant by algorithm;
# sift (widthSubregion, widthGrid, numHistogramBins, weightingSigmaFraction, maxDescriptorElementValue, periodX, periodY)
CASES = {}
for alg in ("fast", "std"):
    CASES.update({
        alg + "-64x48": (alg, 64, 48, "noise", 1, HOG_DEFAULT),                    # 8 x 6 cells, 24 descriptors of 81
        alg + "-61x45": (alg, 61, 45, "noise", 2, (10, 8, 2, 2, 1)),               # trailing pixels ignored; the reference tests' config
        alg + "-odd-cell": (alg, 64, 48, "noise", 3, (9, 5, 3, 2, 2)),             # odd cell, non-square block, step 2
        alg + "-u8": (alg, 64, 48, "noise-u8", 4, HOG_DEFAULT),
        alg + "-ramp-x": (alg, 64, 48, "ramp-x", 0, HOG_DEFAULT),
        alg + "-ramp-y": (alg, 64, 48, "ramp-y", 0, HOG_DEFAULT),
        alg + "-down": (alg, 64, 48, "down", 0, HOG_DEFAULT),
        alg + "-const": (alg, 64, 48, "const", 0, HOG_DEFAULT),
        alg + "-small": (alg, 20, 20, "noise", 5, HOG_DEFAULT),                    # smaller than one block: count 0
        alg + "-s6": (alg, 64, 48, "noise", 6, HOG_DEFAULT),
        alg + "-s7": (alg, 64, 48, "noise", 7, HOG_DEFAULT),
    })
CASES.update({
    "fast-bins1-cell1": ("fast", 16, 12, "noise", 8, (1, 1, 3, 3, 1)),
    "std-odd-side": ("std", 64, 48, "noise", 9, (9, 5, 3, 3, 1)),                  # a block of 15 x 15 pixels: no 0.5 offset, i <= 2 | i > 2
    "sift-40x33": ("sift", 40, 33, "noise", 1, SIFT_DEFAULT),                      # a 4 x 2 grid
    "sift-periods": ("sift", 40, 33, "noise", 2, (4, 4, 8, 0.5, 0.2, 5.5, 7.25)),
    "sift-grid-3-2-4": ("sift", 40, 33, "noise", 3, (3, 2, 4, 0.5, 0.2, 6.0, 6.0)),
    "sift-64x48-p3": ("sift", 64, 48, "noise", 4, (4, 4, 8, 0.5, 0.2, 3.0, 3.0)),  # heavy overlap
    "sift-u8": ("sift", 40, 33, "noise-u8", 5, SIFT_DEFAULT),
    "sift-ramp-x": ("sift", 40, 33, "ramp-x", 0, SIFT_DEFAULT),
    "sift-ramp-y": ("sift", 40, 33, "ramp-y", 0, SIFT_DEFAULT),
    "sift-down": ("sift", 40, 33, "down", 0, SIFT_DEFAULT),
    "sift-const": ("sift", 40, 33, "const", 0, SIFT_DEFAULT),
    "sift-one-window": ("sift", 16, 40, "noise", 6, SIFT_DEFAULT),                 # exactly one window wide: numX = 0, count 0
    "sift-s6": ("sift", 40, 33, "noise", 6, SIFT_DEFAULT),
    "sift-s7": ("sift", 40, 33, "noise", 7, SIFT_DEFAULT),
})
EMPTY = ("fast-small", "std-small", "sift-one-window")


@functools.lru_cache(maxsize=None)
def _image(W, H, kind, seed):
    if kind.startswith("noise"):
        a = (np.random.default_rng(seed).random((H, W)) * 255.0).astype(np.float32)
        if kind == "noise-u8":
            a = np.floor(a).astype(np.uint8)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        a = {"ramp-x": 2.0 * xx, "ramp-y": 2.0 * yy, "down": 250.0 - 3.0 * yy, "const": 37.0 + 0.0 * xx}[kind].astype(np.float32)
        if kind == "down":
            a[10:17, 12:19] = 200.0
            a[20:24, 28:32] = 0.0
    a.setflags(write=False)
    return a


def _ref_alg(name):
    alg, W, H, kind, seed, cfg = CASES[name]
    return dr.DenseSift(*cfg) if alg == "sift" else dr.Hog(*cfg, fastVariant=(alg == "fast"))


def _mirror_config(name):
    from boofcv_amd import dense, sift
    alg, W, H, kind, seed, cfg = CASES[name]
    if alg == "sift":
        c = dense.ConfigDenseSift(dense.DenseSampling(cfg[5], cfg[6]))
        c.sift = sift.ConfigSiftDescribe(cfg[0], cfg[1], cfg[2], 1.0, cfg[3], cfg[4])
        return c
    return dense.ConfigDenseHoG(*cfg, fastVariant=(alg == "fast"))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(result, stats) of dense_ref, computed once per case and shared by the tests that need it"""
    alg, W, H, kind, seed, cfg = CASES[name]
    img, stats, ref = _image(W, H, kind, seed), dr.new_stats(), _ref_alg(name)
    res = ref.process(img, kind == "noise-u8", stats) if alg == "sift" else ref.process(img, stats)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res, stats


def _check_preconditions(name):
    alg, W, H, kind, seed, cfg = CASES[name]
    res, st = _reference(name)
    print("%s: %d descriptors of %d, atan margin %.3g ulps, dx == 0 with dy >= 0 / < 0: %d / %d of %d pixels, clipped %d, split %d / %d"
          % (name, len(res["desc"]), res["desc"].shape[1], st["atanMargin"], st["axisPos"], st["axisNeg"], st["pixels"], st["clipped"], st["splitLow"], st["splitHigh"]))
    if alg != "sift":
        assert st["atanMargin"] >= ATAN_MARGIN, st
    if kind in ("ramp-y", "const"):
        assert st["axisPos"] == st["pixels"] and st["axisNeg"] == 0, st
    if kind == "down":
        assert st["axisNeg"] >= st["pixels"] // 2 and st["axisPos"] >= 1, st
    if kind.startswith("noise") and name not in EMPTY:
        assert st["clipped"] >= 1, st
        if alg == "std":
            assert st["splitLow"] >= 1 and st["splitHigh"] >= 1, st
    assert (len(res["desc"]) == 0) == (name in EMPTY)
    return res, st


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _assert_result(desc, xy, res, what, n=None, cells=None):
    n = len(res["desc"]) if n is None else n
    assert len(desc) == n and len(xy) == n, (what, len(desc), n)
    assert xy.dtype == np.int32 and np.array_equal(xy, res["xy"][:n]), what + ": locations"
    if cells is not None:
        assert _same(cells, res["cells"]), what + ": cell histograms"
    err = float(np.abs(desc - res["desc"][:n]).max()) if n else 0.0
    print("%s: %d descriptors, max element difference %.3g, bit-identical %s" % (what, n, err, _same(desc, res["desc"][:n])))
    assert desc.shape == res["desc"][:n].shape and np.isfinite(desc).all(), what
    assert err <= DESC_TOL, (what, err)


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _device_run(dev, frames, name, cap=None, with_cells=True):
    """-> (desc, xy, count, cells or None) as numpy"""
    ops, torch = dev
    alg = CASES[name][0]
    t = frames if torch.is_tensor(frames) else torch.from_numpy(np.array(frames)).cuda()
    cells = None
    if alg == "sift":
        out = ops.denseSift(t, _mirror_config(name), cap)
    else:
        bins, ppc = CASES[name][5][:2]
        if alg == "fast" and with_cells:
            cells = vl.sentinel_buffer(t.shape[0] * (t.shape[1] // ppc) * (t.shape[2] // ppc) * bins, torch.float32, t.device).reshape(t.shape[0], t.shape[1] // ppc, t.shape[2] // ppc, bins)
        out = ops.denseHog(t, _mirror_config(name), cap, cells)
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in out] + [None if cells is None else cells.cpu().numpy()]


NAMES = sorted(n for n in CASES if not n.endswith(("-s6", "-s7")))


@pytest.mark.parametrize("name", NAMES)
def test_descriptors_equal_the_reference(dev, name):
    ops, torch = dev
    alg, W, H, kind, seed, cfg = CASES[name]
    res, st = _check_preconditions(name)
    ops.ctx.profileReset()
    ops.ctx.profile(True)
    try:
        desc, xy, count, cells = _device_run(dev, _image(W, H, kind, seed)[None], name)
        launches = ops.ctx.profileReport()
    finally:
        ops.ctx.profile(False)
    n = len(res["desc"])
    assert count.tolist() == [n] and desc.shape == (1, n, res["desc"].shape[1])
    _assert_result(desc[0], xy[0], res, name, cells=None if cells is None else cells[0])
    if kind == "const":
        assert not desc.any()
    if n:
        kernels = {"fast": ("k_dense_hog_cells", "k_dense_hog_blocks"), "std": ("k_dense_hog_pixels", "k_dense_hog_std"),
                   "sift": ("k_dense_sift_pixels", "k_dense_sift_generic" if cfg[:3] != (4, 4, 8) else "k_dense_sift")}[alg]
        assert all(launches.get(k, {"launches": 0})["launches"] == 1 for k in kernels), launches
    if alg == "fast" and n:   # without the cell output the histograms live in scratch: the same descriptors
        desc2, xy2, count2, _ = _device_run(dev, _image(W, H, kind, seed)[None], name, with_cells=False)
        assert _same(desc2, desc) and _same(xy2, xy) and count2.tolist() == [n]


@pytest.mark.parametrize("alg", ["fast", "std", "sift"])
def test_batch_of_three_frames(dev, alg):
    """three different frames in one call: per-frame offsets"""
    names = [alg + "-64x48", alg + "-s6", alg + "-s7"] if alg != "sift" else ["sift-40x33", "sift-s6", "sift-s7"]
    refs = [_check_preconditions(n)[0] for n in names]
    desc, xy, count, cells = _device_run(dev, np.stack([_image(*CASES[n][1:5]) for n in names]), names[0])
    assert count.tolist() == [len(refs[0]["desc"])] * 3
    for b, n in enumerate(names):
        _assert_result(desc[b], xy[b], refs[b], "%s frame %d" % (alg, b), cells=None if cells is None else cells[b])
    assert not _same(desc[0], desc[1])


@pytest.mark.parametrize("layout", [l for l in vl.LAYOUTS if l != "dense"])
@pytest.mark.parametrize("name", ["fast-61x45", "fast-u8", "std-61x45", "std-u8", "sift-periods", "sift-u8"])
def test_strided_input_views(dev, name, layout):
    """two frames as a strided window into a sentinel-filled parent (float32: a NaN pattern): a read outside the window would show in the result"""
    ops, torch = dev
    alg, W, H, kind, seed, cfg = CASES[name]
    res, _ = _check_preconditions(name)
    img = _image(W, H, kind, seed)
    dtype = torch.uint8 if img.dtype == np.uint8 else torch.float32
    parent, view = vl.make_view(layout, 2, H, W, dtype, "cuda")
    view.copy_(torch.from_numpy(np.stack([img, img[::-1].copy()])).cuda())
    before = vl.snapshot(parent)
    desc, xy, count, cells = _device_run(dev, view, name)
    assert vl.bits(parent).equal(before)
    _assert_result(desc[0], xy[0], res, "%s %s" % (name, layout), cells=None if cells is None else cells[0])
    assert count.tolist() == [len(res["desc"])] * 2 and not _same(desc[0], desc[1])


def _raw_call(ops, name, p_src, geom, desc, xy, count, cap, cells=None):
    alg, W, H, kind, seed, cfg = CASES[name]
    u8 = kind == "noise-u8"
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    if alg == "sift":
        fn = ops.L.bhip_dense_sift_dev_u8 if u8 else ops.L.bhip_dense_sift_dev_f32
        return fn(ops.ctx._h, *cfg, p_src, *geom, p(desc), p(xy), p(count), cap)
    fn = ops.L.bhip_dense_hog_dev_u8 if u8 else ops.L.bhip_dense_hog_dev_f32
    return fn(ops.ctx._h, *cfg, int(alg == "fast"), p_src, *geom, p(desc), p(xy), p(count), cap, p(cells))


@pytest.mark.parametrize("name", ["fast-64x48", "std-64x48", "sift-64x48-p3"])
def test_small_cap_counts_everything_and_writes_only_its_records(dev, name):
    """cap = 5: the count is the full number, the first 5 records are right, the memory behind them keeps its guard value; cap 0: only the count"""
    ops, torch = dev
    alg, W, H, kind, seed, cfg = CASES[name]
    res, _ = _check_preconditions(name)
    n, cap, extra, dof = len(res["desc"]), 5, 16, res["desc"].shape[1]
    assert n > 2 * cap
    src = torch.from_numpy(np.stack([_image(W, H, kind, seed)] * 2)).cuda()
    desc = torch.full((2 * cap + extra, dof), -5.0, dtype=torch.float64, device="cuda")
    xy = torch.full((2 * cap + extra, 2), -7, dtype=torch.int32, device="cuda")
    count = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    assert _raw_call(ops, name, C.c_void_p(src.data_ptr()), (W * H, W, W, H, 2), desc, xy, count[1:], cap) == 0
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [-9, n, n, -9]
    for b in range(2):
        _assert_result(desc.cpu().numpy()[b * cap:(b + 1) * cap], xy.cpu().numpy()[b * cap:(b + 1) * cap], res, "%s cap 5 frame %d" % (name, b), cap)
    assert (desc[2 * cap:] == -5).all() and (xy[2 * cap:] == -7).all()
    count.fill_(-9)
    assert _raw_call(ops, name, C.c_void_p(src.data_ptr()), (W * H, W, W, H, 2), None, None, count[1:], 0) == 0
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [-9, n, n, -9]


def test_a_single_column_of_windows_is_refused(dev):
    """24 x 40 with period 6: numX = (int)((24 - 16) / 6) = 1 and numY = 4: the reference divides by numX - 1"""
    ops, torch = dev
    from boofcv_amd import _lib
    from boofcv_amd.api.core import IllegalArgumentException
    src = torch.zeros((1, 40, 24), dtype=torch.float32, device="cuda")
    count = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    p = lambda v: C.c_void_p(v.data_ptr())
    assert ops.L.bhip_dense_sift_dev_f32(ops.ctx._h, *SIFT_DEFAULT, p(src), 40 * 24, 24, 24, 40, 1, None, None, p(count), 0) == _lib.BHIP_ERR_INVALID
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [-9]
    with pytest.raises(IllegalArgumentException):
        ops.denseSift(src)
    with pytest.raises(ZeroDivisionError):
        dr.DenseSift().layout(24, 40)


@pytest.mark.parametrize("name", ["fast-61x45", "fast-u8", "fast-small", "std-odd-cell", "std-u8", "sift-periods", "sift-u8", "sift-one-window"])
def test_host_forms_and_mirror_classes(dev, name):
    """bhip_dense_*_f32 / _u8 through the mirror's factory, on a sub-image (start index and stride): the same bits as the device call, and the methods
    of DescribeImageDense"""
    ops, torch = dev
    from boofcv_amd import dense
    from boofcv_amd.api.image import GrayF32, GrayU8, TupleDesc_F64
    alg, W, H, kind, seed, cfg = CASES[name]
    res, _ = _check_preconditions(name)
    img = _image(W, H, kind, seed)
    desc, xy, count, cells = _device_run(dev, img[None], name)
    T = GrayU8 if img.dtype == np.uint8 else GrayF32
    big = np.full((H + 5, W + 7), 99, img.dtype)
    big[2:2 + H, 3:3 + W] = img
    view = T.wrap(big).subimage(3, 2, 3 + W, 2 + H)
    F = dense.FactoryDescribeImageDense
    d = (F.sift if alg == "sift" else F.hog)(_mirror_config(name), T, ctx=ops.ctx)
    d.process(view)
    n = len(res["desc"])
    assert _same(d.descriptors, desc[0]) and d.descriptors.shape == (n, res["desc"].shape[1])
    _assert_result(d.descriptors, d.topLeft if alg != "sift" else d.locations, res, name + " mirror")
    assert d.getImageType() is T and d.getDescriptionType() is TupleDesc_F64 and d.createDescription().size() == res["desc"].shape[1]
    locs, descs = d.getLocations(), d.getDescriptions()
    assert len(locs) == len(descs) == n
    if alg != "sift":   # DescribeImageDenseHoG.process centres the regions
        rx, ry = cfg[1] * cfg[2] // 2, cfg[1] * cfg[3] // 2
        assert [(p.x, p.y) for p in locs] == [(int(x) + rx, int(y) + ry) for x, y in res["xy"]]
    else:
        assert [(p.x, p.y) for p in locs] == [(int(x), int(y)) for x, y in res["xy"]]
    if n:
        assert _same(descs[n - 1].value, desc[0, n - 1])
    if alg == "fast":
        assert (d.getCellRows(), d.getCellCols()) == res["cells"].shape[:2]
        if n:
            assert _same(d._cells, cells[0])
            r, c = res["cells"].shape[0] - 1, res["cells"].shape[1] - 1
            assert _same(d.getCell(r, c).histogram, res["cells"][r, c])
            # the first one or two rows of blocks: the reference's index y * cellCols + x leaves the list of numX-wide rows further down
            region = (cfg[1], 0, W - 1, 4 * cfg[1] - 1)
            out = []
            d.getDescriptorsInRegion(*region, out)
            want = _ref_alg(name).descriptors_in_region(n, res["cells"].shape[1], *region)
            assert len(out) == len(want) > 0 and all(_same(o.value, desc[0, k]) for o, k in zip(out, want))
