"""The Hough line detectors on the GPU against tests/hough_ref.py, exactly: the stages through DeviceImageOps (prewitt, intensity on int16
derivatives, edgeNonMaxCrude4, houghBinaryPolar, houghGradientFoot, nonmaxRelaxed, meanShiftPeak), the whole detectors through
boofcv_amd.lines.FactoryDetectLine, and the refusals.

Shapes and inputs: tests/hough_cases.py (61x47, 64x32, 2x3, 3x2, 130x70; batches of 3 with different content).  Inputs are windows of larger
tensors (row and image strides beyond the width, a non-zero offset), outputs are views inside sentinel-filled parents (tests/view_layouts.py), so
a store outside a view is found.  Float results are compared by their bits; NaN cells (a zero gradient gives 0/0) must be NaN in the same
places -- the sign and payload of a NaN are the platform's, in Java as well."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hough_cases as HC
import hough_ref as R
import threshold_ref
import view_layouts as VL
from boofcv_amd import _lib, device, lines
from boofcv_amd.api import GrayF32, GrayS32, GrayU8, IllegalArgumentException

pytestmark = pytest.mark.gpu
F = np.float32
SIZE_IDS = ["%dx%d" % s for s in HC.SIZES]
TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}


@pytest.fixture(scope="module")
def ops():
    return device.DeviceImageOps()


def _window(frames, dev, layout="odd", shift=0):
    """the frames [B,H,W] as a strided window at a non-zero offset of a larger device tensor"""
    B, H, W = frames.shape
    _, view = VL.make_view(layout, B, H, W, TORCH[frames.dtype], dev, shift)
    view.copy_(torch.from_numpy(np.array(frames)).to(dev))
    return view


def _out(ops, layout, B, H, W, dtype=torch.float32, shift=0):
    parent, view = VL.make_view(layout, B, H, W, dtype, ops.device, shift)
    return parent, view, VL.snapshot(parent)


def _same_bits(got, exp, what):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if got.dtype == np.float32:
        nan_g, nan_e = np.isnan(got), np.isnan(exp)
        bad = (nan_g != nan_e) | (~nan_e & (got.view(np.int32) != exp.view(np.int32)))
    else:
        bad = got != exp
    idx = np.argwhere(bad)
    assert idx.size == 0, "%s: %d elements differ, first %s: got %r want %r" % (what, len(idx), idx[0], got[tuple(idx[0])], exp[tuple(idx[0])])


# ---------------- Prewitt ----------------
@functools.lru_cache(maxsize=None)
def _prewitt_ref(w, h, dtype, border):
    frames = HC.gray_frames(w, h, dtype)
    pairs = [R.prewitt(f, border) for f in frames]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.mark.parametrize("layout", ("pad4", "odd"))
@pytest.mark.parametrize("border", (None, 0, "EXTENDED"))
@pytest.mark.parametrize("dtype", ("u8", "f32"))
@pytest.mark.parametrize("size", HC.SIZES, ids=SIZE_IDS)
def test_prewitt(ops, size, dtype, border, layout):
    w, h = size
    frames = HC.gray_frames(w, h, dtype)
    want_x, want_y = _prewitt_ref(w, h, dtype, {None: 0, 0: 1, "EXTENDED": 2}[border])
    src = _window(frames, ops.device, layout)
    dt = torch.int16 if dtype == "u8" else torch.float32
    px, dx, bx = _out(ops, layout, 3, h, w, dt)
    py, dy, by = _out(ops, layout, 3, h, w, dt)
    rx, ry = ops.prewitt(src, border, dx, dy)
    assert rx is dx and ry is dy
    torch.cuda.synchronize()
    VL.assert_only_view_written(px, dx, bx, "derivX")
    VL.assert_only_view_written(py, dy, by, "derivY")
    inner = np.zeros((h, w), bool)
    inner[1:-1, 1:-1] = True
    sel = inner if border is None else np.ones((h, w), bool)
    _same_bits(dx.cpu().numpy()[:, sel], want_x[:, sel], "derivX")
    _same_bits(dy.cpu().numpy()[:, sel], want_y[:, sel], "derivY")
    if border is None:   # the frame keeps what the caller had there
        VL.assert_kept(dx, ~inner, "derivX frame")
        VL.assert_kept(dy, ~inner, "derivY frame")


# ---------------- intensityAbs on GrayS16, crude suppression ----------------
@functools.lru_cache(maxsize=None)
def _derivs(w, h, dtype):
    """derivatives with zeros (the step is -1 there) and a noise intensity with ties and zeros"""
    rng = np.random.RandomState(600 + 10 * w + h)
    if dtype == "s16":
        dx, dy = (rng.randint(-3, 4, (3, h, w)) * rng.randint(0, 11000, (3, h, w))).astype(np.int16), rng.randint(-32768, 32768, (3, h, w)).astype(np.int16)
        dx[0].flat[0], dy[0].flat[0] = -32768, -32768
    else:
        dx, dy = ((rng.rand(3, h, w) - 0.5) * rng.randint(0, 3, (3, h, w))).astype(F), (rng.rand(3, h, w) - 0.5).astype(F)
        dy[1].flat[-1] = np.nan
    inten = rng.randint(0, 6, (3, h, w)).astype(F) * F(0.5)
    for a in (dx, dy, inten):
        a.setflags(write=False)
    return dx, dy, inten


@pytest.mark.parametrize("size", HC.SIZES, ids=SIZE_IDS)
def test_intensity_abs_s16(ops, size):
    w, h = size
    dx, dy, _ = _derivs(w, h, "s16")
    want = np.stack([R.intensity_abs(dx[b], dy[b]) for b in range(3)])
    assert want.max() == 65536.0   # |Short.MIN_VALUE| twice: the sum is formed in int
    parent, out, before = _out(ops, "odd", 3, h, w)
    ops.intensity(device.INTENSITY_ABS, _window(dx, ops.device, "pad4_x1"), _window(dy, ops.device, "pad4_x1"), out)
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before)
    _same_bits(out.cpu().numpy(), want, "intensityAbs")
    with pytest.raises(IllegalArgumentException):
        ops.intensity(device.INTENSITY_E, _window(dx, ops.device), _window(dy, ops.device))


@pytest.mark.parametrize("dtype", ("f32", "s16"))
@pytest.mark.parametrize("size", HC.SIZES, ids=SIZE_IDS)
def test_edge_nonmax_crude4(ops, size, dtype):
    w, h = size
    dx, dy, inten = _derivs(w, h, dtype)
    want = np.stack([R.nonmax_crude4(inten[b], dx[b], dy[b]) for b in range(3)])
    parent, out, before = _out(ops, "pad4_x1", 3, h, w)
    res = ops.edgeNonMaxCrude4(_window(inten, ops.device, "pad4"), _window(dx, ops.device, "odd"), _window(dy, ops.device, "odd"), out)
    assert res is out
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before)
    _same_bits(out.cpu().numpy(), want, "nonMaxSuppressionCrude4")
    for edge in (np.s_[:, 0, :], np.s_[:, -1, :], np.s_[:, :, 0], np.s_[:, :, -1]):   # rows and columns 0 and last, named
        _same_bits(out.cpu().numpy()[edge], want[edge], "frame")


# ---------------- binary vote ----------------
@functools.lru_cache(maxsize=None)
def _binary_ref(w, h, angles, res):
    par = R.Polar(res, angles)
    return np.stack([R.hough_binary(f, par) for f in HC.binary_frames(w, h)]), par


@pytest.mark.parametrize("res", (2.0, 0.5))
@pytest.mark.parametrize("angles", (180, 7))
@pytest.mark.parametrize("size", HC.SIZES, ids=SIZE_IDS)
def test_binary_vote(ops, size, angles, res):
    w, h = size
    want, par = _binary_ref(w, h, angles, res)
    bins, r_max = ops.houghPolarBins(w, h, res)
    assert (bins, F(r_max)) == (par.num_bins_range, par.r_max) and want.shape == (3, angles, bins)
    parent, out, before = _out(ops, "odd", 3, angles, bins)
    res_ = ops.houghBinaryPolar(_window(HC.binary_frames(w, h), ops.device), res, angles, par.c, par.s, out)
    assert res_ is out
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before)
    _same_bits(out.cpu().numpy(), want, "transform")
    # the default tables are the reference's
    _same_bits(ops.houghBinaryPolar(_window(HC.binary_frames(w, h), ops.device), res, angles).cpu().numpy(), want, "transform, default tables")


def test_binary_vote_wraps_into_the_next_row(ops):
    """an even numBinsRange and a pixel at distance r_max from the origin: col == numBinsRange is the first cell of the next row, and in the
    last row it is dropped"""
    par = R.Polar(0.5, 4)                     # 8x6: origin (4, 3), r_max = 5, numBinsRange = 10, w2 = 5
    binary = np.zeros((6, 8), np.uint8)
    binary[0, 0] = 1                          # (-4, -3): p = -4c - 3s
    par.initialize(8, 6)
    assert (par.num_bins_range, float(par.r_max)) == (10, 5.0)
    par.c, par.s = np.array([-0.8, 0.8, -0.8, -0.8], F), np.array([-0.6, 0.6, -0.6, -0.6], F)   # rows 0, 2, 3: p = r_max exactly; row 1: -r_max
    t = R.hough_binary(binary, par)
    assert t.sum() == 3 and t[1, 0] == 2 and t[3, 0] == 1      # row 0 -> (1, 0); row 1 -> col 0; row 2 -> (3, 0); row 3: past the end, dropped
    got = ops.houghBinaryPolar(torch.from_numpy(binary).to(ops.device).unsqueeze(0), 0.5, 4, par.c, par.s).cpu().numpy()[0]
    _same_bits(got, t, "wrap")


# ---------------- gradient vote ----------------
@functools.lru_cache(maxsize=None)
def _gradient_ref(case, w, h):
    dx, dy, binary = HC.gradient_case(case, w, h)
    return np.stack([R.hough_gradient(dx[b], dy[b], binary[b], R.FootOfNorm(5)) for b in range(3)])


@pytest.mark.parametrize("case", HC.GRADIENT_CASES)
@pytest.mark.parametrize("size", HC.SIZES, ids=SIZE_IDS)
def test_gradient_vote(ops, size, case):
    w, h = size
    dx, dy, binary = HC.gradient_case(case, w, h)
    want = _gradient_ref(case, w, h)
    parent, out, before = _out(ops, "pad4_x1", 3, h, w)
    res, n = ops.houghGradientFoot(_window(dx, ops.device, "odd"), _window(dy, ops.device, "odd"), _window(binary, ops.device, "pad4_x1"), out)
    assert res is out
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before)
    assert n.cpu().numpy().tolist() == [int(np.count_nonzero(binary[b])) for b in range(3)]
    _same_bits(out.cpu().numpy(), want, "transform")


def test_gradient_vote_with_a_cap(ops):
    """only the first `cap` edge pixels (raster order) vote; the count still is the number of edge pixels"""
    w, h = 61, 47
    dx, dy, binary = HC.gradient_case("noise100", w, h)
    cap = 1000
    want = []
    for b in range(3):
        cut = np.array(binary[b])
        cut.reshape(-1)[np.flatnonzero(cut.reshape(-1))[cap:]] = 0
        want.append(R.hough_gradient(dx[b], dy[b], cut, R.FootOfNorm(5)))
    got, n = ops.houghGradientFoot(_window(dx, ops.device), _window(dy, ops.device), _window(binary, ops.device), cap=cap)
    assert n.cpu().numpy().tolist() == [w * h] * 3
    _same_bits(got.cpu().numpy(), np.stack(want), "transform")


def test_gradient_vote_takes_sobel_derivatives(ops):
    """the stage has its own entry point: any derivatives of the right type do"""
    w, h = 61, 47
    img = torch.from_numpy(np.array(HC.gray_frames(w, h, "u8"))).to(ops.device)
    dx, dy = ops.sobel(img, "EXTENDED")
    binary = (ops.intensity(device.INTENSITY_ABS, dx, dy) > 900).to(torch.uint8)
    got, n = ops.houghGradientFoot(dx, dy, binary)
    hx, hy, hb = dx.cpu().numpy(), dy.cpu().numpy(), binary.cpu().numpy()
    assert 0 < int(n[0]) < w * h
    _same_bits(got.cpu().numpy(), np.stack([R.hough_gradient(hx[b], hy[b], hb[b], R.FootOfNorm(5)) for b in range(3)]), "transform")


# ---------------- relaxed NMS ----------------
@pytest.mark.parametrize("radius", (1, 2, 3))
@pytest.mark.parametrize("size", ((61, 47), (130, 70)), ids=("61x47", "130x70"))
def test_nonmax_relaxed_on_binary_transforms(ops, size, radius):
    w, h = size
    transforms, _ = _binary_ref(w, h, 180, 2.0)
    threshold = F(max(0.001 * transforms[0].size, 1.0))
    want = [R.nonmax_relaxed(t, radius, threshold) for t in transforms]
    xy, n = ops.nonmaxRelaxed(_window(transforms, ops.device), radius, threshold)
    torch.cuda.synchronize()
    assert n.cpu().numpy().tolist() == [len(v) for v in want] and min(len(v) for v in want) > 0
    for b in range(3):
        assert np.array_equal(xy[b, :len(want[b])].cpu().numpy(), want[b]), "image %d: the list or its order differs" % b
    # the host-buffer form
    t = GrayF32.wrap(transforms[1])
    out, count = np.zeros((len(want[1]) + 3, 2), np.int16), C.c_int()
    ctx = ops.ctx
    st = _lib.load().bhip_nonmax_block_relaxed_f32(ctx._h, *t._in(), radius, float(threshold), 0, out.ctypes.data_as(_lib._i16p), len(out), C.byref(count))
    assert st == 0 and count.value == len(want[1]) and np.array_equal(out[:count.value], want[1])


@pytest.mark.parametrize("radius", (1, 2, 3))
def test_nonmax_relaxed_plateau_and_cap(ops, radius):
    """all cells equal to the threshold: every cell is reported, block by block; with a cap below the count the count is still exact and only
    cap pairs are written"""
    w, h = 13, 9
    img = np.full((2, h, w), F(2.5))
    img[1, 4, 6] = R.FLOAT_MAX      # its block reports nothing and its window rejects its neighbours
    noise = np.random.RandomState(3).randint(0, 3, (1, h, w)).astype(F)
    want = [R.nonmax_relaxed(img[0], radius, 2.5), R.nonmax_relaxed(img[1], radius, 2.5), R.nonmax_relaxed(noise[0], radius, 1.0, 1)]
    assert len(want[0]) == w * h
    xy, n = ops.nonmaxRelaxed(_window(img, ops.device), radius, 2.5)
    assert n.cpu().numpy().tolist() == [w * h, len(want[1])]
    assert np.array_equal(xy[0].cpu().numpy(), want[0]) and np.array_equal(xy[1, :len(want[1])].cpu().numpy(), want[1])
    xy2, n2 = ops.nonmaxRelaxed(_window(noise, ops.device), radius, 1.0, border=1)
    assert int(n2[0]) == len(want[2]) > 0 and np.array_equal(xy2[0, :len(want[2])].cpu().numpy(), want[2])
    cap = 10
    lists = torch.full((2 * cap * 2 + 8,), -7, dtype=torch.int16, device=ops.device)   # two lists of cap pairs, then a guard
    counts = torch.zeros(2, dtype=torch.int32, device=ops.device)
    ip, iis, irs, W, H, B = device._geom(_window(img, ops.device))
    st = ops.L.bhip_nonmax_block_relaxed_dev_f32(ops.ctx._h, ip, iis, irs, W, H, B, radius, 2.5, 0, C.c_void_p(lists.data_ptr()), cap, C.c_void_p(counts.data_ptr()))
    torch.cuda.synchronize()
    assert st == 0 and counts.cpu().numpy().tolist() == [w * h, len(want[1])]
    got = lists.cpu().numpy()
    assert np.array_equal(got[:2 * cap * 2].reshape(2, cap, 2), np.stack([want[0][:cap], want[1][:cap]])) and (got[2 * cap * 2:] == -7).all()


# ---------------- mean shift ----------------
def test_mean_shift_peak(ops):
    """peaks in the interior, on the frame where isInFastBounds fails, and on an all-zero neighbourhood (total == 0)"""
    w, h = 40, 30
    rng = np.random.RandomState(12)
    img = (rng.rand(3, h, w) * 5).astype(F)
    img[:, 10:22, 24:36] = 0                      # (30, 16): nothing within radius 3
    img[0, 8, 8] = 40
    img[1] = _gradient_ref("noise100", 61, 47)[0][:h, :w]
    pts = [(8, 8), (20, 15), (12, 22), (0, 0), (1, 1), (39, 29), (38, 28), (37, 2), (3, 26), (2, 14), (36, 27), (30, 16), (39, 0)]
    xy = np.tile(np.array(pts, np.int16), (3, 1, 1))
    counts = np.array([len(pts), len(pts) - 2, 5], np.int32)
    for radius in (3, 1):
        refs = [R.MeanShiftPeak(img[b], radius) for b in range(3)]
        peak, inten = ops.meanShiftPeak(_window(img, ops.device), torch.from_numpy(xy).to(ops.device), torch.from_numpy(counts).to(ops.device), radius=radius)
        torch.cuda.synchronize()
        peak, inten = peak.cpu().numpy(), inten.cpu().numpy()
        for b in range(3):
            want = np.array([refs[b].search(x, y) for x, y in pts[:counts[b]]], F)
            _same_bits(peak[b, :counts[b]], want, "peaks of image %d, radius %d" % (b, radius))
            _same_bits(inten[b, :counts[b]], np.array([img[b, y, x] for x, y in pts[:counts[b]]], F), "intensity")
        moved = np.abs(peak[0, :len(pts)] - xy[0]).max(axis=1)
        assert moved[0] > 0 and moved[3] > 0 and moved[11] == 0      # interior and frame peaks move, the one on zeros stays
    peak, inten = ops.meanShiftPeak(_window(img, ops.device), torch.from_numpy(xy).to(ops.device), None, radius=0)   # no refinement, no counts
    assert np.array_equal(peak.cpu().numpy(), xy.astype(F)) and inten[2, 0].item() == img[2, 8, 8]


# ---------------- whole detectors ----------------
def _lines_equal(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        _same_bits(np.array([g.p.x, g.p.y, g.slope.x, g.slope.y], F), np.array(w, F), "line %d" % i)


@pytest.mark.parametrize("max_lines", (0, 10))
def test_detector_binary_polar(ops, max_lines):
    img = HC.scene("dark")
    want = R.detect_binary(img, max_lines=max_lines)
    det = lines.FactoryDetectLine.houghLinePolar(lines.ConfigHoughBinary(max_lines), None, None, GrayU8, ops=ops)
    got = det.detect(GrayU8.wrap(img))
    assert 3 <= len(want) and (max_lines == 0 or len(want) <= max_lines)
    _lines_equal(got, want)
    _same_bits(det.getBinary().array(), threshold_ref.global_otsu(img, 1.0, True), "binary")
    if max_lines:   # the three drawn lines are found: y = 30, x = 45, 0.6 x + 0.8 y = 70
        def off(l, a, b, c):
            return abs(a * float(l.p.x) + b * float(l.p.y) + c) < 4.0 and abs(a * float(l.slope.x) + b * float(l.slope.y)) < 0.05   # two range bins, three angle bins
        for a, b, c in ((0.0, 1.0, -30.0), (1.0, 0.0, -45.0), (0.6, 0.8, -70.0)):
            assert any(off(l, a, b, c) for l in got), (a, b, c)


@pytest.mark.parametrize("max_lines", (0, 10))
@pytest.mark.parametrize("kind", ("bars_u8", "bars_f32"))
def test_detector_gradient_foot(ops, kind, max_lines):
    img = HC.scene(kind)
    want = R.detect_gradient(img, max_lines=max_lines)
    cls = GrayU8 if kind == "bars_u8" else GrayF32
    det = lines.FactoryDetectLine.houghLineFoot(lines.ConfigHoughGradient(max_lines), None, cls, ops=ops)
    got = det.detect(cls.wrap(img))
    assert len(want) >= 3
    _lines_equal(got, want)


# ---------------- refusals: nothing is written ----------------
def test_refusals_leave_the_outputs_untouched(ops):
    L, h = ops.L, ops.ctx._h
    dev = ops.device
    # houghLinePolar(ConfigHoughGradient, ...), houghLineFootSub, lineRansac, GrayS32 derivatives, Planar images
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.houghLinePolar(lines.ConfigHoughGradient(), lines.ConfigParamPolar(), GrayU8)
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.houghLineFootSub(None, GrayU8)
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.lineRansac(None, GrayU8)
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.houghLineFoot(None, None, GrayS32)
    from boofcv_amd.api import Planar
    with pytest.raises(IllegalArgumentException):
        lines.FactoryDetectLine.houghLineFoot(None, None, Planar)
    out = torch.full((1, 8, 8), -3.0, device=dev)
    counts = torch.full((1,), -3, dtype=torch.int32, device=dev)
    s32 = torch.zeros((1, 8, 8), dtype=torch.int32, device=dev)
    with pytest.raises(IllegalArgumentException):
        ops.houghGradientFoot(s32, s32, torch.ones((1, 8, 8), dtype=torch.uint8, device=dev), out, counts=counts)
    with pytest.raises(IllegalArgumentException):
        ops.edgeNonMaxCrude4(out, s32, s32, torch.empty_like(out))
    # width * height > 2^24: BHIP_ERR_UNSUPPORTED before anything is queued
    big = torch.zeros((1, 4097, 4096), dtype=torch.uint8, device=dev)
    bins, _ = ops.houghPolarBins(4096, 4097, 2.0)
    t = torch.full((1, 4, bins), -3.0, device=dev)
    table = np.zeros(4, F).ctypes.data_as(_lib._fp)
    st = L.bhip_hough_binary_polar_dev_u8(h, C.c_void_p(big.data_ptr()), 4097 * 4096, 4096, 4096, 4097, 1, 2.0, 4, table, table, C.c_void_p(t.data_ptr()), 4 * bins, bins,
                                          bins, 4)
    assert st == _lib.BHIP_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError):
        ops.houghBinaryPolar(big)
    # numBinsRange == 0 (a 1x1 image: r_max = 0): BHIP_ERR_INVALID
    assert ops.houghPolarBins(1, 1, 2.0)[0] == 0
    one = torch.ones((1, 1, 1), dtype=torch.uint8, device=dev)
    st = L.bhip_hough_binary_polar_dev_u8(h, C.c_void_p(one.data_ptr()), 1, 1, 1, 1, 1, 2.0, 4, table, table, C.c_void_p(t.data_ptr()), 4 * bins, bins, bins, 4)
    assert st == _lib.BHIP_ERR_INVALID
    with pytest.raises(IllegalArgumentException):
        ops.houghBinaryPolar(one)
    with pytest.raises(IllegalArgumentException):   # a transform view of another size
        ops.houghBinaryPolar(torch.ones((1, 8, 8), dtype=torch.uint8, device=dev), 2.0, 4, out=out)
    # a Prewitt border policy that does not exist, a relaxed radius of 0, overlapping crude suppression
    st = L.bhip_prewitt_dev_f32(h, C.c_void_p(out.data_ptr()), 64, 8, 8, 8, 1, C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), 64, 8, 3)
    assert st == _lib.BHIP_ERR_UNSUPPORTED
    xy = torch.full((1, 4, 2), -3, dtype=torch.int16, device=dev)
    st = L.bhip_nonmax_block_relaxed_dev_f32(h, C.c_void_p(out.data_ptr()), 64, 8, 8, 8, 1, 0, 1.0, 0, C.c_void_p(xy.data_ptr()), 4, C.c_void_p(counts.data_ptr()))
    assert st == _lib.BHIP_ERR_INVALID
    with pytest.raises(IllegalArgumentException):
        ops.edgeNonMaxCrude4(out, out, out, out)
    torch.cuda.synchronize()
    assert (out == -3).all() and (t == -3).all() and (counts == -3).all() and (xy == -3).all()
