"""EnhanceImageOps on the GPU against tests/enhance_ref.py, bit for bit: DeviceImageOps.histogram / equalizeTable / applyTransform /
equalizeLocal / sharpen, the host-view forms through boofcv_amd.enhance, and the refusals.  tests/test_enhance_reference.py shows on the CPU
that the one-rule forms used as the expectation here (rank_local, sharpen_rule) equal the reference's loops.

The shapes are where the kernels can go wrong, not what the workload looks like (enhance.hip): the direct equalizeLocal kernel owns 64 x 16
tiles and reads its windows as aligned 32-bit words out of an LDS tile with a halo, inner tiles in a launch of their own; the sliding kernel
gives a wave a run of 128 pixels of a row and stores 64 answers at a time; the streaming kernels give a lane 16 pixels of a row, sharpen four.
  15x20            the reference's own test image size
  70x37, 131x67    cross the tile and the run boundaries in both directions with a ragged last tile (131: two runs, 67: five tile rows)
  64x64            exact tiles
  9x40, 40x9       one side below 2r+1 (the reference's naive branch);  5x4  both below (its whole-image branch)
Radii 0, 1, 2, 3, 7, 8, 16, 17, 33 as far as the size tells them apart; 8 is the first radius whose window (289 pixels) is beyond a byte
counter, which the all-255 / all-0 / checkerboard frames drive to its maximum.
Every device output is a strided view inside a sentinel-filled parent (tests/view_layouts.py), every device input a window of a larger tensor."""
import functools

import numpy as np
import pytest
import torch

import enhance_ref as R
import view_layouts as VL
from boofcv_amd import _lib, api, device, enhance

pytestmark = pytest.mark.gpu
SIZES = ((15, 20), (70, 37), (131, 67), (64, 64), (9, 40), (40, 9), (5, 4))   # (width, height)
RADII = (0, 1, 2, 3, 7, 8, 16, 17, 33)
PATHS = ("direct", "sliding", "auto")
LAYOUTS = ("odd", "pad4_x1", "dense", "pad4", "pad4_x4")
SHARPEN_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (2, 9), (3, 3), (70, 37))


@pytest.fixture(scope="module")
def ops():
    return device.DeviceImageOps()


def _radii(w, h):
    """the radii that differ on a w x h image: once a window covers the whole image a larger radius gives the same result"""
    out = []
    for r in RADII:
        out.append(r)
        if 2 * r + 1 >= max(w, h):
            break
    return out


@functools.lru_cache(maxsize=None)
def _noise(w, h, levels):
    """[3,H,W]: three different frames of uniform noise in 0 .. levels-1"""
    f = np.random.RandomState(1000 * w + h + levels).randint(0, levels, (3, h, w)).astype(np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _ties(w, h):
    """[3,H,W]: all 255, all 0, a two-level checkerboard -- ties dominate and a window's count reaches its area"""
    board = np.where(np.indices((h, w)).sum(0) % 2 == 0, 40, 200).astype(np.uint8)
    f = np.stack([np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8), board])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _expected(kind, w, h, radius, length):
    frames = _ties(w, h) if kind == "ties" else _noise(w, h, 256 if length == 256 else 10)
    return np.stack([R.rank_local(f, radius, length) for f in frames])


def _window(frames, device_, pad=(3, 2, 5), fill=77):
    """the frames [B,H,W] as a window of a larger device tensor at an odd offset"""
    frames = np.asarray(frames)
    B, H, W = frames.shape
    top, left, right = pad
    t = torch.from_numpy(np.array(frames))
    parent = torch.full((B, H + top + 1, W + left + right), fill, dtype=t.dtype, device=device_)
    view = parent[:, top:top + H, left:left + W]
    view.copy_(t.to(device_))
    return view


def _run(ops, call, frames, layout, dtype=torch.uint8):
    B, H, W = frames.shape
    src = _window(frames, ops.device)
    parent, out = VL.make_view(layout, B, H, W, dtype, ops.device)
    before = VL.snapshot(parent)
    res = call(ops, src, out)
    assert res is out
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before, layout)
    return out.cpu().numpy()


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, what
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d pixels differ, first index %s: got %s want %s" % (what, len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])])


# ---------------- equalizeLocal ----------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_equalize_local_noise(ops, size, path):
    w, h = size
    for length in (256, 10):
        frames = _noise(w, h, 256 if length == 256 else 10)
        for r in _radii(w, h):
            layout = LAYOUTS[(w + r + len(path)) % len(LAYOUTS)]
            got = _run(ops, lambda o, s, out: o.equalizeLocal(s, r, length, out=out, path=path), frames, layout)
            _same(got, _expected("noise", w, h, r, length), "%s %dx%d r=%d length=%d" % (path, w, h, r, length))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("size", ((15, 20), (70, 37), (64, 64), (9, 40), (5, 4)), ids=lambda s: "%dx%d" % s)
def test_equalize_local_ties(ops, size, path):
    w, h = size
    frames = _ties(w, h)
    for r in _radii(w, h):
        got = _run(ops, lambda o, s, out: o.equalizeLocal(s, r, 256, out=out, path=path), frames, LAYOUTS[(h + r) % len(LAYOUTS)])
        exp = _expected("ties", w, h, r, 256)
        _same(got, exp, "%s %dx%d r=%d" % (path, w, h, r))
        assert (exp[0] == 255).all() and (exp[1] == 255).all()   # a constant frame: every pixel is histogramLength - 1


def test_equalize_local_value_beyond_histogram_length_is_ranked(ops):
    """the documented deviation: the reference throws on a pixel >= histogramLength"""
    frames = _noise(70, 37, 256)
    for path in PATHS:
        got = _run(ops, lambda o, s, out: o.equalizeLocal(s, 3, 10, out=out, path=path), frames, "odd")
        _same(got, np.stack([R.rank_local(f, 3, 10) for f in frames]), path)


def test_equalize_local_radius_limits(ops):
    frames = _noise(70, 37, 256)
    whole = np.stack([R.rank_local(f, 255, 256) for f in frames])
    for path in PATHS:
        got = _run(ops, lambda o, s, out: o.equalizeLocal(s, 255, 256, out=out, path=path), frames, "pad4_x1")
        _same(got, whole, "r=255 " + path)
    src = _window(frames, ops.device)
    out = torch.zeros((3, 37, 70), dtype=torch.uint8, device=ops.device)
    with pytest.raises(api.IllegalArgumentException):
        ops.equalizeLocal(src, 256, out=out)
    for length in (0, 257):
        with pytest.raises(api.IllegalArgumentException):
            ops.equalizeLocal(src, 2, length, out=out)
    # the C entry refuses them too, and an overlap
    g = device._geom(src, torch.uint8)
    o = device._geom(out, torch.uint8)[:3]
    L = ops.L
    assert L.bhip_equalize_local_dev_u8(ops.ctx._h, *g, 256, 256, _lib.BHIP_EQLOCAL_AUTO, *o) == _lib.BHIP_ERR_UNSUPPORTED
    assert L.bhip_equalize_local_dev_u8(ops.ctx._h, *g, 2, 257, _lib.BHIP_EQLOCAL_AUTO, *o) == _lib.BHIP_ERR_INVALID
    assert L.bhip_equalize_local_dev_u8(ops.ctx._h, *g, -1, 256, _lib.BHIP_EQLOCAL_AUTO, *o) == _lib.BHIP_ERR_INVALID
    assert L.bhip_equalize_local_dev_u8(ops.ctx._h, *g, 2, 256, 3, *o) == _lib.BHIP_ERR_INVALID
    assert L.bhip_equalize_local_dev_u8(ops.ctx._h, *g, 2, 256, _lib.BHIP_EQLOCAL_AUTO, *g[:3]) == _lib.BHIP_ERR_INVALID
    torch.cuda.synchronize()
    assert not bool(out.any())
    # a forced direct form whose tile does not fit LDS is refused, the other two run it
    wide = torch.zeros((1, 300, 300), dtype=torch.uint8, device=ops.device)
    with pytest.raises(Exception) as e:
        ops.equalizeLocal(wide, 120, path="direct")
    assert "LDS" in str(e.value)


# ---------------- histogram -> table -> applyTransform ----------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_global_chain(ops, size):
    w, h = size
    for length, minValue in ((256, 0), (256, 3), (10, 0), (10, 3)):
        frames = _noise(w, h, 256 if length == 256 else 10)
        src = _window(frames, ops.device, (1, 5, 2))
        hist = ops.histogram(src, minValue, length)
        exp_hist = np.stack([R.histogram(f, minValue, length, drop=True) for f in frames])
        _same(hist.cpu().numpy(), exp_hist, "histogram %d %d" % (length, minValue))
        if not exp_hist.sum(1).all():
            continue   # 5x4 with minValue 3 may leave a frame without a counted pixel: the table of an empty histogram is the deviation below
        table = ops.equalizeTable(hist)
        exp_table = np.stack([R.equalize(e) for e in exp_hist])
        _same(table.cpu().numpy(), exp_table, "table")
        got = _run(ops, lambda o, s, out: o.applyTransform(s, table, out=out), frames, LAYOUTS[(w + length + minValue) % len(LAYOUTS)])
        _same(got, np.stack([R.applyTransform(f, t, drop=True) for f, t in zip(frames, exp_table)]), "applyTransform, a table per image")
        shared = table[1].contiguous()
        got = _run(ops, lambda o, s, out: o.applyTransform(s, shared, out=out), frames, "odd")
        _same(got, np.stack([R.applyTransform(f, exp_table[1], drop=True) for f in frames]), "applyTransform, one table")


def test_global_chain_details(ops):
    frames = _noise(70, 37, 256)
    src = _window(frames, ops.device)
    # in place, tables in place, histograms into a caller's tensor (cleared first)
    hist = torch.full((3, 256), 9, dtype=torch.int32, device=ops.device)
    assert ops.histogram(src, 0, 256, out=hist) is hist
    exp_hist = np.stack([R.histogram(f, 0, 256) for f in frames])
    _same(hist.cpu().numpy(), exp_hist, "histogram into out")
    assert ops.equalizeTable(hist, out=hist) is hist
    exp_table = np.stack([R.equalize(e) for e in exp_hist])
    _same(hist.cpu().numpy(), exp_table, "table in place")
    cur = _window(frames, ops.device)
    assert ops.applyTransform(cur, hist, out=cur) is cur
    _same(cur.cpu().numpy(), np.stack([R.applyTransform(f, t) for f, t in zip(frames, exp_table)]), "applyTransform in place")
    # deviations: an empty histogram gives zeros, a pixel beyond a short table gives 0
    empty = ops.equalizeTable(torch.zeros((2, 10), dtype=torch.int32, device=ops.device))
    assert not bool(empty.any())
    short = torch.arange(100, 110, dtype=torch.int32, device=ops.device)
    got = ops.applyTransform(src, short).cpu().numpy()
    _same(got, np.where(frames < 10, frames.astype(np.int32) + 100, 0).astype(np.uint8), "short table")
    # the (byte) cast of a table entry beyond 255
    big = (torch.arange(256, dtype=torch.int32, device=ops.device) * 3)
    _same(ops.applyTransform(src, big).cpu().numpy(), (frames.astype(np.int32) * 3 & 0xFF).astype(np.uint8), "byte cast")
    with pytest.raises(api.IllegalArgumentException):
        ops.applyTransform(src, big[:-1].reshape(5, 51))   # 5 tables for 3 images
    with pytest.raises(api.IllegalArgumentException):
        ops.histogram(src, 0, 257)


# ---------------- sharpen ----------------
@functools.lru_cache(maxsize=None)
def _sharpen_frames(w, h, f32):
    """[3,H,W].  GrayU8: noise, a frame of 0 / 255 blocks (both clamps fire), noise of small steps (no clamp).  GrayF32: values with full
    mantissas, so that k*c is rounded before the subtraction and a fused multiply-add would give other bits."""
    rng = np.random.RandomState(7 * w + h)
    if f32:
        f = np.stack([rng.rand(h, w) * 255, 100 + rng.rand(h, w), rng.rand(h, w) * 3e4 - 1e4]).astype(np.float32)
    else:
        f = np.stack([rng.randint(0, 256, (h, w)), np.where(rng.rand(h, w) < 0.5, 0, 255), 100 + rng.randint(0, 6, (h, w))]).astype(np.uint8)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("rule", (4, 8))
@pytest.mark.parametrize("size", SHARPEN_SIZES, ids=lambda s: "%dx%d" % s)
def test_sharpen_u8(ops, size, rule):
    w, h = size
    frames = _sharpen_frames(w, h, False)
    exp = np.stack([R.sharpen_rule(f, rule) for f in frames])
    if (w, h) == (70, 37):
        assert (exp[1] == 0).any() and (exp[1] == 255).any() and (exp[0] > 0).any()
    got = _run(ops, lambda o, s, out: o.sharpen(s, rule, out=out), frames, LAYOUTS[(w + h + rule) % len(LAYOUTS)])
    _same(got, exp, "sharpen%d %dx%d" % (rule, w, h))


@pytest.mark.parametrize("rule", (4, 8))
@pytest.mark.parametrize("size", SHARPEN_SIZES, ids=lambda s: "%dx%d" % s)
def test_sharpen_f32(ops, size, rule):
    w, h = size
    frames = _sharpen_frames(w, h, True)
    exp = np.stack([R.sharpen_rule(f, rule) for f in frames])
    if w >= 3 and h >= 3:
        # the reference tells the fused evaluation from its own on these inputs: a contracted multiply-add fails the comparison below
        fused = np.stack([R.sharpen_rule(f, rule, fused=True) for f in frames])
        assert (fused.view(np.uint32) != exp.view(np.uint32)).any()
    got = _run(ops, lambda o, s, out: o.sharpen(s, rule, out=out), frames, LAYOUTS[(w + h + rule + 1) % len(LAYOUTS)], torch.float32)
    _same(got.view(np.uint32), exp.view(np.uint32), "sharpen%d f32 %dx%d (bit patterns)" % (rule, w, h))


def test_overlapping_views_are_refused(ops):
    buf = torch.zeros((1, 40, 64), dtype=torch.uint8, device=ops.device)
    src, dst = buf[:, 0:20, 0:30], buf[:, 10:30, 20:50]
    fbuf = torch.zeros((1, 40, 64), dtype=torch.float32, device=ops.device)
    for call in (lambda: ops.equalizeLocal(src, 2, out=dst), lambda: ops.equalizeLocal(src, 20, out=src, path="sliding"), lambda: ops.sharpen(src, 4, out=dst),
                 lambda: ops.sharpen(fbuf[:, 0:20, 0:30], 8, out=fbuf[:, 10:30, 20:50])):
        with pytest.raises(Exception) as e:
            call()
        assert "overlap" in str(e.value)
    with pytest.raises(api.IllegalArgumentException):
        ops.sharpen(src, 5)
    torch.cuda.synchronize()
    assert not bool(buf.any()) and not bool(fbuf.any())


# ---------------- the host-buffer entry points on sub-images ----------------
def _sub(img, kind):
    """a sub-image view of a larger image: startIndex > 0, stride > width"""
    h, w = img.shape
    big = kind(w + 7, h + 3)
    big.data[...] = 9
    v = big.subimage(4, 2, 4 + w, 2 + h)
    v.array()[...] = img
    return v


def _kept(out, name):
    """nothing outside the view of `out` was written (the parent was filled with 9)"""
    keep = out.array().copy()
    out.array()[...] = 9
    assert (out.data == 9).all(), name + " wrote outside its view"
    out.array()[...] = keep


def test_host_views_through_the_mirror():
    E, S = enhance.EnhanceImageOps, enhance.ImageStatistics
    w, h = 70, 37
    a = _noise(w, h, 256)[0]
    ga = _sub(a, api.GrayU8)
    for path in PATHS:
        for r in (2, 8, 17):
            out = _sub(np.zeros((h, w), np.uint8), api.GrayU8)
            assert E.equalizeLocal(ga, r, out, 256, None, path=path) is out
            _same(out.array(), _expected("noise", w, h, r, 256)[0], "equalizeLocal %s r=%d" % (path, r))
            _kept(out, "equalizeLocal")
    small = _noise(15, 20, 10)[0]
    _same(E.equalizeLocal(_sub(small, api.GrayU8), 3, None, 10).array(), _expected("noise", 15, 20, 3, 10)[0], "equalizeLocal, new output, 10 bins")
    reshaped = api.GrayU8(3, 3)
    assert E.equalizeLocal(ga, 1, reshaped) is reshaped and (reshaped.width, reshaped.height) == (w, h)   # output.reshape
    hist = np.full(256, 5, np.int32)
    assert S.histogram(ga, 0, hist) is hist
    _same(hist, R.histogram(a, 0, 256), "histogram")
    h10 = np.zeros(10, np.int32)
    _same(S.histogram(ga, 3, h10), R.histogram(a, 3, 10, drop=True), "histogram minValue 3")
    table = E.equalize(hist, np.zeros(256, np.int32))
    _same(table, R.equalize(hist), "equalize")
    out = _sub(np.zeros((h, w), np.uint8), api.GrayU8)
    assert E.applyTransform(ga, table, out) is out
    _same(out.array(), R.applyTransform(a, table), "applyTransform")
    _kept(out, "applyTransform")
    for rule, fn in ((4, E.sharpen4), (8, E.sharpen8)):
        for f32 in (False, True):
            img = _sharpen_frames(w, h, f32)[0]
            kind = api.GrayF32 if f32 else api.GrayU8
            out = _sub(np.zeros((h, w), img.dtype), kind)
            assert fn(_sub(img, kind), out) is out
            bits = np.uint32 if f32 else np.uint8
            _same(out.array().view(bits), R.sharpen_rule(img, rule).view(bits), "sharpen%d %s" % (rule, kind.__name__))
            _kept(out, "sharpen")
            _same(fn(_sub(img, kind), None).array().view(bits), R.sharpen_rule(img, rule).view(bits), "sharpen, new output")
