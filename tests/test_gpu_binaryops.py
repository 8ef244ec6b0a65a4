"""BinaryImageOps pixel operations on the GPU against tests/binaryops_ref.py, bit for bit: DeviceImageOps.binaryLogic / binaryInvert / erode /
dilate / edge / removePointNoise, the host-view forms through boofcv_amd.binaryops, and the refusals.

The shapes are where the kernels can go wrong, not what the workload looks like (binary_ops.hip): the neighbourhood kernel owns 64 x 32 tiles
and fuses up to K = 4 iterations inside LDS with a K-pixel halo; the logic kernels give a lane 16 pixels of a row.
  1x1 1x7 7x1 2x2 2x9 3x3    no inner pixels, or one: the border forms only, in the reference's write order
  13x8                       the reference's own test image size
  67x35                      two tiles each way, a tail of 3 pixels behind four full lanes
  150x75                     three tiles each way, no multiple of the tile
numTimes 1, 2, 3, K = 4 (the longest single launch), K + 1 = 5 (two launches through context scratch) and 9 (three).
Every device output is a strided view inside a sentinel-filled parent (tests/view_layouts.py), every device input a window of a larger tensor."""
import functools

import numpy as np
import pytest
import torch

import binaryops_ref as R
import view_layouts as VL
from boofcv_amd import _lib, api, binaryops, device

pytestmark = pytest.mark.gpu
K = 4
SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (2, 9), (3, 3), (13, 8), (67, 35), (150, 75))   # (width, height)
LAYOUTS = ("odd", "pad4_x1", "dense", "pad4", "pad4_x4")


@pytest.fixture(scope="module")
def ops():
    return device.DeviceImageOps()


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    """[5,H,W]: densities 0.1 / 0.5 / 0.9, all zeros, all ones (all ones tells erode8, outside 1, from erode4, outside 0)"""
    rng = np.random.RandomState(1000 * w + h)
    f = np.stack([(rng.rand(h, w) < d).astype(np.uint8) for d in (0.1, 0.5, 0.9)] + [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)])
    f.setflags(write=False)
    return f


SINGLE = {
    "erode4": (lambda i: R.erode4(i, 1), lambda o, s, out: o.erode(s, 4, 1, out=out)),
    "dilate4": (lambda i: R.dilate4(i, 1), lambda o, s, out: o.dilate(s, 4, 1, out=out)),
    "erode8": (lambda i: R.erode8(i, 1), lambda o, s, out: o.erode(s, 8, 1, out=out)),
    "dilate8": (lambda i: R.dilate8(i, 1), lambda o, s, out: o.dilate(s, 8, 1, out=out)),
    "edge4_outside0": (lambda i: R.edge4(i, True), lambda o, s, out: o.edge(s, 4, True, out=out)),
    "edge4_outside1": (lambda i: R.edge4(i, False), lambda o, s, out: o.edge(s, 4, False, out=out)),
    "edge8_outside0": (lambda i: R.edge8(i, True), lambda o, s, out: o.edge(s, 8, True, out=out)),
    "edge8_outside1": (lambda i: R.edge8(i, False), lambda o, s, out: o.edge(s, 8, False, out=out)),
    "removePointNoise": (R.removePointNoise, lambda o, s, out: o.removePointNoise(s, out=out)),
}


def _window(frames, device_, pad=(3, 2, 5)):
    """the frames [B,H,W] as a window of a larger device tensor at an odd byte offset"""
    B, H, W = frames.shape
    top, left, right = pad
    parent = torch.full((B, H + top + 1, W + left + right), 77, dtype=torch.uint8, device=device_)
    view = parent[:, top:top + H, left:left + W]
    view.copy_(torch.from_numpy(np.array(frames)).to(device_))
    return view


def _run(ops, call, frames, layout):
    B, H, W = frames.shape
    src = _window(frames, ops.device)
    parent, out = VL.make_view(layout, B, H, W, torch.uint8, ops.device)
    before = VL.snapshot(parent)
    res = call(ops, src, out)
    assert res is out
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before, layout)
    return out.cpu().numpy()


def _same(got, exp, what):
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d pixels differ, first (y, x) %s: got %d want %d" % (what, len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_pass_batch_of_five(ops, name, size):
    w, h = size
    frames = _frames(w, h)
    ref, call = SINGLE[name]
    layout = LAYOUTS[(w + h + len(name)) % len(LAYOUTS)]
    got = _run(ops, call, frames, layout)
    for b in range(frames.shape[0]):
        _same(got[b], ref(frames[b]), "%s image %d" % (name, b))


def _edge_touching(w, h):
    """foreground on every image edge: a full frame plus a cross, holes inside"""
    img = np.zeros((h, w), np.uint8)
    img[0, :] = img[-1, :] = 1
    img[:, 0] = img[:, -1] = 1
    img[h // 2, :] = 1
    img[:, w // 2] = 1
    return img


@pytest.mark.parametrize("n", (2, 3, K, K + 1, 9))
@pytest.mark.parametrize("name", ("erode4", "dilate4", "erode8", "dilate8"))
def test_num_times(ops, name, n):
    rule, fn = int(name[-1]), (ops.erode if name.startswith("erode") else ops.dilate)
    for w, h in ((1, 7), (2, 9), (3, 3), (13, 8), (67, 35)) + (((150, 75),) if n <= K + 1 else ()):
        f = _frames(w, h)
        dense = (np.random.RandomState(w + n).rand(h, w) < (0.97 if name.startswith("erode") else 0.03)).astype(np.uint8)
        frames = np.stack([f[0 if name.startswith("dilate") else 2], f[4], _edge_touching(w, h), dense])
        got = _run(ops, lambda o, s, out: fn(s, rule, n, out=out), frames, LAYOUTS[(w + n) % len(LAYOUTS)])
        for b in range(frames.shape[0]):
            _same(got[b], R.MORPH[name](frames[b], n), "%s x%d %dx%d image %d" % (name, n, w, h, b))
        # the fused launches equal n single launches
        cur = _window(frames, ops.device)
        for _ in range(n):
            cur = fn(cur, rule, 1)
        torch.cuda.synchronize()
        assert np.array_equal(cur.cpu().numpy(), got)


def test_num_times_below_one(ops):
    frames = _frames(13, 8)
    src = _window(frames, ops.device)
    for fn, rule, name in ((ops.dilate, 4, "dilate4"), (ops.erode, 8, "erode8"), (ops.dilate, 8, "dilate8")):
        for n in (0, -3):
            got = fn(src, rule, n).cpu().numpy()
            for b in range(frames.shape[0]):
                _same(got[b], R.MORPH[name](frames[b], n), name)
    with pytest.raises(api.IllegalArgumentException):
        ops.erode(src, 4, 0)
    # the C entry refuses it too
    out = torch.zeros_like(src)
    st = ops.L.bhip_binary_morph_dev_u8(ops.ctx._h, _lib.BHIP_MORPH_ERODE4, 0, *device._geom(src, torch.uint8), *device._geom(out, torch.uint8)[:3])
    assert st == _lib.BHIP_ERR_INVALID


@pytest.mark.parametrize("size", ((1, 1), (13, 8), (67, 35), (4200, 3)), ids=lambda s: "%dx%d" % s)
def test_logic_and_invert(ops, size):
    w, h = size
    rng = np.random.RandomState(w)
    a = (rng.rand(3, h, w) < 0.5).astype(np.uint8)
    b = (rng.rand(3, h, w) < 0.5).astype(np.uint8)
    a[0, 0, 0], b[0, 0, 0] = 2, 2   # not 0 / 1: the reference tests == 1, == 0 and !=
    b[1, -1, -1] = 255
    tb = _window(b, ops.device, (1, 3, 2))
    for op, ref in (("and", R.logicAnd), ("or", R.logicOr), ("xor", R.logicXor)):
        got = _run(ops, lambda o, s, out: o.binaryLogic(op, s, tb, out=out), a, LAYOUTS[(w + len(op)) % len(LAYOUTS)])
        _same(got, ref(a, b), op)
        # in place: out == a, then out == b
        ta, tb2 = _window(a, ops.device), _window(b, ops.device, (2, 1, 1))
        assert ops.binaryLogic(op, ta, tb2, out=ta) is ta
        _same(ta.cpu().numpy(), ref(a, b), op + " in place (a)")
        ta = _window(a, ops.device)
        ops.binaryLogic(op, ta, tb2, out=tb2)
        _same(tb2.cpu().numpy(), ref(a, b), op + " in place (b)")
    got = _run(ops, lambda o, s, out: o.binaryInvert(s, out=out), a, "odd")
    _same(got, R.invert(a), "invert")
    ta = _window(a, ops.device)
    ops.binaryInvert(ta, out=ta)
    _same(ta.cpu().numpy(), R.invert(a), "invert in place")


def test_overlapping_neighbourhood_views_are_refused(ops):
    buf = torch.zeros((1, 40, 64), dtype=torch.uint8, device=ops.device)
    src, dst = buf[:, 0:20, 0:30], buf[:, 10:30, 20:50]
    for call in (lambda: ops.erode(src, 4, 1, out=dst), lambda: ops.dilate(src, 8, 6, out=dst), lambda: ops.edge(src, 8, True, out=dst),
                 lambda: ops.removePointNoise(src, out=dst), lambda: ops.erode(src, 8, 1, out=src)):
        with pytest.raises(Exception) as e:
            call()
        assert "overlap" in str(e.value)
    torch.cuda.synchronize()
    assert not bool(buf.any())


def test_host_views_through_the_mirror():
    ops = binaryops.BinaryImageOps
    rng = np.random.RandomState(5)
    w, h = 67, 35
    a, b = (rng.rand(h, w) < 0.6).astype(np.uint8), (rng.rand(h, w) < 0.4).astype(np.uint8)

    def sub(img):   # a sub-image view: startIndex > 0, stride > width
        big = api.GrayU8(w + 7, h + 3)
        v = big.subimage(4, 2, 4 + w, 2 + h)
        v.array()[...] = img
        return v

    ga, gb = sub(a), sub(b)
    for fn, ref in ((ops.logicAnd, R.logicAnd), (ops.logicOr, R.logicOr), (ops.logicXor, R.logicXor)):
        _same(fn(ga, gb, None).array(), ref(a, b), fn.__name__)
    _same(ops.invert(ga, None).array(), R.invert(a), "invert")
    for name in sorted(R.MORPH):
        out = sub(np.full((h, w), 9, np.uint8))
        before = out.data.copy()
        assert getattr(ops, name)(ga, K + 2, out) is out
        _same(out.array(), R.MORPH[name](a, K + 2), name)
        out.array()[...] = 9
        assert np.array_equal(out.data, before), name + " wrote outside its view"
    _same(ops.edge4(ga, None, False).array(), R.edge4(a, False), "edge4")
    _same(ops.edge8(ga, None, True).array(), R.edge8(a, True), "edge8")
    _same(ops.removePointNoise(ga, None).array(), R.removePointNoise(a), "removePointNoise")
