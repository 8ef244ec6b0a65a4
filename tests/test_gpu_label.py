"""Blob labelling on the GPU (DeviceImageOps.labelBlobs, binaryops.BinaryImageOps.contourLabels) and the label utilities against
tests/binaryops_ref.py, exactly: the labelled GrayS32 image and the contour count of LinearContourLabelChang2004, both rules.

label.hip unites pixels inside 32 x 32 tiles in LDS and then across tile edges in global memory, so the shapes put single-pixel structures
across tile edges and tile corners; 100 x 70 is 4 x 3 tiles and no multiple of the tile."""
import functools

import numpy as np
import pytest
import torch

import binaryops_ref as R
import test_binaryops_reference as F
import view_layouts as VL
from boofcv_amd import api, binaryops, device

pytestmark = pytest.mark.gpu
RULES = (R.FOUR, R.EIGHT)
T = 32   # tile side of label.hip


@pytest.fixture(scope="module")
def ops():
    return device.DeviceImageOps()


def _serpentine(w, h):
    img = np.zeros((h, w), np.uint8)
    for i, y in enumerate(range(0, h, 2)):
        img[y, :] = 1
        if y + 1 < h:
            img[y + 1, w - 1 if i % 2 == 0 else 0] = 1
    return img


def _comb(w, h):
    img = np.zeros((h, w), np.uint8)
    img[h - 1, :] = 1
    img[1:, ::2] = 1
    img[0, 6::4] = 1    # every other tooth starts a row higher, and not the leftmost one
    return img


def _rings(w, h):
    img = np.zeros((h, w), np.uint8)
    for k in range(0, min(w, h) // 2 - 1, 4):   # nested one-pixel rings, three pixels apart: separate blobs for both rules
        img[k, k:w - k] = img[h - 1 - k, k:w - k] = 1
        img[k:h - k, k] = img[k:h - k, w - 1 - k] = 1
    return img


def _u(w, h):
    """the right arm starts higher than the left one: the root is the raster-first pixel, in another tile than the left arm's top"""
    img = np.zeros((h, w), np.uint8)
    img[10:h - 5, 5] = 1
    img[3:h - 5, w - 9] = 1
    img[h - 6, 5:w - 8] = 1
    img[1, 2] = 1   # an earlier blob, so the U is not number 1
    return img


def _corner_touch():
    img = np.zeros((70, 100), np.uint8)
    img[T - 3:T, T - 3:T] = 1            # ends at (31, 31)
    img[T:T + 3, T:T + 3] = 1            # starts at (32, 32): they touch across a tile corner only
    img[T - 1, 2 * T] = 1                # (64, 31) and (63, 32): the other diagonal
    img[T, 2 * T - 1] = 1
    return img


@functools.lru_cache(maxsize=None)
def _cases():
    rng = np.random.RandomState(42)
    c = {"TEST": F.TEST, "chang1": F.CHANG1, "chang2": F.CHANG2, "chang3": F.CHANG3, "chang4": F.CHANG4,
         "1x1_one": np.ones((1, 1), np.uint8), "1x1_zero": np.zeros((1, 1), np.uint8),
         "1xN": (rng.rand(100, 1) < 0.6).astype(np.uint8), "Nx1": (rng.rand(1, 100) < 0.6).astype(np.uint8),
         "zeros": np.zeros((70, 100), np.uint8), "ones": np.ones((70, 100), np.uint8),
         "checkerboard": (np.indices((45, 70)).sum(0) % 2).astype(np.uint8),
         "diagonal": np.eye(80, dtype=np.uint8), "antidiagonal": np.eye(80, dtype=np.uint8)[:, ::-1].copy(),
         "serpentine": _serpentine(100, 70), "comb": _comb(100, 70), "rings": _rings(90, 70), "ring": _rings(90, 70) * 0,
         "u": _u(100, 70), "corner_touch": _corner_touch()}
    c["ring"][5:60, 7:80] = 1
    c["ring"][20:40, 30:50] = 0
    for d in (0.3, 0.55, 0.8):
        c["random_%d" % int(d * 100)] = (rng.rand(70, 100) < d).astype(np.uint8)
    c["not_binary"] = (rng.randint(0, 4, (40, 50)) * 85).astype(np.uint8)   # 0, 85, 170, 255: no pixel equals 1
    c["twos"] = rng.randint(0, 3, (40, 50)).astype(np.uint8)                # only the 1s are foreground
    return c


@functools.lru_cache(maxsize=None)
def _expected(name, rule):
    """The restated reference.  "twos" holds 0, 1 and 2: there the library defines the result (include/boofhip.h: a pixel equal to 1 is
    foreground, anything else background), which is the flood fill; the reference itself tests `!= 1` in its scan and tracer but `== 0` for the
    pixel below in step 2, so on such an input it skips internal contours next to a 2 and starts extra blobs."""
    labeled, n = (R.floodLabels if name == "twos" else R.contourLabels)(_cases()[name], rule)
    labeled.setflags(write=False)
    return labeled, n


def _label(ops, frames, rule, layout="dense"):
    B, H, W = frames.shape
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(ops.device)
    parent, out = VL.make_view(layout, B, H, W, torch.int32, ops.device)
    before = VL.snapshot(parent)
    res, n = ops.labelBlobs(src, rule, out=out)
    assert res is out
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before, layout)
    return out.cpu().numpy(), n.cpu().numpy()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(_cases()))
def test_labels_and_count(ops, name, rule):
    img = _cases()[name]
    want, n = _expected(name, rule)
    got, count = _label(ops, img[None], rule)
    assert int(count[0]) == n
    bad = np.argwhere(got[0] != want)
    assert bad.size == 0, "%d pixels differ, first (y, x) %s: got %d want %d" % (len(bad), bad[0], got[0][tuple(bad[0])], want[tuple(bad[0])])


def test_known_counts():
    """the figures the cases are there for"""
    n = {(name, rule): _expected(name, rule)[1] for name in ("checkerboard", "diagonal", "ones", "zeros", "corner_touch", "chang2") for rule in RULES}
    board = int(_cases()["checkerboard"].sum())
    assert n["checkerboard", 4] == board and n["checkerboard", 8] == 1
    assert n["diagonal", 4] == 80 and n["diagonal", 8] == 1
    assert n["ones", 4] == n["ones", 8] == 1 and n["zeros", 4] == n["zeros", 8] == 0
    assert n["corner_touch", 4] == 4 and n["corner_touch", 8] == 2
    assert n["chang2", 4] == 14 and n["chang2", 8] == 4


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("layout", ("odd", "pad4_x1", "pad4"))
def test_batch_of_three_into_a_strided_view(ops, layout, rule):
    names = ("random_55", "u", "comb")
    frames = np.stack([_cases()[n] for n in names])
    got, count = _label(ops, frames, rule, layout)
    for b, name in enumerate(names):
        want, n = _expected(name, rule)
        assert int(count[b]) == n and np.array_equal(got[b], want), name   # labels restart at 1 in every image
    # a strided input window as well
    big = torch.full((3, 75, 111), 1, dtype=torch.uint8, device=ops.device)
    win = big[:, 2:72, 5:105]
    win.copy_(torch.from_numpy(frames).to(ops.device))
    out, n2 = ops.labelBlobs(win, rule)
    assert np.array_equal(out.cpu().numpy(), got) and np.array_equal(n2.cpu().numpy(), count)


def test_same_input_twice_and_scratch_reuse(ops):
    a = _cases()["random_30"][None]
    first = _label(ops, a, 8)
    _label(ops, _cases()["ones"][None], 4)           # another image through the same scratch in between
    _label(ops, _cases()["chang1"][None], 8)         # and a smaller one
    second = _label(ops, a, 8)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    assert np.array_equal(first[0][0], _expected("random_30", 8)[0])


def test_host_view_through_the_mirror():
    img = _cases()["random_55"]
    h, w = img.shape
    big = api.GrayU8(w + 5, h + 2)
    src = big.subimage(3, 1, 3 + w, 1 + h)
    src.array()[...] = img
    lab = api.GrayS32(w + 4, h + 2).subimage(1, 1, 1 + w, 1 + h)
    for rule in (binaryops.ConnectRule.FOUR, binaryops.ConnectRule.EIGHT):
        lab.data[...] = -7
        n = binaryops.BinaryImageOps.contourLabels(src, rule, lab)
        want, m = _expected("random_55", int(rule))
        assert n == m and np.array_equal(lab.array(), want)
        lab.array()[...] = -7
        assert (lab.data == -7).all()
    assert binaryops.BinaryImageOps.contourLabels(src, binaryops.ConnectRule.EIGHT) == _expected("random_55", 8)[1]


# ---- label utilities, on the labelling's own output ----
def test_relabel(ops):
    img = _cases()["random_30"]
    want, n = _expected("random_30", 8)
    labels, _ = ops.labelBlobs(torch.from_numpy(img[None]).to(ops.device), 8)
    perm = np.random.RandomState(3).permutation(n + 1).astype(np.int32)
    parent, view = VL.make_view("odd", 1, *img.shape, torch.int32, ops.device)
    view.copy_(labels)
    before = VL.snapshot(parent)
    assert ops.relabel(view, torch.from_numpy(perm).to(ops.device)) is view
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, view, before)
    assert np.array_equal(view.cpu().numpy()[0], R.relabel(want, perm))
    # a table shorter than the labels: pixels outside it stay (the documented deviation)
    short = perm[:n // 2].copy()
    view.copy_(labels)
    view[0, 0, 0] = -5
    ops.relabel(view, torch.from_numpy(short).to(ops.device))
    w2 = want.copy()
    w2[0, 0] = -5
    exp = R.relabel(w2, short)
    assert exp[0, 0] == -5 and (exp == w2)[w2 >= len(short)].all()
    assert np.array_equal(view.cpu().numpy()[0], exp)
    # host view
    g = api.GrayS32.wrap(want.copy())   # relabel works in place, and wrap() takes a contiguous array as it is
    binaryops.BinaryImageOps.relabel(g, perm)
    assert np.array_equal(g.array(), R.relabel(want, perm))


def test_label_to_binary(ops):
    img = _cases()["random_30"]
    want, n = _expected("random_30", 4)
    labels, _ = ops.labelBlobs(torch.from_numpy(img[None]).to(ops.device), 4)
    parent, out = VL.make_view("odd", 1, *img.shape, torch.uint8, ops.device)
    before = VL.snapshot(parent)
    ops.labelToBinary(labels, out=out)
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before)
    assert np.array_equal(out.cpu().numpy()[0], R.labelToBinary(want)) and np.array_equal(out.cpu().numpy()[0], img)
    sel = np.random.RandomState(9).rand(n + 1) < 0.5
    sel[0] = False
    got = ops.labelToBinary(labels, torch.from_numpy(sel).to(ops.device), out=out)
    assert np.array_equal(got.cpu().numpy()[0], R.labelToBinary(want, sel))
    # host views: the boolean[] form and the varargs form
    g = api.GrayS32.wrap(want)
    B = binaryops.BinaryImageOps
    assert np.array_equal(B.labelToBinary(g, None).array(), R.labelToBinary(want))
    assert np.array_equal(B.labelToBinary(g, None, list(sel)).array(), R.labelToBinary(want, sel))
    picked = [int(i) for i in np.nonzero(sel)[0]]
    assert np.array_equal(B.labelToBinary(g, None, n + 1, *picked).array(), R.labelToBinary(want, sel))
