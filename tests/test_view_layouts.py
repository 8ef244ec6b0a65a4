"""CPU self-test of tests/view_layouts.py: a correct op passes, every single-element fault outside the view is caught, the layouts have the
alignment they are named for; and DeviceImageOps refuses the views it cannot describe to the library before calling it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import view_layouts as vl

DTYPES = [torch.float32, torch.uint8, torch.int16, torch.int32]
SHAPES = [(2, 9, 30), (2, 5, 7), (3, 4, 13)]   # B, H, W


def _payload(B, H, W, dtype):
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W)
    if dtype == torch.float32:
        return torch.rand((B, H, W), generator=g) * 255 - 100
    hi = {torch.uint8: 0xA5, torch.int16: 2000, torch.int32: 1 << 20}[dtype]   # (a byte image may hold 0xA5; this one does not)
    return torch.randint(0, hi, (B, H, W), generator=g).to(dtype)


def _faults(B, H, W, offset, image, pitch):
    """parent indices of the single-element faults a strided store can commit"""
    last = offset + (B - 1) * image
    return {
        "one past the row end": offset + (H // 2) * pitch + W,
        "one past the last row's end": last + (H - 1) * pitch + W,
        "one before the row start": offset + image + (H // 2) * pitch - 1,
        "one before the first row's start": offset - 1,
        "inter-image gap": offset + image - 1,
        "row above image 0": offset - pitch + W // 2,
        "row below image B-1": last + H * pitch + W // 2,
    }


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("layout", vl.LAYOUTS)
def test_faults_outside_the_view_are_caught(layout, dtype):
    for B, H, W in SHAPES:
        x = _payload(B, H, W, dtype)
        parent, view = vl.make_view(layout, B, H, W, dtype, "cpu")
        assert parent.dim() == 1 and tuple(view.shape) == (B, H, W) and view.stride(2) == 1
        assert bool((vl.bits(parent) == vl.SENTINEL[dtype]).all())
        before = vl.snapshot(parent)
        view.copy_(x)   # a correct op
        vl.assert_only_view_written(parent, view, before)
        assert torch.equal(vl.bits(view), vl.bits(x))
        assert not bool((vl.bits(view) == vl.SENTINEL[dtype]).any())   # no payload value looks like the sentinel
        offset, image, pitch, total = vl.geometry(layout, B, H, W)
        assert (view.storage_offset(), view.stride(0), view.stride(1)) == (offset, image, pitch)
        inside = vl.inside_mask(parent, view)
        assert int(inside.sum()) == B * H * W
        for name, at in _faults(B, H, W, offset, image, pitch).items():
            assert 0 <= at < parent.numel(), name
            if bool(inside[at]):   # dense rows touch: the neighbouring pixel belongs to the view (the next row, or the next image)
                assert layout == "dense" and name in ("one past the row end", "one before the row start", "inter-image gap"), (name, layout)
                continue
            parent2, view2 = vl.make_view(layout, B, H, W, dtype, "cpu")
            before2 = vl.snapshot(parent2)
            view2.copy_(x)
            parent2[at] = x.flatten()[0]   # an ordinary result value, one element off
            with pytest.raises(AssertionError, match="outside the view"):
                vl.assert_only_view_written(parent2, view2, before2, name)
        # a fault that happens to store the value already there is no fault; one that flips a single bit is
        parent3, view3 = vl.make_view(layout, B, H, W, dtype, "cpu")
        before3 = vl.snapshot(parent3)
        view3.copy_(x)
        raw = parent3.view(torch.int32) if dtype == torch.float32 else parent3
        raw[offset - 1] = raw[offset - 1] ^ 1
        with pytest.raises(AssertionError):
            vl.assert_only_view_written(parent3, view3, before3)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("layout", vl.LAYOUTS)
def test_guards_and_alignment(layout, dtype):
    size = torch.empty(0, dtype=dtype).element_size()
    for B, H, W in SHAPES + [(2, 131, 259)]:
        parent, view = vl.make_view(layout, B, H, W, dtype, "cpu")
        offset, image, pitch = view.storage_offset(), view.stride(0), view.stride(1)
        x0 = {"dense": 0, "pad4": 0, "pad4_x4": 4, "pad4_x1": 1, "odd": 2}[layout]
        # two full guard rows above and below, 64 elements at either end
        assert offset - x0 >= max(vl.GUARD_ROWS * pitch, vl.GUARD_ELEMS)
        end = offset + (B - 1) * image + (H - 1) * pitch + W
        assert parent.numel() - end >= max(vl.GUARD_ROWS * pitch, vl.GUARD_ELEMS)
        assert parent.data_ptr() % 16 == 0 and (offset - x0) % 16 == 0
        rel = (view.data_ptr() - parent.data_ptr())
        assert rel == offset * size
        if layout == "dense":
            assert (pitch, image) == (W, H * W) and view.data_ptr() % 16 == 0
        elif layout.startswith("pad4"):
            assert pitch == (W + 3) // 4 * 4 + 8 and pitch % 4 == 0 and image % 4 == 0 and image == pitch * (H + 2)
            assert view.data_ptr() % (4 * size) == {"pad4": 0, "pad4_x4": 0, "pad4_x1": size}[layout]
            if dtype == torch.float32:   # what the launchers' vec4() asks of base, pitch and image stride
                assert (view.data_ptr() % 16 == 0) == (layout != "pad4_x1")
            if dtype == torch.int16 and layout == "pad4_x1":   # rows start 2-byte but not 4-byte aligned, every one of them
                assert all((view[b, y].data_ptr() % 4) == 2 for b in range(B) for y in (0, 1, H - 1))
        else:
            assert pitch == W + 3 and image == pitch * (H + 2) + 1 and x0 == 2
            assert image % 4 != 0 or pitch % 4 != 0
    # a shifted window (derivY beside an aligned derivX): same strides, base `shift` elements on
    p0, v0 = vl.make_view("pad4", 2, 9, 30, dtype, "cpu")
    p1, v1 = vl.make_view("pad4", 2, 9, 30, dtype, "cpu", shift=1)
    assert v1.stride() == v0.stride() and v1.storage_offset() == v0.storage_offset() + 1
    assert v0.data_ptr() % 16 == 0 and v1.data_ptr() % 16 == size


def test_assert_kept():
    for dtype in DTYPES:
        parent, view = vl.make_view("pad4_x4", 2, 9, 30, dtype, "cpu")
        x = _payload(2, 9, 30, dtype)
        frame = np.ones((9, 30), bool)
        frame[1:-1, 1:-1] = False
        view[:, 1:-1, 1:-1] = x[:, 1:-1, 1:-1]
        vl.assert_kept(view, frame)
        view[1, 0, 29] = x[1, 0, 29]
        with pytest.raises(AssertionError, match="frame elements"):
            vl.assert_kept(view, frame)


class _FakeTensor:
    """what _geom reads of a tensor, with strides torch itself would not build (torch.as_strided has no negative strides)"""

    def __init__(self, shape, strides, dtype=torch.float32):
        self.shape, self._strides, self.dtype, self.is_cuda, self.device = shape, strides, dtype, True, "cuda:0"

    def dim(self):
        return len(self.shape)

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def unsqueeze(self, d):
        return _FakeTensor((1,) + tuple(self.shape), (self.shape[0] * self._strides[0],) + tuple(self._strides), self.dtype)

    def data_ptr(self):
        return 4096


class _Recorder:
    """stands for libboofhip.so: any call into it is recorded"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append(name)
            return 0
        return fn


@pytest.mark.parametrize("strides", [(9 * 32, -32, 1), (-9 * 32, 32, 1), (9 * 64, 64, 2), (9 * 32, 32, -1), (9 * 32, 32, 0)],
                         ids=["negative-row", "negative-image", "x-stride-2", "x-stride-negative", "x-stride-0"])
def test_device_ops_refuse_views_the_library_cannot_address(strides):
    from boofcv_amd import device as dv
    from boofcv_amd.api import IllegalArgumentException
    bad = _FakeTensor((2, 9, 30), strides)
    good = _FakeTensor((2, 9, 30), (9 * 32, 32, 1))
    assert dv._geom(good)[1:] == (9 * 32, 32, 30, 9, 2)
    with pytest.raises(IllegalArgumentException):
        dv._geom(bad)
    ops = dv.DeviceImageOps.__new__(dv.DeviceImageOps)   # no GPU here: the object without a context, the library replaced by a recorder
    ops.L, ops.ctx, ops.device = _Recorder(), None, "cuda:0"
    k = np.ones(3, np.float32) / 3
    calls = [lambda: ops.convolveHorizontal(k, 1, bad, good), lambda: ops.convolveNormalizedVertical(k, 1, good, bad), lambda: ops.gaussian(bad, -1, 2, good),
             lambda: ops.gaussian(good, -1, 2, bad), lambda: ops.sobel(good, 0, bad, bad), lambda: ops.three(bad, None, good, good),
             lambda: ops.intensity(0, good, good, bad), lambda: ops.cornerIntensity(0, 2, 0.04, bad, bad, good), lambda: ops.nonmax(bad, 2, 1.0, 0, cap=4),
             lambda: ops.fast(bad, 7.5, 9, 1.0, intensity=False, cap=4), lambda: ops.fast(good, 7.5, 9, 1.0, intensity=bad, cap=4)]
    for call in calls:
        with pytest.raises(IllegalArgumentException):
            call()
    assert ops.L.calls == []
