"""CPU checks of tests/enhance_ref.py (the oracle of the GPU enhancement tests) against the reference's own answers, of the one-rule forms the
kernels implement against the literal loops, and of the Python mirror's argument checks.  Known answers: TestEnhanceImageOps,
TestImplEnhanceHistogram, TestImplEnhanceFilter."""
import os

import numpy as np
import pytest

import enhance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("bhip_histogram_dev_u8", "bhip_histogram_u8", "bhip_equalize_table_dev", "bhip_apply_transform_dev_u8", "bhip_apply_transform_u8",
           "bhip_equalize_local_dev_u8", "bhip_equalize_local_u8", "bhip_sharpen_dev_u8", "bhip_sharpen_dev_f32", "bhip_sharpen_u8", "bhip_sharpen_f32")


def _reference_image(orc):
    """TestEnhanceImageOps.equalizeLocal's input: 15 x 20, GImageMiscOps.fillUniform(input, new Random(234), 0, 9) -- (byte)(rand.nextInt(9) + 0)
    in raster order (ImageMiscOps.java:346-357)"""
    rand = orc.JavaRandom(234)
    return np.array([rand.nextInt(9) for _ in range(15 * 20)], np.uint8).reshape(20, 15)


def test_equalize_known_answer():
    """TestEnhanceImageOps.equalize"""
    assert ref.equalize([2, 2, 2, 2, 2, 0, 0, 0, 0, 0])[:5].tolist() == [1, 3, 5, 7, 9]


def test_apply_transform_and_histogram():
    """TestImplEnhanceHistogram.applyTransform: the output is transform[input]; histogram with a minValue"""
    rng = np.random.RandomState(3)
    img = rng.randint(0, 10, (20, 15)).astype(np.uint8)
    transform = np.array([i * 2 for i in range(10)], np.int32)
    assert np.array_equal(ref.applyTransform(img, transform), (img * 2).astype(np.uint8))
    assert ref.applyTransform(np.array([[1]], np.uint8), [0, 300]).tolist() == [[300 & 0xFF]]   # the (byte) cast
    h = ref.histogram(img, 0, 10)
    assert h.tolist() == np.bincount(img.ravel(), minlength=10).tolist()
    shifted = ref.histogram(img + 3, 3, 10)
    assert shifted.tolist() == h.tolist()
    with pytest.raises(IndexError):
        ref.histogram(img, 3, 10)          # a pixel below minValue: Java throws
    assert ref.histogram(img, 3, 10, drop=True).tolist() == h.tolist()[3:] + [0, 0, 0]


def test_equalize_local_of_the_reference_test(orc):
    """TestEnhanceImageOps.equalizeLocal: the dispatch equals equalizeLocalNaive for radius 1 .. 10 with a histogram of 10 bins; on 15 x 20 the
    radii 1 .. 7 take the inner / row / column branch, 8 and 9 the naive one, 10 the whole-image one"""
    img = _reference_image(orc)
    assert img.max() <= 8 and img.min() == 0
    branches = []
    for radius in range(1, 11):
        expected = np.zeros_like(img)
        ref.equalizeLocalNaive(img, radius, expected, 10)
        found, branch = ref.equalizeLocal(img, radius, 10)
        branches.append(branch)
        assert np.array_equal(expected, found), radius
    assert branches == ["inner"] * 7 + ["naive"] * 2 + ["whole"]


def test_literal_dispatch_equals_the_window_rank(orc):
    img = _reference_image(orc)
    for radius in range(0, 13):
        lit, _ = ref.equalizeLocal(img, radius, 10)
        assert np.array_equal(lit, ref.rank_local(img, radius, 10)), radius
    rng = np.random.RandomState(11)
    seen = set()
    for (w, h) in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 3), (17, 17), (16, 18)):
        full = rng.randint(0, 256, (h, w)).astype(np.uint8)
        for radius in (0, 1, 2, 4, 7, 8, 9):
            lit, branch = ref.equalizeLocal(full, radius, 256)
            seen.add(branch)
            assert np.array_equal(lit, ref.rank_local(full, radius, 256)), (w, h, radius)
    assert seen == {"inner", "naive", "whole"}
    assert ref.equalizeLocal(rng.randint(0, 256, (17, 17)).astype(np.uint8), 8, 256)[1] == "inner"   # exactly 2r+1
    const = np.full((11, 7), 5, np.uint8)
    for length in (256, 10, 6):
        for radius in (0, 2, 3, 5, 9):
            lit, _ = ref.equalizeLocal(const, radius, length)
            assert (lit == length - 1).all() and np.array_equal(lit, ref.rank_local(const, radius, length))


def test_window_is_shifted_not_cropped():
    assert ref.window(0, 2, 10) == (0, 5) and ref.window(9, 2, 10) == (5, 10) and ref.window(4, 2, 10) == (2, 7)
    assert ref.window(1, 2, 3) == (0, 3) and ref.window(0, 0, 1) == (0, 1)


@pytest.mark.parametrize("dtype", (np.uint8, np.float32))
def test_sharpen_inner_is_the_clamped_convolution(dtype):
    """TestImplEnhanceFilter.sharpenInner4 / 8: inner pixels equal the convolution with kernelEnhance4 / 8 bounded to [0, 255]"""
    rng = np.random.RandomState(234)
    img = rng.randint(0, 10, (20, 15)).astype(dtype)       # the reference's 15 x 20 image of 0 .. 9: sums exact in float32
    img[5:9, 4:8] = rng.randint(0, 256, (4, 4))            # and a patch where both clamps fire
    for fn, k in ((ref.sharpen4, ref.KERNEL_ENHANCE4), (ref.sharpen8, ref.KERNEL_ENHANCE8)):
        got, want = fn(img), ref.convolve_clamped(img, k)
        assert np.array_equal(got[1:-1, 1:-1].astype(np.float64), want[1:-1, 1:-1])
    assert (ref.sharpen4(img) == 0).any() and (ref.sharpen4(img) == 255).any()


def test_sharpen_border_literals():
    """the border forms by hand on a 3 x 3 image: safeGet clamps, the corner reads itself"""
    img = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    o4 = ref.sharpen4(img)
    assert o4[0, 0] == min(255, max(0, 4 * 10 - (10 + 20 + 40)))          # TOP at x = 0: g(-1,0) is the pixel itself
    assert o4[1, 0] == min(255, max(0, 4 * 40 - (50 + 10 + 70)))          # LEFT
    assert o4[1, 2] == min(255, max(0, 4 * 60 - (50 + 30 + 90)))          # RIGHT
    assert o4[2, 1] == min(255, max(0, 4 * 80 - (70 + 90 + 50)))          # BOTTOM
    assert o4[1, 1] == min(255, max(0, 5 * 50 - (40 + 60 + 20 + 80)))
    o8 = ref.sharpen8(img)
    assert o8[0, 0] == min(255, max(0, 9 * 10 - (10 + 10 + 20 + 10 + 20 + 40 + 40 + 50)))


@pytest.mark.parametrize("dtype", (np.uint8, np.float32))
@pytest.mark.parametrize("rule", (4, 8))
def test_sharpen_owner_table_equals_the_loops(rule, dtype):
    """sides 1, 2, 3 and 8 in every combination: the last write of the reference's loops is the owner table's formula"""
    rng = np.random.RandomState(rule)
    for h in (1, 2, 3, 8):
        for w in (1, 2, 3, 8):
            img = rng.randint(0, 256, (h, w)).astype(dtype)
            if dtype == np.float32:
                img = (img + rng.rand(h, w).astype(np.float32) * np.float32(0.37)).astype(np.float32)
            lit = ref.sharpen4(img) if rule == 4 else ref.sharpen8(img)
            one = ref.sharpen_rule(img, rule)
            assert np.array_equal(lit.view(np.uint32 if dtype == np.float32 else np.uint8), one.view(np.uint32 if dtype == np.float32 else np.uint8)), (w, h)
    assert ref.sharpen_owner(0, 0, 1, 1) == "BOTTOM" and ref.sharpen_owner(0, 1, 1, 3) == "RIGHT" and ref.sharpen_owner(0, 0, 3, 2) == "TOP"
    assert ref.sharpen_owner(0, 1, 3, 3) == "LEFT" and ref.sharpen_owner(1, 1, 3, 3) == "INNER" and ref.sharpen_owner(2, 1, 3, 3) == "RIGHT"


# ---- the Python mirror (these need the built library, not a GPU) ----
def test_mirror_module_refuses_before_c():
    from boofcv_amd import api, enhance
    ops = enhance.EnhanceImageOps
    u8, f32, s16, s32 = api.GrayU8(5, 4), api.GrayF32(5, 4), api.GrayS16(5, 4), api.GrayS32(5, 4)
    for bad in (f32, s16, s32):
        with pytest.raises(api.IllegalArgumentException):
            ops.equalizeLocal(bad, 2, None)
        with pytest.raises(api.IllegalArgumentException):
            ops.applyTransform(bad, np.arange(256, dtype=np.int32), None)
        with pytest.raises(api.IllegalArgumentException):
            enhance.ImageStatistics.histogram(bad, 0, np.zeros(256, np.int32))
    with pytest.raises(api.IllegalArgumentException) as e:
        ops.equalizeLocal(s16, 2, None)
    assert "GrayS16" in str(e.value)
    for bad in (s16, s32):
        with pytest.raises(api.IllegalArgumentException):
            ops.sharpen4(bad, None)
    with pytest.raises(api.IllegalArgumentException):
        ops.sharpen8(u8, f32)                       # input and output of one type
    with pytest.raises(api.IllegalArgumentException):
        ops.sharpen4(u8, api.GrayU8(4, 4))          # checkSameShape
    with pytest.raises(api.IllegalArgumentException):
        ops.sharpen4(u8, u8)                        # overlap
    with pytest.raises(api.IllegalArgumentException):
        ops.equalizeLocal(u8, 256, None)
    with pytest.raises(api.IllegalArgumentException):
        ops.equalizeLocal(u8, -1, None)
    for length in (0, 257):
        with pytest.raises(api.IllegalArgumentException):
            ops.equalizeLocal(u8, 2, None, length)
    with pytest.raises(api.IllegalArgumentException):
        ops.equalizeLocal(u8, 2, u8)                # overlap
    big = api.GrayU8(12, 9)
    with pytest.raises(api.IllegalArgumentException):
        ops.equalizeLocal(big.subimage(0, 0, 5, 4), 2, big.subimage(2, 2, 7, 6))
    with pytest.raises(api.IllegalArgumentException):
        ops.equalizeLocal(u8, 2, None, 256, None, None, "fastest")
    with pytest.raises(api.IllegalArgumentException):
        ops.applyTransform(u8, np.zeros(300, np.int32), None)
    with pytest.raises(api.IllegalArgumentException):
        enhance.ImageStatistics.histogram(u8, 0, np.zeros(256, np.int64))   # filled in place: int32 only
    with pytest.raises(api.IllegalArgumentException):
        enhance.ImageStatistics.histogram(u8, 256, np.zeros(10, np.int32))
    # equalize is host logic and equals the restatement
    t = np.zeros(10, np.int32)
    assert ops.equalize([2, 2, 2, 2, 2, 0, 0, 0, 0, 0], t) is t and t[:5].tolist() == [1, 3, 5, 7, 9]
    h = np.random.RandomState(1).randint(0, 5000, 256)
    assert np.array_equal(ops.equalize(h, np.zeros(256, np.int32)), ref.equalize(h))
    with pytest.raises(ZeroDivisionError):
        ops.equalize([0, 0, 0], [0, 0, 0])


def test_new_exports_are_in_the_header_the_binding_and_the_library():
    from boofcv_amd import _lib
    header = open(os.path.join(ROOT, "include", "boofhip.h")).read()
    L = _lib.load()
    for name in EXPORTS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(L, name), name
    assert (_lib.BHIP_EQLOCAL_AUTO, _lib.BHIP_EQLOCAL_DIRECT, _lib.BHIP_EQLOCAL_SLIDING) == (0, 1, 2)


def test_device_ops_have_the_new_methods():
    from boofcv_amd import device
    for name in ("histogram", "equalizeTable", "applyTransform", "equalizeLocal", "sharpen"):
        assert callable(getattr(device.DeviceImageOps, name))
