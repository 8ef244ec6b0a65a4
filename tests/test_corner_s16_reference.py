"""CPU checks of tests/corner_ref.py (the reference for the integer gradient / S16 corner / weighted corner paths) and of the host-only
bhip_gaussian_kernel1d_s32.  Re-expressed reference tests cite their Java source."""
import numpy as np
import pytest

import corner_ref as cr


def _u8_frame(orc, w, h, seed):
    img = orc.noise_image(w, h, seed, 0.0, 255.0).array()
    return np.floor(img).astype(np.uint8)


@pytest.mark.parametrize("border", [False, True])
@pytest.mark.parametrize("kind,scale", [("sobel", 4), ("three", 2)])
def test_u8_gradients_are_scaled_float_gradients(orc, kind, scale, border):
    img = _u8_frame(orc, 37, 23, 11)
    fdx, fdy = orc.gradient(kind, orc.Gray.from_array(img.astype(np.float32)), border_zero=border)
    dx, dy = cr.gradient_u8(kind, img, border)
    assert np.array_equal(dx.astype(np.float32), scale * fdx.array())   # small integers: the float results are exact
    assert np.array_equal(dy.astype(np.float32), scale * fdy.array())


def _manual_box(p, x, y, r):
    return int(sum(int(p[i, j]) for i in range(y - r, y + r + 1) for j in range(x - r, x + r + 1)))


def test_box_s16_compare_to_manual(orc):
    """TestImplSsdCorner_S16.compareToManual (F:.../intensity/impl/TestImplSsdCorner_S16.java:55-103), MockSum score"""
    r, width, height = 2, 40, 50
    img = _u8_frame(orc, width, height, 234) % 100
    dx, dy = cr.gradient_u8("sobel", img, True)
    out = cr.corner_box_s16(dx, dy, r, "mocksum")
    pxx, pxy, pyy = cr.products_s32(dx, dy)
    for y in range(r, height - r, 3):
        for x in range(r, width - r, 3):
            assert out[y, x] == np.float32(_manual_box(pxx, x, y, r) + _manual_box(pxy, x, y, r) + _manual_box(pyy, x, y, r))
    assert not out[:r].any() and not out[-r:].any() and not out[:, :r].any() and not out[:, -r:].any()


def test_weighted_s16_compare_to_manual(orc):
    """TestImplSsdCornerWeighted_S16.compareToManual (F:.../intensity/impl/TestImplSsdCornerWeighted_S16.java:55-110): MockSum within 4 of
    the manual weighted sum, and exactly equal to the normalised separable form written pixel by pixel"""
    r, width, height = 4, 40, 50
    img = _u8_frame(orc, width, height, 234) % 100
    dx, dy = cr.gradient_u8("sobel", img, True)
    out = cr.corner_weighted_s16(dx, dy, r, "mocksum")
    k = [int(v) for v in cr.gaussian_kernel_s32(r)]
    planes = cr.products_s32(dx, dy)

    def manual(p, x, y):   # TestImplSsdCornerWeighted_S16.sum
        ret = tw = 0
        for i in range(-r, r + 1):
            hs = sum(int(p[y + i, x + j]) * k[j + r] for j in range(-r, r + 1))
            ws = sum(k)
            ret += int(cr.trunc_div(k[i + r] * hs, ws))
            tw += k[i + r]
        return int(cr.trunc_div(ret, tw))

    for y in range(r, height - r, 5):
        for x in range(r, width - r, 5):
            assert abs(float(out[y, x]) - sum(manual(p, x, y) for p in planes)) <= 4

    def norm_at(p, x, y, axis):
        n = p.shape[1 - axis] if axis == 0 else p.shape[0]
        pos = x if axis == 0 else y
        total = weight = 0
        for t in range(2 * r + 1):
            q = pos - r + t
            if 0 <= q < n:
                v = p[y, q] if axis == 0 else p[q, x]
                total += int(v) * k[t]
                weight += k[t]
        num = int(cr.wrap32(total + weight // 2))
        return num // weight if num >= 0 else -((-num) // weight)

    xx, xy, yy = planes
    for (x, y) in [(0, 0), (3, 7), (39, 49), (20, 1), (38, 25)]:
        sums = []
        for p in planes:
            h = np.array([[norm_at(p, xi, yi, 0) for xi in range(width)] for yi in range(height)], dtype=np.int64)
            sums.append(norm_at(h, x, y, 1))
        assert out[y, x] == np.float32(int(cr.wrap32(sum(sums))))


def test_harris_s32_check_score():
    """TestHarrisCorner_S32.checkScore (F:.../intensity/impl/TestHarrisCorner_S32.java:33-44)"""
    kappa = np.float32(0.04)
    got = cr.score_s32("harris", np.array([50]), np.array([70]), np.array([80]), kappa=kappa)[0]
    expected = np.float32(50 * 80 - 70 * 70) - kappa * np.float32((50 + 80) ** 2)
    assert abs(got - expected) < 1e-4 * abs(expected)


def test_shitomasi_s32_closed_form_on_constant_gradient():
    """a patch with dx = a, dy = b everywhere: XX = n a^2, XY = n a b, YY = n b^2 -> smallest eigenvalue 0"""
    dx = np.full((9, 11), 7, np.int16)
    dy = np.full((9, 11), -3, np.int16)
    out = cr.corner_box_s16(dx, dy, 2, "shitomasi")
    assert np.all(out[2:-2, 2:-2] == 0.0)
    dy[:, :] = 0
    out = cr.corner_box_s16(dx, dy, 2, "shitomasi")   # eigenvalues n a^2 and 0
    assert np.all(out[2:-2, 2:-2] == 0.0)
    out = cr.corner_box_s16(dx, dx, 1, "shitomasi")
    assert np.all(out[1:-1, 1:-1] == 0.0)


def test_gaussian_kernel_s32_matches_the_library():
    import ctypes as C
    from boofcv_amd import _lib
    L = _lib.load()
    for r in range(1, 51):
        want = cr.gaussian_kernel_s32(r)
        w = -L.bhip_gaussian_kernel1d_s32(r, None, 0)
        assert w == 2 * r + 1
        out = np.zeros(w, np.int32)
        assert L.bhip_gaussian_kernel1d_s32(r, out.ctypes.data_as(_lib._i32p), w) == w
        assert np.array_equal(out, want), r
        assert out[r] == out.max() and np.array_equal(out, out[::-1]) and out.min() >= 1
    assert L.bhip_gaussian_kernel1d_s32(0, None, 0) == -1
    small = np.zeros(2, np.int32)
    assert L.bhip_gaussian_kernel1d_s32(3, small.ctypes.data_as(C.POINTER(C.c_int32)), 2) == -7


def test_window_sums_wrap_like_java_int():
    """S16 values near +-32767: the products fit an int, the window sums wrap"""
    dx = np.full((5, 5), 32767, np.int16)
    dy = np.full((5, 5), -32768, np.int16)
    out = cr.corner_box_s16(dx, dy, 2, "mocksum")
    xx, xy, yy = 25 * 32767 * 32767, 25 * 32767 * -32768, 25 * 32768 * 32768
    want = np.int64(xx + xy + yy)
    java = ((int(want) + (1 << 31)) % (1 << 32)) - (1 << 31)
    assert out[2, 2] == np.float32(java)
    # each sum on its own wraps too: XX = 25 * 32767^2 > 2^31
    s = cr.wrap32(cr.box_sum(cr.products_s32(dx, dy)[0], 2))[0, 0]
    assert s == ((25 * 32767 * 32767 + (1 << 31)) % (1 << 32)) - (1 << 31) and s != 25 * 32767 * 32767
    # the truncating division of a negative total
    assert cr.trunc_div(-7, 2) == -3 and cr.trunc_div(7, 2) == 3
    assert cr.conv_norm_s32(np.array([[-5, -5, -5]]), [1, 2, 1], 1).tolist() == [[-4, -4, -4]]   # (-15 + 1) / 3 -> -4, (-20 + 2) / 4 -> -4


def test_factory_weighted_radius_zero_raises():
    from boofcv_amd import api
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryIntensityPointAlg.shiTomasi(0, True, api.GrayS16, ctx=object())
    with pytest.raises(RuntimeError):
        api.FactoryIntensityPointAlg.harris(2, 0.04, False, api.GrayS32, ctx=object())
