"""CPU: tests/klt_u8_ref.py (the yardstick of test_gpu_klt_u8.py) against the reference's own checks, re-expressed, and the conditions the GPU
test scenes must meet, evaluated by the reference alone.

  TestConvolveImageDownNormalized / TestConvolveDownNormalized_JustBorder*: the border form and the naive form agree where both write
      (main/boofcv-ip/src/test/java/boofcv/alg/filter/convolve/, .../convolve/down/)
  TestUtilDownConvolve.java:31-55: the literals tests/test_oracle_known_answers.py already re-expresses for the F32 path
  GeneralBilinearRectangleChecks.java:174: region() against the per-pixel interpolator, tolerance 1e-4 (TestBilinearRectangle_U8 / _S16 extend it)
  TestKltTracker.java / TestPyramidKltTracker.java are written for KltTracker<GrayF32, GrayF32> only (createDefaultTracker :354-365 builds
      GrayF32 interpolators; PyramidKltTestBase allocates GrayF32 pyramids): the reference has no GrayU8 form of them.  Their
      setDescription recipes (outside / NaN count) are type independent and run here on a GrayU8 scene.  Their tracking recipes state
      convergence bounds that hold for the GrayF32 Sobel only: the integer Sobel is four times larger, which quarters every Lucas-Kanade
      step (test_u8_tracker_is_the_f32_tracker_with_derivatives_times_four states that relation exactly instead).

The library divides with plain integer division in every GrayU8 down-convolution kernel; there is no multiply-shift to check."""
import numpy as np
import pytest

import corner_ref
import klt_ref as kr
import klt_u8_ref as ku

F = np.float32


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- down convolution
def test_util_down_convolve_known_answers():   # the literals of test_oracle_known_answers.test_down_convolve_util_known_answers
    for expect, args in [(8, (10, 1, 1)), (7, (10, 1, 2)), (8, (10, 2, 1)), (6, (10, 2, 2)), (6, (10, 2, 3)), (4, (10, 2, 4)),
                         (6, (10, 3, 1)), (6, (10, 3, 2)), (6, (10, 3, 3)), (3, (10, 3, 4)), (4, (11, 4, 2))]:
        assert ku.compute_max_side(*args) == expect
    for expect, args in [(1, (1, 1)), (2, (1, 2)), (3, (1, 3)), (2, (2, 1)), (2, (2, 2)), (4, (2, 3))]:
        assert ku.compute_offset(*args) == expect


def test_kernel_is_1_4_7_4_1():
    assert corner_ref.gaussian_kernel_s32(2).tolist() == [1, 4, 7, 4, 1]


SIZES = [(15, 20), (16, 21), (17, 13), (9, 9), (8, 7), (7, 8), (6, 11), (5, 12), (4, 9), (3, 10), (31, 6), (23, 5)]   # (W, H)


@pytest.mark.parametrize("skip", [1, 2, 3, 4])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_border_form_and_naive_form_agree(skip, radius):
    """on every pixel both write; sizes odd, not divisible by the skip, and widths on both sides of kernel.width"""
    kernel = corner_ref.gaussian_kernel_s32(radius)
    kw = len(kernel)
    compared = switched = 0
    for W, H in SIZES:
        img = _u8((H, W), 100 * W + H + skip)
        for axis in (1, 0):
            side = W if axis == 1 else H
            naive, wn = ku.conv_down_norm_u8(img, kernel, skip, axis, form="naive", return_written=True)
            assert wn.all() and naive.shape == ((H, W // skip) if axis == 1 else (H // skip, W))
            # the switch tests the image WIDTH on both axes
            picked = ku.conv_down_norm_u8(img, kernel, skip, axis) if kw >= W else None
            if picked is not None:
                assert np.array_equal(picked, naive)
                switched += 1
            try:
                border, wb = ku.conv_down_norm_u8(img, kernel, skip, axis, form="border", return_written=True)
            except ValueError:
                # the reference's loops leave the row: only where the kernel is about as wide as the filtered side
                assert side < kw + skip, (W, H, axis)
                continue
            assert wb.any()
            assert np.array_equal(border[wb], naive[wb]), (W, H, axis)
            if kw < W:
                assert np.array_equal(ku.conv_down_norm_u8(img, kernel, skip, axis), border)
            compared += 1
    assert compared >= 12 and (switched >= 1 or radius == 1)


def test_rounding_and_byte_intermediate():
    """(total + weight/2) / weight on a hand case, and the pyramid's intermediate image is a byte image"""
    k = [1, 4, 7, 4, 1]
    row = np.array([[10, 20, 30, 40, 50, 60, 70, 80, 90, 100]], np.uint8)
    out = ku.conv_down_norm_u8(row, k, 2, 1)
    # x = 0: taps 0..2 weights 7,4,1 -> (70 + 80 + 30 + 6) // 12; x = 2, 4, 6: full kernel, divisor 17; x = 8: taps -2..1, weight 16
    assert out.tolist() == [[(180 + 6) // 12, (10 + 80 + 210 + 160 + 50 + 8) // 17, (30 + 160 + 350 + 240 + 70 + 8) // 17,
                             (50 + 240 + 490 + 320 + 90 + 8) // 17, (70 + 320 + 630 + 400 + 8) // 16]]
    img = _u8((41, 27), 5)
    layers = ku.pyramid_u8(img, [1, 2, 4])
    assert [l.shape for l in layers] == [(41, 27), (21, 14), (11, 7)] and all(l.dtype == np.uint8 for l in layers)
    assert np.array_equal(layers[0], img)
    temp = ku.conv_down_norm_u8(img, k, 2, 1)
    assert np.array_equal(layers[1][:20, :13], ku.conv_down_norm_u8(temp, k, 2, 0))
    assert not layers[1][20, :].any() and not layers[1][:, 13].any()        # ceil-sized layer, floor-sized result
    # a layer narrower than the kernel takes the naive form in both passes
    narrow = ku.pyramid_u8(_u8((30, 9), 6), [1, 2, 4])
    t = ku.conv_down_norm_u8(narrow[1], k, 2, 1)
    assert t.shape[1] == 2 and np.array_equal(narrow[2][:7, :2], ku.conv_down_norm_u8(t, k, 2, 0, form="naive"))
    # an un-rounded intermediate would differ: the byte rounding between the passes is observable
    exact = np.zeros((20, 13))
    a = img.astype(np.float64)
    kk = np.array(k, np.float64)
    for Y in range(20):
        for X in range(13):
            ys = [y for y in range(2 * Y - 2, 2 * Y + 3) if 0 <= y < 41]
            xs = [x for x in range(2 * X - 2, 2 * X + 3) if 0 <= x < 27]
            wy, wx = kk[[y - 2 * Y + 2 for y in ys]], kk[[x - 2 * X + 2 for x in xs]]
            exact[Y, X] = (wy @ a[np.ix_(ys, xs)] @ wx) / (wy.sum() * wx.sum())
    assert np.abs(layers[1][:20, :13] - exact).max() <= 1.0 + 1e-9         # two roundings of at most half a level each


# ---------------------------------------------------------------------------------------------------------------- EXTENDED Sobel
@pytest.mark.parametrize("shape", [(37, 23), (256, 9), (3, 3), (1, 5), (5, 1), (2, 2)])
def test_sobel_extended_u8(shape):
    w, h = shape
    img = _u8((h, w), 7 + w)
    ex, ey = ku.sobel_extended_u8(img)
    assert ex.dtype == np.int16 and ey.dtype == np.int16
    # a constant image has a zero gradient everywhere, frame included
    cx, cy = ku.sobel_extended_u8(np.full((h, w), 201, np.uint8))
    assert not cx.any() and not cy.any()
    gx, gy = corner_ref.gradient_u8("sobel", img, False)
    if h > 2 and w > 2:
        assert np.array_equal(ex[1:-1, 1:-1], gx[1:-1, 1:-1]) and np.array_equal(ey[1:-1, 1:-1], gy[1:-1, 1:-1])
    # the zero-padded variant of the same construction is corner_ref's border form
    zx, zy = ku.sobel_border_u8(img, "constant")
    bx, by = corner_ref.gradient_u8("sobel", img, True)
    assert np.array_equal(zx, bx) and np.array_equal(zy, by)


# ---------------------------------------------------------------------------------------------------------------- region
def test_region_on_u8_equals_the_per_pixel_interpolator():   # GeneralBilinearRectangleChecks.java:150-176, tolerance 1e-4
    img = np.random.default_rng(3).integers(0, 20, (40, 30), dtype=np.uint8).astype(np.float32)   # checkRegion: fillUniform(img, rand, 0, 20)
    for tl_x, tl_y, w, h in ((5.4, 6.3, 5, 5), (0.0, 0.0, 7, 3), (10.75, 20.5, 3, 9), (2.1, 30.9, 11, 5)):
        out = kr.region(img, tl_x, tl_y, w, h)
        for y in range(h):
            for x in range(w):
                assert abs(float(out[y, x]) - float(kr.bilinear_pixel(img, F(tl_x) + F(x), F(tl_y) + F(y)))) <= 1e-4
    s16 = np.random.default_rng(4).integers(-20, 20, (40, 30)).astype(np.int16).astype(np.float32)
    out = kr.region(s16, 3.3, 4.6, 5, 5)
    for y in range(5):
        for x in range(5):
            assert abs(float(out[y, x]) - float(kr.bilinear_pixel(s16, F(3.3) + F(x), F(4.6) + F(y)))) <= 1e-4


def test_region_border_cases_by_hand():
    raw = _u8((8, 10), 9)
    img = raw.astype(np.float32)
    # right border: xt + w == W; the last column is the vertical two-tap form of handleBorder
    out = kr.region(img, 6.0, 1.5, 4, 3)
    ay, by = F(0.5), F(0.5)
    for y in range(3):
        assert out[y, 3] == by * F(raw[1 + y, 9]) + ay * F(raw[2 + y, 9])
    assert out[1, 1] == F(0.5) * F(raw[2, 7]) + F(0.0) * F(raw[2, 8]) + F(0.0) * F(raw[3, 8]) + F(0.5) * F(raw[3, 7])
    # bottom only: yt + h == H, not at the right border -- the corner element reads orig.get(xt + regWidth, regHeight), row regHeight of the image
    out = kr.region(img, 2.25, 5.0, 4, 3)
    ax, bx = F(0.25), F(0.75)
    for x in range(3):
        assert out[2, x] == bx * F(raw[7, 2 + x]) + ax * F(raw[7, 3 + x])
    assert out[2, 3] == F(1.0) * F(raw[7, 5]) + F(0.0) * F(raw[2, 6])      # by * XY + ay * Xy with Xy = img[regHeight = 2][xt + regWidth = 6]
    # both: the corner is the pixel itself
    out = kr.region(img, 6.0, 5.0, 4, 3)
    assert out[2, 3] == F(raw[7, 9])


# ---------------------------------------------------------------------------------------------------------------- known answers on U8
W, H = 40, 50   # TestKltTracker: imageWidth, imageHeight


def test_u8_tracker_is_the_f32_tracker_with_derivatives_times_four(orc):
    """kernelDerivX/Y_I32 is 4 x kernelDerivX/Y_F32 (GradientSobel.java:64-74) and nothing divides it back: on a byte-valued image the GrayS16
    derivative templates are exactly 4 x the GrayF32 ones, G exactly 16 x (powers of two: exact in fp32), so a Lucas-Kanade step E/G of the
    GrayU8 tracker is a quarter of the GrayF32 step.  That is the reference's behaviour and the reason the convergence bounds of
    TestKltTracker (0.01 px after at most 30 iterations) are not stated for GrayU8 here: they do not hold for it."""
    img = np.floor(orc.noise_image(W, H, 234, 0, 100).array()).astype(np.uint8)   # TestKltTracker's scene, drawn as integers
    ix, iy = ku.sobel_extended_u8(img)
    fx, fy = kr.sobel_extended(orc, img.astype(np.float32))
    assert np.array_equal(ix.astype(np.float32), fx * F(4)) and np.array_equal(iy.astype(np.float32), fy * F(4))
    cfg = dict(maxPerPixelError=10, maxIterations=30, minDeterminant=0.01, minPositionDelta=0.001)
    ti, tf = kr.KltTracker(kr.KltConfig(**cfg)), kr.KltTracker(kr.KltConfig(**cfg))
    ti.setImage(img.astype(np.float32), ix.astype(np.float32), iy.astype(np.float32))
    tf.setImage(img.astype(np.float32), fx, fy)
    for x, y in ((20.6, 25.1), (W - 4, H - 4), (2, 1), (W - 1.5, 3.25)):
        a, b = kr.KltFeature(3), kr.KltFeature(3)
        a.setPosition(x, y)
        b.setPosition(x, y)
        assert ti.setDescription(a) and tf.setDescription(b)
        vis = ~np.isnan(b.desc)
        assert np.array_equal(np.isnan(a.desc), np.isnan(b.desc)) and np.array_equal(a.desc[vis], b.desc[vis])
        assert np.array_equal(a.derivX[vis], b.derivX[vis] * F(4)) and np.array_equal(a.derivY[vis], b.derivY[vis] * F(4))
        assert (a.Gxx, a.Gyy, a.Gxy) == (b.Gxx * F(16), b.Gyy * F(16), b.Gxy * F(16))
    # one iteration from the same start: the GrayU8 step is the quarter step (position rounding aside)
    one = dict(cfg, maxIterations=1)
    ti.config, tf.config = kr.KltConfig(**one), kr.KltConfig(**one)
    a, b = kr.KltFeature(3), kr.KltFeature(3)
    for f, t in ((a, ti), (b, tf)):
        f.setPosition(20, 25)
        t.setDescription(f)
        f.setPosition(20.5, 25.25)
        t.track(f)
    assert abs((float(a.x) - 20.5) * 4 - (float(b.x) - 20.5)) < 1e-4 and abs((float(a.y) - 25.25) * 4 - (float(b.y) - 25.25)) < 1e-4
    assert abs(float(b.x) - 20.5) > 0.05


def test_set_description_outside_and_nan_count_on_u8():   # TestKltTracker.java:177-185, :219-235
    t = kr.KltTracker(kr.KltConfig(maxPerPixelError=10, maxIterations=30, minDeterminant=0.01, minPositionDelta=0.001))
    z = np.zeros((H, W), np.uint8).astype(np.float32)
    t.setImage(z, z, z)
    f = kr.KltFeature(3)
    f.setPosition(-100, 200)
    assert not t.setDescription(f)
    f.setPosition(2, 1)
    t.setDescription(f)
    assert int(np.isnan(f.desc).sum()) == 19


# ---------------------------------------------------------------------------------------------------------------- the GPU test scenes
# figures of a CPU run of klt_u8_ref.run_case, pinned: test_gpu_klt_u8.py compares the library against these same runs
PINNED = {
    # name: (spawned on frame 0, of them with a NaN-marked template, re-spawned after frame 2, (tracks, iterations, border iterations) of frames 1..3, faults)
    "small_r2": (425, 96, 19, [(430, 11596, 2447), (418, 9013, 1575), (431, 9520, 1911)], {kr.SUCCESS: 1269, kr.OUT_OF_BOUNDS: 8, kr.FAILED: 2}),
    "medium_r3": (425, 135, 65, [(430, 15429, 4038), (389, 7545, 1657), (444, 8836, 2245)],
                  {kr.SUCCESS: 1237, kr.OUT_OF_BOUNDS: 23, kr.FAILED: 2, kr.LARGE_ERROR: 1}),
    "medium_r2_large_error": (386, 86, 332, [(391, 7114, 1624), (61, 1194, 135), (382, 7318, 1425)],
                              {kr.LARGE_ERROR: 487, kr.SUCCESS: 339, kr.OUT_OF_BOUNDS: 6, kr.FAILED: 2}),
    "large_r2": (399, 82, 215, [(404, 16427, 2410), (344, 7346, 984), (554, 11887, 1734)],
                 {kr.SUCCESS: 1244, kr.OUT_OF_BOUNDS: 26, kr.LARGE_ERROR: 21, kr.DRIFTED: 8, kr.FAILED: 3}),
}


@pytest.mark.parametrize("name", list(ku.CASES))
def test_gpu_scene_conditions(orc, name):
    """by the reference alone: no Thrown anywhere (run_case would raise), border-form iterations, NaN-marked templates, and the fault kinds"""
    _, trk, info = ku.run_case(orc, name)
    spawned, nan, respawned, stats, faults = PINNED[name]
    got = (info["spawned"], info["nan"], info["respawned"], [info["stats%d" % k] for k in (1, 2, 3)], dict(info["faults"]))
    print(name, got)
    assert got == (spawned, nan, respawned, stats, faults)
    assert all(info["added"])
    assert info["nan"] >= 50                                   # spawned tracks with a NaN template element
    assert all(s[2] >= 100 for s in stats)                     # Lucas-Kanade iterations in the border form, in every frame
    assert info["faults"][kr.OUT_OF_BOUNDS] >= 1 and info["faults"][kr.FAILED] >= 2   # the two tracks added inside the flat blocks: exact zero determinant
    assert info["steps"] == ["process0", "spawn0", "add", "process1", "process2", "spawn2", "drop", "process3", "dropAll", "spawn3", "reset", "spawn4"]


def test_every_required_fault_kind_occurs_across_the_scenes(orc):
    seen = set()
    for name in ku.CASES:
        seen |= {k for k, v in PINNED[name][4].items() if v > 0}
    assert {kr.SUCCESS, kr.DRIFTED, kr.OUT_OF_BOUNDS, kr.FAILED, kr.LARGE_ERROR} <= seen   # every KltTrackFault


def test_added_tracks_in_flat_blocks_have_exact_zero_gradient_templates(orc):
    fr, _ = ku.frames(orc, (3, -2))
    layers, dx, dy = ku.pyramid_gradient_u8(fr[0], ku.SCALES)
    for (x, y), value in zip(ku.ADDED[:2], (255, 0)):
        ix, iy = int(x), int(y)
        assert (layers[0][iy - 3:iy + 5, ix - 3:ix + 5] == value).all()
        assert not dx[0][iy - 2:iy + 4, ix - 2:ix + 4].any() and not dy[0][iy - 2:iy + 4, ix - 2:ix + 4].any()
