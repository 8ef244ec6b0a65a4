"""CPU: tests/klt_ref.py (the yardstick of test_gpu_klt.py) against the reference's own known answers -- TestKltTracker.java, TestPyramidKltTracker.java
(main/boofcv-feature/src/test/java/boofcv/alg/tracker/klt/), GeneralBilinearRectangleChecks.java (main/boofcv-ip/src/test/java/boofcv/alg/interpolate/impl/)
-- and the checks of the KLT C ABI that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import klt_ref as kr

F = np.float32
W, H = 40, 50   # TestKltTracker: imageWidth, imageHeight


def _default_config():   # TestKltTracker.createDefaultTracker :354-365
    return kr.KltConfig(maxPerPixelError=10, maxIterations=30, minDeterminant=0.01, minPositionDelta=0.001)


@pytest.fixture()
def noise_tracker(orc):
    """fillUniform(image, new Random(234), 0, 100) + GradientSobel with BorderIndex1D_Extend, as the tracking tests of TestKltTracker start"""
    img = orc.noise_image(W, H, 234, 0, 100).array().copy()
    dx, dy = kr.sobel_extended(orc, img)
    t = kr.KltTracker(_default_config())
    t.setImage(img, dx, dy)
    return t


def test_chain_is_the_sequential_fp32_sum():
    v = (np.random.default_rng(3).standard_normal(225) * 1e3).astype(np.float32)
    s = F(0)
    for x in v:
        s = F(s + x)
    assert kr.chain(v).dtype == np.float32 and kr.chain(v) == s
    assert kr.chain(v[:0]) == 0


@pytest.mark.parametrize("shape", [(37, 23), (3, 3), (1, 5), (5, 1), (2, 2)])
def test_border_construction_matches_the_oracle_for_the_zero_border(orc, shape):
    """sobel_border is the construction the EXTENDED frame is taken from; with zero padding its frame must be the oracle's ImageBorderValue(0) frame"""
    w, h = shape
    img = orc.noise_image(w, h, 5 + w, 0, 255).array().copy()
    gx, gy = orc.gradient("sobel", orc.Gray.from_array(img), True)
    bx, by = kr.sobel_border(img, "constant")
    frame = np.ones((h, w), bool)
    if h > 2 and w > 2:
        frame[1:-1, 1:-1] = False
    assert np.array_equal(bx[frame], gx.array()[frame]) and np.array_equal(by[frame], gy.array()[frame])
    ex, ey = kr.sobel_extended(orc, img)
    if h > 2 and w > 2:   # interior untouched, and equal to the unfactored nine-tap sum within rounding
        assert np.array_equal(ex[1:-1, 1:-1], gx.array()[1:-1, 1:-1])
    # a constant image has a zero gradient everywhere with the EXTENDED border (and not with the zero border)
    cx, cy = kr.sobel_extended(orc, np.full((h, w), 7, np.float32))
    assert not cx.any() and not cy.any()


# ---- TestKltTracker.java ----
def test_tracking_border1(noise_tracker):   # :106-137
    t = noise_tracker
    f = kr.KltFeature(3)
    f.setPosition(W - 4, H - 4)
    t.setDescription(f)
    f.setPosition(W - 2, H - 1)
    assert t.track(f) == kr.SUCCESS
    assert abs(f.x - (W - 4)) < 0.01 and abs(f.y - (H - 4)) < 0.01
    f.setPosition(3, 3)
    t.setDescription(f)
    f.setPosition(1, 2)
    assert t.track(f) == kr.SUCCESS
    assert abs(f.x - 3) < 0.01 and abs(f.y - 3) < 0.01


def test_tracking_border2(noise_tracker):   # :142-172
    t = noise_tracker
    f = kr.KltFeature(3)
    f.setPosition(W - 3 - 1 + 2, H - 3 - 1 + 1)
    t.setDescription(f)
    f.setPosition(W - 3 - 1, H - 3 - 1)
    assert t.track(f) == kr.SUCCESS
    assert abs(f.x - (W - 3 - 1 + 2)) < 0.01 and abs(f.y - (H - 3 - 1 + 1)) < 0.01
    f.setPosition(2, 1)
    t.setDescription(f)
    f.setPosition(3, 3)
    assert t.track(f) == kr.SUCCESS
    assert abs(f.x - 2) < 0.01 and abs(f.y - 1) < 0.01


def test_set_description_outside_fail_and_border_nan():   # :177-185, :219-235
    t = kr.KltTracker(_default_config())
    z = np.zeros((H, W), np.float32)
    t.setImage(z, z, z)
    f = kr.KltFeature(3)
    f.setPosition(-100, 200)
    assert not t.setDescription(f)
    f.setPosition(2, 1)
    t.setDescription(f)
    assert int(np.isnan(f.desc).sum()) == 19


def test_set_description_compare(noise_tracker):   # :190-214: the border form on an inside feature gives the inside form's templates
    t = noise_tracker
    a, b = kr.KltFeature(3), kr.KltFeature(3)
    a.setPosition(20.6, 25.1)
    b.setPosition(20.6, 25.1)
    t._bounds(a)
    t._setDescriptionInside(a)
    t._setDescriptionBorder(b)
    for k in ("desc", "derivX", "derivY"):
        assert np.array_equal(getattr(a, k), getattr(b, k))


def test_detect_bad_feature(noise_tracker):   # :241-254
    f = kr.KltFeature(2)
    f.setPosition(20, 20)
    assert noise_tracker.track(f) != kr.SUCCESS


def test_compare_computeGandE_border_to_inside_image(noise_tracker):   # :256-289
    t = noise_tracker
    f = kr.KltFeature(2)
    f.setPosition(20, 22)
    t.setDescription(f)
    tD, tX, tY = f.desc.reshape(-1), f.derivX.reshape(-1), f.derivY.reshape(-1)

    def inside(x, y):   # computeE
        d = tD - kr.region(t.image, F(x) - F(2), F(y) - F(2), 5, 5).reshape(-1)
        return kr.chain(d * tX), kr.chain(d * tY)

    def border(x, y):   # computeGandE_border
        x0, y0, x1, y1, sx, sy = t._subBounds(f, F(x), F(y))
        cur = np.full((5, 5), np.nan, np.float32)
        cur[y0:y1, x0:x1] = kr.region(t.image, sx, sy, x1 - x0, y1 - y0)
        ok = ~(np.isnan(tD) | np.isnan(cur.reshape(-1)))
        d = tD[ok] - cur.reshape(-1)[ok]
        return int(ok.sum()), kr.chain(d * tX[ok]), kr.chain(d * tY[ok]), kr.chain(tX[ok] * tX[ok]), kr.chain(tX[ok] * tY[ok]), kr.chain(tY[ok] * tY[ok])

    Ex, Ey = inside(21, 23)
    assert f.Gxx != 0 and Ey != 0
    n, _, _, Gxx, Gxy, Gyy = border(20, 22)
    assert n == 25 and (Gxx, Gxy, Gyy) == (f.Gxx, f.Gxy, f.Gyy)
    n, bEx, bEy, _, _, _ = border(21, 23)
    assert n == 25 and (bEx, bEy) == (Ex, Ey)


def test_is_fully_inside_and_outside():   # :308-352
    t = kr.KltTracker()
    t.image = np.zeros((H, W), np.float32)
    r = 2
    t._bounds(kr.KltFeature(r))
    assert t.isFullyInside(F(W // 2), F(H // 2)) and t.isFullyInside(F(2), F(2)) and t.isFullyInside(F(W - 3), F(H - 3))
    assert not t.isFullyInside(F(1.99), F(H // 2)) and not t.isFullyInside(F(W / 2), F(1.99))
    assert not t.isFullyInside(F(W - 2.99), F(H - 3)) and not t.isFullyInside(F(W - 3), F(H - 2.99))
    assert not t.isFullyInside(F(-W // 2), F(H // 2)) and not t.isFullyInside(F(W // 2), F(-H // 2))
    assert not t.isFullyOutside(F(-r), F(-r)) and not t.isFullyOutside(F(W // 2), F(H // 2)) and not t.isFullyOutside(F(W + r - 1), F(H + r - 1))
    assert t.isFullyOutside(F(W // 2), F(1000)) and t.isFullyOutside(F(1000), F(H // 2))
    assert t.isFullyOutside(F(-r - 0.001), F(-r)) and t.isFullyOutside(F(-r), F(-r - 0.001))
    assert t.isFullyOutside(F(W + r - 0.999), F(H + r - 1)) and t.isFullyOutside(F(W + r - 1), F(H + r - 0.999))


# ---- TestPyramidKltTracker.java (PyramidKltTestBase: 50x60, Random(234), scales 1,2,4, radius 2, corner at 20,22) ----
PW, PH, CORNER_X, CORNER_Y, RADIUS = 50, 60, 20, 22, 2


def _pyramid_tracker(orc, retarget=False):
    rand = orc.JavaRandom(234)
    img = rand.fillUniform(orc.Gray(PW, PH), 0, 10).array().copy()
    img[CORNER_Y:CORNER_Y + 20, CORNER_X:CORNER_X + 20] = 100      # ImageMiscOps.fillRectangle(image, 100, cornerX, cornerY, 20, 20)
    if retarget:   # setTargetLocation :40-48
        img = rand.fillUniform(orc.Gray(PW, PH), 0, 1).array().copy()
        img[CORNER_Y:CORNER_Y + 20, CORNER_X:CORNER_X + 20] = 100
    layers, dx, dy = kr.pyramid_gradient(orc, img, [1, 2, 4])
    t = kr.PyramidKltTracker(kr.KltTracker(_default_config()), [1, 2, 4])
    t.setImage(layers, dx, dy)
    return t


def test_pyramid_set_description(orc):   # :53-96
    t = _pyramid_tracker(orc)
    f = kr.PyramidKltFeature(3, RADIUS)
    f.setPosition(25, 20)
    assert t.setDescription(f) and all(d.Gxx != 0 for d in f.desc)
    f = kr.PyramidKltFeature(3, RADIUS)
    f.setPosition(RADIUS - 1, RADIUS - 1)
    assert t.setDescription(f) and all(d.x != 0 and d.y != 0 and d.Gxx != 0 for d in f.desc)
    f = kr.PyramidKltFeature(3, RADIUS)
    f.setPosition(-RADIUS - 1, -RADIUS - 1)
    assert not t.setDescription(f)


@pytest.mark.parametrize("ox,oy", [(-1.3, 1.2), (-5.4, 5.3)])
def test_pyramid_track_offsets(orc, ox, oy):   # track_smallOffset :103-119, track_largeOffset :126-142
    t = _pyramid_tracker(orc)
    f = kr.PyramidKltFeature(3, RADIUS)
    f.setPosition(CORNER_X, CORNER_Y)
    t.setDescription(f)
    f.setPosition(F(CORNER_X) + F(ox), F(CORNER_Y) + F(oy))
    assert t.track(f) == kr.SUCCESS
    assert abs(f.x - CORNER_X) < 0.2 and abs(f.y - CORNER_Y) < 0.2


def test_pyramid_track_border(orc):   # :147-164
    t = _pyramid_tracker(orc)
    tx, ty = PW - RADIUS, PH - RADIUS - 3
    f = kr.PyramidKltFeature(3, RADIUS)
    f.setPosition(tx, ty)
    t.setDescription(f)
    f.setPosition(PW - RADIUS + 2, PH - RADIUS - 1)
    assert t.track(f) == kr.SUCCESS
    assert abs(f.x - tx) < 0.2 and abs(f.y - ty) < 0.2


def test_pyramid_track_oob_and_large_error(orc):   # :169-202
    t = _pyramid_tracker(orc, retarget=True)
    f = kr.PyramidKltFeature(3, 4)
    f.setPosition(21, 22)
    t.setDescription(f)
    f.setPosition(-20, -20)
    assert t.track(f) == kr.OUT_OF_BOUNDS
    f = kr.PyramidKltFeature(3, 4)
    f.setPosition(21, 22)
    t.setDescription(f)
    f.desc[0].desc[0, 0] = 1000
    assert t.track(f) == kr.LARGE_ERROR


# ---- GeneralBilinearRectangleChecks.java ----
@pytest.mark.parametrize("x,y", [(2.11, 5.23), (0, 0), (320 - 10 - 1, 240 - 15 - 1)])
def test_region_against_per_pixel_bilinear(orc, x, y):   # checkCenter, checkBottomRightEdge :69-81,151-177
    img = orc.noise_image(320, 240, 0xff34, 0, 20).array().copy()
    out = kr.region(img, x, y, 10, 15)
    for j in range(15):
        for i in range(10):
            assert abs(float(kr.bilinear_pixel(img, F(i) + F(x), F(j) + F(y))) - float(out[j, i])) < 1e-4, (i, j)


def test_region_outside_the_image_throws():   # :84-115
    img = np.zeros((240, 320), np.float32)
    with pytest.raises(kr.Thrown):
        kr.region(img, 319, 239, 20, 20)
    small = np.zeros((25, 20), np.float32)
    for c in (-0.1, 0.1):
        with pytest.raises(kr.Thrown):
            kr.region(small, c, c, 20, 25)


def test_region_touching_the_image_border(orc):
    """handleBorder: a patch that ends on the last column / row takes the two-tap forms; integer corners copy the pixels"""
    img = orc.noise_image(12, 9, 3, 0, 50).array().copy()
    assert np.array_equal(kr.region(img, 5, 2, 7, 7), img[2:9, 5:12])        # right and bottom border, ax = ay = 0
    out = kr.region(img, 5, F(1.5), 7, 7)                                    # right border only
    assert np.array_equal(out[:, 6], F(0.5) * img[1:8, 11] + F(0.5) * img[2:9, 11])


# ---- C ABI checks that need no GPU ----
def test_klt_cfg_default_matches_klt_config():
    from boofcv_amd import _lib
    c = _lib.KltCfg(9, 9, 9, 9, 9)
    _lib.load().bhip_klt_cfg_default(C.byref(c))
    assert (c.forbiddenBorder, c.maxPerPixelError, c.maxIterations) == (0, 25.0, 15)     # KltConfig.java:32-49
    assert F(c.minDeterminant) == F(0.001) and F(c.minPositionDelta) == F(0.01)
    from boofcv_amd import api
    k = api.KltConfig()
    assert (k.forbiddenBorder, k.maxPerPixelError, k.maxIterations, k.minDeterminant, k.minPositionDelta) == (0, 25.0, 15, 0.001, 0.01)
    p = api.PkltConfig()
    assert p.templateRadius == 2 and p.pyramidScaling == [1, 2, 4]                       # PkltConfig.java:28-34
    assert (api.KltTrackFault.SUCCESS, api.KltTrackFault.DRIFTED, api.KltTrackFault.OUT_OF_BOUNDS, api.KltTrackFault.FAILED,
            api.KltTrackFault.LARGE_ERROR) == (0, 1, 2, 3, 4)                            # KltTrackFault.java:28-44
    assert api.ConfigGeneralDetector().maxFeatures == -1


def test_klt_create_refuses_dead_contexts_and_unsupported_sizes():
    from boofcv_amd import _lib
    L = _lib.load()
    junk = C.create_string_buffer(4096)
    p = C.c_void_p(C.addressof(junk))
    scales = (C.c_int * 8)(1, 2, 4, 8, 16, 32, 64, 128)
    h = C.c_void_p(1)
    assert L.bhip_klt_create(p, None, 2, scales, 3, 3, 1.0, 0, 320, 240, 1, C.byref(h)) == _lib.BHIP_ERR_INVALID and not h.value
    assert L.bhip_klt_create(None, None, 2, scales, 3, 3, 1.0, 0, 320, 240, 1, C.byref(h)) == _lib.BHIP_ERR_INVALID
    for radius, layers in ((0, 3), (8, 3), (2, 0), (2, 9)):
        h = C.c_void_p(1)
        assert L.bhip_klt_create(p, None, radius, scales, layers, 3, 1.0, 0, 320, 240, 1, C.byref(h)) == _lib.BHIP_ERR_UNSUPPORTED and not h.value
    assert L.bhip_klt_destroy(p) == _lib.BHIP_ERR_INVALID and L.bhip_klt_destroy(None) == _lib.BHIP_OK
    for fn in (L.bhip_klt_drop_all, L.bhip_klt_reset):
        assert fn(None) == _lib.BHIP_ERR_INVALID
    # the stage-level calls answer an unsupported radius before anything is written
    img = np.zeros(100, np.float32)
    fp = img.ctypes.data_as(_lib._fp)
    out = np.full(3 * 17 * 17, 5, np.float32)
    ok = np.full(1, 7, np.uint8)
    xy = np.zeros(2, np.float32)
    for radius in (0, 8):
        st = L.bhip_klt_set_description_f32(None, None, radius, fp, 0, 10, fp, fp, 0, 10, 10, 10, xy.ctypes.data_as(_lib._fp), 1, out.ctypes.data_as(_lib._fp),
                                            out.ctypes.data_as(_lib._fp), out.ctypes.data_as(_lib._fp), out.ctypes.data_as(_lib._fp), ok.ctypes.data_as(_lib._u8p))
        assert st == _lib.BHIP_ERR_UNSUPPORTED and (out == 5).all() and ok[0] == 7
