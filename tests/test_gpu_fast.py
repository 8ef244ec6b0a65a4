"""GPU: the FAST-9..12 corner detector (GrayU8 / GrayF32), the strict Min / Max / MinMax block non-maximum suppression and
GeneralFeatureDetector over both, bit for bit against tests/fast_ref.py, through the host-buffer API (api.py), the device-batched API
(device.py) and the C ABI.  Every comparison is exact: intensity bit patterns, both lists with their order, counts."""
import ctypes as C
import functools

import numpy as np
import pytest

import fast_ref as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _u8(w, h, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, size=(h, w), dtype=np.uint8)


def _checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx // 8) + (yy // 8)) & 1) * 255).astype(np.uint8)


def _squares(w, h, size=4, pitch=8):
    """white size x size squares on black, the right half inverted: dark and bright corners with equal scores inside one NMS window (the
    junctions of a checkerboard, whose ring alternates by quadrant, are no FAST-9 corners at all)"""
    yy, xx = np.mgrid[0:h, 0:w]
    img = (((xx % pitch) < size) & ((yy % pitch) < size)).astype(np.uint8) * 255
    img[:, w // 2:] = 255 - img[:, w // 2:]
    return img


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(api, img, tol, n, fraction, intensity=True, sub=False):
    """FastCornerDetector through api.py -> (intensity array | None, low, high)"""
    T = api.GrayU8 if img.dtype == np.uint8 else api.GrayF32
    H, W = img.shape
    src = T.wrap(img)
    if sub:   # a view with an odd startIndex and stride > width
        big = T(W + 5, H + 3)
        src = big.subimage(1, 2, 1 + W, 2 + H)
        src.array()[:, :] = img
    alg = api.FactoryIntensityPointAlg.fast(tol, n, T)
    alg.setMaxFeaturesFraction(fraction)
    out = api.GrayF32(W, H) if intensity else None
    if intensity:
        out.data[:] = -7.0   # every pixel of the view is written
        alg.process(src, out)
    else:
        alg.process(src)
    return (out.array().copy() if intensity else None), alg.lowXY.copy(), alg.highXY.copy()


def _same(got, want):
    inten, low, high = got
    winten, wlow, whigh, _ = want
    assert np.array_equal(low, wlow), "dark corners differ"
    assert np.array_equal(high, whigh), "bright corners differ"
    if winten is not None:
        assert np.array_equal(_bits(inten), _bits(winten)), "intensity differs"


def _u8_inputs(w, h):
    """(image, tol, fraction) of every GrayU8 input class"""
    noise = _u8(w, h, 1000 * w + h)
    return [(noise, 20, 0.1), (noise, 40, 0.1), (noise, 20, 1.0), (noise, 20, 1e-9), (noise, 0, 0.1), (noise, 255, 0.1),
            (np.full((h, w), 93, np.uint8), 20, 0.1), (_checker(w, h), 20, 1.0), (_squares(w, h), 20, 1.0)]


SHAPES = [(7, 7), (6, 9), (9, 6), (12, 14), (67, 41), (261, 35), (256, 9)]
U8_CASES = [(s, n) for s in SHAPES for n in (9, 12)] + [((261, 35), 10), ((261, 35), 11)]


@pytest.mark.parametrize("shape,n", U8_CASES)
def test_fast_u8(api, shape, n):
    W, H = shape
    for img, tol, fraction in _u8_inputs(W, H):
        _same(_run(api, img, tol, n, fraction), fr.fast(img, tol, n, fraction))


def test_fast_u8_counts_of_the_input_classes():
    """the inputs above do what they are there for (reference only): the default fraction stops early on noise, a tiny fraction keeps row 3
    only, tol 255 / a constant image / the checkerboard have no corners, the squares have corners of both polarities with equal scores inside
    one NMS window (tol 40 without a stop: the 97x64 test)"""
    img = _u8(67, 41, 1000 * 67 + 41)
    _, low, high, stop = fr.fast(img, 20, 9, 0.1)
    assert len(low) + len(high) >= fr.max_features(0.1, 67, 41) == 274 and stop < 41 - 4
    assert fr.fast(img, 20, 9, 1e-9)[3] == 3 and fr.fast(img, 20, 9, 1.0)[3] == 41 - 4
    assert len(fr.fast(img, 255, 9, 0.1)[1]) == 0 and len(fr.fast(np.full((41, 67), 93, np.uint8), 20, 9, 0.1)[2]) == 0
    assert not fr.fast(_checker(67, 41), 20, 9, 1.0)[0].any()
    inten, low, high, _ = fr.fast(_squares(67, 41), 20, 9, 1.0)
    assert len(low) > 50 and len(high) > 50
    tied = [(x, y) for x, y in np.concatenate([low, high]) if (inten[y - 2:y + 3, x - 2:x + 3] == inten[y, x]).sum() > 1]
    assert len(tied) > 50


@pytest.mark.parametrize("n", [9, 12])
def test_fast_u8_reference_naive_test_size(api, n):
    """GenericFastCorner.compareToNaiveDetection's image: 40x50, U[0,50), tol 10"""
    img = _u8(40, 50, 234, hi=50)
    want = fr.fast(img, 10, n, 1.0)
    assert n == 12 or (len(want[1]) > 20 and len(want[2]) > 20)
    _same(_run(api, img, 10, n, 1.0), want)


def test_fast_u8_no_stop_97x64(api):
    img = _u8(97, 64, 5)
    want = fr.fast(img, 40, 10, 0.1)
    assert want[3] == 64 - 4 and 0 < len(want[1]) + len(want[2]) < fr.max_features(0.1, 97, 64) == 620
    _same(_run(api, img, 40, 10, 0.1), want)


@pytest.mark.parametrize("n", [9, 12])
def test_fast_u8_perfect_circle(api, n):
    """GenericFastCorner.perfectCircle on the GPU, all 16 rotations, both polarities"""
    w, h = 12, 14
    for high in (True, False):
        for i in range(16):
            img = np.full((h, w), 99, np.uint8)
            for j in range(n):
                dx, dy = fr.CIRCLE[(i + j) % 16]
                img[h // 2 + dy, w // 2 + dx] = 255 if high else 0
            img[h // 2, w // 2] = 100
            inten, low, hi = _run(api, img, 20, n, 1.0)
            assert np.array_equal(hi if high else low, [[w // 2, h // 2]])
            if n == 9 and high:
                assert inten[h // 2, w // 2] == 1395.0


def test_fast_u8_vga_early_stop(api):
    img = _u8(640, 480, 77)
    want = fr.fast(img, 20, 9, 0.1)
    assert 3 < want[3] < 300   # the default fraction stops well inside the frame
    _same(_run(api, img, 20, 9, 0.1), want)


def _f32_inputs(w, h):
    rng = np.random.default_rng(31 * w + h)
    return [((rng.random((h, w)) * 100).astype(np.float32), 7.5), ((rng.random((h, w)) * 100 - 50).astype(np.float32), 7.5),
            (rng.random((h, w)).astype(np.float32), 0.2)]


@pytest.mark.parametrize("shape,n", [((7, 7), 9), ((12, 14), 12), ((67, 41), 9), ((67, 41), 12), ((261, 35), 9), ((261, 35), 10), ((261, 35), 11),
                                     ((261, 35), 12), ((256, 9), 9)])
def test_fast_f32(api, shape, n):
    W, H = shape
    for k, (img, tol) in enumerate(_f32_inputs(W, H)):
        for fraction in (0.1, 1.0):
            want = fr.fast(img, tol, n, fraction)
            _same(_run(api, img, tol, n, fraction, sub=(k == 1)), want)
        if k == 2 and W == 67 and n == 9:   # U[0,1): the int total truncates to 0, so bright corners score below zero
            inten = want[0]
            assert len(want[2]) > 0 and all(inten[y, x] < 0 for x, y in want[2])


def test_fast_f32_truncation_literals(api):
    for centre, ring, tol in ((0.1, 0.4, 0.2), (10.0, -2.5, 1.0)):
        img = np.full((7, 7), centre, np.float32)
        for dx, dy in fr.CIRCLE[:9]:
            img[3 + dy, 3 + dx] = ring
        _same(_run(api, img, tol, 9, 1.0), fr.fast(img, tol, 9, 1.0))


# ---- views ----
@pytest.mark.parametrize("shape", [(67, 41), (261, 35), (12, 14)])
def test_fast_u8_subimage_and_intensity_view(api, shape):
    """input: a sub-image with an odd startIndex and stride; intensity: a view into a larger buffer, whose other bytes stay as they were"""
    W, H = shape
    img = _u8(W, H, 3 * W + H)
    want = fr.fast(img, 20, 9, 0.1)
    _same(_run(api, img, 20, 9, 0.1, sub=True), want)
    big = api.GrayF32(W + 6, H + 4)
    big.data[:] = 123.25
    view = big.subimage(5, 1, 5 + W, 1 + H)
    alg = api.FactoryIntensityPointAlg.fast(20, 9, api.GrayU8)
    alg.setMaxFeaturesFraction(0.1)
    alg.process(api.GrayU8.wrap(img), view)
    got = view.array()
    assert np.array_equal(_bits(got), _bits(want[0]))
    assert not got[:3].any() and not got[-3:].any() and not got[:, :3].any() and not got[:, -3:].any() and not got[want[3] + 1:].any()
    outside = np.ones((H + 4, W + 6), bool)
    outside[1:1 + H, 5:5 + W] = False
    assert np.all(big.data.reshape(H + 4, W + 6)[outside] == 123.25)
    assert np.array_equal(alg.lowXY, want[1]) and np.array_equal(alg.highXY, want[2])
    # the list objects of the reference interface
    assert [(p.x, p.y) for p in alg.getCornersLow()] == [tuple(p) for p in want[1].tolist()]
    assert alg.getRadius() == 3 and alg.getIgnoreBorder() == 3 and alg.getMaxFeaturesFraction() == 0.1


def test_fast_without_intensity_gives_the_same_lists(api):
    img = _u8(261, 35, 8)
    want = fr.fast(img, 20, 9, 0.1, intensity=False)
    _same(_run(api, img, 20, 9, 0.1, intensity=False), want)
    det = api.FactoryDetectPoint.createFast(api.ConfigFastCorner(20, 9, 0.1), api.GrayU8)   # WrapFastToPointDetector
    det.process(api.GrayU8.wrap(img))
    assert det.totalSets() == 2
    assert [(p.x, p.y) for p in det.getPointSet(0)] == [tuple(p) for p in want[1].tolist()]
    assert [(p.x, p.y) for p in det.getPointSet(1)] == [tuple(p) for p in want[2].tolist()]
    with pytest.raises(api.IllegalArgumentException):
        det.getPointSet(2)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_fast_device_batch_with_odd_image_stride(api, dev, kind):
    """5 frames of 261x35 inside one buffer: first byte at an odd offset, rows 263 elements apart, frames an odd number of elements apart"""
    ops, torch = dev
    W, H, B, stride = 261, 35, 5, 263
    frame = stride * H + 1
    if kind == "u8":
        imgs = [_u8(W, H, 50 + b) for b in range(B)]
        tol, dt = 20, torch.uint8
    else:
        imgs = [_f32_inputs(W, H)[b % 3][0] for b in range(B)]
        tol, dt = 7.5, torch.float32
    buf = torch.zeros(1 + frame * B, dtype=dt, device=ops.device)
    src = torch.as_strided(buf, (B, H, W), (frame, stride, 1), 1)
    src.copy_(torch.from_numpy(np.stack(imgs)).to(ops.device))
    assert kind == "f32" or (src.data_ptr() % 4 == 1 and frame % 4 != 0)
    for n, fraction in ((9, 0.1), (12, 1.0)):
        inten, xyLow, nLow, xyHigh, nHigh = ops.fast(src, tol, n, fraction)
        ops.ctx.synchronize()
        inten, xyLow, nLow, xyHigh, nHigh = (t.cpu().numpy() for t in (inten, xyLow, nLow, xyHigh, nHigh))
        for b in range(B):
            _same((inten[b], xyLow[b, :nLow[b]], xyHigh[b, :nHigh[b]]), fr.fast(imgs[b], tol, n, fraction))
            _same(_run(api, imgs[b], tol, n, fraction), (inten[b], xyLow[b, :nLow[b]], xyHigh[b, :nHigh[b]], None))   # five single calls
    # process(image): no intensity
    none, xyLow2, nLow2, xyHigh2, nHigh2 = ops.fast(src, tol, 12, 1.0, intensity=False)
    ops.ctx.synchronize()
    assert none is None and np.array_equal(nLow2.cpu().numpy(), nLow) and np.array_equal(xyHigh2.cpu().numpy()[0, :nHigh[0]], xyHigh[0, :nHigh[0]])


def test_fast_cap_smaller_than_the_count(api, dev):
    ops, torch = dev
    img = _u8(67, 41, 12)
    _, wlow, whigh, _ = fr.fast(img, 20, 9, 1.0)
    cap = 10
    assert len(wlow) > cap and len(whigh) > cap
    # device form: counts exact, the first cap pairs written, nothing after them
    src = torch.from_numpy(img[None]).to(ops.device)
    xy = torch.full((2, 64, 2), -5, dtype=torch.int16, device=ops.device)
    cnt = torch.full((2,), -1, dtype=torch.int32, device=ops.device)
    st = ops.L.bhip_fast_dev_u8(ops.ctx._h, C.c_void_p(src.data_ptr()), 67 * 41, 67, 67, 41, 1, 20, 9, 1.0, None, 0, 0, C.c_void_p(xy[0].data_ptr()),
                                C.c_void_p(cnt[0:].data_ptr()), C.c_void_p(xy[1].data_ptr()), C.c_void_p(cnt[1:].data_ptr()), cap)
    assert st == 0
    ops.ctx.synchronize()
    xy, cnt = xy.cpu().numpy(), cnt.cpu().numpy()
    assert list(cnt) == [len(wlow), len(whigh)]
    assert np.array_equal(xy[0, :cap], wlow[:cap]) and np.array_equal(xy[1, :cap], whigh[:cap]) and np.all(xy[:, cap:] == -5)
    # host form
    from boofcv_amd import _lib
    low, high = np.full((64, 2), -5, np.int16), np.full((64, 2), -5, np.int16)
    nLow, nHigh = C.c_int(-1), C.c_int(-1)
    ctx = api.Context.default()
    st = _lib.load().bhip_fast_u8(ctx._h, img.ctypes.data_as(_lib._u8p), 0, 67, 67, 41, 20, 9, 1.0, None, 0, 0, low.ctypes.data_as(_lib._i16p), C.byref(nLow),
                                  high.ctypes.data_as(_lib._i16p), C.byref(nHigh), cap)
    assert st == 0 and (nLow.value, nHigh.value) == (len(wlow), len(whigh))
    assert np.array_equal(low[:cap], wlow[:cap]) and np.array_equal(high[:cap], whigh[:cap]) and np.all(low[cap:] == -5) and np.all(high[cap:] == -5)


# ---- NMS ----
@functools.lru_cache(maxsize=None)
def _nms_images():
    inten = fr.fast(_u8(67, 41, 21), 20, 9, 1.0)[0]
    marked = inten.copy()
    rng = np.random.default_rng(3)
    for k in range(40):
        marked[rng.integers(0, 41), rng.integers(0, 67)] = fr.FLOAT_MAX if k & 1 else -fr.FLOAT_MAX
    ys, xs = np.nonzero(inten > 0)
    marked[ys[0], xs[0]] = fr.FLOAT_MAX      # markers on corners too, as the KLT exclusion list puts them
    ys, xs = np.nonzero(inten < 0)
    marked[ys[0], xs[0]] = -fr.FLOAT_MAX
    return inten, marked, fr.fast(_squares(67, 41), 20, 9, 1.0)[0]   # the last one: ties inside the windows


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("border", [0, 3, 5])
def test_nonmax_min_max(api, dev, radius, border):
    ops, torch = dev
    from boofcv_amd import _lib
    L = _lib.load()
    ctx = api.Context.default()
    images = _nms_images()
    batch = torch.from_numpy(np.stack(images)).to(ops.device)
    for threshold in (0.0, 50.0):
        want = [fr.nonmax_block(im, radius, -threshold, threshold, border, True, True) for im in images]
        assert len(want[0][0]) > 0 and len(want[0][1]) > 0
        assert len(want[2][0]) + len(want[2][1]) < 20 < np.count_nonzero(images[2])   # hundreds of corners, nearly all tied inside a window: dropped
        for dmin, dmax in ((True, False), (False, True), (True, True)):
            # device form, both images as one batch
            xyMin, nMin, xyMax, nMax = ops.nonmaxMinMax(batch, radius, -threshold, threshold, border, dmin, dmax)
            ops.ctx.synchronize()
            xyMin, nMin, xyMax, nMax = (t.cpu().numpy() for t in (xyMin, nMin, xyMax, nMax))
            for b, im in enumerate(images):
                wmin, wmax = want[b][0] if dmin else want[b][0][:0], want[b][1] if dmax else want[b][1][:0]
                assert np.array_equal(xyMin[b, :nMin[b]], wmin) and np.array_equal(xyMax[b, :nMax[b]], wmax), (threshold, dmin, dmax, b, "device")
                # host form through the extractor of the reference's factory
                e = api.FactoryFeatureExtractor.nonmax(api.ConfigExtract(radius, threshold, border, True, dmin, dmax))
                assert (e.canDetectMinimums(), e.canDetectMaximums()) == (dmin, dmax)
                fmin, fmax = [api.Point2D_I16(1, 1)], [api.Point2D_I16(2, 2)]
                e.process(api.GrayF32.wrap(im), None, None, fmin, fmax)
                assert np.array_equal(e.foundMinXY, wmin) and np.array_equal(e.foundMaxXY, wmax), (threshold, dmin, dmax, b, "host")
                assert [(p.x, p.y) for p in fmin] == [tuple(p) for p in wmin.tolist()] and [(p.x, p.y) for p in fmax] == [tuple(p) for p in wmax.tolist()]
        # maxima only == the existing maxima entry point
        for b, im in enumerate(images):
            cap = 67 * 41
            old, new = np.zeros((cap, 2), np.int16), np.zeros((cap, 2), np.int16)
            nOld, nNew = C.c_int(), C.c_int()
            flat = np.ascontiguousarray(im)
            assert L.bhip_nonmax_block_f32(ctx._h, flat.ctypes.data_as(_lib._fp), 0, 67, 67, 41, radius, threshold, border, old.ctypes.data_as(_lib._i16p), cap,
                                           C.byref(nOld)) == 0
            assert L.bhip_nonmax_block_minmax_f32(ctx._h, flat.ctypes.data_as(_lib._fp), 0, 67, 67, 41, radius, -threshold, threshold, border, 0, 1, None, None,
                                                  new.ctypes.data_as(_lib._i16p), C.byref(nNew), cap) == 0
            assert nOld.value == nNew.value == len(want[b][1]) and np.array_equal(old[:nOld.value], new[:nNew.value])


def test_nonmax_separate_thresholds(api):
    """the wrapper lets thresholdMin and thresholdMax be set separately"""
    inten = _nms_images()[0]
    e = api.FactoryFeatureExtractor.nonmax(api.ConfigExtract(2, 0.0, 3, True, True, True))
    e.setThresholdMinimum(-2000.0)
    e.setThresholdMaximum(100.0)
    e.process(api.GrayF32.wrap(inten))
    wmin, wmax = fr.nonmax_block(inten, 2, -2000.0, 100.0, 3, True, True)
    assert len(wmin) > 0 and len(wmax) > 0 and len(wmin) != len(fr.nonmax_block(inten, 2, -100.0, 100.0, 3, True, True)[0])
    assert np.array_equal(e.foundMinXY, wmin) and np.array_equal(e.foundMaxXY, wmax)


# ---- GeneralFeatureDetector via FactoryDetectPoint.createFast ----
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("detectMin", [True, False])
@pytest.mark.parametrize("maxFeatures", [0, 50])
def test_general_detector_create_fast(api, kind, detectMin, maxFeatures):
    W, H = 97, 64
    if kind == "u8":
        img, tol, T = _u8(W, H, 17), 20, api.GrayU8
    else:
        img, tol, T = _f32_inputs(W, H)[1][0], 7.5, api.GrayF32
    radius, threshold, ignore = 2, 5.0, 1
    select = api.SelectNBestFeatures(10)

    def pick(inten, corners, N, positive):
        select.setN(N)
        select.process(api.GrayF32.wrap(inten), [api.Point2D_I16(int(x), int(y)) for x, y in corners], positive)
        return np.array([(p.x, p.y) for p in select.getBestCorners()], np.int16).reshape(-1, 2)

    cfg = api.ConfigGeneralDetector(radius, threshold, ignore, True, detectMin, True, maxFeatures)
    first = fr.general_detector(img, tol, 9, 1.0, radius, threshold, ignore, detectMin, True, maxFeatures, None, None, pick)
    assert len(first[2]) > 5 and (len(first[1]) > 5) == detectMin
    exMax = [tuple(p) for p in first[2][:4].tolist()] + [(50, 30)]
    exMin = ([tuple(p) for p in first[1][:3].tolist()] if detectMin else []) + [(20, 20), (21, 40)]
    for exclude_min, exclude_max in ((None, None), (exMin, exMax), (None, exMax)):
        det = api.FactoryDetectPoint.createFast(api.ConfigFastCorner(tol, 9, 1.0), cfg, T)
        assert isinstance(det, api.GeneralFeatureDetector) and not det.getRequiresGradient() and det.extractor.getIgnoreBorder() == 3
        if exclude_min is not None:
            det.setExcludeMinimum([api.Point2D_I16(x, y) for x, y in exclude_min])
        if exclude_max is not None:
            det.setExcludeMaximum([api.Point2D_I16(x, y) for x, y in exclude_max])
        det.process(T.wrap(img), None, None)
        winten, wmin, wmax = fr.general_detector(img, tol, 9, 1.0, radius, threshold, ignore, detectMin, True, maxFeatures, exclude_min, exclude_max, pick)
        assert np.array_equal(_bits(det.getIntensity().array()), _bits(winten))
        assert [(p.x, p.y) for p in det.getMinimums()] == [tuple(p) for p in wmin.tolist()]
        assert [(p.x, p.y) for p in det.getMaximums()] == [tuple(p) for p in wmax.tolist()]
        if maxFeatures > 0:
            assert len(wmax) == maxFeatures - (len(exclude_max) if exclude_max else 0)


def test_general_detector_no_room_on_either_side(api):
    det = api.FactoryDetectPoint.createFast(None, api.ConfigGeneralDetector(2, 1.0, 0, True, True, True, 3), api.GrayU8)
    full = [api.Point2D_I16(10 + i, 10) for i in range(3)]
    det.setExcludeMinimum(full)
    det.setExcludeMaximum(full)
    det.process(api.GrayU8.wrap(_u8(40, 30, 1)), None, None)
    assert det.getMinimums() == [] and det.getMaximums() == []


# ---- errors ----
def test_fast_errors(api):
    from boofcv_amd import _lib
    for bad in (8, 13):
        with pytest.raises(api.IllegalArgumentException):
            api.FactoryIntensityPointAlg.fast(20, bad, api.GrayU8)
        with pytest.raises(api.IllegalArgumentException):
            api.FactoryDetectPoint.createFast(api.ConfigFastCorner(20, bad), api.GrayU8)
    alg = api.FactoryIntensityPointAlg.fast(20, 9, api.GrayU8)
    for bad in (0, -0.5, 1.5):
        with pytest.raises(api.IllegalArgumentException):
            alg.setMaxFeaturesFraction(bad)
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryDetectPoint.createFast(api.ConfigFastCorner(20, 9, 0.0), api.GrayU8)   # the fraction 0 reaches the setter
    # the C ABI refuses the same, and a negative tolerance, without touching the outputs
    img = _u8(20, 20, 2)
    ctx = api.Context.default()
    L = _lib.load()
    for tol, n, fraction in ((20, 8, 0.1), (20, 13, 0.1), (20, 9, 0.0), (20, 9, 1.5), (-1, 9, 0.1)):
        inten = np.full(400, 5.5, np.float32)
        low, high = np.full((400, 2), -5, np.int16), np.full((400, 2), -5, np.int16)
        nLow, nHigh = C.c_int(-9), C.c_int(-9)
        st = L.bhip_fast_u8(ctx._h, img.ctypes.data_as(_lib._u8p), 0, 20, 20, 20, tol, n, fraction, inten.ctypes.data_as(_lib._fp), 0, 20,
                            low.ctypes.data_as(_lib._i16p), C.byref(nLow), high.ctypes.data_as(_lib._i16p), C.byref(nHigh), 400)
        assert st == _lib.BHIP_ERR_INVALID, (tol, n, fraction)
        assert np.all(inten == 5.5) and np.all(low == -5) and np.all(high == -5) and (nLow.value, nHigh.value) == (-9, -9)
    with pytest.raises(api.IllegalArgumentException):
        a = api.FactoryIntensityPointAlg.fast(-1.0, 9, api.GrayF32)
        a.process(api.GrayF32.wrap(np.zeros((9, 9), np.float32)))
