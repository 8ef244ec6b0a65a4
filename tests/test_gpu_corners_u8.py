"""GPU: GrayU8 -> GrayS16 gradients, the fused S16 box corner intensity and the Gaussian-weighted corner intensity (F32 and S16), bit for
bit against tests/corner_ref.py, through the host-buffer API (api.py) and the device-batched API (device.py)."""
import numpy as np
import pytest

import corner_ref as cr

pytestmark = pytest.mark.gpu

WEIGHTED_MAX = 15


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _u8(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


def _s16(w, h, seed, lo=-1020, hi=1021):
    rng = np.random.default_rng(seed)
    return rng.integers(lo, hi, size=(h, w)).astype(np.int16), rng.integers(lo, hi, size=(h, w)).astype(np.int16)


def _intensity(api, kind, radius, kappa, weighted, dx, dy, derivType, sub=False):
    T = api.GrayS16 if derivType == "s16" else api.GrayF32
    X, Y = T.wrap(dx), T.wrap(dy)
    if sub:   # views inside a larger buffer sharing startIndex / stride
        H, W = dx.shape
        bx, by = T(W + 7, H + 5), T(W + 7, H + 5)
        X, Y = bx.subimage(3, 2, 3 + W, 2 + H), by.subimage(3, 2, 3 + W, 2 + H)
        X.array()[:, :] = dx
        Y.array()[:, :] = dy
    alg = (api.FactoryIntensityPointAlg.shiTomasi(radius, weighted, T) if kind == 0 else
           api.FactoryIntensityPointAlg.harris(radius, kappa, weighted, T))
    out = api.GrayF32(1, 1)
    alg.process(X, Y, out)
    return out.array().copy(), alg


def _ref(orc, kind, radius, kappa, weighted, dx, dy, derivType):
    if derivType == "s16":
        return (cr.corner_weighted_s16 if weighted else cr.corner_box_s16)(dx, dy, radius, kind, kappa)
    if weighted:
        return cr.corner_weighted_f32(orc, dx, dy, radius, kind, kappa)
    return orc.corner_intensity(orc.Gray.from_array(dx), orc.Gray.from_array(dy), radius, "shitomasi" if kind == 0 else "harris", kappa)


GRAD_CASES = [(g, b, s, 0) for g in ("sobel", "three") for b in (False, True) for s in ((37, 23), (256, 9), (261, 35), (3, 3), (1, 5))] + \
             [(g, b, (261, 35), 1) for g in ("sobel", "three") for b in (False, True)]


@pytest.mark.parametrize("grad,border,shape,kind", GRAD_CASES)
def test_u8_gradients(api, grad, border, shape, kind):
    W, H = shape
    img = _u8(W, H, 7 + W)
    dx0, dy0 = np.full((H, W), 1234, np.int16), np.full((H, W), -77, np.int16)
    src = api.GrayU8.wrap(img)
    if kind == 1:   # sub-image views with odd offsets
        big = api.GrayU8(W + 5, H + 3)
        src = big.subimage(1, 2, 1 + W, 2 + H)
        src.array()[:, :] = img
    X, Y = api.GrayS16.wrap(dx0), api.GrayS16.wrap(dy0)
    (api.GradientSobel if grad == "sobel" else api.GradientThree).process(src, X, Y, 0 if border else None)
    want_x, want_y = cr.gradient_u8(grad, img, border, dx0, dy0)
    assert np.array_equal(X.array(), want_x) and np.array_equal(Y.array(), want_y)


CASES = [(k, r, w, d) for d in ("s16", "f32") for w in (False, True) for k in (0, 1) for r in range(1, 9)
         if not (d == "f32" and not w)]


@pytest.mark.parametrize("kind,radius,weighted,derivType", CASES)
def test_corner_intensity_radii(api, orc, kind, radius, weighted, derivType):
    kappa = 0.0625
    for (W, H) in [(2 * radius + 1, 2 * radius + 1), (67, 41), (97, 35)]:
        dx, dy = _s16(W, H, radius * 100 + W)
        if derivType == "f32":
            dx, dy = dx.astype(np.float32) * 0.25, dy.astype(np.float32) * 0.25
        got, alg = _intensity(api, kind, radius, kappa, weighted, dx, dy, derivType, sub=(W == 67))
        want = _ref(orc, kind, radius, kappa, weighted, dx, dy, derivType)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (W, H)
        assert alg.getIgnoreBorder() == (0 if weighted else radius)


@pytest.mark.parametrize("weighted,derivType", [(False, "s16"), (True, "s16"), (True, "f32")])
def test_corner_shapes(api, orc, weighted, derivType):
    """tile edges (64 x 32 box, 32 x 16 weighted), odd sizes, and kernels as wide as the image (the naive normalised axis)"""
    r = 3
    for (W, H) in [(63, 31), (64, 32), (65, 33), (129, 17), (7, 40), (40, 7), (8, 9), (33, 16), (31, 15), (7, 7)]:
        if not weighted and (2 * r + 1 > W or 2 * r + 1 > H):
            continue
        dx, dy = _s16(W, H, W * 1000 + H)
        if derivType == "f32":
            dx, dy = dx.astype(np.float32) * 0.5, dy.astype(np.float32) * 0.5
        got, _ = _intensity(api, 0, r, 0.04, weighted, dx, dy, derivType)
        want = _ref(orc, 0, r, 0.04, weighted, dx, dy, derivType)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (W, H)
    if weighted:   # both axes narrower than the kernel
        dx, dy = _s16(5, 4, 99)
        if derivType == "f32":
            dx, dy = dx.astype(np.float32), dy.astype(np.float32)
        got, _ = _intensity(api, 1, 6, 0.04, True, dx, dy, derivType)
        assert np.array_equal(got, _ref(orc, 1, 6, 0.04, True, dx, dy, derivType))


@pytest.mark.parametrize("derivType", ["s16", "f32"])
def test_weighted_limit(api, orc, derivType):
    W, H = 71, 45
    dx, dy = _s16(W, H, 5)
    if derivType == "f32":
        dx, dy = dx.astype(np.float32), dy.astype(np.float32)
    got, _ = _intensity(api, 0, WEIGHTED_MAX, 0.04, True, dx, dy, derivType)
    assert np.array_equal(got, _ref(orc, 0, WEIGHTED_MAX, 0.04, True, dx, dy, derivType))
    from boofcv_amd import _lib
    T = api.GrayS16 if derivType == "s16" else api.GrayF32
    alg = (api.FactoryIntensityPointAlg.shiTomasi(WEIGHTED_MAX + 1, True, T))
    out = api.GrayF32(W, H)
    out.array()[:, :] = 3.5
    with pytest.raises(RuntimeError) as e:
        alg.process(T.wrap(dx), T.wrap(dy), out)
    assert str(_lib.BHIP_ERR_UNSUPPORTED) in str(e.value) or "supported" in str(e.value)
    assert np.all(out.array() == 3.5)


def test_large_box_radius(api):
    W, H = 150, 121
    dx, dy = _s16(W, H, 77)
    for r in (13, 40, 60):   # beyond the fused block: the two-pass form
        got, _ = _intensity(api, 0, r, 0.04, False, dx, dy, "s16")
        assert np.array_equal(got, cr.corner_box_s16(dx, dy, r, 0)), r


@pytest.mark.parametrize("weighted", [False, True])
def test_extreme_s16_wraps(api, weighted):
    W, H = 70, 40
    dx, dy = _s16(W, H, 3, -32768, 32768)
    dx[10:30, 10:40] = 32767
    dy[10:30, 10:40] = -32768
    for kind in (0, 1):
        got, _ = _intensity(api, kind, 4, 0.04, weighted, dx, dy, "s16")
        want = (cr.corner_weighted_s16 if weighted else cr.corner_box_s16)(dx, dy, 4, kind)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_device_batches(dev, orc):
    ops, torch = dev
    B, W, H = 5, 131, 37
    frames = np.stack([_u8(W, H, 40 + b) for b in range(B)])
    for pitch in (W, W + 5):   # dense and odd-pitch views
        big = torch.zeros((B, H + 2, pitch + 3), dtype=torch.uint8, device="cuda")
        src = big[:, 1:H + 1, 2:W + 2]
        src.copy_(torch.from_numpy(frames))
        for grad in ("sobel", "three"):
            for border in (None, 0):
                dx, dy = (ops.sobel if grad == "sobel" else ops.three)(src, border)
                torch.cuda.synchronize()
                for b in range(B):
                    wx, wy = cr.gradient_u8(grad, frames[b], border is not None)
                    assert np.array_equal(dx[b].cpu().numpy(), wx) and np.array_equal(dy[b].cpu().numpy(), wy)
        dx, dy = ops.sobel(src, 0)
        dxv = torch.zeros((B, H, pitch), dtype=torch.int16, device="cuda")[:, :, :W]
        dyv = torch.zeros((B, H, pitch), dtype=torch.int16, device="cuda")[:, :, :W]
        dxv.copy_(dx); dyv.copy_(dy)
        for weighted in (False, True):
            for kind, r in ((0, 2), (1, 5)):
                out = ops.cornerIntensity(kind, r, 0.05, dxv, dyv, weighted=weighted)
                torch.cuda.synchronize()
                ddx, ddy = dx.cpu().numpy(), dy.cpu().numpy()
                for b in range(B):
                    want = (cr.corner_weighted_s16 if weighted else cr.corner_box_s16)(ddx[b], ddy[b], r, kind, 0.05)
                    assert np.array_equal(out[b].cpu().numpy(), want), (pitch, weighted, kind, b)
        fdx, fdy = dx.float().contiguous(), dy.float().contiguous()
        out = ops.cornerIntensity(0, 3, 0.04, fdx, fdy, weighted=True)
        torch.cuda.synchronize()
        for b in range(B):
            want = cr.corner_weighted_f32(orc, fdx[b].cpu().numpy(), fdy[b].cpu().numpy(), 3, 0)
            assert np.array_equal(out[b].cpu().numpy(), want)


@pytest.mark.parametrize("weighted", [False, True])
def test_general_feature_detector_1080p(api, orc, weighted):
    W, H = 1920, 1080
    img = _u8(W, H, 2024)
    dx, dy = api.GrayS16(W, H), api.GrayS16(W, H)
    api.GradientSobel.process(api.GrayU8.wrap(img), dx, dy, 0)
    wx, wy = cr.gradient_u8("sobel", img, True)
    assert np.array_equal(dx.array(), wx) and np.array_equal(dy.array(), wy)
    alg = api.FactoryIntensityPointAlg.shiTomasi(2, weighted, api.GrayS16)
    cfg = api.ConfigExtract(2, 10.0, 0, True)
    det = api.GeneralFeatureDetector(alg, api.FactoryFeatureExtractor.nonmax(cfg))
    det.setMaxFeatures(500)
    det.process(None, dx, dy)
    want = (cr.corner_weighted_s16 if weighted else cr.corner_box_s16)(wx, wy, 2, 0)
    assert np.array_equal(det.getIntensity().array(), want)
    ref_img = orc.Gray.from_array(want)
    border = max(cfg.ignoreBorder, 0 if weighted else 2)
    found = orc.nonmax(ref_img, 2, 10.0, border)
    best = orc.select_nbest(ref_img, found, 500, True)
    got = np.array([[p.x, p.y] for p in det.getMaximums()], dtype=np.int16).reshape(-1, 2)
    assert len(found) > 500
    assert np.array_equal(got, best)


def test_batch_of_64_1080p_frames(dev):
    ops, torch = dev
    B, W, H = 64, 1920, 1080
    gen = torch.Generator(device="cuda").manual_seed(5)
    src = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    dx, dy = ops.sobel(src, 0)
    box = ops.cornerIntensity(0, 2, 0.04, dx, dy)
    torch.cuda.synchronize()
    frames = src.cpu().numpy()
    boxes = box.cpu().numpy()
    for b in range(B):
        wx, wy = cr.gradient_u8("sobel", frames[b], True)
        assert np.array_equal(boxes[b], cr.corner_box_s16(wx, wy, 2, 0)), b
