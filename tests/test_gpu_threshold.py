"""Thresholding on the GPU against tests/threshold_ref.py, bit for bit: device API (DeviceImageOps.threshold / meanU8 / gaussianU8), host API
(binary.InputToBinary, api.BlurImageOps on GrayU8) and direct C-ABI calls.

Which kernel path a shape targets (threshold.hip): streaming kernels give a lane 16 GrayU8 or 4 GrayF32 pixels of a row (one vector load / store
where all are inside the image, single elements otherwise), 256 lanes per workgroup row; the fused GrayU8 local kernel works on 64 x 32 tiles
up to radius 16; block statistics take one wave (or one lane: GrayF32 mean) per block.
  67 x 37    4 full GrayU8 lanes and a tail of 3 (GrayF32: 16 lanes and 3); two fused tiles in x and in y; blocks of 8 x 9, the last 11 wide, 10 high
  131 x 19   three fused tiles in x, one (partial) in y; 19 < 33: kernels higher than the image (two-pass path)
  19 x 131   the transpose: kernels wider than the image only
  259 x 17   five fused tiles in x; a single row of block statistics (neighbourhood 1 x 3)
  5 x 5      smaller than a tile, a lane and a block: tails only, most kernels wider than the image both ways
  32 x 32    block width 16 divides evenly, lanes without a tail
  300 x 70   batch 3 with distinct frames: per-image thresholds, histograms and statistics
  4200 x 3   rows wider than one workgroup of the streaming kernels (4096 GrayU8 / 1024 GrayF32 pixels)
Local widths 3, 11, 33 (radius 16: the last fused radius) and 35 (radius 17: the two-pass path through the GrayU8 blurs).
Every device output is a strided view inside a sentinel-filled parent (tests/view_layouts.py), every device input a window of a larger tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

import threshold_ref as R
import view_layouts as VL
from boofcv_amd import _lib, api, binary, device

pytestmark = pytest.mark.gpu
T = binary.ThresholdType
LAYOUTS = ("odd", "pad4_x1", "dense", "pad4", "pad4_x4")


@pytest.fixture(scope="module")
def ops():
    return device.DeviceImageOps()


def _image(dtype, w, h, seed):
    return R.image_u8(w, h, seed) if dtype == np.uint8 else R.image_f32(w, h, seed)


_KERNELS = {}


def _expected(img, cfg):
    kernel = None
    if cfg.type == T.LOCAL_GAUSSIAN and img.dtype == np.float32:
        radius = R.local_radius(img, cfg.width.length, cfg.width.fraction)
        if radius not in _KERNELS:
            _KERNELS[radius] = api.FactoryKernelGaussian.gaussian1D_F32(-1, radius).data.copy()
        kernel = _KERNELS[radius]
    return R.threshold_config(img, cfg, kernel)


def _window(frames, device_, pad=(3, 2, 5)):
    """the frames [B,H,W] as a window of a larger device tensor: startIndex > 0, row stride > width, image stride > H * row stride"""
    B, H, W = frames.shape
    top, left, right = pad
    parent = torch.full((B, H + top + 1, W + left + right), 77, dtype=torch.from_numpy(frames).dtype, device=device_)
    view = parent[:, top:top + H, left:left + W]
    view.copy_(torch.from_numpy(frames).to(device_))
    return view


def _run(ops, call, frames, layout):
    """call(src_view, out_view) on a windowed input and a guarded output view -> the output as numpy, after the guard check"""
    B, H, W = frames.shape
    src = _window(frames, ops.device)
    parent, out = VL.make_view(layout, B, H, W, torch.uint8, ops.device)
    before = VL.snapshot(parent)
    res = call(src, out)
    assert res is out
    torch.cuda.synchronize()
    VL.assert_only_view_written(parent, out, before, layout)
    return out.cpu().numpy()


def _check(ops, frames, cfg, layout):
    got = _run(ops, lambda s, o: ops.threshold(s, cfg, out=o), frames, layout)
    for b in range(frames.shape[0]):
        exp = _expected(frames[b], cfg)
        bad = np.argwhere(got[b] != exp)
        assert bad.size == 0, "image %d: %d pixels differ, first (y, x) %s: got %d" % (b, len(bad), bad[0], got[b][tuple(bad[0])])
    assert set(np.unique(got)) <= {0, 1}


def _local(t, width, scale=0.95, down=True):
    c = binary.ConfigThreshold.local(t, width)
    c.scale, c.down = scale, down
    return c


# ---------------- local thresholds ----------------
LOCAL_CASES = [
    # (w, h, width, down, scale)
    (67, 37, 3, True, 0.95), (67, 37, 11, True, 0.95), (67, 37, 11, False, 1.0), (67, 37, 33, True, 1.0), (67, 37, 35, False, 0.95),
    (131, 19, 3, False, 0.95), (131, 19, 11, True, 1.0), (131, 19, 33, True, 0.95),      # 33 > height only
    (19, 131, 33, False, 1.0),                                                        # 33 > width only
    (259, 17, 11, True, 0.95), (259, 17, 3, False, 1.0),
    (5, 5, 3, True, 0.95), (5, 5, 11, False, 0.95),                                   # 11 > both
    (67, 37, binary.ConfigLength.relative(0.2, 5), True, 0.95),                       # max(0.2 * 37, 5) -> 7
]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("t", [T.LOCAL_MEAN, T.LOCAL_GAUSSIAN], ids=["mean", "gaussian"])
@pytest.mark.parametrize("case", range(len(LOCAL_CASES)))
def test_local(ops, case, t, dtype):
    w, h, width, down, scale = LOCAL_CASES[case]
    seed = R.LOCAL_MEAN_U8_INPUT["seed"] if (w, h) == (67, 37) else 20 + case
    _check(ops, _image(dtype, w, h, seed)[None], _local(t, width, scale, down), LAYOUTS[case % len(LAYOUTS)])


# ---------------- GrayU8 blurs on their own ----------------
@pytest.mark.parametrize("case", range(len(LOCAL_CASES) - 1))
def test_blur_u8(ops, case):
    w, h, width, _, _ = LOCAL_CASES[case]
    radius = width // 2
    frames = R.image_u8(w, h, 40 + case)[None]
    layout = LAYOUTS[(case + 2) % len(LAYOUTS)]
    got = _run(ops, lambda s, o: ops.meanU8(s, radius, out=o), frames, layout)
    assert (got[0] == R.mean_u8(frames[0], radius)).all()
    got = _run(ops, lambda s, o: ops.gaussianU8(s, radius, out=o), frames, layout)
    assert (got[0] == R.gaussian_u8(frames[0], radius)).all()
    if case == 1:   # radiusX != radiusY goes through the two passes
        got = _run(ops, lambda s, o: ops.meanU8(s, 2, 6, out=o), frames, layout)
        assert (got[0] == R.mean_u8(frames[0], 2, 6)).all()


# ---------------- block thresholds ----------------
BLOCK_SHAPES = [(67, 37, 8), (259, 17, 10), (5, 5, 8), (32, 32, 16)]
BLOCK_KINDS = [(T.BLOCK_MIN_MAX, np.uint8), (T.BLOCK_MIN_MAX, np.float32), (T.BLOCK_MEAN, np.uint8), (T.BLOCK_MEAN, np.float32), (T.BLOCK_OTSU, np.uint8)]


@pytest.mark.parametrize("local", [True, False], ids=["3x3", "single"])
@pytest.mark.parametrize("kind", range(len(BLOCK_KINDS)), ids=["minmax_u8", "minmax_f32", "mean_u8", "mean_f32", "otsu_u8"])
@pytest.mark.parametrize("shape", range(len(BLOCK_SHAPES)))
def test_block(ops, shape, kind, local):
    w, h, width = BLOCK_SHAPES[shape]
    t, dtype = BLOCK_KINDS[kind]
    seed = R.BLOCK_MEAN_F32_INPUT["seed"] if (w, h) == (67, 37) else 60 + shape
    for down in (True, False):
        c = _local(t, width, 0.95, down)
        c.thresholdFromLocalBlocks = local
        _check(ops, _image(dtype, w, h, seed)[None], c, LAYOUTS[(shape + kind) % len(LAYOUTS)])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("spread", [-1.0, 10.0])
def test_block_min_max_flat_region_and_nan(ops, spread, dtype):
    img = _image(dtype, 67, 37, 3)
    img[:20, :30] = 90          # flat: the textureless branch where spread >= 0
    img[20:, 40:] = img[20:, 40:] // 32 + 100         # spread <= 7 but not 0
    if dtype == np.float32:
        img[9, 16] = np.nan     # first pixel of block (2, 1)
        img[30, 50] = np.nan    # inside block (6, 3)
    for down in (True, False):
        c = _local(T.BLOCK_MIN_MAX, 8, 0.85, down)
        c.minimumSpread = spread
        _check(ops, img[None], c, "odd")


def test_block_mean_u8_byte_wrap(ops):
    img = np.clip(R.image_u8(67, 37, 8).astype(int) // 4 + 190, 0, 255).astype(np.uint8)   # bright: 1.3 * mean wraps past 255
    assert (R.block_stats(img, R.BLOCK_MEAN, 8, 1.3) < 100).any()
    for local in (True, False):
        c = _local(T.BLOCK_MEAN, 8, 1.3, True)
        c.thresholdFromLocalBlocks = local
        _check(ops, img[None], c, "pad4_x1")


@pytest.mark.parametrize("otsu2", [False, True])
@pytest.mark.parametrize("tuning", [0.0, 12.0])
def test_block_otsu_variants(ops, otsu2, tuning):
    noisy = R.image_u8(67, 37, 13)
    constant = np.full((37, 67), 140, np.uint8)              # wF == 0 on the first occupied bin
    two = np.where(R.image_u8(67, 37, 14) > 100, 200, 30).astype(np.uint8)
    for img in (noisy, constant, two):
        for down, scale in ((True, 0.95), (False, 1.1)):
            c = binary.ConfigThresholdLocalOtsu(8, tuning)
            c.useOtsu2, c.down, c.scale = otsu2, down, scale
            _check(ops, img[None], c, "odd")


# ---------------- global thresholds ----------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("w, h", [(67, 37), (131, 19), (259, 17), (5, 5)])
def test_fixed(ops, w, h, dtype):
    img = _image(dtype, w, h, 70)
    if dtype == np.float32:
        img[h // 2, w // 2] = np.nan
    for down in (True, False):
        for thr in (100.7, -3.0, 255.0):
            c = binary.ConfigThreshold.fixed(thr)
            c.down = down
            _check(ops, img[None], c, "odd" if down else "pad4")


@pytest.mark.parametrize("w, h", [(67, 37), (259, 17), (5, 5)])
def test_global_otsu(ops, w, h):
    bimodal = np.where(R.image_u8(w, h, 81) > 110, 180, 40).astype(np.uint8) + (R.image_u8(w, h, 82) % 16)
    constant = np.full((h, w), 99, np.uint8)
    for img in (bimodal, constant, R.image_u8(w, h, 83)):
        for down, scale in ((True, 1.0), (True, 0.8), (False, 1.0), (False, 0.8), (False, 0.0)):
            c = binary.ConfigThreshold.global_(T.GLOBAL_OTSU)
            c.down, c.scale = down, scale
            _check(ops, img[None], c, "pad4_x1")


# ---------------- a batch: images must not share thresholds ----------------
@pytest.mark.parametrize("t, dtype", [(T.FIXED, np.uint8), (T.GLOBAL_OTSU, np.uint8), (T.LOCAL_MEAN, np.uint8), (T.LOCAL_GAUSSIAN, np.uint8), (T.BLOCK_MIN_MAX, np.uint8),
                                      (T.BLOCK_MEAN, np.uint8), (T.BLOCK_OTSU, np.uint8), (T.FIXED, np.float32), (T.LOCAL_MEAN, np.float32),
                                      (T.LOCAL_GAUSSIAN, np.float32), (T.BLOCK_MIN_MAX, np.float32), (T.BLOCK_MEAN, np.float32)])
def test_batch_of_three(ops, t, dtype):
    frames = np.stack([_image(dtype, 300, 70, 90 + b) for b in range(3)])
    frames[1] = frames[1] // 2 if dtype == np.uint8 else frames[1] * np.float32(0.5)      # a darker frame: another global / block threshold
    frames[2] = 255 - frames[2] if dtype == np.uint8 else np.float32(255) - frames[2]
    c = binary.ConfigThreshold.fixed(120) if t == T.FIXED else binary.ConfigThreshold.global_(t) if t.isGlobal() else binary.ConfigThreshold.local(t, 13)
    _check(ops, frames, c, "odd")


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_rows_wider_than_a_workgroup(ops, dtype):
    """4200 x 3: the second workgroup of a row in the compare, histogram, local-compare (two-pass path: 35 > height) and block apply kernels"""
    img = _image(dtype, 4200, 3, 31)
    types = [T.FIXED, T.LOCAL_MEAN, T.LOCAL_GAUSSIAN, T.BLOCK_MEAN, T.BLOCK_MIN_MAX] + ([T.GLOBAL_OTSU, T.BLOCK_OTSU] if dtype == np.uint8 else [])
    for t in types:
        c = binary.ConfigThreshold.fixed(99.5) if t == T.FIXED else binary.ConfigThreshold.global_(t) if t.isGlobal() else binary.ConfigThreshold.local(t, 35)
        _check(ops, img[None], c, "odd")


def test_second_call_with_another_shape(ops):
    """stale scratch geometry: the same context, a large shape, then a small one, then the large one again"""
    for w, h in ((300, 70), (67, 37), (300, 70), (5, 5)):
        for t, dtype in ((T.BLOCK_OTSU, np.uint8), (T.BLOCK_MEAN, np.float32), (T.LOCAL_GAUSSIAN, np.uint8), (T.GLOBAL_OTSU, np.uint8)):
            c = binary.ConfigThreshold.global_(t) if t.isGlobal() else binary.ConfigThreshold.local(t, 9)
            _check(ops, _image(dtype, w, h, w)[None], c, "dense")


# ---------------- host API and the C ABI ----------------
@pytest.mark.parametrize("t, imageType", [(T.LOCAL_MEAN, api.GrayU8), (T.LOCAL_GAUSSIAN, api.GrayF32), (T.BLOCK_MIN_MAX, api.GrayF32), (T.BLOCK_OTSU, api.GrayU8),
                                          (T.GLOBAL_OTSU, api.GrayU8), (T.BLOCK_MEAN, api.GrayF32)])
def test_host_api_on_sub_images(t, imageType):
    w, h = 67, 37
    dtype = np.uint8 if imageType is api.GrayU8 else np.float32
    img = _image(dtype, w, h, 7)
    whole = imageType(w + 9, h + 6)
    whole.data[:] = 33
    sub = whole.subimage(4, 3, 4 + w, 3 + h)     # startIndex > 0, stride > width
    sub.array()[:] = img
    outWhole = api.GrayU8(w + 5, h + 4)
    outWhole.data[:] = 0xA5
    out = outWhole.subimage(2, 1, 2 + w, 1 + h)
    c = binary.ConfigThreshold.global_(t) if t.isGlobal() else binary.ConfigThreshold.local(t, 11)
    alg = binary.FactoryThresholdBinary.threshold(c, imageType)
    assert alg.process(sub, out) is out and alg.getInputType() is imageType
    assert (out.array() == _expected(img, c)).all()
    guard = np.ones((h + 4, w + 5), bool)
    guard[1:1 + h, 2:2 + w] = False
    assert (outWhole.array()[guard] == 0xA5).all()
    with pytest.raises(api.IllegalArgumentException):     # a radius / block width of 0 where the reference throws
        binary.FactoryThresholdBinary.threshold(binary.ConfigThreshold.local(T.LOCAL_MEAN if not t.isGlobal() else T.BLOCK_MEAN, 0.4), imageType).process(sub, out)
    assert (outWhole.array()[guard] == 0xA5).all() and (out.array() == _expected(img, c)).all()


def test_host_blurs_and_ops_on_gray_u8():
    img = R.image_u8(67, 37, 17)
    src = api.GrayU8.wrap(img)
    assert (api.BlurImageOps.mean(src, None, 4).array() == R.mean_u8(img, 4)).all()
    assert (api.BlurImageOps.mean(src, None, 2, 20).array() == R.mean_u8(img, 2, 20)).all()
    assert (api.BlurImageOps.gaussian(src, None, -1, 5).array() == R.gaussian_u8(img, 5)).all()
    assert (binary.GThresholdImageOps.threshold(src, None, 120.9, False).array() == R.threshold(img, 120.9, False)).all()
    assert (binary.ThresholdImageOps.localMean(src, None, binary.ConfigLength.fixed(9), 0.95, True).array() == R.local_mean(img, 9, -1, 0.95, True)).all()
    assert (binary.GThresholdImageOps.localGaussian(src, None, binary.ConfigLength.fixed(9), 1.0, False).array() == R.local_gaussian(img, 9, -1, 1.0, False)).all()
    assert binary.GThresholdImageOps.computeOtsu(src, 0, 255) == R.compute_otsu(np.bincount(img.reshape(-1), minlength=256), 256, img.size)
    with pytest.raises(api.IllegalArgumentException):
        api.BlurImageOps.mean(src, None, 0)


def test_direct_c_call_and_refusals(ops):
    """bhip_threshold_u8 with plain ctypes buffers; every refused type / image type answers BHIP_ERR_UNSUPPORTED (invalid ones BHIP_ERR_INVALID) through
    the host and the device entry points and leaves a sentinel-filled output untouched"""
    L, ctx = _lib.load(), ops.ctx
    w, h = 67, 37
    img = R.image_u8(w, h, 19)
    cfg = _lib.ThresholdCfg()
    assert L.bhip_threshold_cfg_default(_lib.BHIP_THRESHOLD_BLOCK_MEAN, cfg) == _lib.BHIP_OK
    cfg.widthLength = 8
    out = np.full((h, w + 3), 0xA5, np.uint8)
    flat = np.ascontiguousarray(img).reshape(-1)
    assert L.bhip_threshold_u8(ctx._h, cfg, flat.ctypes.data_as(_lib._u8p), 0, w, w, h, out.ctypes.data_as(_lib._u8p), 1, w + 3) == _lib.BHIP_OK
    flatOut = out.reshape(-1)
    view = np.lib.stride_tricks.as_strided(flatOut[1:], (h, w), (w + 3, 1))   # rows start one element in, w + 3 apart
    assert (view == R.threshold_block(img, R.BLOCK_MEAN, 8, 0.95, True)).all()
    inside = np.zeros(flatOut.size, bool)
    np.lib.stride_tricks.as_strided(inside[1:], (h, w), (w + 3, 1))[:] = True
    assert (flatOut[~inside] == 0xA5).all()

    f32 = R.image_f32(w, h, 19).reshape(-1)
    dsrc8, dsrc32 = torch.from_numpy(img).to(ops.device), torch.from_numpy(f32).to(ops.device)
    refused = [(t, u8) for t in (T.GLOBAL_ENTROPY, T.GLOBAL_LI, T.GLOBAL_HUANG, T.LOCAL_SAVOLA, T.LOCAL_NICK, T.LOCAL_OTSU) for u8 in (True, False)]
    refused += [(T.GLOBAL_OTSU, False), (T.BLOCK_OTSU, False), ("range", True)]
    invalid = [("radius", True), ("radius", False), ("block", True), ("block", False), ("type", True)]
    for (t, u8), status in [(r, _lib.BHIP_ERR_UNSUPPORTED) for r in refused] + [(r, _lib.BHIP_ERR_INVALID) for r in invalid]:
        c = _lib.ThresholdCfg()
        base = {"range": T.GLOBAL_OTSU, "radius": T.LOCAL_MEAN, "block": T.BLOCK_MIN_MAX, "type": T.FIXED}.get(t, t)
        assert L.bhip_threshold_cfg_default(int(base), c) == _lib.BHIP_OK
        if t == "range":
            c.maxPixelValue = 200
        elif t in ("radius", "block"):
            c.widthLength = 0.4
        elif t == "type":
            c.type = 13
        hout = np.full(h * w, 0xA5, np.uint8)
        dout = torch.full((h, w), 0xA5, dtype=torch.uint8, device=ops.device)
        if u8:
            st_h = L.bhip_threshold_u8(ctx._h, c, flat.ctypes.data_as(_lib._u8p), 0, w, w, h, hout.ctypes.data_as(_lib._u8p), 0, w)
            st_d = L.bhip_threshold_dev_u8(ctx._h, c, C.c_void_p(dsrc8.data_ptr()), w * h, w, w, h, 1, C.c_void_p(dout.data_ptr()), w * h, w)
        else:
            st_h = L.bhip_threshold_f32(ctx._h, c, f32.ctypes.data_as(_lib._fp), 0, w, w, h, hout.ctypes.data_as(_lib._u8p), 0, w)
            st_d = L.bhip_threshold_dev_f32(ctx._h, c, C.c_void_p(dsrc32.data_ptr()), w * h, w, w, h, 1, C.c_void_p(dout.data_ptr()), w * h, w)
        torch.cuda.synchronize()
        assert (st_h, st_d) == (status, status), (t, u8, st_h, st_d)
        assert (hout == 0xA5).all() and bool((dout == 0xA5).all()), (t, u8)
    # the device API refuses the same combinations before any C call
    with pytest.raises(api.IllegalArgumentException):
        ops.threshold(dsrc32.reshape(1, h, w), binary.ConfigThreshold.global_(T.GLOBAL_OTSU))
    with pytest.raises(api.IllegalArgumentException):
        ops.threshold(dsrc8.reshape(1, h, w), binary.ConfigThreshold.local(T.LOCAL_NICK, 11))
