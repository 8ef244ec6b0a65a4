"""Wide filter kernels on every dispatch path, bit for bit against the CPU oracle (tests/test_oracle_wide_filters.py checks the oracle
itself against an fp64 reference at the same widths).

bhip_launch_conv (boofcv_amd/csrc/conv.hip) picks one of four kernels for a separable convolution; each case id names the class it targets:
  stream    widths 3..11, centred: k_conv_{h,v}_stream + the border fix-up of the general kernel
  tile      any other width up to 97 on 16-byte aligned rows: k_conv_h_tile<0> / k_conv_v_tile<0,16> (coefficients in LDS, a four-tap
            ds_read2st64 loop plus a remainder loop, packed fp32); the vertical block takes (32 + kw - 1) KiB of LDS, above 64 KiB from
            kw = 33 (vlds-over-64KiB) and about 128 KiB at kw = 97
  general   98..255 taps, or rows that are not 16-byte aligned: k_conv<V>, one pixel per thread
  naive     normalised variants with the kernel at least as wide as the image: k_conv<V> mode 2
  unsupported  kw > 255 (and the mean / median / 2-D limits): BHIP_ERR_UNSUPPORTED, the caller's output untouched
The host path re-pitches rows to a multiple of 4 floats, so it takes the tiled kernels wherever the width allows them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENT = -12345.5   # sentinel: pixels a call must not write keep it
RANGES = ((0.0, 255.0), (-5.0, 5.0), (1e3, 1e4))
SEP_WIDTHS = (11, 13, 18, 19, 20, 21, 22, 33, 41, 64, 65, 96, 97, 98, 99, 129, 255)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()  # fails loudly without a GPU / without libboofhip.so
    return a


def G(api, g):
    """oracle Gray -> api.GrayF32 over the same buffer (same startIndex / stride)"""
    return api.GrayF32(g.width, g.height, g.buf, g.startIndex, g.stride)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sep_class(kw):
    if kw > 97:
        c = "general"
    elif kw == 97:
        c = "tile"   # + vlds-128KiB below
    elif kw >= 33:
        c = "tile-vlds-over-64KiB"
    else:
        c = "tile"
    if kw <= 11:
        c = "stream+tile"   # centred: streaming kernels; off-centre: tiled
    return "kw%d-%s%s" % (kw, c, {97: "-vlds-128KiB-last-tiled", 98: "-first-general", 255: "-max-taps"}.get(kw, ""))


def _kinds(api):
    return {"h": (api.ConvolveImageNoBorder, "horizontal"), "v": (api.ConvolveImageNoBorder, "vertical"),
            "norm_h": (api.ConvolveImageNormalized, "horizontal"), "norm_v": (api.ConvolveImageNormalized, "vertical")}


def _kernels(orc, rng, kw):
    """a Gaussian (even widths: the next odd one without its last tap), a positive kernel whose sum is 1.3 (re-normalised), a signed kernel
    (no-border variants only: the clipped weights of a signed kernel can sum to 0)"""
    g = orc.gaussian1d_f32(-1, kw // 2)[:kw].copy()
    pos = rng.uniform(0.5, 1.5, kw).astype(np.float32)
    pos = (pos * np.float32(1.3 / pos.sum())).astype(np.float32)
    signed = (rng.uniform(-1, 1, kw) / np.sqrt(kw)).astype(np.float32)
    return [("gauss", g), ("pos", pos), ("signed", signed)]


def _origins(rng, kw):
    return [("centre", kw // 2), ("off0", 0), ("offlast", kw - 1), ("offrand", int(rng.integers(0, kw)))]


def _frame(kind, w, h, kw, off):
    """pixels a no-border convolution leaves untouched"""
    keep = np.ones((h, w), bool)
    offR = kw - off - 1
    if kind.endswith("h"):
        keep[:, off:max(off, w - offR)] = False
    else:
        keep[off:max(off, h - offR), :] = False
    return keep


def _check_host_conv(api, orc, kind, k, off, img, ctx):
    w, h = img.width, img.height
    out = api.GrayF32(w, h)
    out.data[:] = SENT
    cls, fn = _kinds(api)[kind]
    getattr(cls, fn)(api.Kernel1D_F32(k, offset=off), G(api, img), out)
    exp = orc.conv(kind, k, off, img, threads=1).array().copy()
    if not kind.startswith("norm"):
        exp[_frame(kind, w, h, len(k), off)] = SENT
    got = out.array()
    if not np.array_equal(bits(got), bits(exp)):
        bad = np.argwhere(bits(got) != bits(exp))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ, first (x=%d, y=%d): got %r expected %r" % (ctx, len(bad), x, y, got[y, x], exp[y, x]))


# ------------------------------------------------------------------------------------------------------------------ separable, host path
@pytest.mark.parametrize("kw", SEP_WIDTHS, ids=_sep_class)
def test_separable_wide_host(api, orc, kw):
    """every origin x kernel at this width, all four variants, on images wider / taller than the kernel: rows ending inside a 256-column
    tile, at a tile edge and off a multiple of 4; heights across CT_ROWS = 8 and CV_ROWS = 32; a 2-pixel interior (extent = kw + 1)"""
    rng = np.random.default_rng(7000 + kw)
    widths = [kw + 1] + [x for x in (255, 256, 257, 513) if x > kw]
    heights = [kw + 1] + [x for x in (31, 32, 33, 100) if x > kw] + [kw + 31, kw + 64]
    for oi, (oname, off) in enumerate(_origins(rng, kw)):
        for ki, (kname, k) in enumerate(_kernels(orc, rng, kw)):
            i = 3 * oi + ki
            lo, hi = RANGES[i % 3]
            for kind in ("h", "v", "norm_h", "norm_v"):
                if kind.startswith("norm") and kname == "signed":
                    continue
                for j in (i, i + 5):   # two shapes per case
                    if kind.endswith("h"):
                        w, h = widths[j % len(widths)], (31, 32, 33, 100)[j % 4]
                    else:
                        w, h = (255, 256, 257, 513)[j % 4], heights[j % len(heights)]
                    img = orc.Gray.from_array(rng.uniform(lo, hi, (h, w)).astype(np.float32))
                    _check_host_conv(api, orc, kind, k, off, img, (_sep_class(kw), oname, kname, kind, w, h, lo))


@pytest.mark.parametrize("kw", SEP_WIDTHS, ids=lambda kw: "kw%d-naive" % kw)
def test_separable_kernel_wider_than_image_host(api, orc, kw):
    """extent = kw and extent < kw: the normalised variants take the naive form (k_conv mode 2); the no-border variants write one pixel
    per row / column at extent = kw (through the tiled or general kernel) and nothing below it"""
    rng = np.random.default_rng(8000 + kw)
    for oi, (oname, off) in enumerate(_origins(rng, kw)):
        for ki, (kname, k) in enumerate(_kernels(orc, rng, kw)):
            i = 3 * oi + ki
            lo, hi = RANGES[i % 3]
            for L in (kw, max(kw - 5, 1), max(kw // 3, 1)):
                other = (20, 33, 64, 7)[i % 4]
                for kind in ("h", "v", "norm_h", "norm_v"):
                    if kind.startswith("norm") and kname == "signed":
                        continue
                    w, h = (L, other) if kind.endswith("h") else (other, L)
                    img = orc.Gray.from_array(rng.uniform(lo, hi, (h, w)).astype(np.float32))
                    _check_host_conv(api, orc, kind, k, off, img, ("kw%d-naive" % kw, oname, kname, kind, w, h, lo))


# ------------------------------------------------------------------------------------------------------------------ separable, device batches
@pytest.mark.parametrize("kw", (20, 41, 97, 129), ids=lambda kw: _sep_class(kw) + "-device-batch")
def test_separable_wide_device_batch(api, orc, kw):
    """B = 3 frames; dense (tiled for kw <= 97), 4-aligned pitched view (tiled) and odd-pitch view (general); every image equals its
    single-image oracle result"""
    import torch
    from boofcv_amd import device as dv
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    ops = dv.DeviceImageOps(ctx)
    B, w, h = 3, 260, kw + 45
    rng = np.random.default_rng(9000 + kw)
    frames = [orc.Gray.from_array(rng.uniform(*RANGES[b], (h, w)).astype(np.float32)) for b in range(B)]
    dense = torch.from_numpy(np.stack([f.array() for f in frames])).cuda()
    views = [("dense", dense)]
    for name, pitch in (("pitch4", (w + 3) // 4 * 4 + 8), ("pitch-odd", w + 3)):
        big = torch.full((B, h + 2, pitch), -7.0, dtype=torch.float32, device="cuda")
        big[:, 1:h + 1, :w] = dense
        views.append((name, big[:, 1:h + 1, :w]))
    torch.cuda.synchronize()
    g = orc.gaussian1d_f32(-1, kw // 2)[:kw].copy()
    fns = {"h": ops.convolveHorizontal, "v": ops.convolveVertical, "norm_h": ops.convolveNormalizedHorizontal,
           "norm_v": ops.convolveNormalizedVertical}
    try:
        for vname, src in views:
            for off in (kw // 2, int(rng.integers(0, kw))):
                for kind, fn in fns.items():
                    out = torch.full_like(dense, SENT)
                    fn(g, off, src, out)
                    ctx.synchronize()
                    got = out.cpu().numpy()
                    for b in range(B):
                        exp = orc.conv(kind, g, off, frames[b], threads=1).array().copy()
                        if not kind.startswith("norm"):
                            exp[_frame(kind, w, h, kw, off)] = SENT
                        assert np.array_equal(bits(got[b]), bits(exp)), (_sep_class(kw), vname, off, kind, b)
            for sigma, radius in ((-1, kw // 2), (kw / 5.0, -1)):
                got = ops.gaussian(src, sigma, radius)
                ctx.synchronize()
                for b in range(B):
                    exp = orc.gaussian_blur(frames[b], sigma, radius, threads=1).array()
                    assert np.array_equal(bits(got[b].cpu().numpy()), bits(exp)), (vname, sigma, radius, b)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ Gaussian blur
@pytest.mark.parametrize("sigma,radius", [pytest.param(-1, r, id="r%d-%dtaps" % (r, 2 * r + 1)) for r in (6, 10, 16, 20, 48, 49, 64, 127)] +
                         [pytest.param(s, -1, id="sigma%g-%dtaps" % (s, t)) for s, t in ((2.5, 13), (7.0, 35), (20.0, 101), (42.0, 211))] +
                         [pytest.param(3.0, 30, id="sigma3-r30")])
def test_gaussian_blur_two_pass_wide(api, orc, sigma, radius):
    """BlurImageOps.gaussian beyond the one-pass widths: two normalised passes (tile / general / naive per axis); host path and a device
    batch; an image smaller than the kernel on one axis only"""
    import torch
    from boofcv_amd import device as dv
    r = radius if radius > 0 else int(np.ceil((5 * sigma - 1) / 2))
    kw = 2 * r + 1
    rng = np.random.default_rng(kw)
    shapes = [(kw + 40, 37), (29, kw + 30), (kw + 3, kw - 1 if kw > 1 else 1)]
    for (w, h), (lo, hi) in zip(shapes, RANGES):
        img = orc.Gray.from_array(rng.uniform(lo, hi, (h, w)).astype(np.float32))
        exp = orc.gaussian_blur(img, sigma, radius, threads=1).array()
        out = api.GrayF32(w, h)
        out.data[:] = SENT
        api.BlurImageOps.gaussian(G(api, img), out, sigma, radius)
        assert np.array_equal(bits(out.array()), bits(exp)), (sigma, radius, w, h)
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    try:
        ops = dv.DeviceImageOps(ctx)
        w, h = shapes[0]
        imgs = [orc.Gray.from_array(rng.uniform(0, 100, (h, w)).astype(np.float32)) for _ in range(2)]
        t = torch.from_numpy(np.stack([g.array() for g in imgs])).cuda()
        torch.cuda.synchronize()
        got = ops.gaussian(t, sigma, radius)
        ctx.synchronize()
        for b, g in enumerate(imgs):
            assert np.array_equal(bits(got[b].cpu().numpy()), bits(orc.gaussian_blur(g, sigma, radius, threads=1).array())), (sigma, radius, b)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ mean / median / 2-D
@pytest.mark.parametrize("rx,ry,w,h", [
    (5, 5, 37, 29), (8, 8, 51, 17), (8, 3, 17, 45),                       # 2r+1 == width
    (20, 20, 41, 100), (20, 7, 42, 60), (20, 2, 40, 61),                  # equal to, one less than, greater than the width
    (3, 20, 77, 41), (4, 20, 77, 40),                                     # the same on the height
    (60, 5, 121, 30), (60, 4, 122, 33), (60, 5, 130, 9),
    (127, 1, 255, 13), (127, 3, 254, 17), (127, 2, 256, 9), (127, 2, 301, 11),
], ids=lambda v: str(v))
def test_mean_blur_wide(api, orc, rx, ry, w, h):
    """interior running sums, the normalised border (k_conv mode 3), and the normalised form (general kernel, the mean does not re-pitch)
    when the window is wider than the image on one axis"""
    rng = np.random.default_rng(rx * 1000 + ry * 7 + w)
    for lo, hi in RANGES:
        img = orc.Gray.from_array(rng.uniform(lo, hi, (h, w)).astype(np.float32))
        out = api.GrayF32(w, h)
        out.data[:] = SENT
        api.BlurImageOps.mean(G(api, img), out, rx, ry)
        assert np.array_equal(bits(out.array()), bits(orc.blur_mean(img, rx, ry).array())), (rx, ry, w, h, lo)


@pytest.mark.parametrize("radius,w,h", [(4, 37, 23), (5, 50, 19), (6, 33, 47), (7, 29, 61), (8, 45, 35), (8, 13, 11), (7, 40, 9), (5, 7, 70)],
                         ids=lambda v: str(v))
def test_median_wide(api, orc, radius, w, h):
    """k_median: LDS tile of (16 + 2r)^2 on shapes that are not multiples of 16; radii larger than half the image"""
    rng = np.random.default_rng(radius * 100 + w)
    a = rng.uniform(-5, 5, (h, w)).astype(np.float32)
    a[::2, ::3] = np.round(a[::2, ::3]) + np.float32(0)   # ties (+0: no -0 the order statistic cannot tell from 0)
    img = orc.Gray.from_array(a)
    out = api.GrayF32(w, h)
    out.data[:] = SENT
    api.BlurImageOps.median(G(api, img), out, radius)
    assert np.array_equal(bits(out.array()), bits(orc.blur_median(img, radius).array())), (radius, w, h)


@pytest.mark.parametrize("kw", (8, 9, 11, 13, 16, 21), ids=lambda kw: "kw%d" % kw)
def test_conv2d_wide(api, orc, kw):
    """ConvolveImageNoBorder.convolve(Kernel2D_F32) up to 21 x 21, centred and off-centre; the frame keeps the caller's pixels"""
    rng = np.random.default_rng(kw)
    for i, off in enumerate((kw // 2, 0, kw - 1, int(rng.integers(0, kw)))):
        w, h = [(kw + 9, kw + 4), (67, 33), (kw, kw + 1), (29, 50)][i]
        lo, hi = RANGES[i % 3]
        k = (rng.uniform(-1, 1, (kw, kw)) / kw).astype(np.float32)
        img = orc.Gray.from_array(rng.uniform(lo, hi, (h, w)).astype(np.float32))
        exp = orc.Gray(w, h)
        exp.buf[:] = SENT
        orc.conv2d(k, off, img, exp)
        out = api.GrayF32(w, h)
        out.data[:] = SENT
        api.ConvolveImageNoBorder.convolve(api.Kernel2D_F32(k, offset=off), G(api, img), out)
        assert np.array_equal(bits(out.array()), bits(exp.array())), (kw, off, w, h)


# ------------------------------------------------------------------------------------------------------------------ down-sampling
@pytest.mark.parametrize("kw", (23, 25, 41, 61, 97, 99, 121, 255), ids=lambda kw: "kw%d-general" % kw)
def test_down_convolution_wide(api, orc, kw):
    """ConvolveImageDownNormalized (general k_conv_down above 11 taps) with skip 1..5: GPU acceptance equals the oracle's
    (ValueError <=> IllegalArgumentException), accepted shapes bit for bit, including the naive form and the off-grid skip >= 3 interior"""
    rng = np.random.default_rng(kw)
    k = orc.gaussian1d_f32(-1, kw // 2)
    cases = rejected = 0
    for skip in (1, 2, 3, 4, 5):
        for (w, h) in [(kw + 4 * skip + 13, kw + 2 * skip + 9), (kw - 2, kw + 30), (kw + 1, 21), (kw // 2 + 3, kw + 11)]:
            lo, hi = RANGES[(skip + w) % 3]
            img = orc.Gray.from_array(rng.uniform(lo, hi, (h, w)).astype(np.float32))
            for kind in ("h", "v"):
                ow, oh = (w // skip, h) if kind == "h" else (w, h // skip)
                exp = orc.Gray(ow, oh)
                exp.buf[:] = SENT
                try:
                    orc.conv_down(kind, k, img, skip, out=exp)
                except ValueError:
                    exp = None
                out = api.GrayF32(ow, oh)
                out.data[:] = SENT
                fn = api.ConvolveImageDownNormalized.horizontal if kind == "h" else api.ConvolveImageDownNormalized.vertical
                if exp is None:
                    with pytest.raises(api.IllegalArgumentException):
                        fn(api.Kernel1D_F32(k), G(api, img), out, skip)
                    rejected += 1
                else:
                    fn(api.Kernel1D_F32(k), G(api, img), out, skip)
                    assert np.array_equal(bits(out.array()), bits(exp.array())), (kw, skip, kind, w, h)
                    cases += 1
    assert cases >= 10


@pytest.mark.parametrize("scales,sigma,radius", [([1, 2, 4], -1, 12), ([1, 3, 6], -1, 20), ([2, 4], 5.0, -1)], ids=lambda v: str(v))
def test_discrete_pyramid_wide(api, orc, scales, sigma, radius):
    img = orc.noise_image(331, 257, 5, 0, 255)
    ker = orc.gaussian1d_f32(sigma, radius)
    assert len(ker) >= 25
    try:
        exp, _ = orc.pyramid(ker, sigma, scales, img)
    except ValueError:
        with pytest.raises((api.IllegalArgumentException, RuntimeError)):
            api.FactoryPyramid.discreteGaussian(scales, sigma, radius).process(G(api, img))
        return
    pyr = api.FactoryPyramid.discreteGaussian(scales, sigma, radius)
    pyr.process(G(api, img))
    for i, e in enumerate(exp):
        assert np.array_equal(bits(pyr.getLayer(i).array()), bits(e)), (scales, i)


# ------------------------------------------------------------------------------------------------------------------ BHIP_ERR_UNSUPPORTED
def _conv2d_ref(orc, k, g):
    exp = orc.Gray(g.width, g.height)
    exp.buf[:] = SENT
    return orc.conv2d(k, k.shape[0] // 2, g, exp).array()


def _unsupported_calls(api, orc, rng):
    """(id, call(img, out), accepted, reference or None); accepted calls at the limits must match the oracle"""
    k255 = rng.uniform(0.5, 1.5, 255).astype(np.float32)
    k256 = rng.uniform(0.5, 1.5, 256).astype(np.float32)
    k2d21 = (rng.uniform(-1, 1, (21, 21)) / 21).astype(np.float32)
    k2d22 = (rng.uniform(-1, 1, (22, 22)) / 22).astype(np.float32)
    kinds = _kinds(api)
    calls = []
    for kind, (cls, fn) in kinds.items():
        calls.append(("conv-%s-kw255-runs" % kind, lambda i, o, c=cls, f=fn: getattr(c, f)(api.Kernel1D_F32(k255), i, o), True,
                      lambda g, kind=kind: orc.conv(kind, k255, 127, g, threads=1).array()))
        calls.append(("conv-%s-kw256-unsupported" % kind, lambda i, o, c=cls, f=fn: getattr(c, f)(api.Kernel1D_F32(k256), i, o), False, None))
    calls += [
        ("gaussian-sigma52-261taps-unsupported", lambda i, o: api.BlurImageOps.gaussian(i, o, 52.0, -1), False, None),
        ("mean-r127-runs", lambda i, o: api.BlurImageOps.mean(i, o, 127), True, lambda g: orc.blur_mean(g, 127).array()),
        ("mean-r128-unsupported", lambda i, o: api.BlurImageOps.mean(i, o, 128), False, None),
        ("mean-r128x1-unsupported", lambda i, o: api.BlurImageOps.mean(i, o, 128, 1), False, None),
        ("median-r8-runs", lambda i, o: api.BlurImageOps.median(i, o, 8), True, lambda g: orc.blur_median(g, 8).array()),
        ("median-r9-unsupported", lambda i, o: api.BlurImageOps.median(i, o, 9), False, None),
        ("conv2d-kw21-runs", lambda i, o: api.ConvolveImageNoBorder.convolve(api.Kernel2D_F32(k2d21), i, o), True, lambda g: _conv2d_ref(orc, k2d21, g)),
        ("conv2d-kw22-unsupported", lambda i, o: api.ConvolveImageNoBorder.convolve(api.Kernel2D_F32(k2d22), i, o), False, None),
    ]
    return calls


def test_unsupported_limits_host(api, orc):
    """The limits of the GPU path: the widest accepted calls run and equal the oracle; one beyond raises RuntimeError with status -2
    (BHIP_ERR_UNSUPPORTED, the BOverride signal to fall back to Java) and the caller's output buffer is unchanged"""
    rng = np.random.default_rng(256)
    w, h = 300, 270
    img = orc.Gray.from_array(rng.uniform(0, 255, (h, w)).astype(np.float32))
    for name, call, accepted, ref in _unsupported_calls(api, orc, rng):
        out = api.GrayF32(w, h)
        out.data[:] = SENT
        if accepted:
            call(G(api, img), out)
            exp = ref(img)
            if name.startswith("conv-h") or name.startswith("conv-v"):
                exp = exp.copy()
                exp[_frame(name[5], w, h, 255, 127)] = SENT
            assert np.array_equal(bits(out.array()), bits(exp)), name
        else:
            with pytest.raises(RuntimeError) as e:
                call(G(api, img), out)
            assert "status -2" in str(e.value) and not isinstance(e.value, api.IllegalArgumentException), (name, str(e.value))
            assert np.all(bits(out.data) == bits(np.float32(SENT))), name + ": the output buffer was written"
    # down-sampling convolution: 255 taps run, 257 are unsupported
    k255 = orc.gaussian1d_f32(-1, 127)
    k257 = orc.gaussian1d_f32(-1, 128)
    for kind, fn in (("h", api.ConvolveImageDownNormalized.horizontal), ("v", api.ConvolveImageDownNormalized.vertical)):
        ow, oh = (w // 2, h) if kind == "h" else (w, h // 2)
        exp = orc.Gray(ow, oh)
        exp.buf[:] = SENT
        orc.conv_down(kind, k255, img, 2, out=exp)
        out = api.GrayF32(ow, oh)
        out.data[:] = SENT
        fn(api.Kernel1D_F32(k255), G(api, img), out, 2)
        assert np.array_equal(bits(out.array()), bits(exp.array())), ("down-kw255-runs", kind)
        out.data[:] = SENT
        with pytest.raises(RuntimeError) as e:
            fn(api.Kernel1D_F32(k257), G(api, img), out, 2)
        assert "status -2" in str(e.value), ("down-kw257-unsupported", kind)
        assert np.all(bits(out.data) == bits(np.float32(SENT))), ("down-kw257-unsupported", kind)


def test_unsupported_kw256_device_batch(api, orc):
    import torch
    from boofcv_amd import device as dv
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    try:
        ops = dv.DeviceImageOps(ctx)
        src = torch.rand((2, 300, 280), dtype=torch.float32, device="cuda")
        out = torch.full_like(src, SENT)
        torch.cuda.synchronize()
        for fn in (ops.convolveHorizontal, ops.convolveVertical, ops.convolveNormalizedHorizontal, ops.convolveNormalizedVertical):
            with pytest.raises(RuntimeError) as e:
                fn(np.full(256, 1.0 / 256, np.float32), 128, src, out)
            assert "status -2" in str(e.value)
        ctx.synchronize()
        assert bool(torch.all(out == SENT))
    finally:
        ctx.close()
