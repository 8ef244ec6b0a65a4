"""GPU: the device-resident image ops (bhip_*_dev_* of include/boofhip.h, through boofcv_amd.device.DeviceImageOps) writing into strided
OUTPUT views with guard bands (tests/view_layouts.py).  Every image output is a [B,H,W] window of a sentinel-filled parent: the window must
hold the reference's result bit for bit, every element of the parent outside it must keep its bits (a store past a row's end, before its start,
between two images, above the first or below the last image lands in the parent and fails the assertion), and the frame that the no-border
convolutions and the border=None gradients leave to the caller must still hold the sentinel.  The input parents must come back unchanged.

Shapes.  B = 2.  (W,H) = (259,131) is the smallest shape that crosses every strip boundary of the vector kernels of conv.hip and gradient.hip: 256 columns per block
with a 3-pixel scalar tail in the second strip (259 = 256 + 3), and more rows than 4*CS_ROWS = 32 (k_conv_h_stream), 4*CS_ROWS_V = 64
(k_conv_v_stream), 4*GR_ROWS = 32 (k_grad_stream, k_grad_u8), 4*BF_ROWS = 128 (k_blur_fused) and CV_ROWS = 32 (k_conv_v_tile), with a partial
last strip for each (131 = 128 + 3).  (30,9) covers kernels barely narrower than the image and the naive form of the normalised convolution.

Layouts.  For each output layout of view_layouts.LAYOUTS the input is dense, and then in the output's layout: with pad4 / pad4_x4 the launchers'
vec4(in) && vec4(out) holds in the second combination only.

Which kernel serves which layout (from the launchers' predicates in conv.hip, gradient.hip, corner.hip and fast.hip; float32 unless named):
  convolve*            dense (pitch 259 or 30: no multiple of 4), pad4_x1, odd, and every pair with one of them on either side: k_conv (general).
                       pad4 and pad4_x4 on both sides: widths 3 and 11 k_conv_h_stream / k_conv_v_stream (+ k_conv borderOnly for the normalised
                       forms), widths 13 and 41 and the even kernel k_conv_h_tile<0> / k_conv_v_tile<0,16>; a kernel at least as wide as the
                       axis (normalised forms): k_conv, naive form, whatever the layout.
  gaussian             vec4 on both sides and radius 2 / 5 narrower than the image: k_blur_fused<5> / <11>; else two passes of the above through the
                       library's temporary (radius 6 always).
  sobel / three        vec4(in) && vec4(dx) && 16-byte aligned dy: k_grad_stream; else k_grad (so a derivY 4 bytes off its derivX goes to k_grad).
  sobel / three u8     always k_grad_u8; per four pixels a packed 8-byte store when both row addresses are 8-byte aligned, else four scalar stores.
  intensity            k_grad_intensity (one pixel per thread, any layout).
  cornerIntensity      float32: k_corner_rows + k_corner_cols; weighted: k_corner_weighted_f32 / _s16; int16 box: k_corner_box_s16.
  fast                 k_fast writes the intensity one pixel per thread, any layout (k_fast_lists clears the rows past the stop row)."""
import ctypes as C
import functools

import numpy as np
import pytest

import corner_ref as cr
import fast_ref as fr
import klt_ref as kr
import klt_u8_ref as ku
import view_layouts as vl

pytestmark = pytest.mark.gpu

B = 2
SHAPES = [(259, 131), (30, 9)]
K4 = np.array([0.1, 0.5, -0.2, 0.3], np.float32)   # even width, off-centre origin: the standard (not unrolled) form
K5 = np.array([1, 4, 7, 4, 1], np.int32)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _combos():
    """(input layout, output layout): a dense input and an input in the output's layout, for every output layout"""
    out = []
    for lo in vl.LAYOUTS:
        for li in ("dense", lo):
            if (li, lo) not in out:
                out.append((li, lo))
    return out


COMBOS = _combos()


def _fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- inputs and references: computed once per shape, shared, never modified ----
@functools.lru_cache(maxsize=None)
def _f32_frames(orc, w, h):
    frames = [orc.noise_image(w, h, 700 + b, 0, 255) for b in range(B)]
    host = np.stack([f.array() for f in frames]).astype(np.float32)
    host.setflags(write=False)
    return frames, host


@functools.lru_cache(maxsize=None)
def _u8_frames(w, h):
    a = np.stack([np.random.default_rng(1000 * w + h + b).integers(0, 256, size=(h, w), dtype=np.uint8) for b in range(B)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _f32_derivs(orc, w, h):
    """Sobel derivatives (zero border) of the float32 frames, from the oracle -> (dx, dy) float32 [B,H,W]"""
    frames, _ = _f32_frames(orc, w, h)
    g = [orc.gradient("sobel", f, border_zero=True) for f in frames]
    dx, dy = np.stack([x.array() for x, _ in g]).astype(np.float32), np.stack([y.array() for _, y in g]).astype(np.float32)
    dx.setflags(write=False); dy.setflags(write=False)
    return dx, dy


@functools.lru_cache(maxsize=None)
def _s16_derivs(w, h):
    g = [cr.gradient_u8("sobel", f, True) for f in _u8_frames(w, h)]
    dx, dy = np.stack([x for x, _ in g]), np.stack([y for _, y in g])
    dx.setflags(write=False); dy.setflags(write=False)
    return dx, dy


class Checker:
    """runs one library call on views and checks the parents; failures are collected so that one run names every failing case"""

    def __init__(self, dev):
        self.ops, self.torch = dev
        self.errors = []
        self.seen = set()
        self.calls = 0

    def put(self, layout, host, shift=0):
        """a host [B,H,W] array inside a view of `layout` on the device -> (parent, view)"""
        t = self.torch.from_numpy(np.array(host))   # (a copy: the shared inputs are read-only)
        b, h, w = t.shape
        parent, view = vl.make_view(layout, b, h, w, t.dtype, self.ops.device, shift)
        view.copy_(t.to(self.ops.device))
        return parent, view

    def out(self, layout, w, h, dtype=None, shift=0):
        return vl.make_view(layout, B, h, w, dtype or self.torch.float32, self.ops.device, shift)

    def run(self, what, op, fn, inputs, outputs):
        """fn() with the given (parent, view) inputs and outputs: only the output views are written; on the first call of each `op` the
        input parents are compared as well"""
        first = op not in self.seen
        self.seen.add(op)
        before = [vl.snapshot(p) for p, _ in outputs]
        before_in = [vl.snapshot(p) for p, _ in inputs] if first else []
        fn()
        self.ops.ctx.synchronize()
        self.calls += 1
        for (p, v), b in zip(outputs, before):
            self.check(what, lambda: vl.assert_only_view_written(p, v, b, "output"))
        for (p, v), b in zip(inputs, before_in):
            self.check(what, lambda: vl.assert_only_view_written(p, v, b, "input"))
            self.check(what, lambda: self.same_bits(vl.bits(p), b, "input parent"))

    def same_bits(self, a, b, name):
        assert self.torch.equal(a, b), name + " changed"

    def check(self, what, fn):
        try:
            fn()
        except AssertionError as e:
            self.errors.append("%s: %s" % (what, str(e).splitlines()[0] if str(e) else "assertion failed"))

    def equal(self, what, view, want, keep=None):
        """the view's bits == want's ([B,H,W] host array) where keep ([H,W] bool) is False; where it is True the sentinel is still there"""
        got = view.cpu().numpy()
        want = np.asarray(want)

        def cmp():
            assert got.dtype == want.dtype and got.shape == want.shape, "dtype / shape"
            g, e = (_fbits(got), _fbits(want)) if got.dtype == np.float32 else (got, want)
            sel = np.broadcast_to(~keep, g.shape) if keep is not None else np.ones(g.shape, bool)
            bad = (g != e) & sel
            assert not bad.any(), "%d pixels differ from the reference, first (image, y, x) %s" % (bad.sum(), tuple(int(i[0]) for i in np.nonzero(bad)))
        self.check(what, cmp)
        if keep is not None:
            self.check(what, lambda: vl.assert_kept(view, keep, "frame"))

    def done(self):
        assert self.calls > 0
        assert not self.errors, "%d failures:\n%s" % (len(self.errors), "\n".join(self.errors[:40]))


# ---------------------------------------------------------------------------------------------------------------- convolutions
@pytest.mark.parametrize("kind", ["h", "v", "norm_h", "norm_v"])
def test_convolve_into_views(dev, orc, kind):
    ck = Checker(dev)
    ops = ck.ops
    fn = {"h": ops.convolveHorizontal, "v": ops.convolveVertical, "norm_h": ops.convolveNormalizedHorizontal, "norm_v": ops.convolveNormalizedVertical}[kind]
    kernels = [(orc.gaussian1d_f32(-1, r), r) for r in (1, 5, 6, 20)] + [(K4, 1)]   # 3 / 11 taps: stream; 13 / 41 taps: tile; even: standard form
    ran = set()
    for w, h in SHAPES:
        frames, host = _f32_frames(orc, w, h)
        extent = w if kind.endswith("h") else h
        for k, off in kernels:
            if not kind.startswith("norm") and len(k) > extent:
                continue   # the no-border form needs the kernel inside the image
            ran.add((w, len(k)))
            want = np.stack([orc.conv(kind, k, off, f).array() for f in frames])
            keep = None
            if not kind.startswith("norm"):   # the frame keeps the caller's pixels
                keep = np.ones((h, w), bool)
                right = len(k) - off - 1
                if kind == "h":
                    keep[:, off:w - right] = False
                else:
                    keep[off:h - right, :] = False
            for li, lo in COMBOS:
                src, dst = ck.put(li, host), ck.out(lo, w, h)
                what = "%s %dx%d taps=%d in=%s out=%s" % (kind, w, h, len(k), li, lo)
                ck.run(what, kind, lambda: fn(k, off, src[1], dst[1]), [src], [dst])
                ck.equal(what, dst[1], want, keep)
    assert {(259, 3), (259, 11), (259, 13), (259, 41), (259, 4), (30, 3), (30, 4)} <= ran
    ck.done()


def test_gaussian_into_views(dev, orc):
    ck = Checker(dev)
    for w, h in SHAPES:
        frames, host = _f32_frames(orc, w, h)
        for sigma, radius in [(-1, 2), (-1, 5), (-1, 6)]:   # one fused pass (5, 11 taps); two passes through the library's temporary (13 taps)
            want = np.stack([orc.gaussian_blur(f, sigma, radius).array() for f in frames])
            for li, lo in COMBOS:
                src, dst = ck.put(li, host), ck.out(lo, w, h)
                what = "gaussian r=%d %dx%d in=%s out=%s" % (radius, w, h, li, lo)
                ck.run(what, "gaussian", lambda: ck.ops.gaussian(src[1], sigma, radius, dst[1]), [src], [dst])
                ck.equal(what, dst[1], want)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- gradients
def _frame(w, h):
    keep = np.ones((h, w), bool)
    keep[1:-1, 1:-1] = False
    return keep


@pytest.mark.parametrize("grad", ["sobel", "three"])
def test_gradient_f32_into_views(dev, orc, grad):
    ck = Checker(dev)
    fn = ck.ops.sobel if grad == "sobel" else ck.ops.three
    for w, h in SHAPES:
        frames, host = _f32_frames(orc, w, h)
        for border in (None, 0) + (("EXTENDED",) if grad == "sobel" else ()):
            if border == "EXTENDED":
                g = [kr.sobel_extended(orc, f.array()) for f in frames]
                wx, wy = np.stack([x for x, _ in g]), np.stack([y for _, y in g])
            else:
                g = [orc.gradient(grad, f, border_zero=border is not None) for f in frames]
                wx, wy = np.stack([x.array() for x, _ in g]), np.stack([y.array() for _, y in g])
            keep = _frame(w, h) if border is None else None
            # derivX and derivY share strides, not necessarily alignment: derivY 4 bytes (16: aligned again, another parent) further along
            cases = [(li, lo, 0) for li, lo in COMBOS] + [(li, "pad4", s) for li in ("dense", "pad4") for s in (1, 4)]
            for li, lo, shift in cases:
                src, dx, dy = ck.put(li, host), ck.out(lo, w, h), ck.out(lo, w, h, shift=shift)
                assert dx[1].stride() == dy[1].stride() and dy[1].data_ptr() % 16 == (dx[1].data_ptr() + 4 * shift) % 16
                what = "%s border=%s %dx%d in=%s out=%s dy+%d" % (grad, border, w, h, li, lo, shift)
                ck.run(what, grad, lambda: fn(src[1], border, dx[1], dy[1]), [src], [dx, dy])
                ck.equal(what + " dx", dx[1], wx, keep)
                ck.equal(what + " dy", dy[1], wy, keep)
    ck.done()


@pytest.mark.parametrize("grad", ["sobel", "three"])
def test_gradient_u8_s16_into_views(dev, grad):
    ck = Checker(dev)
    torch = ck.torch
    fn = ck.ops.sobel if grad == "sobel" else ck.ops.three
    for w, h in SHAPES:
        imgs = _u8_frames(w, h)
        for border in (None, 0) + (("EXTENDED",) if grad == "sobel" else ()):
            if border == "EXTENDED":
                g = [ku.sobel_extended_u8(im) for im in imgs]
            else:
                g = [cr.gradient_u8(grad, im, border is not None) for im in imgs]
            wx, wy = np.stack([x for x, _ in g]), np.stack([y for _, y in g])
            keep = _frame(w, h) if border is None else None
            # int16 pad4_x1: rows start 2-byte but not 4-byte aligned (no packed store); derivY 2 / 8 bytes off derivX: the packed store needs both
            cases = [(li, lo, 0) for li, lo in COMBOS] + [(li, "pad4", s) for li in ("dense", "pad4") for s in (1, 4)]
            for li, lo, shift in cases:
                src, dx, dy = ck.put(li, imgs), ck.out(lo, w, h, torch.int16), ck.out(lo, w, h, torch.int16, shift=shift)
                if lo == "pad4_x1":
                    assert dx[1].data_ptr() % 4 == 2 and dx[1].stride(1) % 4 == 0
                what = "%s u8 border=%s %dx%d in=%s out=%s dy+%d" % (grad, border, w, h, li, lo, shift)
                ck.run(what, grad, lambda: fn(src[1], border, dx[1], dy[1]), [src], [dx, dy])
                ck.equal(what + " dx", dx[1], wx, keep)
                ck.equal(what + " dy", dy[1], wy, keep)
    ck.done()


def test_gradient_intensity_into_views(dev, orc):
    ck = Checker(dev)
    for w, h in SHAPES:
        gx, gy = _f32_derivs(orc, w, h)
        for kind in (0, 1, 2):
            want = [np.sqrt(gx * gx + gy * gy), np.abs(gx) + np.abs(gy), gx * gx + gy * gy][kind].astype(np.float32)
            for li, lo in COMBOS:
                dx, dy, dst = ck.put(li, gx), ck.put(li, gy), ck.out(lo, w, h)
                what = "intensity kind=%d %dx%d in=%s out=%s" % (kind, w, h, li, lo)
                ck.run(what, "intensity", lambda: ck.ops.intensity(kind, dx[1], dy[1], dst[1]), [dx, dy], [dst])
                ck.equal(what, dst[1], want)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- corner intensities
@pytest.mark.parametrize("form", ["f32_box", "f32_weighted", "s16_box", "s16_weighted"])
def test_corner_intensity_into_views(dev, orc, form):
    ck = Checker(dev)
    s16, weighted = form.startswith("s16"), form.endswith("weighted")
    radius = 3 if form == "f32_weighted" else 2
    for w, h in SHAPES:
        gx, gy = _s16_derivs(w, h) if s16 else _f32_derivs(orc, w, h)
        for kind, kname, kappa in [(0, "shitomasi", 0.0), (1, "harris", 0.04)]:
            if form == "f32_box":
                want = [orc.corner_intensity(orc.Gray.from_array(gx[b]), orc.Gray.from_array(gy[b]), radius, kname, kappa) for b in range(B)]
            elif form == "f32_weighted":
                want = [cr.corner_weighted_f32(orc, gx[b], gy[b], radius, kind, kappa) for b in range(B)]
            else:
                want = [(cr.corner_weighted_s16 if weighted else cr.corner_box_s16)(gx[b], gy[b], radius, kind, kappa) for b in range(B)]
            want = np.stack(want)
            for li, lo in COMBOS:
                dx, dy, dst = ck.put(li, gx), ck.put(li, gy), ck.out(lo, w, h)
                what = "corner %s %s %dx%d in=%s out=%s" % (form, kname, w, h, li, lo)
                ck.run(what, form, lambda: ck.ops.cornerIntensity(kind, radius, kappa, dx[1], dy[1], dst[1], weighted=weighted), [dx, dy], [dst])
                ck.equal(what, dst[1], want)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- FAST
@pytest.mark.parametrize("pix", ["u8", "f32"])
def test_fast_intensity_into_views(dev, pix):
    ck = Checker(dev)
    torch = ck.torch
    for w, h in SHAPES:
        if pix == "u8":
            imgs, tol = _u8_frames(w, h), 20
        else:
            rng = np.random.default_rng(31 * w + h)
            imgs, tol = (rng.random((B, h, w)) * 100).astype(np.float32), 7.5
        want = [fr.fast(im, tol, 9, 1.0) for im in imgs]
        winten = np.stack([x[0] for x in want])
        if w > 100:
            assert all(len(x[1]) > 10 and len(x[2]) > 10 for x in want)
        lists = {}
        for li, lo in COMBOS:
            src, dst = ck.put(li, imgs), ck.out(lo, w, h)
            what = "fast %s %dx%d in=%s out=%s" % (pix, w, h, li, lo)
            res = []
            ck.run(what, "fast", lambda: res.extend(ck.ops.fast(src[1], tol, 9, 1.0, intensity=dst[1])), [src], [dst])
            ck.equal(what, dst[1], winten)
            _, xyLow, nLow, xyHigh, nHigh = (None if t is None else t.cpu().numpy() for t in res)
            lists[(li, lo)] = [(xyLow[b, :nLow[b]], xyHigh[b, :nHigh[b]]) for b in range(B)]

            def cmp():
                for b in range(B):
                    got, first = lists[(li, lo)][b], lists[COMBOS[0]][b]
                    assert np.array_equal(got[0], want[b][1]) and np.array_equal(got[1], want[b][2]), "corner lists differ from the reference"
                    assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), "corner lists differ from the dense run"
            ck.check(what, cmp)
    assert COMBOS[0] == ("dense", "dense")
    ck.done()


# ---------------------------------------------------------------------------------------------------------------- list outputs
GUARD = 32   # int16 / int32 elements in front of and behind a list buffer


def _list_buffers(torch, device, cap, lists):
    """-> (xy buffers, n buffer): `lists` flat int16 buffers of B*cap pairs filled with -5, each between two guards, and one int32 buffer of
    lists*B counts filled with -1 between two guards"""
    xy = [torch.full((GUARD + B * cap * 2 + GUARD,), -5, dtype=torch.int16, device=device) for _ in range(lists)]
    n = torch.full((GUARD + lists * B + GUARD,), -1, dtype=torch.int32, device=device)
    return xy, n


def _check_lists(what, xy, n, cap, wants):
    """wants[l][b] = the reference's list l of image b"""
    n = n.cpu().numpy()
    assert np.all(n[:GUARD] == -1) and np.all(n[GUARD + len(wants) * B:] == -1), what + ": a count was written outside its slots"
    for l, want in enumerate(wants):
        buf = xy[l].cpu().numpy()
        assert np.all(buf[:GUARD] == -5) and np.all(buf[GUARD + B * cap * 2:] == -5), what + ": a pair was written outside the lists"
        pairs = buf[GUARD:GUARD + B * cap * 2].reshape(B, cap, 2)
        for b in range(B):
            assert n[GUARD + l * B + b] == len(want[b]), (what, "count", l, b)
            k = min(cap, len(want[b]))
            assert np.array_equal(pairs[b, :k], np.asarray(want[b], np.int16).reshape(-1, 2)[:k]), (what, "pairs", l, b)
            assert np.all(pairs[b, k:] == -5), (what, "entries past the count", l, b)


def _ptr(t, offset):
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


def test_nonmax_lists_with_a_small_cap(dev, orc):
    """cap below the true count: exact counts, the first cap pairs, nothing behind them -- for strided inputs as well"""
    ops, torch = dev
    from boofcv_amd.device import _geom
    w, h = SHAPES[0]
    gx, gy = _f32_derivs(orc, w, h)
    inten = np.sqrt(gx * gx + gy * gy).astype(np.float32)
    ck = Checker(dev)
    for radius, thr, border in [(2, 100.0, 0), (3, 50.0, 1)]:
        want = [orc.nonmax(orc.Gray.from_array(inten[b]), radius, thr, border) for b in range(B)]
        cap = min(len(x) for x in want) // 2
        assert cap > 8
        for layout in ("dense", "pad4_x4", "odd"):
            src = ck.put(layout, inten)
            before = vl.snapshot(src[0])
            xy, n = _list_buffers(torch, ops.device, cap, 1)
            ip, iis, irs, W, H, nb = _geom(src[1])
            st = ops.L.bhip_nonmax_block_dev_f32(ops.ctx._h, ip, iis, irs, W, H, nb, radius, thr, border, _ptr(xy[0], GUARD), cap, _ptr(n, GUARD))
            assert st == 0
            ops.ctx.synchronize()
            _check_lists("nonmax r=%d %s" % (radius, layout), xy, n, cap, [want])
            assert torch.equal(vl.bits(src[0]), before)
            # and with room for everything, through DeviceImageOps
            gxy, gn = ops.nonmax(src[1], radius, thr, border)
            ops.ctx.synchronize()
            gxy, gn = gxy.cpu().numpy(), gn.cpu().numpy()
            for b in range(B):
                assert gn[b] == len(want[b]) and np.array_equal(gxy[b, :gn[b]], want[b]), (layout, b)


def test_nonmax_min_max_lists_with_a_small_cap(dev, orc):
    ops, torch = dev
    from boofcv_amd.device import _geom
    w, h = SHAPES[0]
    gx, _ = _f32_derivs(orc, w, h)   # a signed image: minima and maxima
    ck = Checker(dev)
    for radius, thr, border in [(2, 60.0, 0), (3, 20.0, 2)]:
        want = [fr.nonmax_block(gx[b], radius, -thr, thr, border, True, True) for b in range(B)]
        wmin, wmax = [x[0] for x in want], [x[1] for x in want]
        cap = min(min(len(x) for x in wmin), min(len(x) for x in wmax)) // 2
        assert cap > 8
        for layout in ("dense", "pad4_x4", "odd"):
            src = ck.put(layout, gx)
            before = vl.snapshot(src[0])
            xy, n = _list_buffers(torch, ops.device, cap, 2)
            ip, iis, irs, W, H, nb = _geom(src[1])
            st = ops.L.bhip_nonmax_block_minmax_dev_f32(ops.ctx._h, ip, iis, irs, W, H, nb, radius, -thr, thr, border, 1, 1, _ptr(xy[0], GUARD), _ptr(n, GUARD),
                                                        _ptr(xy[1], GUARD), _ptr(n, GUARD + B), cap)
            assert st == 0
            ops.ctx.synchronize()
            _check_lists("nonmaxMinMax r=%d %s" % (radius, layout), xy, n, cap, [wmin, wmax])
            assert torch.equal(vl.bits(src[0]), before)
            xyMin, nMin, xyMax, nMax = (t.cpu().numpy() for t in ops.nonmaxMinMax(src[1], radius, -thr, thr, border))
            for b in range(B):
                assert np.array_equal(xyMin[b, :nMin[b]], wmin[b]) and np.array_equal(xyMax[b, :nMax[b]], wmax[b]), (layout, b)


# ---------------------------------------------------------------------------------------------------------------- input views
def test_brief_and_pyramid_from_input_views(dev, orc):
    ops, torch = dev
    ck = Checker(dev)
    sp, cp = orc.brief_definition()
    ran = 0
    for w, h in SHAPES:
        frames, host = _f32_frames(orc, w, h)
        imgs = _u8_frames(w, h)
        rng = np.random.default_rng(w * 1000 + h)
        counts = [int(c) for c in rng.integers(5, 40, B)]
        start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        pts = np.stack([rng.uniform(-2, w + 2, start[-1]), rng.uniform(-2, h + 2, start[-1])], axis=1)
        wbrief = np.concatenate([orc.brief_describe(frames[b], pts[start[b]:start[b + 1]], 16, sp, cp) for b in range(B)])
        scales = [1, 2, 4] if w > 100 else [1, 2]
        ker = orc.gaussian1d_f32(-1, 2)
        try:
            wpyr = [orc.pyramid(ker, -1, scales, f)[0] for f in frames]
        except ValueError:
            wpyr = None   # a shape the reference rejects
        wpyr8 = [ku.pyramid_u8(im, scales) for im in imgs]
        for layout in ("dense", "pad4_x4", "odd"):
            src, src8 = ck.put(layout, host), ck.put(layout, imgs)
            before, before8 = vl.snapshot(src[0]), vl.snapshot(src8[0])
            words = ops.brief(src[1], 16, sp, cp, torch.from_numpy(pts).to(ops.device), start)
            ops.ctx.synchronize()
            assert np.array_equal(words.cpu().numpy(), wbrief), ("brief", w, h, layout)
            if wpyr is not None:
                layers = ops.pyramid(ker, scales, src[1])
                ops.ctx.synchronize()
                for b in range(B):
                    for i, e in enumerate(wpyr[b]):
                        assert np.array_equal(_fbits(layers[i][b].cpu().numpy()), _fbits(e)), ("pyramid f32", w, h, layout, b, i)
                ran += 1
            layers = ops.pyramid(K5, scales, src8[1])
            ops.ctx.synchronize()
            for b in range(B):
                for i, e in enumerate(wpyr8[b]):
                    got = layers[i][b].cpu().numpy()
                    assert got.dtype == e.dtype and np.array_equal(got, e), ("pyramid u8", w, h, layout, b, i)
            assert torch.equal(vl.bits(src[0]), before) and torch.equal(vl.bits(src8[0]), before8), ("an input parent changed", w, h, layout)
    assert ran >= 3
