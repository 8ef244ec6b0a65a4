"""The CPU oracle's wide filters against an fp64 reference written from BoofCV's definitions (not from the oracle's code).

The GPU tests compare the HIP kernels with the oracle bit for bit, so the oracle is the yardstick of every filter.  Here it is checked on
its own at the wide widths the GPU dispatches differently (13 ... 255 taps, off-centre and even kernels, kernels wider than the image):

  no-border convolution      out(x) = sum_i s(x - off + i) k_i on the interior, the frame untouched
  normalised convolution     interior as above with the kernel divided by its sum when |sum - 1| > 1e-4; border and kernels wider than
                             the image: the sum over the part of the window inside the image divided by the weight of that part
  mean blur                  the plain average over the window clipped to the image, rows then columns
  median blur                the (count // 2)-th order statistic of the clipped window (exact)
  2-D convolution            sum_ij s k_ij on the interior, the frame untouched
  down-sampling convolution  output D centred on D * skip: the plain sum where the whole window is inside the image, the clipped sum over
                             the clipped weight where it is not

Tolerances (u = 2^-24, gamma_n = n u / (1 - n u); Higham, Accuracy and Stability of Numerical Algorithms, sec. 3.1):
  * The inputs and the kernel are fp32 values; the reference evaluates them exactly enough in fp64 (its own error, about n 2^-53 of the
    same sums, is below 1e-6 of every bound used here).
  * A sum of n products evaluated in fp32 in any order, starting from 0, is within gamma_n * A of the exact sum, A = sum |s_i k_i|.
  * Re-normalised kernel: the sequential fp32 sum S^ = S (1 + t), |t| <= gamma_{n-1} for a positive kernel, and each k_i / S^ is rounded
    once more, so k'_i = (k_i / S)(1 + eta_i) with |eta_i| <= gamma_{n+1}.  An interior output is then within gamma_{2n+1} * A / S of
    sum s k / S (gamma_a + gamma_b + gamma_a gamma_b <= gamma_{a+b}).
  * Clipped window of m taps, T = sum s k and W = sum k over the clipped part (the common factor 1 / S cancels in T / W).  With g = gamma_m
    (plain kernel) or gamma_{m+n+1} (re-normalised kernel), T^ = T + e_T, |e_T| <= g A, and W^ = W + e_W, |e_W| <= g B with
    B = sum |k| over the clipped part; one more rounding for the division gives
        |r^ - T/W| <= (g A + |T/W| g B) / (|W| - g B) * (1 + u) + u |T/W|.
  * Mean blur, one axis, window of w = 2r + 1 taps over an axis of length L, M = max |s|.  Border (and kernel wider than the axis): the
    clipped-window bound above with all weights fl(1/w), so B = W and A <= M W: at most 2 gamma_w M / (1 - gamma_w) (1 + u) + u M.
    Interior: the running sum starts as w additions (error gamma_w w M) and each of the t <= L later steps subtracts one sample and adds
    one (two roundings of a value <= w M + error), so after t steps the error is at most gamma_{w+2t} w M; divided by w and rounded:
    gamma_{w+2L} M (1 + u) + u M.  This bound grows with the row length, as the running sum's error does.  The column pass averages the
    row pass's output, so its error adds to the row pass's (the average of errors <= e is <= e), with M grown by that error.
  * 2-D convolution: gamma_{kw*kw} A for the standard form (one running total); gamma_{2 kw} A for the unrolled widths (row sums from 0,
    then kw - 1 additions of the row sums).
  * Down-sampling convolution: where the whole window is inside the image the library's classes may take the interior (plain sum) or a
    border class (normalised) -- the two differ by |P| |1 - K| / K, K = sum k, which is added to the larger of the two bounds.
A subtly wrong oracle (a tap dropped or repeated, a window shifted by one, a weight not clipped) is off by about M / kw or more, orders of
magnitude above these bounds (at most about 2e-5 M at 255 taps on a 513-pixel row).
"""
import numpy as np
import pytest

U = 2.0 ** -24
WIDTHS = (13, 18, 19, 20, 21, 22, 33, 41, 64, 65, 96, 97, 98, 99, 129, 255)
RANGES = ((0.0, 255.0), (-5.0, 5.0), (1e3, 1e4))


def gamma(n):
    assert n * U < 0.5
    return n * U / (1.0 - n * U)


def _image(orc, rng, w, h, lo, hi):
    return orc.Gray.from_array(rng.uniform(lo, hi, (h, w)).astype(np.float32))


def _axis_sums(src, k, off):
    """Clipped-window sums along the rows of src (fp64): T = sum s k, A = sum |s k|, W = sum k, B = sum |k|, m = taps inside the image,
    for every output x with the window x - off ... x - off + kw - 1."""
    H, L = src.shape
    kw = len(k)
    pad = np.zeros((H, L + kw - 1))
    pad[:, off:off + L] = src
    inside = np.zeros(L + kw - 1)
    inside[off:off + L] = 1.0
    T = np.zeros((H, L)); A = np.zeros((H, L)); W = np.zeros(L); B = np.zeros(L); m = np.zeros(L)
    for i in range(kw):
        seg, ins = pad[:, i:i + L], inside[i:i + L]
        T += seg * k[i]; A += np.abs(seg) * abs(k[i])
        W += ins * k[i]; B += ins * abs(k[i]); m += ins
    return T, A, W, B, m


def _along(kind, a):
    """rows for horizontal kinds, columns (transposed) for vertical ones"""
    return a if kind in ("h", "norm_h") else a.T


def _clipped_bound(T, A, W, B, g):
    r = T / W
    return r, (g * A + np.abs(r) * g * B) / (np.abs(W) - g * B) * (1 + U) + U * np.abs(r)


def _renorm_sum(k):
    """the re-normalisation rule (ConvolveImageNormalized): divide by the sum when it is off 1 by more than 1e-4.  The fp32 sum the rule
    tests is within gamma_n sum|k| of the fp64 one: the cases here stay clear of the threshold by more than that, so both decide alike."""
    s = float(np.sum(k, dtype=np.float64))
    assert abs(abs(s - 1.0) - 1e-4) > 2 * gamma(len(k)) * float(np.sum(np.abs(k), dtype=np.float64)), "kernel too close to the threshold"
    return s if abs(s - 1.0) > 1e-4 else None


def _kernels(rng, kw):
    """(name, fp32 kernel): a Gaussian (odd widths: FactoryKernelGaussian's; even widths: the next odd one without its last tap, which
    puts its sum off 1 by more than 1e-4), a positive kernel that is re-normalised, a signed kernel"""
    from oracle import pyoracle as orc
    g = orc.gaussian1d_f32(-1, kw // 2)[:kw]
    pos = rng.uniform(0.5, 1.5, kw).astype(np.float32)
    pos = (pos * np.float32(1.3 / pos.sum())).astype(np.float32)
    signed = (rng.uniform(-1, 1, kw) / np.sqrt(kw)).astype(np.float32)
    return [("gauss", g), ("pos", pos), ("signed", signed)]


def _origins(rng, kw):
    return [("centre", kw // 2), ("off0", 0), ("offlast", kw - 1), ("offrand", int(rng.integers(0, kw)))]


@pytest.mark.parametrize("kw", WIDTHS)
def test_separable_convolution_matches_fp64(orc, kw):
    rng = np.random.default_rng(1000 + kw)
    n = 0
    for oi, (oname, off) in enumerate(_origins(rng, kw)):
        for ki, (kname, k) in enumerate(_kernels(rng, kw)):
            i = 3 * oi + ki
            k64 = k.astype(np.float64)
            lo, hi = RANGES[i % 3]
            # along the filtered axis: a 2-pixel interior, wider, exactly the kernel, narrower than the kernel
            L = [kw + 1, kw + 37, kw, max(kw - 5, 1)][i % 4]
            for kind in ("h", "v", "norm_h", "norm_v"):
                norm = kind.startswith("norm")
                if norm and kname == "signed":
                    continue
                w, h = (L, 7) if kind in ("h", "norm_h") else (6, L)
                img = _image(orc, rng, w, h, lo, hi)
                got = _along(kind, orc.conv(kind, k, off, img, threads=1).array().astype(np.float64))
                src = _along(kind, img.array().astype(np.float64))
                T, A, W, B, m = _axis_sums(src, k64, off)
                inter = np.zeros(L, bool)
                inter[off:max(off, L - (kw - off - 1))] = True   # empty when the kernel is wider than the axis
                ctx = (kw, oname, kname, kind, w, h)
                if not norm:
                    # the frame is untouched (the oracle's output starts at 0); the interior is the full sum
                    assert np.all(got[:, ~inter] == 0), ctx
                    err = np.abs(got[:, inter] - T[:, inter])
                    assert np.all(err <= gamma(kw) * A[:, inter]), (ctx, float(np.max(err / np.maximum(A[:, inter], 1e-30))))
                    n += int(inter.sum()) * src.shape[0]
                    continue
                if kw >= L:
                    # ConvolveNormalizedNaive: every output is the clipped ratio with the kernel as given (no re-normalisation)
                    r, bound = _clipped_bound(T, A, W, B, gamma(kw))
                    assert np.all(np.abs(got - r) <= bound), ctx
                    n += got.size
                    continue
                S = _renorm_sum(k)
                g_in = gamma(kw) if S is None else gamma(2 * kw + 1)
                interior = T / (1.0 if S is None else S)
                a_in = A / (1.0 if S is None else S)
                err = np.abs(got[:, inter] - interior[:, inter])
                assert np.all(err <= g_in * a_in[:, inter]), (ctx, "interior")
                g_b = gamma(kw) if S is None else gamma(2 * kw + 1)   # m + n + 1 with m < n taps inside the image
                r, bound = _clipped_bound(T, A, W, B, g_b)
                assert np.all(np.abs(got[:, ~inter] - r[:, ~inter]) <= bound[:, ~inter]), (ctx, "border")
                # and the rule itself: the interior of a re-normalised kernel is NOT the plain sum (the test can tell them apart)
                if S is not None and inter.any():
                    assert np.any(np.abs(T[:, inter] - interior[:, inter]) > g_in * a_in[:, inter]), ctx
                n += got.size
    assert n > 1000


@pytest.mark.parametrize("rx,ry,w,h", [
    (5, 5, 37, 29), (8, 3, 33, 45), (20, 20, 41, 100), (20, 7, 40, 60),   # 2r+1 == extent, one less, and greater (on one axis only)
    (60, 2, 121, 30), (60, 4, 120, 33), (60, 5, 130, 9),
    (20, 3, 42, 30), (127, 1, 255, 13), (127, 3, 254, 17), (127, 2, 256, 9), (127, 2, 301, 11),
])
def test_mean_blur_matches_fp64(orc, rx, ry, w, h):
    rng = np.random.default_rng(rx * 1000 + ry + w)
    for lo, hi in RANGES:
        img = _image(orc, rng, w, h, lo, hi)
        got = orc.blur_mean(img, rx, ry).array().astype(np.float64)
        s = img.array().astype(np.float64)
        M = float(np.max(np.abs(s)))

        def box(a, r):
            T, A, W, B, m = _axis_sums(a, np.ones(2 * r + 1), r)
            return T / m

        def bound(r, L, M):
            kw = 2 * r + 1
            return max(gamma(kw + 2 * L) * M * (1 + U) + U * M, 2 * gamma(kw) * M / (1 - gamma(kw)) * (1 + U) + U * M)

        exp = box(box(s, rx).T, ry).T
        e_h = bound(rx, w, M)
        e_v = bound(ry, h, M + e_h)
        err = np.abs(got - exp)
        assert np.all(err <= e_h + e_v), (rx, ry, w, h, lo, float(err.max()), e_h + e_v)


@pytest.mark.parametrize("r,w,h", [(4, 37, 23), (5, 19, 41), (6, 50, 17), (7, 31, 33), (8, 45, 29), (8, 13, 11), (6, 9, 40)])
def test_median_blur_is_the_order_statistic(orc, r, w, h):
    rng = np.random.default_rng(r * 100 + w)
    for lo, hi in RANGES[:2]:
        a = rng.uniform(lo, hi, (h, w)).astype(np.float32)
        a[::3, ::2] = np.round(a[::3, ::2]) + np.float32(0)   # some ties (+0 turns -0 into 0: the order statistic cannot tell them apart)
        img = orc.Gray.from_array(a)
        got = orc.blur_median(img, r).array()
        exp = np.empty_like(a)
        for y in range(h):
            for x in range(w):
                win = a[max(0, y - r):min(h, y + r + 1), max(0, x - r):min(w, x + r + 1)].ravel()
                exp[y, x] = np.partition(win, win.size // 2)[win.size // 2]
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (r, w, h)


@pytest.mark.parametrize("kw", [8, 9, 11, 13, 16, 21])
def test_conv2d_matches_fp64(orc, kw):
    rng = np.random.default_rng(kw)
    for off, (w, h), (lo, hi) in zip([kw // 2, 0, kw - 1, int(rng.integers(0, kw))], [(kw + 9, kw + 4), (40, 33), (kw, kw + 1), (29, 50)], RANGES + RANGES[:1]):
        k = (rng.uniform(-1, 1, (kw, kw)) / kw).astype(np.float32)
        img = _image(orc, rng, w, h, lo, hi)
        got = orc.conv2d(k, off, img).array().astype(np.float64)
        s = img.array().astype(np.float64)
        oR = kw - off - 1
        T = np.zeros((h - kw + 1, w - kw + 1)); A = np.zeros_like(T)
        for i in range(kw):
            for j in range(kw):
                seg = s[i:i + h - kw + 1, j:j + w - kw + 1]
                T += seg * float(k[i, j]); A += np.abs(seg) * abs(float(k[i, j]))
        unrolled = off == kw // 2 and kw % 2 == 1 and kw <= 11
        g = gamma(2 * kw) if unrolled else gamma(kw * kw)
        inner = got[off:h - oR, off:w - oR]
        assert np.all(np.abs(inner - T) <= g * A), (kw, off, w, h)
        frame = np.ones((h, w), bool); frame[off:h - oR, off:w - oR] = False
        assert np.all(got[frame] == 0), (kw, off, w, h)


def _down_cases():
    for kw in (23, 25, 41, 61, 97, 121, 255):
        r = kw // 2
        for skip in (1, 2, 3, 4, 5):
            if r > skip and r % skip:
                continue   # the off-grid interior of the reference (skip >= 3, radius % skip != 0) is pinned by the GPU tests only
            yield kw, skip


@pytest.mark.parametrize("kw,skip", list(_down_cases()))
def test_down_convolution_matches_fp64(orc, kw, skip):
    rng = np.random.default_rng(kw * 10 + skip)
    k = orc.gaussian1d_f32(-1, kw // 2)
    k64 = k.astype(np.float64)
    K = float(k64.sum())
    r = kw // 2
    checked = 0
    # wider than the kernel (interior + both borders) along the filtered axis, and the naive form (kernel at least as wide as the image)
    for kind, (w, h) in [("h", (kw + 3 * skip + 17, 9)), ("v", (kw + 5, kw + 4 * skip + 11)), ("h", (kw - 3, 8)), ("v", (kw, kw + 9))]:
        lo, hi = RANGES[checked % 3]
        img = _image(orc, rng, w, h, lo, hi)
        try:
            got = orc.conv_down(kind, k, img, skip).array().astype(np.float64)
        except ValueError:
            continue   # a shape the reference rejects (the GPU tests pin the rejection)
        s = img.array().astype(np.float64)
        if kind == "v":
            got, s = got.T, s.T
        T, A, W, B, m = _axis_sums(s, k64, r)
        D = np.arange(got.shape[1]) * skip
        T, A, W, B, m = T[:, D], A[:, D], W[D], B[D], m[D]
        full = m == kw
        P = T
        r_n, b_n = _clipped_bound(T, A, W, B, gamma(kw))
        b_full = np.maximum(gamma(kw) * A, b_n) + np.abs(P) * abs(1 - K) / K
        err_full = np.abs(got[:, full] - P[:, full])
        assert np.all(err_full <= b_full[:, full]), (kw, skip, kind, w, h, "full window")
        assert np.all(np.abs(got[:, ~full] - r_n[:, ~full]) <= b_n[:, ~full]), (kw, skip, kind, w, h, "clipped window")
        checked += 1
    assert checked >= 2, (kw, skip)


def test_gaussian_kernel_host_code_equals_oracle(orc):
    """FactoryKernelGaussian.gaussian1D_F32 in libboofhip.so (host code; no GPU context) == the oracle's, bit for bit, over a grid of
    (sigma, radius) with wide radii and sigma-only calls; sigma-only widths follow radius = ceil((5 sigma - 1) / 2)."""
    from boofcv_amd import api, build
    build.build()
    n = 0
    for sigma in (-1, 0.3, 1.0, 2.5, 7.0, 20.0, 42.0, 52.0):
        for radius in (-1, 1, 6, 20, 48, 49, 64, 127, 130):
            if sigma <= 0 and radius <= 0:
                continue
            got = api.FactoryKernelGaussian.gaussian1D_F32(sigma, radius)
            exp = orc.gaussian1d_f32(sigma, radius)
            assert got.width == len(exp) and got.offset == len(exp) // 2, (sigma, radius)
            assert np.array_equal(got.data.view(np.uint32), exp.view(np.uint32)), (sigma, radius)
            n += 1
    for sigma, taps in [(2.5, 13), (7.0, 35), (20.0, 101), (42.0, 211), (52.0, 261)]:
        assert len(orc.gaussian1d_f32(sigma, -1)) == taps == api.FactoryKernelGaussian.gaussian1D_F32(sigma, -1).width
    assert n > 60
