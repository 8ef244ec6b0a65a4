"""numpy restatement of the integer gradient + corner path and the weighted corner intensity (test reference, not product code).

Written from the cited BoofCV sources:
  GradientSobel_Outer.process_sub(GrayU8, GrayS16, GrayS16)    I:alg/filter/derivative/impl/GradientSobel_Outer.java:76-
  GradientThree_Standard.process(GrayU8, GrayS16, GrayS16)     I:alg/filter/derivative/impl/GradientThree_Standard.java:67-88
    border = ImageBorderValue(0): the integer 3x3 / 3-tap kernels on the zero-padded image (GradientSobel.java:73-74, DerivativeHelperFunctions)
  ImplSsdCorner_S16 + ImplSsdCornerBox                          F:alg/feature/detect/intensity/impl/ImplSsdCorner_S16.java:63-198, ImplSsdCornerBox.java:36-54
  ImplSsdCornerWeighted_S16 / _F32                              F:alg/feature/detect/intensity/impl/ImplSsdCornerWeighted_S16.java:50-108, _F32.java:46-104
  ConvolveImageNormalized (Kernel1D_S32)                        I:alg/filter/convolve/ConvolveImageNormalized.java:768-800
  FactoryKernelGaussian.gaussian(Kernel1D_S32, -1, r)           I:factory/filter/kernel/FactoryKernelGaussian.java:120-160,218-238,388-393
  KernelMath.convert(Kernel1D_F32, minFrac)                     I:alg/filter/kernel/KernelMath.java:556-620
  ShiTomasiCorner_S32 / HarrisCorner_S32                        F:.../impl/ShiTomasiCorner_S32.java:34-42, HarrisCorner_S32.java:45-51

Java int arithmetic wraps: sums are formed exactly in int64 and wrapped to int32 (a wrapping running sum is the exact sum mod 2^32).  Java's
`/` truncates toward zero; numpy's `//` floors, so it is never applied to a value that may be negative.
"""
import math

import numpy as np


def wrap32(a):
    """int64 values -> the int32 value Java's wrapping int arithmetic gives (returned as int64)"""
    a = np.asarray(a, dtype=np.int64)
    return ((a + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def trunc_div(n, d):
    """Java int division: truncates toward zero (d > 0)"""
    n = np.asarray(n, dtype=np.int64)
    q = np.abs(n) // d
    return np.where(n < 0, -q, q)


def _shift(p, dy, dx, H, W):
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def gradient_u8(kind, img, border, dx0=None, dy0=None):
    """GrayU8 (H,W) -> (dx, dy) int16.  border False: only the interior is written (dx0 / dy0 keep the frame, zeros by default)."""
    img = np.asarray(img, dtype=np.uint8)
    H, W = img.shape
    p = np.pad(img.astype(np.int64), 1)
    a = lambda dy, dx: _shift(p, dy, dx, H, W)
    if kind == "sobel":
        v = a(1, 1) - a(-1, -1)
        w = a(1, -1) - a(-1, 1)
        gy = (a(1, 0) - a(-1, 0)) * 2 + v + w
        gx = (a(0, 1) - a(0, -1)) * 2 + v - w
    else:
        gx = a(0, 1) - a(0, -1)
        gy = a(1, 0) - a(-1, 0)
    dx = np.zeros((H, W), np.int16) if dx0 is None else np.array(dx0, dtype=np.int16)
    dy = np.zeros((H, W), np.int16) if dy0 is None else np.array(dy0, dtype=np.int16)
    if border:
        dx[:, :] = gx.astype(np.int16)
        dy[:, :] = gy.astype(np.int16)
    elif H > 2 and W > 2:
        dx[1:-1, 1:-1] = gx[1:-1, 1:-1].astype(np.int16)
        dy[1:-1, 1:-1] = gy[1:-1, 1:-1].astype(np.int16)
    return dx, dy


def products_s32(dx, dy):
    x = np.asarray(dx, dtype=np.int64)
    y = np.asarray(dy, dtype=np.int64)
    return x * x, x * y, y * y   # |product| <= 2^30: no wrap


def score_s32(kind, xx, xy, yy, kappa=0.04):
    """ShiTomasiCorner_S32 (kind 0 / 'shitomasi') or HarrisCorner_S32 (kind 1 / 'harris') on int32 sums -> float32"""
    xx, xy, yy = wrap32(xx), wrap32(xy), wrap32(yy)
    if kind in (0, "shitomasi"):
        left = wrap32(xx + yy).astype(np.float64) * 0.5
        b = wrap32(xx - yy).astype(np.float64) * 0.5
        sxy = xy.astype(np.float64)
        right = np.sqrt(b * b + sxy * sxy)
        return (left - right).astype(np.float32)
    if kind == "mocksum":   # the MockSum of the reference tests: totalXX + totalXY + totalYY (int), to float
        return wrap32(xx + xy + yy).astype(np.float32)
    k = np.float32(kappa)
    fxx, fxy, fyy = xx.astype(np.float32), xy.astype(np.float32), yy.astype(np.float32)
    trace = fxx + fyy
    return (fxx * fyy - fxy * fxy) - k * trace * trace


def score_f32(kind, xx, xy, yy, kappa=0.04):
    """ShiTomasiCorner_F32 / HarrisCorner_F32 on float32 sums"""
    xx, xy, yy = (np.asarray(v, dtype=np.float32) for v in (xx, xy, yy))
    half = np.float32(0.5)
    if kind in (0, "shitomasi"):
        left = (xx + yy) * half
        b = (xx - yy) * half
        return left - np.sqrt(b * b + xy * xy)
    k = np.float32(kappa)
    trace = xx + yy
    return (xx * yy - xy * xy) - k * trace * trace


def box_sum(a, r):
    """exact (2r+1)^2 window sums at every centre (H-2r, W-2r), int64"""
    a = np.asarray(a, dtype=np.int64)
    c = np.pad(np.cumsum(np.cumsum(a, 0), 1), ((1, 0), (1, 0)))
    k = 2 * r + 1
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def corner_box_s16(dx, dy, radius, kind, kappa=0.04):
    """ImplSsdCorner_S16.process: float32 (H,W), 0 on the border of `radius` pixels"""
    H, W = np.shape(dx)
    out = np.zeros((H, W), np.float32)
    sums = [wrap32(box_sum(p, radius)) for p in products_s32(dx, dy)]
    out[radius:H - radius, radius:W - radius] = score_s32(kind, *sums, kappa=kappa)
    return out


def gaussian_kernel_s32(radius):
    """FactoryKernelGaussian.gaussian(Kernel1D_S32, -1, radius): un-normalised float PDF, KernelMath.convert(k, 1/100f)"""
    if radius <= 0:
        raise ValueError("Radius must be > 0")
    sigma = (radius * 2.0 + 1.0) / 5.0
    pdf = [math.exp(-i * i / (2.0 * sigma * sigma)) / (sigma * math.sqrt(2.0 * math.pi)) for i in range(radius, -radius - 1, -1)]
    f = np.array(pdf, dtype=np.float32)
    mx = np.float32(np.max(np.abs(f)))
    min_value = mx * (np.float32(1.0) / np.float32(100.0))
    mn = np.float32(np.finfo(np.float32).max)
    for v in np.abs(f):
        if v < mn and v >= min_value:
            mn = v
    return np.array([int(np.float32(v) / mn) for v in f], dtype=np.int64)   # (int) of a positive float truncates


def conv_norm_s32(a, kernel, axis):
    """ConvolveImageNormalized.horizontal (axis 1) / vertical (axis 0) with a Kernel1D_S32 of offset width/2 on int32 values.
    Interior, border and naive forms all evaluate (total + weight/2) / weight with the weight of the taps inside the image."""
    a = np.asarray(a, dtype=np.int64)
    k = np.asarray(kernel, dtype=np.int64)
    kw, r = len(k), len(k) // 2
    n = a.shape[axis]
    total = np.zeros(a.shape, np.int64)
    weight = np.zeros(n, np.int64)
    pos = np.arange(n)
    for t in range(kw):
        src = pos - r + t
        ok = (src >= 0) & (src < n)
        weight += np.where(ok, k[t], 0)
        taken = np.take(a, np.clip(src, 0, n - 1), axis=axis)
        mask = ok[:, None] if axis == 0 else ok[None, :]
        total += np.where(mask, taken * k[t], 0)
    wshape = (n, 1) if axis == 0 else (1, n)
    weight = weight.reshape(wshape)
    return trunc_div(wrap32(wrap32(total) + weight // 2), weight)   # weight > 0: weight // 2 is weight / 2


def corner_weighted_s16(dx, dy, radius, kind, kappa=0.04):
    """ImplSsdCornerWeighted_S16.process: float32 (H,W) on every pixel"""
    k = gaussian_kernel_s32(radius)
    sums = [conv_norm_s32(conv_norm_s32(p, k, 1), k, 0) for p in products_s32(dx, dy)]
    return score_s32(kind, *sums, kappa=kappa)


def corner_weighted_f32(orc, dx, dy, radius, kind, kappa=0.04):
    """ImplSsdCornerWeighted_F32.process: float32 products, the oracle's ConvolveImageNormalized with FactoryKernelGaussian(-1, r), score"""
    dx = np.asarray(dx, dtype=np.float32)
    dy = np.asarray(dy, dtype=np.float32)
    k = orc.gaussian1d_f32(-1, radius)
    out = []
    for p in (dx * dx, dx * dy, dy * dy):
        h = orc.conv("norm_h", k, radius, orc.Gray.from_array(p))
        out.append(orc.conv("norm_v", k, radius, h).array().copy())
    return score_f32(kind, *out, kappa=kappa)
