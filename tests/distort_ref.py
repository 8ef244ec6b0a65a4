"""NumPy reference of the image remap (ImageDistort on single-band GrayU8 / GrayF32), written from the Java line by line.  All arithmetic is
in np.float32 scalars, one operation at a time, in the order the Java has it.

    I: = main/boofcv-ip/src/main/java/boofcv/

  java_f2i()        Java's (int) of a float
  border_get()      ImageBorder_S32.get / ImageBorder_F32.get over ImageBorderValue (value 0) or BorderIndex1D_Extend   I:core/image/border/
  bilinear_get()    ImplBilinearPixel_U8 / _F32 get, get_fast, get_border            I:alg/interpolate/impl/ImplBilinearPixel_U8.java:48-90
  nearest_get()     NearestNeighborPixel_U8 / _F32 get, get_border                   I:alg/interpolate/impl/NearestNeighborPixel_U8.java:56-72
  assign()          AssignPixelValue_SB.F32 / .I8                                    I:alg/distort/AssignPixelValue_SB.java:31-59
  distort()         ImageDistortCache_SB.renderAll / applyOnlyInside, with and without a mask   I:alg/distort/ImageDistortCache_SB.java:136-206
                    (= ImageDistortBasic_SB.applyAll / applyOnlyInside, :56-135, with the transform that filled the map); the map is indexed
                    by y*dw + x (include/boofhip.h, deviation 1)
  make_map()        the affine and homography formulas of include/boofhip.h at every destination pixel
  fill_uniform()    the images of tests/test_gpu_distort.py (not from the reference)
"""
import numpy as np

INT_MAX = 2147483647
NEAREST_NEIGHBOR, BILINEAR = 0, 1                 # BHIP_INTERP_*
EXTENDED, ZERO = 1, 5                             # BHIP_BORDER_*
AFFINE, HOMOGRAPHY = 1, 2                         # BHIP_DISTORT_*
F = np.float32
ONE = F(1.0)


def java_f2i(v):
    """Java's (int) of a float: toward zero, saturating, NaN -> 0"""
    v = float(v)
    if v != v:
        return 0
    if v >= INT_MAX:
        return INT_MAX
    if v <= -INT_MAX - 1:
        return -INT_MAX - 1
    return int(v)


def border_get(img, x, y, border):
    """border.get(x, y): the pixel when in bounds, else 0 (ZERO) or the pixel at the clamped coordinates (EXTENDED); as a float"""
    h, w = img.shape
    if 0 <= x < w and 0 <= y < h:
        return F(img[y, x])
    if border == ZERO:
        return F(0)
    assert border == EXTENDED
    x = 0 if x < 0 else w - 1 if x >= w else x       # BorderIndex1D_Extend.getIndex
    y = 0 if y < 0 else h - 1 if y >= h else y
    return F(img[y, x])


def bilinear_get(img, x, y, border):
    h, w = img.shape
    x, y = F(x), F(y)
    if x < 0 or y < 0 or x > F(w - 2) or y > F(h - 2):
        xf, yf = F(np.floor(x)), F(np.floor(y))                      # get_border
        xt, yt = java_f2i(xf), java_f2i(yf)
        ax, ay = x - xf, y - yf
        p00, p10, p11, p01 = (border_get(img, xt, yt, border), border_get(img, xt + 1, yt, border), border_get(img, xt + 1, yt + 1, border),
                              border_get(img, xt, yt + 1, border))
    else:
        xt, yt = java_f2i(x), java_f2i(y)                            # get_fast
        ax, ay = x - F(xt), y - F(yt)
        p00, p10, p11, p01 = F(img[yt, xt]), F(img[yt, xt + 1]), F(img[yt + 1, xt + 1]), F(img[yt + 1, xt])
    val = (ONE - ax) * (ONE - ay) * p00
    val = val + ax * (ONE - ay) * p10
    val = val + ax * ay * p11
    val = val + (ONE - ax) * ay * p01
    return F(val)


def nearest_get(img, x, y, border):
    h, w = img.shape
    x, y = F(x), F(y)
    if x < 0 or y < 0 or x > F(w - 1) or y > F(h - 1):
        return border_get(img, java_f2i(np.floor(x)), java_f2i(np.floor(y)), border)
    return F(img[java_f2i(y), java_f2i(x)])


def assign(value, dtype):
    """GrayF32: the float.  GrayU8: (byte)value -- float -> int, then the low eight bits"""
    if np.dtype(dtype) == np.float32:
        return F(value)
    return np.uint8(java_f2i(value) & 0xFF)


def inside(x, y, w, h):
    """the test of applyOnlyInside and of the mask"""
    x, y = F(x), F(y)
    return bool(x >= 0 and x <= F(w - 1) and y >= 0 and y <= F(h - 1))


def distort(src, map_xy, interp, border, renderAll, dst, crop=None):
    """-> (dst after the call, mask, number of pixels assigned).  src [sh,sw] uint8 / float32; map_xy [dh,dw,2] float32; dst [dh,dw] of src's type,
    what the destination held before (it is not modified); crop (x0, y0, x1, y1), None = the whole destination.  mask is 1 / 0 inside the crop and
    255 where the call writes no mask."""
    src = np.asarray(src)
    out = np.array(dst, copy=True)
    assert out.dtype == src.dtype and map_xy.shape == out.shape + (2,) and map_xy.dtype == np.float32
    sh, sw = src.shape
    dh, dw = out.shape
    x0, y0, x1, y1 = (0, 0, dw, dh) if crop is None else crop
    get = bilinear_get if interp == BILINEAR else nearest_get
    mask = np.full((dh, dw), 255, np.uint8)
    assigned = 0
    with np.errstate(all="ignore"):
        for y in range(y0, y1):
            for x in range(x0, x1):
                sx, sy = map_xy[y, x]
                ins = inside(sx, sy, sw, sh)
                mask[y, x] = 1 if ins else 0
                if renderAll or ins:
                    out[y, x] = assign(get(src, sx, sy, border), out.dtype)
                    assigned += 1
    return out, mask, assigned


def make_map(model, coeff, dw, dh):
    """[dh,dw,2] float32: (sx, sy) of the model at every destination pixel, every sum left to right, x and y converted from int to float first"""
    c = [F(v) for v in np.asarray(coeff, np.float32).reshape(-1)]
    m = np.empty((dh, dw, 2), np.float32)
    with np.errstate(all="ignore"):
        for yi in range(dh):
            for xi in range(dw):
                x, y = F(xi), F(yi)
                if model == AFFINE:
                    a11, a12, a21, a22, tx, ty = c
                    sx = tx + a11 * x + a12 * y
                    sy = ty + a21 * x + a22 * y
                else:
                    assert model == HOMOGRAPHY
                    z = c[6] * x + c[7] * y + c[8]
                    sx = (c[0] * x + c[1] * y + c[2]) / z
                    sy = (c[3] * x + c[4] * y + c[5]) / z
                m[yi, xi, 0], m[yi, xi, 1] = sx, sy
    return m


def fill_uniform(w, h, dtype, seed):
    """[h,w] of uniformly random finite pixels: uint8 0..255, float32 -100..400 (fractions included)"""
    rng = np.random.RandomState(seed)
    if np.dtype(dtype) == np.uint8:
        return rng.randint(0, 256, (h, w)).astype(np.uint8)
    return (rng.rand(h, w) * 500 - 100).astype(np.float32)


def rotation_map(dw, dh, sw, sh, degrees):
    """a rotation about the centres: a map with coordinates on both sides of every border"""
    a = np.deg2rad(degrees)
    ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float64)
    cx, cy = (dw - 1) / 2.0, (dh - 1) / 2.0
    sx = np.cos(a) * (xs - cx) - np.sin(a) * (ys - cy) + (sw - 1) / 2.0
    sy = np.sin(a) * (xs - cx) + np.cos(a) * (ys - cy) + (sh - 1) / 2.0
    return np.ascontiguousarray(np.stack([sx, sy], -1).astype(np.float32))
