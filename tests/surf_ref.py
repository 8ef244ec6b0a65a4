"""NumPy fp64 reference of the SURF descriptor on any sample grid, written from the Java.

    F: = main/boofcv-feature/src/main/java/boofcv/     I: = main/boofcv-ip/src/main/java/boofcv/     T: = main/boofcv-types/src/main/java/boofcv/

  gaussian_width()      FactoryKernelGaussian.gaussianWidth              I:factory/filter/kernel/FactoryKernelGaussian.java:418-448
                        (odd widths: gaussian2D_F64 :297-306 = outer product of the 1-D PDF, KernelMath.normalizeSumToOne)
  grad_radius()         SparseIntegralGradient_NoBorder.setWidth         I:alg/transform/ii/SparseIntegralGradient_NoBorder.java:42-47
  gradient_noborder()   SparseIntegralGradient_NoBorder_F32.compute      I:alg/transform/ii/impl/SparseIntegralGradient_NoBorder_F32.java:46-76
  gradient_in_bounds()  SparseScaleGradient.isInBounds                   T:struct/sparse/SparseScaleGradient.java:48-50 (x0 = y0 = -r-1, x1 = y1 = r, _F32.java:38-44)
  gradient_checked()    SparseGradientSafe.compute                       T:struct/sparse/SparseGradientSafe.java:56-61
  gradient_naive()      the same kernel as two box differences of the *pixels* (DerivativeIntegralImage.kernelDerivX / Y): what the twelve taps mean
  features_fast()       DescribePointSurf.features                       F:alg/feature/describe/DescribePointSurf.java:235-295 (weights :122-129)
  features_mod()        DescribePointSurfMod.features                    F:alg/feature/describe/DescribePointSurfMod.java:121-192 (weights :81-90)
  describe()            DescribePointSurf.describe                       F:alg/feature/describe/DescribePointSurf.java:169-213 + UtilFeature.normalizeL2
                        F:alg/descriptor/UtilFeature.java:101-114

The integral image is a (H, W) float32 array.  Gradients are formed in float32 in the reference's order of operations; every sum is a
Python float (fp64) accumulated in the reference's order.  describe() takes the bounds-checked gradient exactly when a sample's box
leaves the image; where every box is inside, the two forms are the same function, so the reference's conservative isInside test
(SurfDescribeOps.java:120-159) selects between two equal results and is not restated here.
"""
import math

import numpy as np

F32 = np.float32


def _pdf(sigma, d):
    """org.ddogleg.stats.UtilGaussian.computePDF(0, sigma, d) (published formula)"""
    return math.exp(-d * d / (2.0 * sigma * sigma)) / (sigma * math.sqrt(2.0 * math.pi))


def gaussian_width(sigma, width):
    """-> (width, width) float64, sum 1"""
    if sigma <= 0:
        sigma = ((width // 2) * 2.0 + 1.0) / 5.0          # sigmaForRadius(width/2, 0) :388
    elif width <= 0:
        raise ValueError("Must specify the width since it doesn't know if it should be even or odd")
    k = np.zeros((width, width))
    if width % 2 == 0:
        r = width // 2 - 1
        for y in range(width):
            dy = (abs(y - r) if y <= r else abs(y - r - 1)) + 0.5
            for x in range(width):
                dx = (abs(x - r) if x <= r else abs(x - r - 1)) + 0.5
                k[y, x] = _pdf(sigma, math.sqrt(dx * dx + dy * dy))
    else:
        radius = width // 2
        k1 = [_pdf(sigma, float(i)) for i in range(radius, -radius - 1, -1)]
        for y in range(width):
            for x in range(width):
                k[y, x] = k1[y] * k1[x]
    total = 0.0
    for v in k.reshape(-1):
        total += float(v)
    return k / total


def grad_radius(kernel_width):
    r = int(kernel_width + 0.5) // 2
    return r if r > 0 else 1


def gradient_in_bounds(shape, r, x, y):
    h, w = shape
    return x - r - 1 >= 0 and y - r - 1 >= 0 and x + r < w and y + r < h


def gradient_noborder(ii, r, x, y):
    """(gx, gy) as float32; every tap must be inside the image"""
    w = 2 * r + 1
    x0, y1 = x - r - 1, y - r - 1
    y2, y3 = y1 + r, y1 + r + 1
    y4 = y3 + r
    if x0 < 0 or y1 < 0 or x0 + w >= ii.shape[1] or y4 >= ii.shape[0]:
        raise IndexError("gradient box leaves the image")
    p0, p1, p2, p3 = ii[y1, x0], ii[y1, x0 + r], ii[y1, x0 + r + 1], ii[y1, x0 + w]
    p11, p4 = ii[y2, x0], ii[y2, x0 + w]
    p10, p5 = ii[y3, x0], ii[y3, x0 + w]
    p9, p8, p7, p6 = ii[y4, x0], ii[y4, x0 + r], ii[y4, x0 + r + 1], ii[y4, x0 + w]
    left = F32(F32(F32(p8 - p9) - p1) + p0)
    right = F32(F32(F32(p6 - p7) - p3) + p2)
    top = F32(F32(F32(p4 - p11) - p3) + p0)
    bottom = F32(F32(F32(p6 - p9) - p5) + p10)
    return F32(right - left), F32(bottom - top)


def gradient_checked(ii, r, x, y):
    if gradient_in_bounds(ii.shape, r, x, y):
        return gradient_noborder(ii, r, x, y)
    return F32(0), F32(0)


def gradient_naive(img, r, x, y):
    """The kernel on the pixels themselves, in fp64: derivX = (columns x+1..x+r) - (columns x-r..x-1) over rows y-r..y+r, derivY likewise
    (I:alg/transform/ii/DerivativeIntegralImage.java kernelDerivX / kernelDerivY: blocks (-r-1,-r-1,-1,r) = -1 and (0,-r-1,r,r) = +1,
    lower-exclusive, upper-inclusive)."""
    a = np.asarray(img, dtype=np.float64)
    gx = a[y - r:y + r + 1, x + 1:x + r + 1].sum() - a[y - r:y + r + 1, x - r:x].sum()
    gy = a[y + 1:y + r + 1, x - r:x + r + 1].sum() - a[y - r:y, x - r:x + r + 1].sum()
    return gx, gy


def _j2i(v):
    """Java's (int) of a finite double of moderate size: toward zero"""
    return int(v)


def features_fast(ii, c_x, c_y, c, s, scale, grad, widthLargeGrid, widthSubRegion, widthSample, weightSigma):
    """DescribePointSurf.features; grad(ii, r, x, y) is gradient_noborder or gradient_checked"""
    regionSize = widthLargeGrid * widthSubRegion
    radius = regionSize // 2
    weight = gaussian_width(weightSigma, radius * 2)
    if weight.shape[0] != regionSize:
        raise ValueError("Weighting kernel has an unexpected size")     # :241-243
    weight = weight / weight[radius, radius]
    r = grad_radius(widthSample * scale)
    regionR = regionSize // 2
    regionEnd = regionSize - regionR
    c_x += 0.5
    c_y += 0.5
    out = []
    for rY in range(-regionR, regionEnd, widthSubRegion):
        for rX in range(-regionR, regionEnd, widthSubRegion):
            sum_dx = sum_dy = sum_adx = sum_ady = 0.0
            for i in range(widthSubRegion):
                regionY = (rY + i) * scale
                for j in range(widthSubRegion):
                    w = float(weight[regionR + rY + i, regionR + rX + j])    # Kernel2D.get(x, y) = data[y*width + x]
                    regionX = (rX + j) * scale
                    pixelX = _j2i(c_x + c * regionX - s * regionY)
                    pixelY = _j2i(c_y + s * regionX + c * regionY)
                    gx, gy = grad(ii, r, pixelX, pixelY)
                    dx = w * float(gx)
                    dy = w * float(gy)
                    pdx = c * dx + s * dy
                    pdy = -s * dx + c * dy
                    sum_dx += pdx
                    sum_adx += abs(pdx)
                    sum_dy += pdy
                    sum_ady += abs(pdy)
            out += [sum_dx, sum_adx, sum_dy, sum_ady]
    return np.array(out)


def features_mod(ii, c_x, c_y, c, s, scale, grad, widthLargeGrid, widthSubRegion, widthSample, overLap, sigmaLargeGrid, sigmaSubRegion):
    """DescribePointSurfMod.features"""
    weightGrid = gaussian_width(sigmaLargeGrid, widthLargeGrid)
    weightSub = gaussian_width(sigmaSubRegion, widthSubRegion + 2 * overLap)
    weightGrid = weightGrid / weightGrid[widthLargeGrid // 2, widthLargeGrid // 2]
    tw = widthSubRegion + 2 * overLap
    weightSub = weightSub / weightSub[tw // 2, tw // 2]
    r = grad_radius(widthSample * scale)
    regionSize = widthLargeGrid * widthSubRegion
    regionR = regionSize // 2
    regionEnd = regionSize - regionR
    gridW = regionSize + 2 * overLap
    c_x += 0.5
    c_y += 0.5
    sX = np.zeros((gridW, gridW))
    sY = np.zeros((gridW, gridW))
    for iy, rY in enumerate(range(-regionR - overLap, regionEnd + overLap)):
        regionY = rY * scale
        for ix, rX in enumerate(range(-regionR - overLap, regionEnd + overLap)):
            regionX = rX * scale
            pixelX = _j2i(c_x + c * regionX - s * regionY)
            pixelY = _j2i(c_y + s * regionX + c * regionY)
            gx, gy = grad(ii, r, pixelX, pixelY)
            sX[iy, ix] = float(gx)
            sY[iy, ix] = float(gy)
    out = []
    gridWeights = weightGrid.reshape(-1)
    k = 0
    for rY in range(-regionR, regionEnd, widthSubRegion):
        for rX in range(-regionR, regionEnd, widthSubRegion):
            sum_dx = sum_dy = sum_adx = sum_ady = 0.0
            for i in range(tw):
                for j in range(tw):
                    w = float(weightSub[i, j])
                    dx = w * float(sX[rY + regionR + i, rX + regionR + j])
                    dy = w * float(sY[rY + regionR + i, rX + regionR + j])
                    pdx = c * dx + s * dy
                    pdy = -s * dx + c * dy
                    sum_dx += pdx
                    sum_adx += abs(pdx)
                    sum_dy += pdy
                    sum_ady += abs(pdy)
            w = float(gridWeights[k])
            k += 1
            out += [w * sum_dx, w * sum_adx, w * sum_dy, w * sum_ady]
    return np.array(out)


def normalize_l2(v):
    norm = 0.0
    for x in v:
        norm += float(x) * float(x)
    if norm == 0:
        return v
    return v / math.sqrt(norm)


def sample_boxes_inside(shape, x, y, c, s, scale, radius, widthSample):
    """Does every sample of the (2*radius or 2*radius+1)-wide grid keep its gradient box inside the image?"""
    r = grad_radius(widthSample * scale)
    for rY in range(-radius, radius + 1):
        for rX in range(-radius, radius + 1):
            px = _j2i(x + 0.5 + c * (rX * scale) - s * (rY * scale))
            py = _j2i(y + 0.5 + s * (rX * scale) + c * (rY * scale))
            if not gradient_in_bounds(shape, r, px, py):
                return False
    return True


def describe(ii, x, y, angle, scale, stable, widthLargeGrid=4, widthSubRegion=5, widthSample=3, weightSigma=4.5, overLap=2,
             sigmaLargeGrid=2.5, sigmaSubRegion=2.5, normalize=True):
    """DescribePointSurf(Mod).describe without the Laplacian sign -> float64[widthLargeGrid^2 * 4]"""
    ii = np.asarray(ii)
    assert ii.dtype == np.float32 and ii.ndim == 2
    c, s = math.cos(angle), math.sin(angle)
    radius = (widthLargeGrid * widthSubRegion) // 2 + (overLap if stable else 0)
    grad = gradient_noborder if sample_boxes_inside(ii.shape, x, y, c, s, scale, radius, widthSample) else gradient_checked
    if stable:
        f = features_mod(ii, x, y, c, s, scale, grad, widthLargeGrid, widthSubRegion, widthSample, overLap, sigmaLargeGrid, sigmaSubRegion)
    else:
        f = features_fast(ii, x, y, c, s, scale, grad, widthLargeGrid, widthSubRegion, widthSample, weightSigma)
    return normalize_l2(f) if normalize else f
