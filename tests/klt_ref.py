"""numpy float32 restatement of the reference's pyramid KLT tracker (test reference, not product code; never imported by boofcv_amd/).

Written from the cited BoofCV sources (F: = main/boofcv-feature/src/main/java/boofcv/, I: = main/boofcv-ip/..., G: = main/boofcv-geo/...):
  GradientSobel.process(GrayF32, ..., BorderType.EXTENDED)      I:alg/filter/derivative/GradientSobel.java:158-173,
                                                                I:alg/filter/convolve/border/ConvolveJustBorder_General_SB.java:110-174
  BilinearRectangle_F32.region + handleBorder                   I:alg/interpolate/impl/BilinearRectangle_F32.java:64-172
  KltTracker                                                    F:alg/tracker/klt/KltTracker.java:147-495
  PyramidKltTracker                                             F:alg/tracker/klt/PyramidKltTracker.java:58-151
  PointTrackerKltPyramid (list logic)                           G:abst/feature/tracker/PointTrackerKltPyramid.java:139-348
  GeneralFeatureDetector (exclusion list)                       F:alg/feature/detect/interest/GeneralFeatureDetector.java:108-160

Every value is np.float32 and every operation is the Java expression in the Java order.  Sums the reference forms in a loop are one fp32 chain in
the same element order (chain(): np.add.accumulate is sequential; test_klt_reference.py checks that against a Python loop).  Patches are
interpolated element-wise with array expressions, which is the same arithmetic per element.  The pyramid, the interior of the Sobel gradient, the
corner intensity, the non-max suppression and select-N-best come from the oracle.
"""
import math

import numpy as np

F = np.float32
NAN = F(np.nan)
SUCCESS, DRIFTED, OUT_OF_BOUNDS, FAILED, LARGE_ERROR = range(5)
FAULT_NAMES = ("SUCCESS", "DRIFTED", "OUT_OF_BOUNDS", "FAILED", "LARGE_ERROR")
FLOAT_MAX = F(np.finfo(np.float32).max)


class Thrown(ValueError):
    """IllegalArgumentException("Region is outside of the image") of computeSubImageBounds / region"""


def chain(values):
    """total = 0; for v in values: total += v   (fp32, in order)"""
    a = np.zeros(len(values) + 1, np.float32)
    a[1:] = values
    return np.add.accumulate(a)[-1]


# ---------------------------------------------------------------------------------------------------------------- gradient
KX = np.array([-0.25, 0, 0.25, -0.5, 0, 0.5, -0.25, 0, 0.25], np.float32)   # GradientSobel.kernelDerivX_F32
KY = np.array([-0.25, -0.5, -0.25, 0, 0, 0, 0.25, 0.5, 0.25], np.float32)   # GradientSobel.kernelDerivY_F32


def sobel_border(img, mode):
    """every pixel as the border code computes it: total = 0; total += get(x+j, y+i) * k[..] over the nine taps in kernel order, on the image
    extended by `mode` ('edge' = BorderIndex1D_Extend, 'constant' = ImageBorderValue(0))"""
    img = np.asarray(img, np.float32)
    H, W = img.shape
    p = np.pad(img, 1, mode=mode)
    tx = np.zeros((H, W), np.float32)
    ty = np.zeros((H, W), np.float32)
    for i in range(3):
        for j in range(3):
            v = p[i:i + H, j:j + W]
            tx = tx + v * KX[i * 3 + j]
            ty = ty + v * KY[i * 3 + j]
    return tx, ty


def sobel_extended(orc, img):
    """GradientSobel.process(img, derivX, derivY, BorderType.EXTENDED) -> (derivX, derivY): the oracle's interior, the frame from sobel_border"""
    img = np.ascontiguousarray(img, np.float32)
    H, W = img.shape
    gx, gy = orc.gradient("sobel", orc.Gray.from_array(img), False)
    dx, dy = gx.array().copy(), gy.array().copy()
    bx, by = sobel_border(img, "edge")
    frame = np.ones((H, W), bool)
    if H > 2 and W > 2:
        frame[1:-1, 1:-1] = False
    dx[frame] = bx[frame]
    dy[frame] = by[frame]
    return dx, dy


def pyramid_gradient(orc, frame, scales):
    """what PointTrackerKltPyramid.process computes before tracking: FactoryPyramid.discreteGaussian(scales, -1, 2) and the EXTENDED Sobel of every layer"""
    layers, _ = orc.pyramid(orc.gaussian1d_f32(-1, 2), -1, scales, orc.Gray.from_array(frame))
    grads = [sobel_extended(orc, l) for l in layers]
    return layers, [g[0] for g in grads], [g[1] for g in grads]


# ---------------------------------------------------------------------------------------------------------------- bilinear patch
def region(img, tl_x, tl_y, w, h):
    """BilinearRectangle_F32.region(tl_x, tl_y, output of w x h) -> (h, w) float32"""
    tl_x, tl_y = F(tl_x), F(tl_y)
    H, W = img.shape
    if tl_x < 0 or tl_y < 0 or tl_x + F(w) > F(W) or tl_y + F(h) > F(H):
        raise Thrown("Region is outside of the image")
    xt = int(tl_x) if tl_x == tl_x else 0   # (int)NaN is 0 in Java
    yt = int(tl_y) if tl_y == tl_y else 0
    ax, ay = tl_x - F(xt), tl_y - F(yt)
    bx, by = F(1.0) - ax, F(1.0) - ay
    a0, a1, a2, a3 = bx * by, ax * by, ax * ay, bx * ay
    regW, regH = w, h
    borderRight = borderBottom = False
    if xt + regW >= W or yt + regH >= H:
        if xt + regW > W or yt + regH > H:
            raise Thrown("requested region is out of bounds")
        if xt + regW == W:
            regW -= 1
            borderRight = True
        if yt + regH == H:
            regH -= 1
            borderBottom = True
    out = np.zeros((h, w), np.float32)
    if regW > 0 and regH > 0:
        XY = img[yt:yt + regH, xt:xt + regW]
        xY = img[yt:yt + regH, xt + 1:xt + regW + 1]
        Xy = img[yt + 1:yt + regH + 1, xt:xt + regW]
        xy = img[yt + 1:yt + regH + 1, xt + 1:xt + regW + 1]
        out[:regH, :regW] = a0 * XY + a1 * xY + a2 * xy + a3 * Xy
    # handleBorder :128-172, as written
    if borderRight:
        for y in range(regH):
            out[y, regW] = by * img[yt + y, xt + regW] + ay * img[yt + y + 1, xt + regW]
        if borderBottom:
            out[regH, regW] = img[yt + regH, xt + regW]
        else:
            out[regH - 1, regW] = by * img[yt + regH - 1, xt + regW] + ay * img[yt + regH, xt + regW]
    if borderBottom:
        for x in range(regW):
            out[regH, x] = bx * img[yt + regH, xt + x] + ax * img[yt + regH, xt + x + 1]
        if not borderRight:
            XY = img[yt + regH, xt + regW - 1]
            Xy = img[regH, xt + regW]          # orig.get(xt+regWidth, regHeight): the row is regHeight, not yt+regHeight
            out[regH, regW - 1] = by * XY + ay * Xy
    return out


def bilinear_pixel(img, x, y):
    """BilinearPixel_F32.get_fast (I:alg/interpolate/impl/ImplBilinearPixel_F32.java): the per-pixel form the reference's
    GeneralBilinearRectangleChecks compares region() with"""
    x, y = F(x), F(y)
    xt, yt = int(x), int(y)
    ax, ay = x - F(xt), y - F(yt)
    v = (F(1.0) - ax) * (F(1.0) - ay) * img[yt, xt]
    v += ax * (F(1.0) - ay) * img[yt, xt + 1]
    v += ax * ay * img[yt + 1, xt + 1]
    v += (F(1.0) - ax) * ay * img[yt + 1, xt]
    return v


# ---------------------------------------------------------------------------------------------------------------- KltTracker
class KltConfig:
    def __init__(self, maxPerPixelError=25.0, maxIterations=15, minDeterminant=0.001, minPositionDelta=0.01):
        self.forbiddenBorder = 0
        self.maxPerPixelError = F(maxPerPixelError)
        self.maxIterations = int(maxIterations)
        self.minDeterminant = F(minDeterminant)
        self.minPositionDelta = F(minPositionDelta)


class KltFeature:
    def __init__(self, radius):
        self.radius = int(radius)
        w = 2 * self.radius + 1
        self.x = self.y = F(0)
        self.desc = np.zeros((w, w), np.float32)
        self.derivX = np.zeros((w, w), np.float32)
        self.derivY = np.zeros((w, w), np.float32)
        self.Gxx = self.Gyy = self.Gxy = F(0)

    def setPosition(self, x, y):
        self.x, self.y = F(x), F(y)


class KltTracker:
    def __init__(self, config=None):
        self.config = config or KltConfig()
        self.image = self.derivX = self.derivY = None
        self.currDesc = None
        self.error = F(0)
        self.iterations = 0          # LK iterations run so far
        self.borderIterations = 0    # ... of which took computeGandE_border

    def setImage(self, image, derivX=None, derivY=None):
        self.image, self.derivX, self.derivY = image, derivX, derivY

    def _bounds(self, f):   # setAllowedBounds :330-344
        r = f.radius
        H, W = self.image.shape
        self.widthFeature = 2 * r + 1
        self.lengthFeature = self.widthFeature * self.widthFeature
        self.allowedLeft, self.allowedTop = F(r), F(r)
        self.allowedRight, self.allowedBottom = F(W - r - 1), F(H - r - 1)
        self.outsideLeft, self.outsideTop = F(-r), F(-r)
        self.outsideRight, self.outsideBottom = F(W + r - 1), F(H + r - 1)

    def isFullyInside(self, x, y):
        if x < self.allowedLeft or x > self.allowedRight:
            return False
        if y < self.allowedTop or y > self.allowedBottom:
            return False
        return True

    def isFullyOutside(self, x, y):
        if x < self.outsideLeft or x > self.outsideRight:
            return True
        if y < self.outsideTop or y > self.outsideBottom:
            return True
        return False

    def setDescription(self, f):   # :147-158
        self._bounds(f)
        if not self.isFullyInside(f.x, f.y):
            if self.isFullyOutside(f.x, f.y):
                return False
            return self._setDescriptionBorder(f)
        return self._setDescriptionInside(f)

    def _setDescriptionInside(self, f):   # :160-191
        w = self.widthFeature
        tl_x, tl_y = f.x - F(f.radius), f.y - F(f.radius)
        f.desc = region(self.image, tl_x, tl_y, w, w)
        f.derivX = region(self.derivX, tl_x, tl_y, w, w)
        f.derivY = region(self.derivY, tl_x, tl_y, w, w)
        dX, dY = f.derivX.reshape(-1), f.derivY.reshape(-1)
        f.Gxx, f.Gyy, f.Gxy = chain(dX * dX), chain(dY * dY), chain(dX * dY)
        det = f.Gxx * f.Gyy - f.Gxy * f.Gxy
        return bool(det >= self.config.minDeterminant * F(self.lengthFeature))

    def _subBounds(self, f, cx, cy):   # computeSubImageBounds :421-457
        H, W = self.image.shape
        w = self.widthFeature
        dstX0, dstY0, dstX1, dstY1 = 0, 0, w, w
        srcX0, srcY0 = cx - F(f.radius), cy - F(f.radius)
        srxX1, srxY1 = srcX0 + F(w), srcY0 + F(w)
        if srcX0 < 0:
            dstX0 = int(-math.floor(float(srcX0)))
            srcX0 = srcX0 + F(dstX0)
        if srxX1 > F(W):
            dstX1 -= int(math.ceil(float(srxX1 - F(W))))
            dstX1 -= 1 if srcX0 + F(dstX1 - dstX0) > F(W) else 0
        if srcY0 < 0:
            dstY0 = int(-math.floor(float(srcY0)))
            srcY0 = srcY0 + F(dstY0)
        if srxY1 > F(H):
            dstY1 -= int(math.ceil(float(srxY1 - F(H))))
            dstY1 -= 1 if srcY0 + F(dstY1 - dstY0) > F(H) else 0
        if srcX0 < 0 or srcY0 < 0 or srcX0 + F(dstX1 - dstX0) > F(W) or srcY0 + F(dstY1 - dstY0) > F(H):
            raise Thrown("Region is outside of the image")
        return dstX0, dstY0, dstX1, dstY1, srcX0, srcY0

    def _setDescriptionBorder(self, f):   # :198-240
        w = self.widthFeature
        x0, y0, x1, y1, sx, sy = self._subBounds(f, f.x, f.y)
        f.desc = np.full((w, w), NAN, np.float32)
        f.desc[y0:y1, x0:x1] = region(self.image, sx, sy, x1 - x0, y1 - y0)
        f.derivX = f.derivX.copy()
        f.derivY = f.derivY.copy()
        f.derivX[y0:y1, x0:x1] = region(self.derivX, sx, sy, x1 - x0, y1 - y0)
        f.derivY[y0:y1, x0:x1] = region(self.derivY, sx, sy, x1 - x0, y1 - y0)
        ok = ~np.isnan(f.desc.reshape(-1))
        dX, dY = f.derivX.reshape(-1)[ok], f.derivY.reshape(-1)[ok]
        f.Gxx, f.Gyy, f.Gxy = chain(dX * dX), chain(dY * dY), chain(dX * dY)
        det = f.Gxx * f.Gyy - f.Gxy * f.Gxy
        return bool(det >= self.config.minDeterminant * F(int(ok.sum())))

    def track(self, f):   # :251-325
        with np.errstate(all="ignore"):
            return self._track(f)

    def _track(self, f):
        cfg = self.config
        self._bounds(f)
        w, n = self.widthFeature, self.lengthFeature
        if self.isFullyOutside(f.x, f.y):
            return OUT_OF_BOUNDS
        origX, origY = f.x, f.y
        tD, tX, tY = f.desc.reshape(-1), f.derivX.reshape(-1), f.derivY.reshape(-1)
        complete = not np.isnan(tD).any()
        det = F(0)
        Gxx = Gyy = Gxy = F(0)
        if complete:
            Gxx, Gyy, Gxy = f.Gxx, f.Gyy, f.Gxy
            det = Gxx * Gyy - Gxy * Gxy
            if det < cfg.minDeterminant * F(n):
                return FAILED
        for _ in range(cfg.maxIterations):
            self.iterations += 1
            if complete and self.isFullyInside(f.x, f.y):   # computeE :361-374
                self.currDesc = region(self.image, f.x - F(f.radius), f.y - F(f.radius), w, w)
                d = tD - self.currDesc.reshape(-1)
                Ex, Ey = chain(d * tX), chain(d * tY)
            else:                                           # computeGandE_border :379-419
                self.borderIterations += 1
                x0, y0, x1, y1, sx, sy = self._subBounds(f, f.x, f.y)
                self.currDesc = np.full((w, w), NAN, np.float32)
                self.currDesc[y0:y1, x0:x1] = region(self.image, sx, sy, x1 - x0, y1 - y0)
                cur = self.currDesc.reshape(-1)
                ok = ~(np.isnan(tD) | np.isnan(cur))
                d = tD[ok] - cur[ok]
                dX, dY = tX[ok], tY[ok]
                Ex, Ey = chain(d * dX), chain(d * dY)
                Gxx, Gyy, Gxy = chain(dX * dX), chain(dY * dY), chain(dX * dY)
                det = Gxx * Gyy - Gxy * Gxy
                if det <= cfg.minDeterminant * F(int(ok.sum())):
                    return FAILED
            dx = (Gyy * Ex - Gxy * Ey) / det
            dy = (Gxx * Ey - Gxy * Ex) / det
            f.x = f.x + dx
            f.y = f.y + dy
            if self.isFullyOutside(f.x, f.y):
                return OUT_OF_BOUNDS
            if abs(f.x - origX) > F(w) or abs(f.y - origY) > F(w):
                return DRIFTED
            if abs(dx) < cfg.minPositionDelta and abs(dy) < cfg.minPositionDelta:
                break
        # computeError :346-359
        cur = self.currDesc.reshape(-1)
        ok = ~(np.isnan(tD) | np.isnan(cur))
        self.error = chain(np.abs(tD[ok] - cur[ok])) / F(int(ok.sum()))
        if self.error > cfg.maxPerPixelError:
            return LARGE_ERROR
        return SUCCESS


# ---------------------------------------------------------------------------------------------------------------- PyramidKltTracker
class PyramidKltFeature:
    def __init__(self, numLayers, radius):
        self.radius = radius
        self.desc = [KltFeature(radius) for _ in range(numLayers)]
        self.x = self.y = F(0)
        self.featureId = 0
        self.px = self.py = F(0)   # the PointTrack's position (updated only when the track survives a frame)
        self.fault = SUCCESS       # result of the last track()
        self.error = F(0)

    def setPosition(self, x, y):
        self.x, self.y = F(x), F(y)


class PyramidKltTracker:
    def __init__(self, tracker, scales):
        self.tracker = tracker
        self.scales = [int(s) for s in scales]
        self.layers = self.derivX = self.derivY = None

    def setImage(self, layers, derivX=None, derivY=None):
        self.layers, self.derivX, self.derivY = layers, derivX, derivY

    def setDescription(self, feature):   # :58-71
        for layer in range(len(self.layers)):
            scale = F(float(self.scales[layer]))
            x, y = feature.x / scale, feature.y / scale
            self.tracker.setImage(self.layers[layer], self.derivX[layer], self.derivY[layer])
            feature.desc[layer].setPosition(x, y)
            if not self.tracker.setDescription(feature.desc[layer]):
                return False
        return True

    def track(self, feature):   # :113-151
        x, y = feature.x, feature.y
        for layer in range(len(self.layers) - 1, -1, -1):
            scale = F(float(self.scales[layer]))
            x, y = x / scale, y / scale
            self.tracker.setImage(self.layers[layer])
            f = feature.desc[layer]
            f.setPosition(x, y)
            ret = self.tracker.track(f)
            if ret != SUCCESS:
                return ret
            x, y = f.x * scale, f.y * scale
        feature.setPosition(x, y)
        return SUCCESS

    def getError(self):
        return self.tracker.error


# ---------------------------------------------------------------------------------------------------------------- detector + track manager
def detect(orc, derivX0, derivY0, exclude, radius, threshold, border, maxFeatures=-1):
    """GeneralFeatureDetector.process with Shi-Tomasi radius 1 (unweighted) and the strict non-max extractor; exclude = [(x, y)] or None"""
    inten = orc.corner_intensity(orc.Gray.from_array(derivX0), orc.Gray.from_array(derivY0), 1, "shitomasi")
    numSelectMax = -1
    if maxFeatures > 0:
        numSelectMax = maxFeatures if exclude is None else maxFeatures - len(exclude)
        if numSelectMax <= 0:
            return np.zeros((0, 2), np.int16)
    for x, y in (exclude or []):
        inten[y, x] = FLOAT_MAX
    g = orc.Gray.from_array(inten)
    found = orc.nonmax(g, radius, threshold, border)
    if numSelectMax > 0:
        found = orc.select_nbest(g, found, numSelectMax, True)
    return found


class PointTrackerKltPyramid:
    """process / spawnTracks / addTrack / dropTrack / dropAllTracks / reset of the reference, for one sequence"""

    def __init__(self, orc, scales, templateRadius, config=None, detectRadius=1, detectThreshold=0.0, detectBorder=0, maxFeatures=-1):
        self.orc = orc
        self.scales = [int(s) for s in scales]
        self.templateRadius = templateRadius
        self.klt = KltTracker(config)
        self.tracker = PyramidKltTracker(self.klt, self.scales)
        self.detectRadius, self.detectThreshold, self.detectBorder, self.maxFeatures = detectRadius, detectThreshold, detectBorder, maxFeatures
        self.active, self.spawned, self.dropped = [], [], []
        self.totalFeatures = 0
        self.shape = None

    def process(self, frame):
        frame = np.ascontiguousarray(frame, np.float32)
        self.shape = frame.shape
        self.spawned, self.dropped = [], []
        self.layers, self.derivX, self.derivY = pyramid_gradient(self.orc, frame, self.scales)
        self.tracker.setImage(self.layers, self.derivX, self.derivY)
        H, W = frame.shape
        i = 0
        while i < len(self.active):
            t = self.active[i]
            ret = self.tracker.track(t)
            t.fault = ret
            success = False
            if ret == SUCCESS:
                t.error = self.klt.error
                ix, iy = int(t.x), int(t.y)
                if 0 <= ix < W and 0 <= iy < H and self.tracker.setDescription(t):
                    t.px, t.py = t.x, t.y
                    i += 1
                    success = True
            if not success:
                self.active.pop(i)
                self.dropped.append(t)

    def spawnTracks(self):
        self.spawned = []
        scaleBottom = F(float(self.scales[0]))
        exclude = [(int(t.x / scaleBottom), int(t.y / scaleBottom)) for t in self.active]
        found = detect(self.orc, self.derivX[0], self.derivY[0], exclude, self.detectRadius, self.detectThreshold, self.detectBorder, self.maxFeatures)
        for x, y in found:
            t = PyramidKltFeature(len(self.scales), self.templateRadius)
            t.x, t.y = F(int(x)) * scaleBottom, F(int(y)) * scaleBottom
            t.described = self.tracker.setDescription(t)   # the result is not looked at: checkValidSpawn() is always true
            t.px, t.py = t.x, t.y
            t.featureId = self.totalFeatures
            self.totalFeatures += 1
            self.active.append(t)
            self.spawned.append(t)

    def addTrack(self, x, y):
        H, W = self.shape
        if not (0 <= int(x) < W and 0 <= int(y) < H):
            return None
        t = PyramidKltFeature(len(self.scales), self.templateRadius)
        t.setPosition(F(x), F(y))
        self.tracker.setDescription(t)      # the result is not looked at
        t.px, t.py = t.x, t.y
        t.featureId = -1                    # the reference assigns none
        self.active.append(t)
        return t

    def dropTrack(self, t):
        if t in self.active:
            self.active.remove(t)
            return True
        return False

    def dropAllTracks(self):
        self.active, self.dropped = [], []

    def reset(self):
        self.dropAllTracks()
        self.totalFeatures = 0
