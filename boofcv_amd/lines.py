"""Line detection: the Hough detectors of FactoryDetectLine (F:factory/feature/detect/line/FactoryDetectLine.java) on the GPU.
  FactoryDetectLine.houghLinePolar(ConfigHoughBinary, ConfigParamPolar, ConfigThreshold, type)   :145-163 -> HoughBinary_to_DetectLine
  FactoryDetectLine.houghLineFoot(ConfigHoughGradient, ConfigParamFoot, type)                     :90-105  -> HoughGradient_to_DetectLine
  HoughTransformBinary / HoughTransformGradient       F:alg/feature/detect/line/HoughTransformBinary.java, HoughTransformGradient.java
  HoughParametersPolar / HoughParametersFootOfNorm    F:alg/feature/detect/line/HoughParametersPolar.java, HoughParametersFootOfNorm.java
  ImageLinePruneMerge, LineImageOps.convert           F:alg/feature/detect/line/ImageLinePruneMerge.java, LineImageOps.java:234-276

A module beside the api package (like binary.py and binaryops.py).  The image stages run on the device through DeviceImageOps: threshold, the
vote, the relaxed block extractor (binary form); Prewitt, intensityAbs, the crude edge suppression, the FIXED threshold, the vote, the strict
block extractor and the mean-shift refinement (gradient form).  What follows the peaks is list logic on a few dozen lines and runs here, in
float32 / float64 scalars where Java has float / double: transformToLine, isTransformValid, the divergence test, pruneSimilar / pruneNBest.

Not pinned against the jars (georegression and ddogleg are not part of the reference tree): CachedSineCosine_F32, UtilAngle.atanSafe /
distHalf, Intersection2D_F32.intersection, Distance2D_F32.distance, Point2D_F32.distance, UtilGaussian.computePDF are restated from their
documented behaviour.

Refused with IllegalArgumentException: houghLinePolar(ConfigHoughGradient, ...), houghLineFootSub, lineRansac, image types other than GrayU8 and
GrayF32, GrayS32 derivatives."""
import functools
import math

import numpy as np

from .api.core import IllegalArgumentException
from .api.image import GrayF32, GrayS16, GrayU8
from .binary import ConfigLength, ConfigThreshold, InputToBinary, ThresholdType

__all__ = ["CachedSineCosine_F32", "ConfigHoughBinary", "ConfigHoughGradient", "ConfigParamFoot", "ConfigParamPolar", "DetectLine", "FactoryDetectLine",
           "HoughBinary_to_DetectLine", "HoughGradient_to_DetectLine", "HoughParametersFootOfNorm", "HoughParametersPolar", "HoughTransformBinary",
           "HoughTransformGradient", "ImageLinePruneMerge", "LineParametric2D_F32", "weightPixelGaussian"]

F = np.float32
_PI_F = F(math.pi)
_PID2_F = F(math.pi / 2.0)


class _Vec2F:
    def __init__(self, x=0.0, y=0.0):
        self.x, self.y = F(x), F(y)

    def set(self, x, y):
        self.x, self.y = F(x), F(y)

    def __eq__(self, o):
        return isinstance(o, _Vec2F) and self.x.tobytes() == o.x.tobytes() and self.y.tobytes() == o.y.tobytes()

    def __repr__(self):
        return "(%r, %r)" % (float(self.x), float(self.y))


class LineParametric2D_F32:
    """georegression's LineParametric2D_F32: the point p and the direction slope, float32"""

    def __init__(self, px=0.0, py=0.0, sx=0.0, sy=0.0):
        self.p, self.slope = _Vec2F(px, py), _Vec2F(sx, sy)

    def getSlopeX(self):
        return self.slope.x

    def getSlopeY(self):
        return self.slope.y

    def getX(self):
        return self.p.x

    def getY(self):
        return self.p.y

    def __eq__(self, o):
        return isinstance(o, LineParametric2D_F32) and self.p == o.p and self.slope == o.slope

    def __repr__(self):
        return "LineParametric2D_F32(p=%r, slope=%r)" % (self.p, self.slope)


class ConfigHoughBinary:
    """F:factory/feature/detect/line/ConfigHoughBinary.java:29-68"""

    def __init__(self, maxLines=10):
        self.localMaxRadius = 1
        self.minCounts = ConfigLength.relative(0.001, 1)
        self.maxLines = int(maxLines)
        self.mergeAngle = math.pi * 0.05
        self.mergeDistance = 10.0

    def checkValidity(self):
        pass


class ConfigHoughGradient:
    """F:factory/feature/detect/line/ConfigHoughGradient.java:28-85: ConfigHoughGradient(), (maxLines) or (localMaxRadius, minCounts,
    minDistanceFromOrigin, thresholdEdge, maxLines)"""

    def __init__(self, *args):
        self.localMaxRadius, self.minCounts, self.minDistanceFromOrigin, self.thresholdEdge, self.maxLines = 2, 5, 5, 30.0, 0
        self.mergeAngle = math.pi * 0.05
        self.mergeDistance = 10.0
        self.refineRadius = 3
        if len(args) == 1:
            self.maxLines = int(args[0])
        elif len(args) == 5:
            self.localMaxRadius, self.minCounts, self.minDistanceFromOrigin, self.thresholdEdge, self.maxLines = args
        elif args:
            raise TypeError("ConfigHoughGradient(), (maxLines) or (localMaxRadius, minCounts, minDistanceFromOrigin, thresholdEdge, maxLines)")

    def checkValidity(self):
        pass


class ConfigParamPolar:
    """F:factory/feature/detect/line/ConfigParamPolar.java:28-50"""

    def __init__(self, resolutionRange=2.0, numBinsAngle=180):
        self.resolutionRange, self.numBinsAngle = float(resolutionRange), int(numBinsAngle)

    def checkValidity(self):
        pass


class ConfigParamFoot:
    """F:factory/feature/detect/line/ConfigParamFoot.java:28-38"""

    def __init__(self, minDistanceFromOrigin=5):
        self.minDistanceFromOrigin = int(minDistanceFromOrigin)

    def checkValidity(self):
        pass


class CachedSineCosine_F32:
    """georegression's CachedSineCosine_F32(minAngle, maxAngle, size): angle = (max-min)*i/(size-1) + min in float, c = (float)Math.cos(angle),
    s = (float)Math.sin(angle) through double.  cosine(i) / sine(i) look an entry up by its index, which is how HoughParametersPolar uses them.
    Not pinned against the jar."""

    def __init__(self, minAngle, maxAngle, size):
        self.minAngle, self.maxAngle, self.size = F(minAngle), F(maxAngle), int(size)
        self.c, self.s = np.zeros(self.size, F), np.zeros(self.size, F)
        with np.errstate(all="ignore"):   # size 1 divides by zero as Java does: NaN entries
            for i in range(self.size):
                angle = F(F(F(self.maxAngle - self.minAngle) * F(i)) / F(self.size - 1)) + self.minAngle
                self.c[i] = F(math.cos(float(angle))) if np.isfinite(angle) else F(np.nan)
                self.s[i] = F(math.sin(float(angle))) if np.isfinite(angle) else F(np.nan)

    def cosine(self, index):
        return self.c[int(index)]

    def sine(self, index):
        return self.s[int(index)]


def weightPixelGaussian(radius):
    """The kernel of WeightPixelGaussian_F32.setRadius(radius, radius, odd = true) (I:alg/weights/WeightPixelGaussian_F32.java:29-43):
    FactoryKernelGaussian.gaussian2D_F32((float)sigmaForRadius(radius, 0), radius, true, true) (I:factory/filter/kernel/FactoryKernelGaussian.java:
    218-238, 269-278, 388-393; KernelMath.convolve2D :338-356, normalizeSumToOne :438-444) -> float32 [(2*radius+1)^2], row-major"""
    if radius <= 0:
        return np.zeros(0, F)
    sigma = float(F((radius * 2.0 + 1.0) / 5.0))
    k1 = np.array([F(math.exp(-float(i) * float(i) / (2.0 * sigma * sigma)) / (sigma * math.sqrt(2.0 * math.pi))) for i in range(radius, -radius - 1, -1)], F)
    k2 = np.array([F(a * b) for a in k1 for b in k1], F)
    total = F(0)
    for v in k2:
        total = F(total + v)
    return np.array([F(v / total) for v in k2], F)


# ---- georegression helpers of the merge (float arithmetic; not pinned against the jar) ----
def _atanSafe(y, x):
    if x == 0:
        return _PID2_F if y >= 0 else F(-_PID2_F)
    with np.errstate(all="ignore"):
        return F(math.atan(float(F(y / x))))


def _distHalf(a, b):
    r = F(abs(F(a - b)))
    return r if float(r) <= math.pi / 2 else F(_PI_F - r)


def _intersectLines(a, b):
    """Intersection2D_F32.intersection(LineParametric2D_F32 a, LineParametric2D_F32 b, ret) -> (x, y) or None"""
    t_b = F(F(a.slope.x * F(b.p.y - a.p.y)) - F(a.slope.y * F(b.p.x - a.p.x)))
    bottom = F(F(a.slope.y * b.slope.x) - F(b.slope.y * a.slope.x))
    if bottom == 0:
        return None
    t_b = F(t_b / bottom)
    return F(F(b.slope.x * t_b) + b.p.x), F(F(b.slope.y * t_b) + b.p.y)


def _pointDistance(ax, ay, bx, by):
    dx, dy = F(bx - ax), F(by - ay)
    return F(math.sqrt(float(F(F(dx * dx) + F(dy * dy)))))


def _intersectSegments(l0, l1):
    """Intersection2D_F32.intersection(LineSegment2D_F32, LineSegment2D_F32, ret); a segment is (ax, ay, bx, by)"""
    a0, b0 = F(l0[2] - l0[0]), F(l0[3] - l0[1])
    a1, b1 = F(l1[2] - l1[0]), F(l1[3] - l1[1])
    top = F(F(b0 * F(l1[0] - l0[0])) + F(a0 * F(l0[1] - l1[1])))
    bottom = F(F(a0 * b1) - F(b0 * a1))
    if bottom == 0:
        return None
    t_1 = F(top / bottom)
    if t_1 < 0 or t_1 > 1:
        return None
    top = F(F(b1 * F(l0[0] - l1[0])) + F(a1 * F(l1[1] - l0[1])))
    bottom = F(F(a1 * b0) - F(b1 * a0))
    with np.errstate(all="ignore"):
        t_0 = F(top / bottom)
    if t_0 < 0 or t_0 > 1:
        return None
    return F(l1[0] + F(a1 * t_1)), F(l1[1] + F(b1 * t_1))


def _segmentDistance(line, px, py):
    """Distance2D_F32.distance(LineSegment2D_F32, Point2D_F32)"""
    a, b = F(line[2] - line[0]), F(line[3] - line[1])
    t = F(F(a * F(px - line[0])) + F(b * F(py - line[1])))
    with np.errstate(all="ignore"):
        t = F(t / F(F(a * a) + F(b * b)))
    if t < 0:
        return _pointDistance(line[0], line[1], px, py)
    if t > 1:
        return _pointDistance(line[2], line[3], px, py)
    return _pointDistance(F(line[0] + F(t * a)), F(line[1] + F(t * b)), px, py)


def _convertToSegment(l, width, height):
    """LineImageOps.convert(LineParametric2D_F32, width, height) -> (ax, ay, bx, by) or None"""
    inside = []

    def checkAddInside(a):
        if a[0] >= 0 and a[0] <= F(F(width) - F(0.999)) and a[1] >= 0 and a[1] <= F(F(height) - F(0.999)):
            for p in inside:
                if float(_pointDistance(p[0], p[1], a[0], a[1])) < 1e-4:
                    return
            inside.append(a)

    for px, py, sx, sy in ((0, 0, 1, 0), (0, 0, 0, 1), (width - 1, height - 1, -1, 0), (width - 1, height - 1, 0, -1)):
        a = _intersectLines(LineParametric2D_F32(px, py, sx, sy), l)
        if a is not None:
            checkAddInside(a)
    if len(inside) != 2:
        return None
    return inside[0][0], inside[0][1], inside[1][0], inside[1][1]


def _floatCompare(a, b):
    """Float.compare"""
    if a < b:
        return -1
    if a > b:
        return 1
    ia, ib = int(np.array(a, F).view(np.int32)), int(np.array(b, F).view(np.int32))
    return 0 if ia == ib else -1 if ia < ib else 1


class ImageLinePruneMerge:
    """F:alg/feature/detect/line/ImageLinePruneMerge.java:35-198"""

    def __init__(self):
        self.lines = []   # [line, intensity]

    def reset(self):
        self.lines = []

    def add(self, line, intensity):
        self.lines.append([line, F(intensity)])

    def pruneNBest(self, N):
        if len(self.lines) <= N:
            return
        self._sortByIntensity()
        self.lines = self.lines[:N]

    def _sortByIntensity(self):
        def cmp(o1, o2):
            if o1[1] < o2[1]:
                return 1
            if o1[1] > o2[1]:
                return -1
            if o1[0].p.x < o2[0].p.x:
                return -1
            if o1[0].p.x > o2[0].p.x:
                return 1
            return _floatCompare(o1[0].p.y, o2[0].p.y)
        self.lines.sort(key=functools.cmp_to_key(cmp))   # stable, as Collections.sort

    def pruneSimilar(self, toleranceAngle, toleranceDist, imgWidth, imgHeight):
        toleranceAngle, toleranceDist = F(toleranceAngle), F(toleranceDist)
        self._sortByIntensity()
        theta = [_atanSafe(d[0].getSlopeY(), d[0].getSlopeX()) for d in self.lines]
        segments = [_convertToSegment(d[0], imgWidth, imgHeight) for d in self.lines]
        for i in range(len(segments)):
            a = segments[i]
            if a is None:
                continue
            for j in range(i + 1, len(segments)):
                b = segments[j]
                if b is None:
                    continue
                if _distHalf(theta[i], theta[j]) > toleranceAngle:
                    continue
                p = _intersectSegments(a, b)
                close = p is not None and p[0] >= 0 and p[1] >= 0 and p[0] < imgWidth and p[1] < imgHeight
                if not close:
                    if _segmentDistance(a, b[0], b[1]) > toleranceDist and _segmentDistance(a, b[2], b[3]) > toleranceDist:
                        continue
                    if _segmentDistance(b, b[0], b[1]) > toleranceDist and _segmentDistance(b, b[2], b[3]) > toleranceDist:
                        continue
                if self.lines[j][1] > self.lines[i][1]:
                    self.lines[i][1] = self.lines[j][1]
                segments[j] = None
        self.lines = [d for d, s in zip(self.lines, segments) if s is not None]

    def createList(self):
        return [d[0] for d in self.lines]


class HoughParametersPolar:
    """F:alg/feature/detect/line/HoughParametersPolar.java:31-146 (the host side: initialize, isTransformValid, transformToLine)"""

    def __init__(self, rangeResolution, numBinsAngle):
        self.rangeResolution, self.numBinsAngle = float(rangeResolution), int(numBinsAngle)
        self.tableTrig = CachedSineCosine_F32(0.0, _PI_F, self.numBinsAngle)
        self.originX = self.originY = self.numBinsRange = 0
        self.r_max = F(0)

    def initialize(self, width, height, ops):
        self.originX, self.originY = width // 2, height // 2
        self.numBinsRange, r = ops.houghPolarBins(width, height, self.rangeResolution)
        self.r_max = F(r)

    def isTransformValid(self, x, y):
        return True

    def transformToLine(self, x, y, line):
        w2 = self.numBinsRange // 2
        with np.errstate(all="ignore"):
            r = F(F(self.r_max * F(F(x) - F(w2))) / F(w2))
        c, s = self.tableTrig.cosine(y), self.tableTrig.sine(y)
        line.p.set(F(F(r * c) + F(self.originX)), F(F(r * s) + F(self.originY)))
        line.slope.set(F(-s), c)


class HoughParametersFootOfNorm:
    """F:alg/feature/detect/line/HoughParametersFootOfNorm.java:29-86"""

    def __init__(self, minDistanceFromOrigin):
        self.minDistanceFromOrigin = int(minDistanceFromOrigin)
        self.originX = self.originY = 0

    def initialize(self, width, height, ops=None):
        self.originX, self.originY = width // 2, height // 2

    def isTransformValid(self, x, y):
        # the reference compares y with originX, too (:54)
        return abs(x - self.originX) >= self.minDistanceFromOrigin or abs(y - self.originX) >= self.minDistanceFromOrigin

    def transformToLine(self, x, y, l):
        l.p.set(x, y)
        l.slope.set(F(-F(l.p.y - F(self.originY))), F(l.p.x - F(self.originX)))


_default_ops = {}


def _ops(ops):
    """the DeviceImageOps a detector runs on: the caller's, or one per process on device 0 (created on first use: torch is imported here)"""
    if ops is not None:
        return ops
    if 0 not in _default_ops:
        from .device import DeviceImageOps
        _default_ops[0] = DeviceImageOps()
    return _default_ops[0]


def _to_device(ops, image):
    import torch
    image._in()
    return torch.from_numpy(np.array(image.array())).to(ops.device).unsqueeze(0)   # (a dense, writable copy: the view may be read-only)


class _HoughTransformBase:
    def __init__(self):
        self.linesAll, self.linesMerged, self.foundIntensity = [], [], np.zeros(0, F)
        self.post = ImageLinePruneMerge()
        self.mergeAngle, self.mergeDistance, self.maxLines = math.pi * 0.05, 10.0, 0
        self._transform = None   # float32 [1, h, w] on the device

    def _finish(self, width, height):
        if self.maxLines <= 0:
            self.linesMerged = list(self.linesAll)
            return
        self.post.reset()
        for l, v in zip(self.linesAll, self.foundIntensity):
            self.post.add(l, v)
        self.post.pruneSimilar(F(self.mergeAngle), F(self.mergeDistance), width, height)
        self.post.pruneNBest(self.maxLines)
        self.linesMerged = self.post.createList()

    def getTransform(self):
        """the transform as a GrayF32 on the host"""
        return GrayF32.wrap(self._transform[0].cpu().numpy())

    def getFoundIntensity(self):
        return self.foundIntensity

    def getLinesAll(self):
        return self.linesAll

    def getLinesMerged(self):
        return self.linesMerged

    def getMergeAngle(self):
        return self.mergeAngle

    def setMergeAngle(self, mergeAngle):
        self.mergeAngle = float(mergeAngle)

    def getMergeDistance(self):
        return self.mergeDistance

    def setMergeDistance(self, mergeDistance):
        self.mergeDistance = float(mergeDistance)

    def getMaxLines(self):
        return self.maxLines

    def setMaxLines(self, maxLines):
        self.maxLines = int(maxLines)

    def getParameters(self):
        return self.parameters


class HoughTransformBinary(_HoughTransformBase):
    """F:alg/feature/detect/line/HoughTransformBinary.java:64-234 with HoughParametersPolar and the relaxed block extractor
    FactoryFeatureExtractor.nonmax(ConfigExtract(localMaxRadius, 0, 0, false)).  transform(binary): a GrayU8, or a uint8 device tensor [H,W]."""

    def __init__(self, localMaxRadius, parameters, ops=None):
        super().__init__()
        if not isinstance(parameters, HoughParametersPolar):
            raise IllegalArgumentException("Not supported")   # HoughParametersFootOfNorm.parameterize(x, y, transform) throws it
        self.localMaxRadius, self.parameters, self.ops = int(localMaxRadius), parameters, ops
        self.thresholdCounts = ConfigLength.relative(0.001, 1)

    def setNumberOfCounts(self, counts):
        self.thresholdCounts = counts

    def transform(self, binary):
        ops = _ops(self.ops)
        dev = _to_device(ops, binary) if isinstance(binary, GrayU8) else binary
        if dev.dim() == 2:
            dev = dev.unsqueeze(0)
        height, width = int(dev.shape[-2]), int(dev.shape[-1])
        par = self.parameters
        par.initialize(width, height, ops)
        if par.numBinsRange <= 0 or par.numBinsAngle <= 0:
            raise IllegalArgumentException("the transform has no bins")
        self._transform = ops.houghBinaryPolar(dev, par.rangeResolution, par.numBinsAngle, par.tableTrig.c, par.tableTrig.s)
        # extractLines
        threshold = F(self.thresholdCounts.compute(par.numBinsRange * par.numBinsAngle))
        xy, n = ops.nonmaxRelaxed(self._transform, self.localMaxRadius, threshold, 0)
        peak, inten = ops.meanShiftPeak(self._transform, xy.contiguous(), n, radius=0)
        count = int(n[0].item())
        pts, vals = xy[0, :count].cpu().numpy(), inten[0, :count].cpu().numpy()
        self.linesAll, found = [], []
        for (x, y), v in zip(pts, vals):
            if not par.isTransformValid(int(x), int(y)):
                continue
            line = LineParametric2D_F32()
            par.transformToLine(F(x), F(y), line)
            self.linesAll.append(line)
            found.append(v)
        self.foundIntensity = np.array(found, F)
        self._finish(width, height)


class HoughTransformGradient(_HoughTransformBase):
    """F:alg/feature/detect/line/HoughTransformGradient.java:54-304 with HoughParametersFootOfNorm and the strict block extractor
    FactoryFeatureExtractor.nonmax(ConfigExtract(localMaxRadius, minCounts, 0, true)).  transform(derivX, derivY, binary): GrayF32 or GrayS16
    derivatives with a GrayU8, or device tensors [H,W] (float32 / int16, uint8).  The candidates list is not produced."""

    def __init__(self, localMaxRadius, minCounts, parameters, derivType=GrayF32, ops=None):
        super().__init__()
        if isinstance(parameters, HoughParametersPolar):
            raise IllegalArgumentException("the polar parameterisation of the gradient transform is not implemented on the GPU")
        if derivType not in (GrayF32, GrayS16):
            raise IllegalArgumentException("only GrayF32 and GrayS16 derivatives are implemented on the GPU")
        self.localMaxRadius, self.minCounts, self.parameters, self.derivType, self.ops = int(localMaxRadius), float(minCounts), parameters, derivType, ops
        self.refineRadius = 3
        self.refineMaxIterations, self.refineConvergenceTol = 10, F(0.001)

    def setRefineRadius(self, radius):
        self.refineRadius = int(radius)

    def getRefineRadius(self):
        return self.refineRadius

    def transform(self, derivX, derivY, binary):
        ops = _ops(self.ops)
        if isinstance(binary, GrayU8):
            if not isinstance(derivX, self.derivType) or not isinstance(derivY, self.derivType):
                raise IllegalArgumentException("expected %s derivatives" % self.derivType.__name__)
            if (derivX.width, derivX.height) != (derivY.width, derivY.height) or (derivX.width, derivX.height) != (binary.width, binary.height):
                raise IllegalArgumentException("Image shapes do not match")   # InputSanityCheck.checkSameShape
            derivX, derivY, binary = _to_device(ops, derivX), _to_device(ops, derivY), _to_device(ops, binary)
        if binary.dim() == 2:
            derivX, derivY, binary = derivX.unsqueeze(0), derivY.unsqueeze(0), binary.unsqueeze(0)
        height, width = int(binary.shape[-2]), int(binary.shape[-1])
        par = self.parameters
        par.initialize(width, height, ops)
        self._transform, _ = ops.houghGradientFoot(derivX, derivY, binary)
        # extractLines
        xy, n = ops.nonmax(self._transform, self.localMaxRadius, self.minCounts, 0)
        peak, inten = ops.meanShiftPeak(self._transform, xy, n, radius=self.refineRadius, maxIterations=self.refineMaxIterations,
                                        convergenceTol=self.refineConvergenceTol)
        count = min(int(n[0].item()), xy.shape[1])
        pts, peaks, vals = xy[0, :count].cpu().numpy(), peak[0, :count].cpu().numpy(), inten[0, :count].cpu().numpy()
        self.linesAll, found = [], []
        for (x, y), (rx, ry), v in zip(pts, peaks, vals):
            if not par.isTransformValid(int(x), int(y)):
                continue
            line = LineParametric2D_F32(x, y)
            # check for divergence
            if _pointDistance(line.p.x, line.p.y, F(rx), F(ry)) < F(self.refineRadius * 2):
                line.p.set(rx, ry)
            par.transformToLine(line.p.x, line.p.y, line)
            self.linesAll.append(line)
            found.append(v)
        self.foundIntensity = np.array(found, F)
        self._finish(width, height)


class DetectLine:
    """F:abst/feature/detect/line/DetectLine.java: detect(input) -> list of LineParametric2D_F32"""

    def detect(self, input):
        raise NotImplementedError

    def getInputType(self):
        return self.inputType


class HoughBinary_to_DetectLine(DetectLine):
    """F:abst/feature/detect/line/HoughBinary_to_DetectLine.java:38-71"""

    def __init__(self, hough, configThreshold, inputType):
        self.hough, self.configThreshold, self.inputType = hough, configThreshold, inputType
        self.thresholder = InputToBinary(configThreshold, inputType)   # what threshold.hip refuses is refused here
        self.binary = None

    def detect(self, input):
        if not isinstance(input, self.inputType):
            raise IllegalArgumentException("expected a %s input" % self.inputType.__name__)
        ops = _ops(self.hough.ops)
        self.binary = ops.threshold(_to_device(ops, input), self.configThreshold)
        self.hough.transform(self.binary)
        return self.hough.getLinesMerged()

    def getHough(self):
        return self.hough

    def getThresholder(self):
        return self.thresholder

    def getBinary(self):
        return GrayU8.wrap(self.binary[0].cpu().numpy())


class HoughGradient_to_DetectLine(DetectLine):
    """F:abst/feature/detect/line/HoughGradient_to_DetectLine.java:50-147 with FactoryDerivative.prewitt (BorderType.EXTENDED)"""

    def __init__(self, hough, inputType):
        self.hough, self.inputType = hough, inputType
        self.thresholdEdge = F(20)
        self.nonMaxSuppression = True
        self.derivX = self.derivY = self.edgeIntensity = self.suppressed = self.binary = None

    def detect(self, input):
        from .device import INTENSITY_ABS
        if not isinstance(input, self.inputType):
            raise IllegalArgumentException("expected a %s input" % self.inputType.__name__)
        ops = _ops(self.hough.ops)
        self.derivX, self.derivY = ops.prewitt(_to_device(ops, input), "EXTENDED")
        self.edgeIntensity = ops.intensity(INTENSITY_ABS, self.derivX, self.derivY)
        edges = self.edgeIntensity
        if self.nonMaxSuppression:
            edges = self.suppressed = ops.edgeNonMaxCrude4(self.edgeIntensity, self.derivX, self.derivY)
        cfg = ConfigThreshold.fixed(float(self.thresholdEdge))
        cfg.down = False
        self.binary = ops.threshold(edges, cfg)
        self.hough.transform(self.derivX, self.derivY, self.binary)
        return self.hough.getLinesMerged()

    def getThresholdEdge(self):
        return self.thresholdEdge

    def setThresholdEdge(self, thresholdEdge):
        self.thresholdEdge = F(thresholdEdge)

    def isNonMaxSuppression(self):
        return self.nonMaxSuppression

    def setNonMaxSuppression(self, nonMaxSuppression):
        self.nonMaxSuppression = bool(nonMaxSuppression)

    def getHough(self):
        return self.hough

    def getBinary(self):
        return GrayU8.wrap(self.binary[0].cpu().numpy())


def _imageType(imageType):
    if imageType not in (GrayU8, GrayF32):
        raise IllegalArgumentException("only GrayU8 and GrayF32 images are implemented on the GPU")
    return imageType


class FactoryDetectLine:
    """F:factory/feature/detect/line/FactoryDetectLine.java.  ops: the DeviceImageOps to run on (default: one per process on device 0)."""

    @staticmethod
    def houghLinePolar(configHough, configParam, *rest, ops=None):
        """houghLinePolar(ConfigHoughBinary, ConfigParamPolar, ConfigThreshold, imageType) (:145-163).  The overload with a ConfigHoughGradient
        (:117-133) is not implemented on the GPU."""
        if isinstance(configHough, ConfigHoughGradient) or len(rest) == 1:
            raise IllegalArgumentException("houghLinePolar(ConfigHoughGradient, ...) is not implemented on the GPU")
        if len(rest) != 2:
            raise TypeError("houghLinePolar(configHough, configParam, configThreshold, imageType)")
        configThreshold, imageType = rest
        _imageType(imageType)
        configHough = configHough or ConfigHoughBinary()
        configParam = configParam or ConfigParamPolar()
        if configThreshold is None:
            configThreshold = ConfigThreshold.global_(ThresholdType.GLOBAL_OTSU)
        param = HoughParametersPolar(configParam.resolutionRange, configParam.numBinsAngle)
        hough = HoughTransformBinary(configHough.localMaxRadius, param, ops)
        hough.setMaxLines(configHough.maxLines)
        hough.setMergeAngle(configHough.mergeAngle)
        hough.setMergeDistance(configHough.mergeDistance)
        hough.setNumberOfCounts(configHough.minCounts.copy())
        return HoughBinary_to_DetectLine(hough, configThreshold, imageType)

    @staticmethod
    def houghLineFoot(configHough, configParam, imageType, ops=None):
        """houghLineFoot(ConfigHoughGradient, ConfigParamFoot, imageType) (:90-105): GrayF32 (GrayF32 derivatives) and GrayU8 (GrayS16)"""
        _imageType(imageType)
        configHough = configHough or ConfigHoughGradient()
        configParam = configParam or ConfigParamFoot()
        param = HoughParametersFootOfNorm(configParam.minDistanceFromOrigin)
        hough = HoughTransformGradient(configHough.localMaxRadius, configHough.minCounts, param, GrayF32 if imageType is GrayF32 else GrayS16, ops)
        hough.setMaxLines(configHough.maxLines)
        hough.setMergeAngle(configHough.mergeAngle)
        hough.setMergeDistance(configHough.mergeDistance)
        hough.setRefineRadius(configHough.refineRadius)
        detector = HoughGradient_to_DetectLine(hough, imageType)
        detector.setThresholdEdge(configHough.thresholdEdge)
        return detector

    @staticmethod
    def houghLineFootSub(config, imageType, ops=None):
        raise IllegalArgumentException("houghLineFootSub is not implemented on the GPU")

    @staticmethod
    def lineRansac(config, imageType, ops=None):
        raise IllegalArgumentException("lineRansac is not implemented on the GPU")
