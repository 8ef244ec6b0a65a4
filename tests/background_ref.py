"""NumPy / pure-Python restatement of BoofCV's stationary background models, line by line, in fp32 with Java's evaluation order.

Reference (F: = main/boofcv-feature/src/main/java/boofcv/):
    BackgroundStationaryBasic_SB / _PL      F:alg/background/stationary/BackgroundStationaryBasic_SB.java:58-123, BackgroundStationaryBasic_PL.java:66-142
    BackgroundStationaryGaussian_SB / _PL   F:alg/background/stationary/BackgroundStationaryGaussian_SB.java:58-142, BackgroundStationaryGaussian_PL.java:72-180
    BackgroundStationaryGmm, _SB, _MB       F:alg/background/stationary/BackgroundStationaryGmm.java:48-78, BackgroundStationaryGmm_SB.java:50-100, _MB.java:54-105
    BackgroundGmmCommon                     F:alg/background/BackgroundGmmCommon.java:78-375
    BackgroundModelStationary               F:alg/background/BackgroundModelStationary.java:48-51  (updateBackground(frame, segment): update THEN segment)
    FactoryBackgroundModel                  F:factory/background/FactoryBackgroundModel.java:47-64,112-141,193-225

A frame is a uint8 or float32 array, [h][w] for a Gray image (bands = 0: the *_SB classes) or [bands][h][w] for a Planar image (*_PL / *_MB).
Basic and Gaussian are whole-array fp32 NumPy (element-wise IEEE operations, one rounding each, no fused multiply-add; the one double
accumulator of Basic_PL.segment is a float64 array); the GMM per-pixel code is plain Python on np.float32 scalars.  Every class counts the
branches it takes in `counts`, so a test can show that its sequence reaches all of them before it asks the GPU.
"""
import collections

import numpy as np

f32 = np.float32
FLOAT_MIN_VALUE = np.float32(1.401298464324817e-45)   # Float.MIN_VALUE


class IllegalArgumentException(ValueError):
    pass


def to_float(frame, bands):
    """GImageGray.getF / GConvertImage.convert: GrayU8 -> data & 0xFF as float.  -> float32 [max(bands,1)][h][w]"""
    a = np.asarray(frame)
    if a.dtype != np.uint8 and a.dtype != np.float32:
        raise IllegalArgumentException("GrayU8 or GrayF32")
    if bands == 0:
        assert a.ndim == 2
        a = a[None]
    else:
        assert a.ndim == 3 and a.shape[0] == bands, "Planar frames are [bands][h][w]"
    return a.astype(np.float32)


class _Model:
    """BackgroundModel + BackgroundModelStationary"""

    def __init__(self, bands):
        self.bands = bands           # 0: single band class
        self.numBands = max(bands, 1)
        self.unknownValue = 0
        self.counts = collections.Counter()

    def setUnknownValue(self, v):
        if v < 0 or v > 255:
            raise IllegalArgumentException("out of range. 0 to 255")
        self.unknownValue = v

    def updateBackground(self, frame, mask=False):
        """mask=True: updateBackground(frame, segment) -> the mask.  BackgroundModelStationary.java:48-51"""
        self._update(to_float(frame, self.bands))
        if mask:
            return self.segment(frame)
        return None


class BasicRef(_Model):
    def __init__(self, learnRate, threshold, bands=0):
        super().__init__(bands)
        if learnRate < 0 or learnRate > 1:
            raise IllegalArgumentException("LearnRate must be 0 <= rate <= 1.0f")
        self.learnRate, self.threshold = f32(learnRate), f32(threshold)
        self.background = np.zeros((self.numBands, 0, 0), np.float32)

    def reset(self):
        self.background = np.zeros((self.numBands, 0, 0), np.float32)

    def state(self):
        return self.background

    def _update(self, fr):
        if self.background.shape[2] != fr.shape[2]:               # background.width != frame.width
            self.background = fr.copy()
            self.counts["init"] += 1
            return
        if self.background.shape != fr.shape:
            raise IllegalArgumentException("Image shapes do not match")
        minusLearn = f32(1.0) - self.learnRate
        self.background = minusLearn * self.background + self.learnRate * fr
        self.counts["update"] += 1

    def segment(self, frame):
        fr = to_float(frame, self.bands)
        h, w = fr.shape[1:]
        if self.background.shape[2] != w:
            self.counts["unknown"] += 1
            return np.full((h, w), self.unknownValue, np.uint8)
        if self.background.shape != fr.shape:
            raise IllegalArgumentException("Image shapes do not match")
        if self.bands == 0:
            thresholdSq = self.threshold * self.threshold
            diff = self.background[0] - fr[0]
            sq = diff * diff
            cmp = thresholdSq
        else:
            thresholdSq = (f32(self.numBands) * self.threshold) * self.threshold
            sq = np.zeros((h, w), np.float64)
            for b in range(self.numBands):
                diff = self.background[b] - fr[b]
                sq += (diff * diff).astype(np.float64)
            cmp = np.float64(thresholdSq)
        self.counts["equal"] += int(np.count_nonzero(sq == cmp))
        self.counts["below"] += int(np.count_nonzero(sq < cmp))
        self.counts["above"] += int(np.count_nonzero(sq > cmp))
        return np.where(sq <= cmp, 0, 1).astype(np.uint8)


class GaussianRef(_Model):
    def __init__(self, learnRate, threshold, bands=0):
        super().__init__(bands)
        if threshold < 0:
            raise IllegalArgumentException("Threshold must be more than 0")
        self.learnRate, self.threshold = f32(learnRate), f32(threshold)
        self.initialVariance = FLOAT_MIN_VALUE
        self.minimumDifference = f32(0)
        self.background = np.zeros((2 * self.numBands, 1, 1), np.float32)

    def reset(self):
        self.background = np.zeros((2 * self.numBands, 1, 1), np.float32)

    def state(self):
        return self.background

    def _update(self, fr):
        if self.background.shape[2] == 1:                         # background.width == 1
            self.background = np.empty((2 * self.numBands,) + fr.shape[1:], np.float32)
            self.background[0::2] = fr
            self.background[1::2] = f32(self.initialVariance)
            self.counts["init"] += 1
            return
        if self.background.shape[1:] != fr.shape[1:]:
            raise IllegalArgumentException("Image shapes do not match")
        minusLearn = f32(1.0) - self.learnRate
        mean, var = self.background[0::2], self.background[1::2]
        diff = mean - fr
        with np.errstate(all="ignore"):
            newMean = minusLearn * mean + self.learnRate * fr
            newVar = minusLearn * var + self.learnRate * diff * diff
        self.background[0::2] = newMean
        self.background[1::2] = newVar
        self.counts["update"] += 1
        self.counts["denormal_variance"] += int(np.count_nonzero((newVar > 0) & (newVar < np.finfo(np.float32).tiny)))
        self.counts["zero_variance"] += int(np.count_nonzero(newVar == 0))

    def segment(self, frame):
        fr = to_float(frame, self.bands)
        h, w = fr.shape[1:]
        if self.background.shape[2] == 1:
            self.counts["unknown"] += 1
            return np.full((h, w), self.unknownValue, np.uint8)
        if self.bands == 0 and self.background.shape[1:] != fr.shape[1:]:   # only _SB checks
            raise IllegalArgumentException("Image shapes do not match")
        mean, var = self.background[0::2], self.background[1::2]
        with np.errstate(all="ignore"):
            if self.bands == 0:
                diff = mean[0] - fr[0]
                chisq = diff * diff / var[0]
                far = (diff >= self.minimumDifference) | (-diff >= self.minimumDifference)
            else:
                chisq = np.zeros((h, w), np.float32)
                for b in range(self.numBands):
                    diff = mean[b] - fr[b]
                    chisq = chisq + diff * diff / var[b]
                if self.minimumDifference == 0:
                    far = np.ones((h, w), bool)
                else:
                    adjusted = self.minimumDifference * f32(self.numBands)
                    sumAbs = np.zeros((h, w), np.float32)
                    for b in range(self.numBands):
                        sumAbs = sumAbs + np.abs(mean[b] - fr[b])
                    far = sumAbs >= adjusted
            near = chisq <= self.threshold
        self.counts["nan"] += int(np.count_nonzero(np.isnan(chisq)))
        self.counts["inf"] += int(np.count_nonzero(np.isinf(chisq)))
        self.counts["within_threshold"] += int(np.count_nonzero(near))
        self.counts["beyond_far"] += int(np.count_nonzero(~near & far))
        self.counts["beyond_close"] += int(np.count_nonzero(~near & ~far))
        return np.where(near, 0, np.where(far, 1, 0)).astype(np.uint8)


class GmmCommon:
    """BackgroundGmmCommon.  dataRow is a 1-D float32 array (one row of model.data)."""

    def __init__(self, learningPeriod, decayCoef, maxGaussians, numBands):
        if learningPeriod <= 0:
            raise IllegalArgumentException("Must be greater than zero")
        if maxGaussians >= 256 or maxGaussians <= 0:
            raise IllegalArgumentException("Maximum number of gaussians per pixel is 255")
        self.learningRate = f32(1.0) / f32(learningPeriod)
        self.decay = f32(decayCoef)
        self.maxGaussians = int(maxGaussians)
        self.maxDistance = f32(3 * 3)
        self.significantWeight = min(f32(0.2), f32(100) * self.learningRate)
        self.initialVariance = f32(100)
        self.unknownValue = 0
        self.numBands = numBands
        self.gaussianStride = 2 + numBands
        self.modelStride = maxGaussians * self.gaussianStride
        self.counts = collections.Counter()

    def updateMixtureMB(self, pixelValue, dataRow, modelIndex):      # :112-183
        lr, stride, nb = self.learningRate, self.gaussianStride, self.numBands
        index = modelIndex
        bestDistance = self.maxDistance * f32(nb)
        bestIndex = -1
        ng = 0
        while ng < self.maxGaussians:
            variance = dataRow[index + 1]
            if variance <= 0:
                break
            mahalanobis = f32(0)
            for i in range(nb):
                mean = dataRow[index + 2 + i]
                delta = pixelValue[i] - mean
                mahalanobis = mahalanobis + delta * delta / variance
            if mahalanobis < bestDistance:
                bestDistance = mahalanobis
                bestIndex = index
            ng += 1
            index += stride
        if bestIndex != -1:
            weight = dataRow[bestIndex]
            variance = dataRow[bestIndex + 1]
            weight = weight + lr * (f32(1) - weight)
            dataRow[bestIndex] = 1
            sumDeltaSq = f32(0)
            for i in range(nb):
                mean = dataRow[bestIndex + 2 + i]
                delta = pixelValue[i] - mean
                dataRow[bestIndex + 2 + i] = mean + delta * lr / weight
                sumDeltaSq = sumDeltaSq + delta * delta
            sumDeltaSq = sumDeltaSq / f32(nb)
            dataRow[bestIndex + 1] = variance + (lr / weight) * (sumDeltaSq * f32(1.2) - variance)
            self.updateWeightAndPrune(dataRow, modelIndex, ng, bestIndex, weight)
            return self._matched(weight)
        return self._unmatched(pixelValue, dataRow, modelIndex, ng)

    def updateMixtureSB(self, pixelValue, dataRow, modelIndex):      # :240-304
        lr = self.learningRate
        index = modelIndex
        bestDistance = self.maxDistance
        bestIndex = -1
        ng = 0
        while ng < self.maxGaussians:
            variance = dataRow[index + 1]
            mean = dataRow[index + 2]
            if variance <= 0:
                break
            delta = pixelValue - mean
            mahalanobis = delta * delta / variance
            if mahalanobis < bestDistance:
                bestDistance = mahalanobis
                bestIndex = index
            ng += 1
            index += 3
        if bestDistance != self.maxDistance:
            weight = dataRow[bestIndex]
            variance = dataRow[bestIndex + 1]
            mean = dataRow[bestIndex + 2]
            delta = pixelValue - mean
            weight = weight + lr * (f32(1) - weight)
            dataRow[bestIndex] = 1
            dataRow[bestIndex + 1] = variance + (lr / weight) * (delta * delta * f32(1.2) - variance)
            dataRow[bestIndex + 2] = mean + delta * lr / weight
            self.updateWeightAndPrune(dataRow, modelIndex, ng, bestIndex, weight)
            return self._matched(weight)
        return self._unmatched([pixelValue], dataRow, modelIndex, ng)

    def _matched(self, weight):
        self.counts["match"] += 1
        if weight >= self.significantWeight:
            return 0
        self.counts["match_insignificant"] += 1
        return 1

    def _unmatched(self, pixelValue, dataRow, modelIndex, ng):
        if ng < self.maxGaussians:
            bestIndex = modelIndex + ng * self.gaussianStride
            dataRow[bestIndex] = 1
            dataRow[bestIndex + 1] = self.initialVariance
            for i in range(self.numBands):
                dataRow[bestIndex + 2 + i] = pixelValue[i]
            if ng == 0:
                self.counts["first_gaussian"] += 1
                return self.unknownValue
            self.counts["new_gaussian"] += 1
            self.updateWeightAndPrune(dataRow, modelIndex, ng + 1, bestIndex, self.learningRate)
            return 1
        self.counts["full"] += 1
        return 1

    def updateWeightAndPrune(self, dataRow, modelIndex, ng, bestIndex, bestWeight):   # :188-234
        stride = self.gaussianStride
        index = modelIndex
        weightTotal = f32(0)
        i = 0
        while i < ng:
            weight = dataRow[index]
            weight = weight - self.learningRate * (weight + self.decay)
            if weight <= 0:
                indexLast = modelIndex + (ng - 1) * stride
                for j in range(stride):
                    dataRow[index + j] = dataRow[indexLast + j]
                self.counts["prune"] += 1
                if indexLast == bestIndex:
                    bestIndex = index
                    if indexLast != index:
                        self.counts["prune_moves_best"] += 1
                dataRow[indexLast + 1] = 0
                ng -= 1
            else:
                dataRow[index] = weight
                weightTotal = weightTotal + weight
                index += stride
                i += 1
        if bestIndex != -1:
            weightTotal = weightTotal - dataRow[bestIndex]
            weightTotal = weightTotal + bestWeight
            dataRow[bestIndex] = bestWeight
        index = modelIndex
        for i in range(ng):
            dataRow[index] = dataRow[index] / weightTotal
            index += stride

    def checkBackground(self, pixelValue, dataRow, modelIndex, single):   # :311-375
        stride, nb = self.gaussianStride, self.numBands
        index = modelIndex
        bestDistance = self.maxDistance if single else self.maxDistance * f32(nb)
        bestWeight = f32(0)
        ng = 0
        while ng < self.maxGaussians:
            variance = dataRow[index + 1]
            if variance <= 0:
                break
            if single:
                delta = pixelValue[0] - dataRow[index + 2]
                mahalanobis = delta * delta / variance
            else:
                mahalanobis = f32(0)
                for i in range(nb):
                    delta = pixelValue[i] - dataRow[index + 2 + i]
                    mahalanobis = mahalanobis + delta * delta / variance
            if mahalanobis < bestDistance:
                bestDistance = mahalanobis
                bestWeight = dataRow[index]
            ng += 1
            index += stride
        if ng == 0:
            self.counts["check_unknown"] += 1
            return self.unknownValue
        self.counts["check_background" if bestWeight >= self.significantWeight else "check_foreground"] += 1
        return 0 if bestWeight >= self.significantWeight else 1


class GmmRef(_Model):
    """BackgroundStationaryGmm_SB (bands = 0) / _MB"""

    def __init__(self, learningPeriod, decayCoef, maxGaussians, bands=0):
        super().__init__(bands)
        self.common = GmmCommon(learningPeriod, decayCoef, maxGaussians, self.numBands)
        self.counts = self.common.counts
        self.imageWidth = self.imageHeight = 0
        self.model = np.zeros((0, 0), np.float32)    # common.model.data[row][col*modelStride + ...]

    def reset(self):
        self.model = np.zeros((0, 0), np.float32)
        self.imageWidth = self.imageHeight = 0

    def state(self):
        return self.model

    def updateBackground(self, frame, mask=False):
        fr = to_float(frame, self.bands)
        h, w = fr.shape[1:]
        c = self.common
        if self.imageWidth != w or self.imageHeight != h:
            self.imageWidth, self.imageHeight = w, h
            self.model = np.zeros((h, w * c.modelStride), np.float32)
        out = np.zeros((h, w), np.uint8) if mask else None
        with np.errstate(all="ignore"):
            for row in range(h):
                dataRow = self.model[row]
                for col in range(w):
                    if self.bands == 0:
                        r = c.updateMixtureSB(fr[0, row, col], dataRow, col * c.modelStride)
                    else:
                        r = c.updateMixtureMB(fr[:, row, col], dataRow, col * c.modelStride)
                    if mask:
                        out[row, col] = r & 255
        return out

    def segment(self, frame):
        fr = to_float(frame, self.bands)
        h, w = fr.shape[1:]
        c = self.common
        if self.imageWidth != w or self.imageHeight != h:
            return np.full((h, w), self.unknownValue, np.uint8)
        c.unknownValue = self.unknownValue
        out = np.zeros((h, w), np.uint8)
        with np.errstate(all="ignore"):
            for row in range(h):
                dataRow = self.model[row]
                for col in range(w):
                    out[row, col] = c.checkBackground(fr[:, row, col], dataRow, col * c.modelStride, self.bands == 0) & 255
        return out


# ---- FactoryBackgroundModel + ConfigBackground* (restated for the reference checks; the product's own mirrors are in boofcv_amd.api) ----
def stationaryBasic(learnRate, threshold, bands):
    if learnRate < 0 or learnRate > 1:
        raise IllegalArgumentException("Learn rate must be 0 <= rate <= 1")
    if threshold <= 0:
        raise IllegalArgumentException("threshold must be > 0")
    return BasicRef(learnRate, threshold, bands)                  # config.unknownValue is not forwarded


def stationaryGaussian(learnRate, threshold, bands, initialVariance=FLOAT_MIN_VALUE, minimumDifference=0, unknownValue=0):
    if learnRate < 0 or learnRate > 1:
        raise IllegalArgumentException("Learn rate must be 0 <= rate <= 1")
    if threshold <= 0:
        raise IllegalArgumentException("threshold must be > 0")
    if initialVariance == 0:
        raise IllegalArgumentException("Don't set initialVariance to zero, set it to Float.MIN_VALUE instead")
    if initialVariance < 0:
        raise IllegalArgumentException("Variance must be set to a value larger than zero")
    if minimumDifference < 0:
        raise IllegalArgumentException("minimumDifference must be >= 0")
    m = GaussianRef(learnRate, threshold, bands)
    m.initialVariance = f32(initialVariance)
    m.minimumDifference = f32(minimumDifference)
    m.setUnknownValue(unknownValue)
    return m


def stationaryGmm(bands, learningPeriod=1000.0, initialVariance=400, decayCoefient=0.005, maxDistance=3, numberOfGaussian=5, significantWeight=0.01,
                  unknownValue=0):
    if learningPeriod <= 0:
        raise IllegalArgumentException("Learning period must be more than zero")
    if decayCoefient < 0:
        raise IllegalArgumentException("Decay coeffient must be more than or equal to zero")
    if initialVariance == 0:
        raise IllegalArgumentException("Don't set initialVariance to zero, set it to Float.MIN_VALUE instead")
    if initialVariance < 0:
        raise IllegalArgumentException("Variance must be set to a value larger than zero")
    m = GmmRef(learningPeriod, decayCoefient, numberOfGaussian, bands)
    m.common.initialVariance = f32(initialVariance)
    m.common.maxDistance = f32(maxDistance)
    m.common.significantWeight = f32(significantWeight)
    m.setUnknownValue(unknownValue)
    return m


def run_sequence(model, frames, masks=True):
    """updateBackground(frame_t[, mask_t]) for every frame -> [T][h][w] masks (or None)"""
    out = [model.updateBackground(f, masks) for f in frames]
    return np.stack(out) if masks else None
