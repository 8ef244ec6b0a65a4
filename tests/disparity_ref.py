"""NumPy reference of dense stereo disparity by SAD block matching on GrayU8 pairs, written from the Java line by line.

    F: = main/boofcv-feature/src/main/java/boofcv/

  sad_scores()     BlockRowScore.ArrayS32.scoreRow + BlockRowScoreSad.U8.score   F:alg/feature/disparity/block/BlockRowScore.java:96-138, BlockRowScoreSad.java:53-67
                   DisparityScoreBM_S32.computeFirstRow / computeRemainingRows   F:alg/feature/disparity/block/score/DisparityScoreBM_S32.java:141-205
  naive_cost()     the definition the running sums implement (four loops)
  select_row()     SelectErrorWithChecks_S32.process / selectRightToLeft         F:alg/feature/disparity/block/select/SelectErrorWithChecks_S32.java:73-162
                   DispU8.setDisparity :187-189; SelectErrorSubpixel.S32_F32.setDisparity   block/select/SelectErrorSubpixel.java:56-69
  set_disparity_subpixel()   SelectErrorSubpixel.S32_F32.setDisparity with a given columnScore / localMaxDisparity
  block_match()    FactoryStereoDisparity.blockMatch (SAD) -> WrapBaseBlockMatch.process on a freshly constructed object
                   F:factory/feature/disparity/FactoryStereoDisparity.java:62-83,116-144,230-240; F:abst/feature/disparity/WrapBaseBlockMatch.java:42-53
  stereo_scene()   the image pairs of tests/test_gpu_disparity.py (not from the reference)

Scores are in the Java layout: scores[W*i + (c - minDisparity)] is the cost of the left block that starts at column c at disparity minDisparity + i.
"""
import numpy as np

INT_MAX = 2147483647
DISCRETIZER = 10000

# class map of block_match / select_row
BORDER, VALID_INT, REJECT_ERROR, REJECT_RTOL, REJECT_TEXTURE, VALID_INTERP = range(6)
CLASS_NAMES = ("border", "valid integer", "rejected by max error", "rejected right to left", "rejected by texture", "valid interpolated")


def i32(v):
    """a Java int: the low 32 bits of v as two's complement"""
    return ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31


def java_d2i(v):
    """Java's (int) of a double: toward zero, saturating, NaN -> 0"""
    if v != v:
        return 0
    if v >= INT_MAX:
        return INT_MAX
    if v <= -INT_MAX - 1:
        return -INT_MAX - 1
    return int(v)


def naive_cost(left, right, y, c, i, minDisparity, rx, ry):
    """C(y, c, i): left block starting at column c, rows y-ry .. y+ry, against the right block starting at c - minDisparity - i"""
    total = 0
    for dy in range(-ry, ry + 1):
        for j in range(2 * rx + 1):
            total += abs(int(left[y + dy][c + j]) - int(right[y + dy][c - minDisparity - i + j]))
    return total


def score_row(left, right, row, minDisparity, maxDisparity, regionWidth):
    """BlockRowScore.ArrayS32.scoreRow: the horizontal scores of one image row, int64 [W * rangeDisparity] (entries it does not write are 0)"""
    W = left.shape[1]
    scores = np.zeros(W * (maxDisparity - minDisparity), np.int64)
    L, R = left[row].astype(np.int64), right[row].astype(np.int64)
    for d in range(minDisparity, maxDisparity):
        dispFromMin = d - minDisparity
        colMax = W - d
        scoreMax = colMax - regionWidth
        indexScore = W * dispFromMin + dispFromMin
        elementScore = np.abs(L[d:d + colMax] - R[:colMax])          # BlockRowScoreSad.U8.score
        cs = np.concatenate(([0], np.cumsum(elementScore)))          # score += elementScore[col+regionWidth] - elementScore[col]
        scores[indexScore:indexScore + scoreMax + 1] = cs[regionWidth:regionWidth + scoreMax + 1] - cs[:scoreMax + 1]
    return scores


def sad_scores(left, right, minDisparity, maxDisparity, rx, ry):
    """DisparityScoreBM_S32 (one block, rows 0 .. H): {y: verticalScore of output row y}, y = ry .. H-ry-1, each int64 [W * rangeDisparity]"""
    H = left.shape[0]
    rw, rh = 2 * rx + 1, 2 * ry + 1
    horizontal = [score_row(left, right, row, minDisparity, maxDisparity, rw) for row in range(H)]
    out = {}
    vertical = np.sum(horizontal[:rh], axis=0)                       # computeFirstRow
    out[ry] = vertical.copy()
    for row in range(rh, H):                                         # computeRemainingRows
        vertical = vertical - horizontal[row - rh] + horizontal[row]
        out[row - rh + 1 + ry] = vertical.copy()
    return out


def set_disparity_subpixel(columnScore, localMaxDisparity, disparityValue):
    """SelectErrorSubpixel.S32_F32.setDisparity -> (float32 value, interpolated?)"""
    if disparityValue <= 0 or disparityValue >= localMaxDisparity - 1:
        return np.float32(disparityValue), False
    c0, c1, c2 = int(columnScore[disparityValue - 1]), int(columnScore[disparityValue]), int(columnScore[disparityValue + 1])
    offset = np.float32(c0 - c2) / np.float32(i32(2 * (c0 - 2 * c1 + c2)))
    return np.float32(np.float32(disparityValue) + offset), True


def select_right_to_left(col, scores, imageWidth, regionWidth, minDisparity, maxDisparity):
    localMax = min(imageWidth - regionWidth, col + maxDisparity) - col - minDisparity
    indexBest = 0
    scoreBest = scores[col]
    if localMax > 1:
        idx = col + (imageWidth + 1) * np.arange(1, localMax)
        s = scores[idx]
        j = int(np.argmin(s))            # first minimum
        if s[j] < scoreBest:
            indexBest = j + 1
    return indexBest


def select_row(scores, imageWidth, minDisparity, maxDisparity, radiusX, maxError, rightToLeftTolerance, texture, subpixel, out, cls=None):
    """SelectErrorWithChecks_S32.process(row, scores) into out (a row of the disparity image: uint8 when not subpixel, float32 otherwise) and
    cls (a row of the class map).  maxError, rightToLeftTolerance, texture: the selector's constructor arguments."""
    scores = np.asarray(scores, np.int64)
    maxError = INT_MAX if maxError <= 0 else maxError                # SelectDisparityWithChecksWta constructor
    textureThreshold = java_d2i(DISCRETIZER * texture)               # setTexture
    rangeDisparity = maxDisparity - minDisparity
    regionWidth = radiusX * 2 + 1
    invalidDisparity = rangeDisparity + 1
    if invalidDisparity > (255 if not subpixel else 3.4028234663852886e38) - 1:
        raise ValueError("Max range exceeds maximum value in disparity image. v=%d" % invalidDisparity)
    for col in range(minDisparity, imageWidth - regionWidth + 1):
        localMaxDisparity = 1 + col - minDisparity - max(0, col - maxDisparity + 1)      # maxDisparityAtColumnL2R
        indexScore = col - minDisparity
        columnScore = scores[indexScore + imageWidth * np.arange(localMaxDisparity)]
        bestDisparity = int(np.argmin(columnScore))                                       # first strict minimum
        scoreBest = int(columnScore[bestDisparity])
        kind = VALID_INT
        if scoreBest > maxError:
            bestDisparity, kind = invalidDisparity, REJECT_ERROR
        elif rightToLeftTolerance >= 0:
            disparityRtoL = select_right_to_left(col - bestDisparity - minDisparity, scores, imageWidth, regionWidth, minDisparity, maxDisparity)
            if abs(disparityRtoL - bestDisparity) > rightToLeftTolerance:
                bestDisparity, kind = invalidDisparity, REJECT_RTOL
        if textureThreshold > 0 and bestDisparity != invalidDisparity and localMaxDisparity >= 3:
            secondBest = INT_MAX
            if bestDisparity - 1 > 0:
                secondBest = min(secondBest, int(columnScore[:bestDisparity - 1].min()))
            if bestDisparity + 2 < localMaxDisparity:
                secondBest = min(secondBest, int(columnScore[bestDisparity + 2:].min()))
            if i32(DISCRETIZER * i32(secondBest - scoreBest)) <= i32(textureThreshold * scoreBest):
                bestDisparity, kind = invalidDisparity, REJECT_TEXTURE
        x = col + radiusX
        if subpixel:
            out[x], interpolated = set_disparity_subpixel(columnScore, localMaxDisparity, bestDisparity)
            if interpolated:
                kind = VALID_INTERP
        else:
            out[x] = bestDisparity & 0xFF                                                 # (byte)value
        if cls is not None:
            cls[x] = kind


def block_match(left, right, minDisparity=0, rangeDisparity=100, regionRadiusX=3, regionRadiusY=3, maxPerPixelError=0.0, validateRtoL=1, texture=0.15,
                subpixel=True):
    """FactoryStereoDisparity.blockMatch(config, GrayU8, GrayU8 | GrayF32).process(left, right) on a new object -> (disparity [H, W] uint8 or
    float32, class map [H, W] uint8).  Raises ValueError where the reference throws."""
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    H, W = left.shape
    if minDisparity < 0:
        raise ValueError("miDisparity < 0")
    if rangeDisparity < 1:
        raise ValueError("rangeDisparity < 1")
    maxDisparity = minDisparity + rangeDisparity
    if maxDisparity > W - 2 * regionRadiusX:
        raise ValueError("The maximum disparity is too large for this image size: max size %d" % (W - 2 * regionRadiusX))
    if H < 2 * regionRadiusY + 1:
        raise ValueError("the image is lower than the region")       # the reference indexes outside the image
    maxError = java_d2i((regionRadiusX * 2 + 1) * (regionRadiusY * 2 + 1) * maxPerPixelError)
    disp = np.full((H, W), rangeDisparity, np.float32 if subpixel else np.uint8)          # GImageMiscOps.fill(disparity, getInvalidValue())
    cls = np.full((H, W), BORDER, np.uint8)
    for y, scores in sad_scores(left, right, minDisparity, maxDisparity, regionRadiusX, regionRadiusY).items():
        select_row(scores, W, minDisparity, maxDisparity, regionRadiusX, maxError, validateRtoL, texture, subpixel, disp[y], cls[y])
    return disp, cls


def class_counts(cls):
    return [int((cls == k).sum()) for k in range(6)]


def stereo_scene(W, H, minDisparity, rangeDisparity, seed):
    """-> (left, right) uint8 [H, W].  The left image is lightly smoothed noise with a low-texture stripe (rows around H/3) and a stripe holding a
    horizontally repeated pattern (rows around 2H/3); the right image is the scene resampled with a disparity that grows with x and y, plus
    noise in [-3, 3]."""
    rng = np.random.RandomState(seed)
    span = W + minDisparity + rangeDisparity + 8
    scene = rng.randint(0, 256, (H, span)).astype(np.float64)
    scene = (scene + np.roll(scene, 1, axis=1) + np.roll(scene, 1, axis=0)) / 3.0
    flat0, flat1 = H // 3 - 1, H // 3 + 3
    scene[flat0:flat1] = 120.0 + rng.randint(-2, 3, (flat1 - flat0, span))
    rep0, rep1 = 2 * H // 3 - 1, 2 * H // 3 + 3
    pattern = rng.randint(40, 216, (rep1 - rep0, 6)).astype(np.float64)
    scene[rep0:rep1] = np.tile(pattern, (1, span // 6 + 1))[:, :span]
    ys, xs = np.mgrid[0:H, 0:W]
    top = minDisparity + 0.45 * min(rangeDisparity, W // 3)
    d = minDisparity + (top - minDisparity) * np.maximum(0.75 * xs / W + 0.25 * ys / H - 0.12, 0.0)   # minDisparity itself on the left
    pos = xs + d                              # right pixel x shows scene position x + d: the left pixel x + d, i.e. disparity d
    x0 = np.floor(pos).astype(int)
    f = pos - x0
    rightf = scene[ys, x0] * (1 - f) + scene[ys, x0 + 1] * f + rng.randint(-3, 4, (H, W))
    left = np.clip(np.rint(scene[:, :W]), 0, 255).astype(np.uint8)
    right = np.clip(np.rint(rightf), 0, 255).astype(np.uint8)
    return left, right
