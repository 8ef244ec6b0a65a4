"""NumPy reference of the census transform and of census block matching on GrayU8 images, written from the Java line by line.

    I: = main/boofcv-ip/src/main/java/boofcv/        F: = main/boofcv-feature/src/main/java/boofcv/

  create_block_samples(), create_circle_samples()   CensusTransform.createBlockSamples / createCircleSamples   I:alg/transform/census/CensusTransform.java:53-98
  variant_samples()        FactoryCensusTransform.variant / blockDense                   I:factory/transform/census/FactoryCensusTransform.java:48-93
  reflect()                BorderIndex1D_Reflect.getIndex                                I:core/image/border/BorderIndex1D_Reflect.java:34-41
  java_bit()               `int bit = 1; ...; bit <<= 1` after i shifts, as the long that `census |= bit` ORs in
  census_pixel()           ImplCensusTransformBorder.regionNxN / sample_S64 on one pixel (the inner loops of ImplCensusTransformInner compute
                           the same thing where no index is reflected)                   I:alg/transform/census/impl/
  census()                 the whole image, vectorised over pixels, one sample at a time in the Java order
  hamming()                DescriptorDistance.hamming(int) / hamming(long)               F:alg/descriptor/DescriptorDistance.java:213-224
  score_row(), census_scores()   BlockRowScore.ArrayS32.scoreRow with BlockRowScoreCensus.U8 / S32 / S64.score, DisparityScoreBM_S32
                           F:alg/feature/disparity/block/BlockRowScore.java:96-138, BlockRowScoreCensus.java:39-85
  block_match()            FactoryStereoDisparity.blockMatch (CENSUS) -> WrapDisparityBlockMatchCensus._process on a freshly constructed object;
                           selection is disparity_ref.select_row, unchanged             F:factory/feature/disparity/FactoryStereoDisparity.java:85-102

The GrayS64 words: `long census; int bit = 1; census |= bit; bit <<= 1` -- samples 0..30 set bits 0..30, sample 31 ORs in 0x80000000 sign-extended
(bits 31..63), samples 32 and up add nothing.
"""
import numpy as np

import disparity_ref as dr

VARIANTS = ("BLOCK_3_3", "BLOCK_5_5", "BLOCK_7_7", "BLOCK_9_7", "BLOCK_13_5", "CIRCLE_9")   # CensusVariants, by ordinal
WORD_DTYPE = {"BLOCK_3_3": np.uint8, "BLOCK_5_5": np.int32}                                  # the others: np.int64


def create_block_samples(radiusX, radiusY=None):
    radiusY = radiusX if radiusY is None else radiusY
    samples = []
    for y in range(-radiusY, radiusY + 1):
        for x in range(-radiusX, radiusX + 1):
            if x == 0 and y == 0:
                continue
            samples.append((x, y))
    return samples


def create_circle_samples():
    samples = []
    for row in range(9):
        col0 = max(0, 3 - row) if row <= 4 else row - 5
        col1 = 9 - col0
        for col in range(col0, col1):
            if row == 4 and col == 4:
                continue
            samples.append((row - 4, col - 4))       # set(row-4, col-4): the row is x
    return samples


def variant_samples(variant):
    return {"BLOCK_3_3": lambda: create_block_samples(1), "BLOCK_5_5": lambda: create_block_samples(2), "BLOCK_7_7": lambda: create_block_samples(3),
            "BLOCK_9_7": lambda: create_block_samples(4, 3), "BLOCK_13_5": lambda: create_block_samples(5, 2), "CIRCLE_9": create_circle_samples}[variant]()


def word_dtype(variant):
    return WORD_DTYPE.get(variant, np.int64)


def sample_radius(samples):
    """sample_S64: the largest |x| or |y|"""
    radius = 0
    for x, y in samples:
        radius = max(radius, abs(x))
        radius = max(radius, abs(y))
    return radius


def reflect(index, length):
    if index < 0:
        return -index
    if index >= length:
        return length - 2 - (index - length)
    return index


def java_bit(i):
    """the int `bit` after i times `bit <<= 1`, widened to long"""
    return dr.i32(1 << i) if i < 32 else 0


def census_pixel(img, cx, cy, samples):
    """one word as a Python int (a Java long; the dense forms stay below 2^24)"""
    H, W = img.shape
    center = int(img[cy][cx])
    census = 0
    for i, (x, y) in enumerate(samples):
        if int(img[reflect(cy + y, H)][reflect(cx + x, W)]) > center:
            census |= java_bit(i)                    # Python's | on a negative int is two's complement, like Java's
    return census


def census(img, samples, dtype=np.int64):
    """the transform of a whole image with the REFLECT border -> [H, W] dtype.  Needs W, H >= radius + 1 (ValueError below that: the reference
    throws or writes outside the image)."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    radius = sample_radius(samples)
    if W < radius + 1 or H < radius + 1:
        raise ValueError("the image is smaller than radius + 1")
    ys = np.array([[reflect(y + d, H) for y in range(H)] for d in range(-radius, radius + 1)])   # [d + radius][y]
    xs = np.array([[reflect(x + d, W) for x in range(W)] for d in range(-radius, radius + 1)])
    center = img.astype(np.int64)
    out = np.zeros((H, W), np.int64)
    for i, (x, y) in enumerate(samples):
        bit = java_bit(i)
        if bit == 0:
            continue
        out |= np.where(img[ys[y + radius]][:, xs[x + radius]].astype(np.int64) > center, np.int64(bit), np.int64(0))
    if dtype == np.uint8:
        return (out & 0xFF).astype(np.uint8)         # (byte)census
    return out.astype(dtype)


def census_variant(img, variant):
    return census(img, variant_samples(variant), word_dtype(variant))


def hamming(v):
    """DescriptorDistance.hamming(int) on int32 / uint8-as-int values, hamming(long) on int64: the number of set bits of the two's complement word"""
    v = np.ascontiguousarray(v)
    if v.dtype == np.uint8:
        v = v.astype(np.int32)
    assert v.dtype in (np.int32, np.int64)
    nbytes = v.dtype.itemsize
    return np.unpackbits(v.reshape(-1).view(np.uint8).reshape(-1, nbytes), axis=1).sum(axis=1).astype(np.int64).reshape(v.shape)


def score_row(cleft, cright, row, minDisparity, maxDisparity, regionWidth):
    """disparity_ref.score_row with BlockRowScoreCensus.*.score as the element score"""
    W = cleft.shape[1]
    scores = np.zeros(W * (maxDisparity - minDisparity), np.int64)
    L, R = cleft[row], cright[row]
    for d in range(minDisparity, maxDisparity):
        dispFromMin = d - minDisparity
        colMax = W - d
        scoreMax = colMax - regionWidth
        indexScore = W * dispFromMin + dispFromMin
        elementScore = hamming(L[d:d + colMax] ^ R[:colMax])
        cs = np.concatenate(([0], np.cumsum(elementScore)))
        scores[indexScore:indexScore + scoreMax + 1] = cs[regionWidth:regionWidth + scoreMax + 1] - cs[:scoreMax + 1]
    return scores


def census_scores(cleft, cright, minDisparity, maxDisparity, rx, ry):
    """DisparityScoreBM_S32 on the census images: {y: verticalScore of output row y} (as disparity_ref.sad_scores)"""
    H = cleft.shape[0]
    rw, rh = 2 * rx + 1, 2 * ry + 1
    horizontal = [score_row(cleft, cright, row, minDisparity, maxDisparity, rw) for row in range(H)]
    out = {}
    vertical = np.sum(horizontal[:rh], axis=0)
    out[ry] = vertical.copy()
    for row in range(rh, H):
        vertical = vertical - horizontal[row - rh] + horizontal[row]
        out[row - rh + 1 + ry] = vertical.copy()
    return out


def naive_cost(cleft, cright, y, c, i, minDisparity, rx, ry):
    """C(y, c, i) on census images, four loops"""
    total = 0
    for dy in range(-ry, ry + 1):
        for j in range(2 * rx + 1):
            total += bin((int(cleft[y + dy][c + j]) ^ int(cright[y + dy][c - minDisparity - i + j])) & 0xFFFFFFFFFFFFFFFF).count("1")
    return total


def block_match(left, right, variant="BLOCK_5_5", minDisparity=0, rangeDisparity=100, regionRadiusX=3, regionRadiusY=3, maxPerPixelError=0.0, validateRtoL=1,
                texture=0.15, subpixel=True):
    """FactoryStereoDisparity.blockMatch(config with errorType = CENSUS, GrayU8, GrayU8 | GrayF32).process(left, right) on a new object ->
    (disparity [H, W] uint8 or float32, class map [H, W] uint8).  Raises ValueError where the reference throws."""
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    H, W = left.shape
    if minDisparity < 0:
        raise ValueError("miDisparity < 0")
    if rangeDisparity < 1:
        raise ValueError("rangeDisparity < 1")
    maxDisparity = minDisparity + rangeDisparity
    cleft, cright = census_variant(left, variant), census_variant(right, variant)        # WrapDisparityBlockMatchCensus._process
    if maxDisparity > W - 2 * regionRadiusX:
        raise ValueError("The maximum disparity is too large for this image size: max size %d" % (W - 2 * regionRadiusX))
    if H < 2 * regionRadiusY + 1:
        raise ValueError("the image is lower than the region")
    maxError = dr.java_d2i((regionRadiusX * 2 + 1) * (regionRadiusY * 2 + 1) * maxPerPixelError)
    disp = np.full((H, W), rangeDisparity, np.float32 if subpixel else np.uint8)
    cls = np.full((H, W), dr.BORDER, np.uint8)
    for y, scores in census_scores(cleft, cright, minDisparity, maxDisparity, regionRadiusX, regionRadiusY).items():
        dr.select_row(scores, W, minDisparity, maxDisparity, regionRadiusX, maxError, validateRtoL, texture, subpixel, disp[y], cls[y])
    return disp, cls
