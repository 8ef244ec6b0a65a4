"""NumPy reference of five-region block matching (FactoryStereoDisparity.blockMatchBest5) on GrayU8 pairs, written from the Java line by line.

    F: = main/boofcv-feature/src/main/java/boofcv/

  compare()             SelectErrorWithChecks_S32.compare                          F:alg/feature/disparity/block/select/SelectErrorWithChecks_S32.java:165-167
  score_five_scalar()   DisparityScoreBMBestFive_S32.computeScoreFive, as written  F:alg/feature/disparity/block/score/DisparityScoreBMBestFive_S32.java:225-267
  score_five()          the same three branches on whole index arrays (np.where)
  rolling_scores()      computeFirstRow / computeRemainingRows: the rolling windows horizontalScore / verticalScore, activeVerticalScore   :147-219
  block_match_best5()   FactoryStereoDisparity.blockMatchBest5 (SAD and CENSUS) -> WrapBaseBlockMatch.process on a freshly constructed object,
                        single threaded (BoofConcurrency.USE_CONCURRENT = false: one block over all rows)
                        F:factory/feature/disparity/FactoryStereoDisparity.java:146-201; the selector is configured with radius 2*rx (:121)
  naive_five()          the definition: four loops per sub-block, the two smallest of the four corner blocks
  region_scores()       the definition on the scores of plain block matching, with the rule exchangeable ("best2" is the reference's; "all4" and
                        "worst2" are the wrong functions tests/test_best5_reference.py tells it from)

Row scores and the selector are those of plain block matching: disparity_ref.score_row / select_row, census_ref.score_row.
Scores are in the Java layout: scores[W*i + (c - minDisparity)].

A fact of the reference this file keeps: computeFirstRow selects nothing and computeRemainingRows starts at image row regionHeight, so the first
selected row is max(2*ry, 1) -- with ry = 0 row 0 stays at the fill value, where plain block matching selects it in its computeFirstRow."""
import numpy as np

import census_ref as cr
import disparity_ref as dr


def compare(scoreA, scoreB):
    """Integer.compare(-scoreA, -scoreB)"""
    a, b = -int(scoreA), -int(scoreB)
    return -1 if a < b else 1 if a > b else 0


def score_five_scalar(top, middle, bottom, score, width, minDisparity, maxDisparity, radiusX):
    """computeScoreFive, statement by statement"""
    for d in range(minDisparity, maxDisparity):
        indexSrc = (d - minDisparity) * width + (d - minDisparity) + radiusX
        indexDst = (d - minDisparity) * width + (d - minDisparity)
        end = indexSrc + (width - d - 4 * radiusX)
        while indexSrc < end:
            val0 = top[indexSrc - radiusX]
            val1 = top[indexSrc + radiusX]
            val2 = bottom[indexSrc - radiusX]
            val3 = bottom[indexSrc + radiusX]
            if compare(val0, val1) < 0:
                val0, val1 = val1, val0
            if compare(val2, val3) < 0:
                val2, val3 = val3, val2
            if compare(val0, val3) < 0:
                s = val2 + val3
            elif compare(val1, val2) < 0:
                s = val2 + val0
            else:
                s = val0 + val1
            score[indexDst] = s + middle[indexSrc]
            indexDst += 1
            indexSrc += 1


def _five_indices(width, minDisparity, maxDisparity, radiusX):
    src, dst = [], []
    for d in range(minDisparity, maxDisparity):
        indexSrc = (d - minDisparity) * width + (d - minDisparity) + radiusX
        indexDst = (d - minDisparity) * width + (d - minDisparity)
        n = max(width - d - 4 * radiusX, 0)
        src.append(np.arange(indexSrc, indexSrc + n))
        dst.append(np.arange(indexDst, indexDst + n))
    return np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)


def score_five(top, middle, bottom, score, width, minDisparity, maxDisparity, radiusX):
    """computeScoreFive on all (d, index) at once; compare(a, b) < 0 is a > b"""
    src, dst = _five_indices(width, minDisparity, maxDisparity, radiusX)
    val0, val1 = top[src - radiusX], top[src + radiusX]
    val2, val3 = bottom[src - radiusX], bottom[src + radiusX]
    swap = val0 > val1                                   # compare(val0, val1) < 0
    val0, val1 = np.where(swap, val1, val0), np.where(swap, val0, val1)
    swap = val2 > val3                                   # compare(val2, val3) < 0
    val2, val3 = np.where(swap, val3, val2), np.where(swap, val2, val3)
    s = np.where(val0 > val3, val2 + val3,               # compare(val0, val3) < 0
                 np.where(val1 > val2, val2 + val0,      # compare(val1, val2) < 0
                          val0 + val1))
    score[dst] = s + middle[src]


def rolling_scores(score_row, H, W, minDisparity, maxDisparity, rx, ry, five=score_five):
    """DisparityScoreBMBestFive_S32.ComputeBlock.accept(workspace, 0, H) -> {y: fiveScore as the selector gets it for output row y}.
    score_row(row) -> the horizontal scores of an image row (BlockRowScore.scoreRow)."""
    regionWidth, regionHeight = 2 * rx + 1, 2 * ry + 1
    lengthHorizontal = W * (maxDisparity - minDisparity)
    row0, row1 = 0, H                                    # max(0, 0 - 2*radiusY), min(height, height + 2*radiusY)
    horizontalScore = [None] * regionHeight
    verticalScore = [np.zeros(lengthHorizontal, np.int64) for _ in range(regionHeight)]
    fiveScore = np.zeros(lengthHorizontal, np.int64)
    out = {}
    # computeFirstRow
    activeVerticalScore = 1
    for row in range(regionHeight):
        horizontalScore[row] = score_row(row0 + row)
    verticalScore[0] = np.sum(horizontalScore, axis=0)
    # computeRemainingRows
    for row in range(row0 + regionHeight, row1):
        activeIndex = activeVerticalScore % regionHeight
        oldRow = (row - row0) % regionHeight
        previous = verticalScore[(activeVerticalScore - 1) % regionHeight]
        active = previous - horizontalScore[oldRow]      # subtract first row from vertical score
        horizontalScore[oldRow] = score_row(row)
        active = active + horizontalScore[oldRow]        # add the new score
        verticalScore[activeIndex] = active
        if activeVerticalScore >= regionHeight - 1:
            top = verticalScore[(activeVerticalScore - 2 * ry) % regionHeight]
            middle = verticalScore[(activeVerticalScore - ry) % regionHeight]
            bottom = verticalScore[activeVerticalScore % regionHeight]
            five(top, middle, bottom, fiveScore, W, minDisparity, maxDisparity, rx)
            out[row - (1 + 4 * ry) + 2 * ry + 1] = fiveScore.copy()
        activeVerticalScore += 1
    return out


def max_error(rx, ry, maxPerPixelError):
    """double maxError = rw*rh*maxPerPixelError; maxError *= 3; (int)maxError"""
    maxError = (rx * 2 + 1) * (ry * 2 + 1) * float(maxPerPixelError)
    maxError *= 3
    return dr.java_d2i(maxError)


def _check(W, H, minDisparity, rangeDisparity, rx, ry):
    if minDisparity < 0:
        raise ValueError("miDisparity < 0")
    if rangeDisparity < 1:
        raise ValueError("rangeDisparity < 1")
    if minDisparity + rangeDisparity > W - 2 * rx:       # DisparityBlockMatchRowFormat.process: radiusX, not 2*radiusX
        raise ValueError("The maximum disparity is too large for this image size: max size %d" % (W - 2 * rx))
    if H < 2 * ry + 1:
        raise ValueError("the image is lower than the region")       # the reference indexes outside the image


def row_scorer(left, right, minDisparity, maxDisparity, rx, variant=None):
    """-> (score_row(row), the images it scores): SAD on the pair, or the Hamming distance on its census images"""
    if variant is None:
        return (lambda row: dr.score_row(left, right, row, minDisparity, maxDisparity, 2 * rx + 1)), (left, right)
    cl, cright = cr.census_variant(left, variant), cr.census_variant(right, variant)   # WrapDisparityBlockMatchCensus._process
    return (lambda row: cr.score_row(cl, cright, row, minDisparity, maxDisparity, 2 * rx + 1)), (cl, cright)


def select_all(scores_by_row, W, H, minDisparity, rangeDisparity, rx, ry, maxPerPixelError, validateRtoL, texture, subpixel, mask16=False):
    """the selector of blockMatchBest5 (radius 2*rx, three regions' maxError) on {y: scores} -> (disparity, class map)"""
    disp = np.full((H, W), rangeDisparity, np.float32 if subpixel else np.uint8)      # GImageMiscOps.fill(disparity, getInvalidValue())
    cls = np.full((H, W), dr.BORDER, np.uint8)
    for y, scores in scores_by_row.items():
        if mask16:
            scores = scores & 0xFFFF                     # what a 16-bit score would hold
        dr.select_row(scores, W, minDisparity, minDisparity + rangeDisparity, 2 * rx, max_error(rx, ry, maxPerPixelError), validateRtoL, texture, subpixel,
                      disp[y], cls[y])
    return disp, cls


def block_match_best5(left, right, minDisparity=0, rangeDisparity=100, regionRadiusX=3, regionRadiusY=3, maxPerPixelError=0.0, validateRtoL=1, texture=0.15,
                      subpixel=True, variant=None):
    """FactoryStereoDisparity.blockMatchBest5(config, GrayU8, GrayU8 | GrayF32).process(left, right) on a new object -> (disparity [H, W] uint8
    or float32, class map [H, W] uint8).  variant None: errorType = SAD; a census_ref variant name: errorType = CENSUS.  ValueError where the
    reference throws."""
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    H, W = left.shape
    if minDisparity >= 0 and rangeDisparity >= 1 and variant is not None:
        cr.census_variant(left, variant)                 # the transform runs first and has its own size rule
    _check(W, H, minDisparity, rangeDisparity, regionRadiusX, regionRadiusY)
    maxDisparity = minDisparity + rangeDisparity
    score_row, _ = row_scorer(left, right, minDisparity, maxDisparity, regionRadiusX, variant)
    rows = rolling_scores(score_row, H, W, minDisparity, maxDisparity, regionRadiusX, regionRadiusY)
    return select_all(rows, W, H, minDisparity, rangeDisparity, regionRadiusX, regionRadiusY, maxPerPixelError, validateRtoL, texture, subpixel)


def naive_five(left, right, y, col, i, minDisparity, rx, ry, cost=dr.naive_cost):
    """F(y, col, i) from the definition: the centre block at column col + rx, plus the two smallest of the four blocks at rows y -+ ry,
    columns col and col + 2*rx; every block by four loops"""
    corners = sorted(cost(left, right, yy, cc, i, minDisparity, rx, ry) for yy in (y - ry, y + ry) for cc in (col, col + 2 * rx))
    return cost(left, right, y, col + rx, i, minDisparity, rx, ry) + corners[0] + corners[1]


def region_scores(V, W, H, minDisparity, maxDisparity, rx, ry, rule="best2"):
    """{y: five-region scores} from V = {y: scores of plain block matching} (disparity_ref.sad_scores), rows 2*ry .. H-2*ry-1, by the definition.
    rule: which corner blocks join the centre -- "best2" the two smallest (the reference), "worst2" the two largest, "all4" all four."""
    rng = maxDisparity - minDisparity
    out = {}
    n = W - minDisparity - 4 * rx                        # selector columns; entry (i, k) exists for i <= k < n
    k = np.arange(max(n, 0))
    for y in range(2 * ry, H - 2 * ry):
        t, m, b = (V[yy].reshape(rng, W) for yy in (y - ry, y, y + ry))
        F = np.zeros((rng, W), np.int64)
        if n > 0:
            corners = np.sort(np.stack([t[:, k], t[:, k + 2 * rx], b[:, k], b[:, k + 2 * rx]]), axis=0)
            add = {"best2": corners[0] + corners[1], "worst2": corners[2] + corners[3], "all4": corners.sum(axis=0)}[rule]
            F[:, :n] = np.where(k[None, :] >= np.arange(rng)[:, None], m[:, k + rx] + add, 0)
        out[y] = F.reshape(-1)
    return out
