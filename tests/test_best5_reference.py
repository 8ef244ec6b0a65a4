"""CPU: tests/best5_ref.py, the line-by-line restatement of FactoryStereoDisparity.blockMatchBest5, against the definition; the cases of the GPU
tests are not vacuous (they tell the five-region rule from its neighbours, hold every pixel class and pass 16 bits); the Python mirror's
factory; the C entry points."""
import re
from pathlib import Path

import numpy as np
import pytest

import best5_cases as bc
import best5_ref as b5
import disparity_ref as dr

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ["bhip_disparity_bm5_u8_u8", "bhip_disparity_bm5_u8_f32", "bhip_disparity_bm5_dev_u8_u8", "bhip_disparity_bm5_dev_u8_f32",
           "bhip_disparity_bm5_census_u8_u8", "bhip_disparity_bm5_census_u8_f32", "bhip_disparity_bm5_census_dev_u8_u8",
           "bhip_disparity_bm5_census_dev_u8_f32"]


# ---- the restatement against the definition ----
@pytest.mark.parametrize("minD,maxD", [(0, 10), (4, 10)])
def test_rolling_form_equals_the_naive_form(minD, maxD):
    """ChecksDisparityBlockMatchNaive.compareToNaive's shapes: 20 x 25, radius 3 x 2, disparities 0..10 and 4..10"""
    W, H, rx, ry = 20, 25, 3, 2
    rng = np.random.RandomState(234)
    left, right = rng.randint(0, 256, (H, W)).astype(np.uint8), rng.randint(0, 256, (H, W)).astype(np.uint8)
    score_row, _ = b5.row_scorer(left, right, minD, maxD, rx)
    rows = b5.rolling_scores(score_row, H, W, minD, maxD, rx, ry)
    scalar = b5.rolling_scores(score_row, H, W, minD, maxD, rx, ry, five=b5.score_five_scalar)
    assert sorted(rows) == list(range(2 * ry, H - 2 * ry))
    checked = 0
    for y, five in rows.items():
        assert (five == scalar[y]).all()                 # np.where branches == the three compare() statements
        for col in range(minD, W - (4 * rx + 1) + 1):
            for i in range(min(col - minD + 1, maxD - minD)):
                assert five[W * i + col - minD] == b5.naive_five(left, right, y, col, i, minD, rx, ry), (y, col, i)
                checked += 1
    assert checked >= 170                                # 17 rows x (8 columns: 36 entries | 4 columns: 10 entries)
    # and the definition on plain block matching's scores is the same thing
    byrule = b5.region_scores(dr.sad_scores(left, right, minD, maxD, rx, ry), W, H, minD, maxD, rx, ry)
    assert all((byrule[y] == rows[y]).all() for y in rows)


def test_two_smallest_of_four_with_ties():
    """computeScoreFive's branches on every ordering and tie pattern of four values: always the sum of the two smallest"""
    vals = (1, 2, 2, 5)
    W, rx = 3, 1                                         # one entry: d = 0, indexSrc = 1, reads top / bottom at 0 and 2
    for a in vals:
        for b in vals:
            for c in vals:
                for d in vals:
                    top, bottom, middle = np.array([a, 0, b]), np.array([c, 0, d]), np.array([0, 100, 0])
                    for five in (b5.score_five_scalar, b5.score_five):
                        score = np.zeros(3, np.int64)
                        five(top, middle, bottom, score, W + 2, 0, 1, rx)   # width 5: end - indexSrc = 5 - 0 - 4 = 1
                        assert score[0] == 100 + sum(sorted((a, b, c, d))[:2])


@pytest.mark.parametrize("subpixel", [True, False])
def test_radius_zero_is_plain_block_matching_below_row_zero(subpixel):
    """rx = ry = 0: the five regions coincide, F = 3 V and the 3x cancels in every rule (first minimum, maxError * 3, the texture ratio, the
    sub-pixel quotient), so Best5 equals plain block matching bit for bit -- on the rows it selects.  computeRemainingRows starts at image row
    regionHeight = 1 and computeFirstRow selects nothing, so row 0 keeps the fill value; plain block matching selects row 0 in computeFirstRow."""
    W, H, minD, rng = 44, 9, 1, 20
    left, right = bc.scene(W, H, minD, rng)
    for mpe in (0, 25):
        got, _ = b5.block_match_best5(left, right, minD, rng, 0, 0, mpe, 1, .15, subpixel)
        plain, cls = dr.block_match(left, right, minD, rng, 0, 0, mpe, 1, .15, subpixel)
        assert (got[1:].view(np.uint8) == plain[1:].view(np.uint8)).all()
        assert (got[0] == rng).all() and (cls[0] != dr.BORDER).any()
        assert len({int(k) for k in np.unique(cls[1:])}) >= 3


def test_max_error_counts_three_regions():
    assert b5.max_error(3, 3, 25) == 3675 and b5.max_error(2, 1, 0) == 0
    assert b5.max_error(1, 1, 0.1) == int(9 * 0.1 * 3) == 2


def test_refusals_of_the_reference():
    z = np.zeros((20, 60), np.uint8)
    for kw in (dict(minDisparity=-1), dict(rangeDisparity=0), dict(rangeDisparity=57, regionRadiusX=2), dict(minDisparity=50, rangeDisparity=7, regionRadiusX=2)):
        with pytest.raises(ValueError):
            b5.block_match_best5(z, z, **kw)
    b5.block_match_best5(z, z, rangeDisparity=56, regionRadiusX=2, regionRadiusY=1)       # radiusX, not 2*radiusX: legal
    with pytest.raises(ValueError):
        b5.block_match_best5(np.zeros((4, 60), np.uint8), np.zeros((4, 60), np.uint8), rangeDisparity=10, regionRadiusY=2)
    # legal shapes without a single selected pixel
    for W, H, minD, rng, rx, ry in ((20, 20, 5, 7, 4, 1), (40, 9, 0, 10, 1, 3)):
        disp, cls = b5.block_match_best5(np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), minD, rng, rx, ry)
        assert (disp == rng).all() and (cls == dr.BORDER).all()


# ---- the GPU cases are not vacuous ----
def _inner(c):
    W, H, minD, rng, rx, ry = c[:6]
    return slice(2 * ry, H - 2 * ry), slice(2 * rx + minD, W - 2 * rx)


DISCRIMINATING = [c for c in bc.SAD_CASES[:12] if c[4] >= 1 and c[5] >= 1 and c[3] >= 20 and not c[10]]


@pytest.mark.parametrize("case", DISCRIMINATING, ids=bc.case_id)
def test_cases_tell_the_rule_from_its_neighbours(case):
    """the GrayU8 disparity differs on at least 2 % of the non-border pixels from plain block matching at the same radius, from "centre + all four
    corners" and from "centre + the two largest" """
    W, H, minD, rng, rx, ry, mpe, rtol, tex = case[:9]
    left, right = bc.scene(W, H, minD, rng)
    want, _ = bc.want(W, H, minD, rng, rx, ry, mpe, rtol, tex, False)
    ys, xs = _inner(case)
    n = want[ys, xs].size
    assert n > 0
    V = dr.sad_scores(left, right, minD, minD + rng, rx, ry)
    assert (b5.select_all(b5.region_scores(V, W, H, minD, minD + rng, rx, ry), W, H, minD, rng, rx, ry, mpe, rtol, tex, False)[0] == want).all()
    others = {"plain": dr.block_match(left, right, minD, rng, rx, ry, mpe, rtol, tex, False)[0]}
    for rule in ("all4", "worst2"):
        others[rule] = b5.select_all(b5.region_scores(V, W, H, minD, minD + rng, rx, ry, rule), W, H, minD, rng, rx, ry, mpe, rtol, tex, False)[0]
    for name, other in others.items():
        frac = float((other[ys, xs] != want[ys, xs]).sum()) / n
        print("%s vs %s: %.1f %% of %d pixels differ" % (bc.case_id(case), name, 100 * frac, n))
        assert frac >= 0.02, (name, frac)


def test_case_list_holds_every_class():
    seen = np.zeros(len(dr.CLASS_NAMES), np.int64)
    for c in bc.SAD_CASES:
        W, H, minD, rng, rx, ry, mpe, rtol, tex, outputs, binary = c
        for output in outputs:
            _, cls = bc.want(W, H, minD, rng, rx, ry, mpe, rtol, tex, output == "f32", binary=binary)
            seen += np.array(dr.class_counts(cls))
    assert (seen >= 10).all(), dict(zip(dr.CLASS_NAMES, seen))


def test_binarised_case_passes_sixteen_bits():
    """(96, 36, 0, 60, 7, 7) binarised: five-region scores above 65535 are common and decide the result; the plain scene never gets there"""
    W, H, minD, rng, rx, ry = 96, 36, 0, 60, 7, 7
    stats = {}
    for binary in (False, True):
        left, right = bc.scene(W, H, minD, rng, binary=binary)
        score_row, _ = b5.row_scorer(left, right, minD, minD + rng, rx)
        rows = b5.rolling_scores(score_row, H, W, minD, minD + rng, rx, ry)
        valid = np.zeros((rng, W), bool)
        k = np.arange(W - minD - 4 * rx)
        valid[:, :len(k)] = k[None, :] >= np.arange(rng)[:, None]
        scores = np.stack([rows[y].reshape(rng, W)[valid] for y in sorted(rows)])
        stats[binary] = (float((scores > 65535).mean()), int(scores.max()))
        if binary:
            want = b5.select_all(rows, W, H, minD, rng, rx, ry, 0, 1, .15, False)[0]
            masked = b5.select_all(rows, W, H, minD, rng, rx, ry, 0, 1, .15, False, mask16=True)[0]
            ys, xs = _inner((W, H, minD, rng, rx, ry))
            changed = float((want[ys, xs] != masked[ys, xs]).mean())
    print("over 65535: plain %.1f %% (max %d), binarised %.1f %% (max %d); masking changes %.1f %%" % (
        100 * stats[False][0], stats[False][1], 100 * stats[True][0], stats[True][1], 100 * changed))
    assert stats[True][0] >= 0.05 and stats[True][1] > 65535
    assert changed >= 0.5
    assert stats[False][1] <= 65535


# ---- the Python mirror ----
def test_factory_behaviour():
    import boofcv_amd as b
    from boofcv_amd import api, best5, census
    F, Cfg = best5.FactoryStereoDisparityBest5, best5.ConfigDisparityBMBest5
    assert all(getattr(b, n) is getattr(best5, n) for n in best5.__all__)
    assert not set(best5.__all__) & set(api.__all__)
    c = Cfg()
    assert isinstance(c, api.ConfigDisparityBM)
    assert (c.minDisparity, c.rangeDisparity, c.regionRadiusX, c.regionRadiusY, c.maxPerPixelError, c.validateRtoL, c.texture, c.subpixel, c.errorType) == \
        (0, 100, 3, 3, 0, 1, 0.15, True, api.DisparityError.SAD)
    alg = F.blockMatchBest5(None, api.GrayU8, api.GrayF32)
    assert (alg.getBorderX(), alg.getBorderY(), alg.getMinDisparity(), alg.getRangeDisparity(), alg.getInvalidValue()) == (6, 6, 0, 100, 100)
    assert alg.getInputType() is api.GrayU8 and alg.getDisparityType() is api.GrayF32
    alg = F.blockMatchBest5(Cfg(regionRadiusX=2, regionRadiusY=1, subpixel=False), api.GrayU8, api.GrayU8)
    assert (alg.getBorderX(), alg.getBorderY()) == (4, 2) and alg.getDisparityType() is api.GrayU8
    alg = F.blockMatchBest5(api.ConfigDisparityBM(regionRadiusX=1), api.GrayU8, api.GrayF32)    # a plain ConfigDisparityBM has the same fields
    assert alg.getBorderX() == 2
    cen = F.blockMatchBest5(Cfg(errorType=api.DisparityError.CENSUS, regionRadiusX=2), api.GrayU8, api.GrayF32)
    assert cen.variant == census.CensusVariants.BLOCK_5_5 and cen.getCensusTran().getOutputType() is api.GrayS32
    assert (cen.getBorderX(), cen.getBorderY()) == (4, 6)
    cen = F.blockMatchBest5(Cfg(errorType=api.DisparityError.CENSUS, configCensus=census.ConfigDisparityError.Census(census.CensusVariants.CIRCLE_9)))
    assert cen.getCensusTran().getOutputType() is census.GrayS64
    for config, imageType, dispType, message in [
        (Cfg(), api.GrayU8, api.GrayU8, "With subpixel on, disparity image must be GrayF32"),
        (Cfg(subpixel=False), api.GrayU8, api.GrayF32, "With subpixel on, disparity image must be GrayU8"),
        (Cfg(errorType=None), api.GrayU8, api.GrayF32, "Unsupported error type"),
        (Cfg(), api.GrayS32, api.GrayF32, "Unsupported image type GrayS32"),
        (Cfg(errorType=api.DisparityError.CENSUS), api.GrayS32, api.GrayF32, "Unknown image type"),
        (Cfg(errorType=api.DisparityError.CENSUS, configCensus=census.ConfigDisparityError.Census(9)), api.GrayU8, api.GrayF32, "Unknown type 9"),
        (Cfg(minDisparity=-1), api.GrayU8, api.GrayF32, "Min disparity must be >= 0"),
        (Cfg(rangeDisparity=0), api.GrayU8, api.GrayF32, "Max disparity must be greater than zero"),
        (Cfg(minDisparity=3, rangeDisparity=0), api.GrayU8, api.GrayF32, "Min disparity must be >= 0 and < maxDisparity. min=3 max=3"),
    ]:
        with pytest.raises(api.IllegalArgumentException, match=re.escape(message)):
            F.blockMatchBest5(config, imageType, dispType)
    for call in (lambda: F.blockMatchBest5(Cfg(errorType=api.DisparityError.NCC), api.GrayU8, api.GrayF32),
                 lambda: F.blockMatchBest5(Cfg(), api.GrayF32, api.GrayF32),
                 lambda: F.blockMatchBest5(Cfg(), api.GrayS16, api.GrayF32),
                 lambda: F.blockMatchBest5(Cfg(errorType=api.DisparityError.CENSUS), api.GrayF32, api.GrayF32),
                 lambda: api.FactoryStereoDisparity.blockMatchBest5(None, api.GrayU8, api.GrayF32)):   # the api package keeps refusing
        with pytest.raises(RuntimeError) as e:
            call()
        assert not isinstance(e.value, api.IllegalArgumentException)


def test_header_declares_and_library_exports_the_entries():
    from boofcv_amd import _lib
    header = (ROOT / "include" / "boofhip.h").read_text()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"^int %s\(bhip_ctx\* ctx, const bhip_disparity_bm_cfg\* cfg, " % name, header, re.M), name
        assert getattr(lib, name).argtypes is not None
    assert "blockMatchBest5, NCC" not in header          # the two comments that said it has no entry point
