"""CPU: tests/census_ref.py, the NumPy restatement of the census transform and of census block matching, against what the reference's own tests
pin (TestCensusTransform, TestImplCensusTransformInner / Border, TestBlockRowScoreCensus) and against hand-computed words; the Python mirror's
factories; and the non-vacuity of the block-matching cases tests/test_gpu_disparity_census.py runs.  No GPU."""
import numpy as np
import pytest

import census_cases as cc
import census_ref as cr
import disparity_ref as dr


# ---- TestCensusTransform: the sample lists ----
def test_block_samples_counts_and_order():
    for r in (1, 2, 3):
        s = cr.create_block_samples(r)
        assert len(s) == (2 * r + 1) ** 2 - 1
        want = [(x, y) for y in range(-r, r + 1) for x in range(-r, r + 1) if (x, y) != (0, 0)]
        assert s == want
    s = cr.create_block_samples(1, 2)                       # createBlockSamples_2
    assert len(s) == 3 * 5 - 1
    assert s == [(x, y) for y in range(-2, 3) for x in range(-1, 2) if (x, y) != (0, 0)]


def test_circle_samples():
    s = cr.create_circle_samples()
    assert len(s) == 9 * 9 - 4 * 6 - 1 == 56
    assert (0, 0) not in s and len(set(s)) == 56
    assert all((x * x + y * y) ** .5 <= 4.5 for x, y in s)
    assert sum(x for x, _ in s) == 0 and sum(y for _, y in s) == 0
    assert s[:3] == [(-4, -1), (-4, 0), (-4, 1)]            # set(row-4, col-4): the first loop row is x = -4


def test_variant_table():
    sizes = {"BLOCK_3_3": (8, 1), "BLOCK_5_5": (24, 2), "BLOCK_7_7": (48, 3), "BLOCK_9_7": (62, 4), "BLOCK_13_5": (54, 5), "CIRCLE_9": (56, 4)}
    for v in cr.VARIANTS:
        s = cr.variant_samples(v)
        assert (len(s), cr.sample_radius(s)) == sizes[v]
    assert max(abs(x) for x, _ in cr.variant_samples("BLOCK_13_5")) == 5      # 11 x 5, despite the name
    assert [cr.word_dtype(v) for v in cr.VARIANTS] == [np.uint8, np.int32] + [np.int64] * 4


def test_library_sample_lists_are_the_references():
    """bhip_census_variant_samples, the one place the product keeps the lists (no GPU needed to ask)"""
    from boofcv_amd import census
    for k, v in enumerate(cr.VARIANTS):
        assert census._variant_samples(k) == cr.variant_samples(v)
    assert census.CensusTransform.createCircleSamples() == cr.create_circle_samples()
    assert census.CensusTransform.createBlockSamples(3) == cr.create_block_samples(3)
    assert census.CensusTransform.createBlockSamples(4, 3) == cr.create_block_samples(4, 3)
    assert [int(v) for v in census.CensusVariants] == list(range(6)) and [v.name for v in census.CensusVariants] == list(cr.VARIANTS)


# ---- TestImplCensusTransformInner / Border: equal to a brute-force region scan (CensusNaive) ----
def _region_scan(img, cx, cy, rx, ry):
    """CensusNaive.region*: the window row by row, an int bit, reflected outside"""
    H, W = img.shape
    census, bit = 0, 1
    for row in range(-ry, ry + 1):
        for col in range(-rx, rx + 1):
            if row == 0 and col == 0:
                continue
            if int(img[cr.reflect(cy + row, H)][cr.reflect(cx + col, W)]) > int(img[cy][cx]):
                census |= dr.i32(bit)
            bit = (bit << 1) & 0xFFFFFFFF
    return census


@pytest.mark.parametrize("variant", cr.VARIANTS[:5])
def test_transform_equals_region_scan(variant):
    rng = np.random.RandomState(234)
    img = rng.randint(0, 256, (30, 20)).astype(np.uint8)    # w = 20, h = 30 as in the reference's tests
    samples = cr.variant_samples(variant)
    rx, ry = max(abs(x) for x, _ in samples), max(abs(y) for _, y in samples)
    got = cr.census_variant(img, variant)
    assert got.dtype == cr.word_dtype(variant)
    for y in range(30):
        for x in range(20):
            want = _region_scan(img, x, y, rx, ry)
            if variant == "BLOCK_3_3":
                want &= 0xFF
            assert int(got[y, x]) == want == (cr.census_pixel(img, x, y, samples) & (0xFF if variant == "BLOCK_3_3" else -1)), (x, y)


def test_circle_equals_pixel_loop():
    rng = np.random.RandomState(5)
    img = rng.randint(0, 256, (11, 13)).astype(np.uint8)
    samples = cr.create_circle_samples()
    got = cr.census(img, samples)
    for y in range(11):
        for x in range(13):
            assert int(got[y, x]) == cr.census_pixel(img, x, y, samples)


# ---- hand-computed words ----
def test_literal_3x3_and_5x5_words():
    img = np.array([[9, 1, 9, 1, 9],
                    [1, 9, 1, 9, 1],
                    [9, 1, 5, 9, 9],
                    [1, 1, 1, 1, 1],
                    [9, 9, 9, 9, 9]], np.uint8)
    # 3x3 at (2, 2), centre 5: samples row-major 9 1 9 / 1 . 9 / 1 1 1 -> bits 0, 2, 4
    assert int(cr.census_variant(img, "BLOCK_3_3")[2, 2]) == 0b00010101
    # 5x5 at (2, 2): rows 9 1 9 1 9 | 1 9 1 9 1 | 9 1 . 9 9 | 1 1 1 1 1 | 9 9 9 9 9 -> bits 0 2 4 | 6 8 | 10 12 13 | - | 19..23
    want = sum(1 << b for b in (0, 2, 4, 6, 8, 10, 12, 13, 19, 20, 21, 22, 23))
    assert int(cr.census_variant(img, "BLOCK_5_5")[2, 2]) == want


def test_reflect_at_the_four_corners():
    img = np.array([[5, 9, 0, 0],
                    [0, 0, 0, 0],
                    [0, 0, 0, 7],
                    [0, 8, 9, 6]], np.uint8)
    got = cr.census_variant(img, "BLOCK_3_3")
    # (0,0), centre 5: the window reads rows 1,0,1 and columns 1,0,1: 0 0 0 / 9 . 9 / 0 0 0 -> bits 3, 4
    assert int(got[0, 0]) == 0b00011000
    # (3,0), centre 0: columns 2,3,2, rows 1,0,1: all 0 -> 0
    assert int(got[0, 3]) == 0
    # (0,3), centre 0: rows 2,3,2, columns 1,0,1: 0 0 0 / 8 . 8 / 0 0 0 -> bits 3, 4
    assert int(got[3, 0]) == 0b00011000
    # (3,3), centre 6: rows 2,3,2, columns 2,3,2: 0 7 0 / 9 . 9 / 0 7 0 -> bits 1, 3, 4, 6
    assert int(got[3, 3]) == 0b01011010
    assert [cr.reflect(k, 4) for k in (-2, -1, 0, 3, 4, 5)] == [2, 1, 0, 3, 2, 1]


def _one_sample_image(index):
    """7x7, centre 10 at (3,3), only sample `index` of the 7x7 block above it"""
    img = np.zeros((7, 7), np.uint8)
    img[3, 3] = 10
    x, y = cr.create_block_samples(3)[index]
    img[3 + y, 3 + x] = 20
    return img


def test_s64_int_bit_counter():
    w31 = int(cr.census_variant(_one_sample_image(31), "BLOCK_7_7")[3, 3])
    assert w31 == -(1 << 31)                                 # 0x80000000 sign-extended: bits 31..63
    assert int(cr.census_variant(_one_sample_image(40), "BLOCK_7_7")[3, 3]) == 0   # bit is 0 from sample 32 on
    assert int(cr.census_variant(_one_sample_image(30), "BLOCK_7_7")[3, 3]) == 1 << 30
    assert [cr.java_bit(i) for i in (0, 30, 31, 32, 47)] == [1, 1 << 30, -(1 << 31), 0, 0]


def test_hamming_of_s64_words_is_33_plus_k():
    a = np.array([-(1 << 31) | 0b1011], np.int64)            # sample 31 and three low samples
    b = np.array([0b0001], np.int64)
    assert int(cr.hamming(a ^ b)[0]) == 33 + 2
    assert int(cr.hamming(np.array([-(1 << 31)], np.int64))[0]) == 33
    assert list(cr.hamming(np.array([0, 1, 0xFF, -1], np.int32))) == [0, 1, 8, 32]
    assert list(cr.hamming(np.array([0, 0x80, 0xFF], np.uint8))) == [0, 1, 8]
    # every GrayS64 word is the sign extension of its low 32 bits, so the distance is that of the low 31 bits plus 33 for bit 31
    rng = np.random.RandomState(2)
    img = rng.randint(0, 256, (12, 15)).astype(np.uint8)
    w = cr.census_variant(img, "BLOCK_9_7").reshape(-1)
    assert (w == w.astype(np.int32).astype(np.int64)).all()
    x = w[:-1] ^ w[1:]
    low = x.astype(np.int32)
    assert (cr.hamming(x) == cr.hamming(low & 0x7FFFFFFF) + 33 * ((low >> 31) & 1)).all()


# ---- TestBlockRowScoreCensus: the row score and the running sums against the four-loop definition ----
@pytest.mark.parametrize("variant", cc.BM_VARIANTS)
def test_scores_equal_the_naive_region_score(variant):
    left, right = dr.stereo_scene(40, 12, 1, 9, seed=3)
    cl, cr_ = cr.census_variant(left, variant), cr.census_variant(right, variant)
    minD, maxD, rx, ry, W = 1, 10, 2, 1, 40
    scores = cr.census_scores(cl, cr_, minD, maxD, rx, ry)
    assert sorted(scores) == list(range(ry, 12 - ry))
    rng = np.random.RandomState(0)
    for _ in range(150):
        y, c = rng.randint(ry, 12 - ry), rng.randint(minD, W - 2 * rx)
        i = rng.randint(0, min(c - minD + 1, maxD - minD))
        assert scores[y][W * i + c - minD] == cr.naive_cost(cl, cr_, y, c, i, minD, rx, ry)
    row = cr.score_row(cl, cr_, 4, minD, maxD, 2 * rx + 1)   # naiveScoreRow
    for c in (3, 10, 35):
        for i in (0, 2):
            assert row[W * i + c - minD] == cr.naive_cost(cl, cr_, 4, c, i, minD, rx, 0)


# ---- the Python mirror: factories, config defaults, refusals ----
def test_factory_exceptions_and_defaults():
    import boofcv_amd as b
    from boofcv_amd import api, census
    assert census.ConfigDisparityError.Census().variant == census.CensusVariants.BLOCK_5_5
    assert census.FactoryCensusTransform.CENSUS_BORDER == api.BorderType.REFLECT
    for v, out in zip(census.CensusVariants, [api.GrayU8, api.GrayS32] + [census.GrayS64] * 4):
        f = census.FactoryCensusTransform.variant(v, api.GrayU8)
        assert f.getOutputType() is out and f.getInputType() is api.GrayU8 and (f.getHorizontalBorder(), f.getVerticalBorder()) == (0, 0)
        assert f.samples == cr.variant_samples(v.name)
    with pytest.raises(api.IllegalArgumentException):
        census.FactoryCensusTransform.variant(6, api.GrayU8)
    for r, out in ((1, api.GrayU8), (2, api.GrayS32), (3, census.GrayS64)):
        assert census.FactoryCensusTransform.blockDense(r, api.GrayU8).getOutputType() is out
    for r in (0, 4):
        with pytest.raises(api.IllegalArgumentException, match="only radius 1 to 3"):
            census.FactoryCensusTransform.blockDense(r, api.GrayU8)
    assert len(census.FactoryCensusTransform.blockDense(4, 3, api.GrayU8).samples) == 62
    with pytest.raises(api.IllegalArgumentException, match="At most 64"):
        census.FactoryCensusTransform.blockDense(4, 4, api.GrayU8)
    with pytest.raises(RuntimeError) as e:
        census.FactoryCensusTransform.variant(census.CensusVariants.BLOCK_5_5, api.GrayF32)
    assert not isinstance(e.value, api.IllegalArgumentException)
    g = census.GrayS64(3, 2)
    assert g.data.dtype == np.int64 and g.array().shape == (2, 3)
    # the module's names reach the package, and none of them is one of api's
    assert all(getattr(b, n) is getattr(census, n) for n in census.__all__)
    assert not set(census.__all__) & set(api.__all__)


def test_stereo_factory_checks():
    from boofcv_amd import api, census
    F = census.FactoryStereoDisparityCensus
    cen = dict(errorType=api.DisparityError.CENSUS)
    alg = F.blockMatch(api.ConfigDisparityBM(**cen), api.GrayU8, api.GrayF32)
    assert alg.variant == census.CensusVariants.BLOCK_5_5 and alg.getCensusTran().getOutputType() is api.GrayS32
    assert (alg.getBorderX(), alg.getBorderY(), alg.getMinDisparity(), alg.getRangeDisparity(), alg.getInvalidValue()) == (3, 3, 0, 100, 100)
    assert alg.getInputType() is api.GrayU8 and alg.getDisparityType() is api.GrayF32
    assert (alg.getCLeft().width, alg.getCLeft().height) == (1, 1) and isinstance(alg.getCRight(), api.GrayS32)   # createImage(1,1) before a pair
    alg = F.blockMatch(api.ConfigDisparityBM(subpixel=False, **cen), api.GrayU8, api.GrayU8, census.ConfigDisparityError.Census(census.CensusVariants.CIRCLE_9))
    assert alg.getCensusTran().getOutputType() is census.GrayS64
    bad = [
        (api.ConfigDisparityBM(**cen), api.GrayU8, api.GrayU8, None),                        # subpixel wants GrayF32
        (api.ConfigDisparityBM(subpixel=False, **cen), api.GrayU8, api.GrayF32, None),
        (api.ConfigDisparityBM(), api.GrayU8, api.GrayF32, None),                             # errorType SAD
        (None, api.GrayU8, api.GrayF32, None),                                                # the default config is SAD
        (api.ConfigDisparityBM(errorType=api.DisparityError.NCC), api.GrayU8, api.GrayF32, None),
        (api.ConfigDisparityBM(**cen), api.GrayS32, api.GrayF32, None),
        (api.ConfigDisparityBM(**cen), api.GrayU8, api.GrayF32, census.ConfigDisparityError.Census(9)),
        (api.ConfigDisparityBM(rangeDisparity=0, **cen), api.GrayU8, api.GrayF32, None),
        (api.ConfigDisparityBM(minDisparity=-1, **cen), api.GrayU8, api.GrayF32, None),
    ]
    for config, imageType, dispType, cc_ in bad:
        with pytest.raises(api.IllegalArgumentException):
            F.blockMatch(config, imageType, dispType, cc_)
    for imageType in (api.GrayF32, api.GrayS16):
        with pytest.raises(RuntimeError) as e:
            F.blockMatch(api.ConfigDisparityBM(**cen), imageType, api.GrayF32)
        assert not isinstance(e.value, api.IllegalArgumentException)


def test_api_factory_still_refuses_census():
    from boofcv_amd import api
    with pytest.raises(RuntimeError) as e:
        api.FactoryStereoDisparity.blockMatch(api.ConfigDisparityBM(errorType=api.DisparityError.CENSUS), api.GrayU8, api.GrayF32)
    assert not isinstance(e.value, api.IllegalArgumentException)


# ---- the block-matching cases of the GPU test are not vacuous ----
@pytest.mark.parametrize("variant", cc.BM_VARIANTS)
@pytest.mark.parametrize("case", cc.BM_CASES, ids=lambda c: c[0])
def test_gpu_cases_hold_the_classes_they_claim(case, variant):
    name, W, H, minD, rng = case[:5]
    outputs, claims = case[10], case[11]
    _, cls = cc.want(variant, W, H, *cc.params(case, variant), outputs[0] == "f32")
    counts = dr.class_counts(cls)
    for k in claims:
        assert counts[k] >= 10, "%s %s: %d pixels %s" % (name, variant, counts[k], dr.CLASS_NAMES[k])
    if outputs[0] != "f32":
        assert counts[dr.VALID_INTERP] == 0


def test_each_check_case_counts():
    """the 'each check disabled on its own' runs of the GPU test: the classes of the checks left on hold at least 10 pixels, the disabled one none"""
    case = next(c for c in cc.BM_CASES if c[0] == "row_bands")
    name, W, H, minD, rng, rx, ry = case[:7]
    for variant in cc.BM_VARIANTS:
        for off in ("maxPerPixelError", "validateRtoL", "texture"):
            mpe, rtol, tex = cc.each_check_params(variant, off)
            _, cls = cc.want(variant, W, H, minD, rng, rx, ry, mpe, rtol, tex, True)
            counts = dr.class_counts(cls)
            disabled = {"maxPerPixelError": dr.REJECT_ERROR, "validateRtoL": dr.REJECT_RTOL, "texture": dr.REJECT_TEXTURE}[off]
            assert counts[disabled] == 0
            assert all(counts[k] >= 10 for k in (dr.REJECT_ERROR, dr.REJECT_RTOL, dr.REJECT_TEXTURE) if k != disabled), (variant, off, counts)
