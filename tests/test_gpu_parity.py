"""GPU parity tests proper: the HIP path (through the C ABI, via boofcv_amd.api) against the CPU oracle on the same seeded inputs.

Bar (BASELINE.json north_star): bit-exact for the fp32/integer stages (integral image, Hessian intensity, NMS, key point
coordinates/scales, Laplacian sign, Hamming / L2 scores and match indices); SURF descriptors within 1e-5 relative.
Run with `pytest -m gpu` on an MI355X.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DESC_TOL = 1e-5  # north_star: "SURF descriptor/L2 scores within 1e-5 relative" (descriptors are unit vectors)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()  # fails loudly without a GPU / without libboofhip.so
    return a


def G(api, g):
    """oracle Gray -> api.GrayF32 over the same buffer (same startIndex / stride)"""
    return api.GrayF32(g.width, g.height, g.buf, g.startIndex, g.stride)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ K1
@pytest.mark.parametrize("w,h,seed", [(20, 30, 234), (64, 64, 1), (65, 63, 2), (640, 480, 234), (1, 1, 3), (1, 50, 4), (200, 1, 5), (1000, 37, 6)])
def test_integral_bit_exact(api, orc, w, h, seed):
    img = orc.noise_image(w, h, seed)
    exp = orc.integral(img).array()
    got = api.IntegralImageOps.transform(G(api, img)).array()
    assert np.array_equal(bits(got), bits(exp))
    # sub-image in and out (BoofTesting.checkSubImage)
    sub = img.sub_image_of(5, 7)
    out = api.GrayF32(w, h).subimage(0, 0, w, h)
    big = api.GrayF32(w + 6, h + 4)
    out = big.subimage(3, 2, 3 + w, 2 + h)
    api.IntegralImageOps.transform(G(api, sub), out)
    assert np.array_equal(bits(out.array()), bits(exp))
    assert big.data[0] == 0 and big.data[-1] == 0  # nothing written outside the view


def test_integral_large_values_exact(api, orc):
    # sums well beyond 2^24 where fp32 addition order matters
    img = orc.noise_image(1920, 300, 9, 0, 255)
    assert np.array_equal(bits(api.IntegralImageOps.transform(G(api, img)).array()), bits(orc.integral(img).array()))


# ------------------------------------------------------------------------------------------------------------------ K2
@pytest.mark.parametrize("skip,size", [(1, 9), (2, 9), (3, 9), (4, 9), (1, 15), (1, 21), (1, 27), (2, 15), (2, 27), (2, 39), (2, 51), (4, 27), (4, 99), (8, 51)])
def test_hessian_bit_exact(api, orc, skip, size):
    w, h = (60, 70) if size <= 27 and skip <= 4 else (260, 230)
    ii = orc.integral(orc.JavaRandom(234).fillUniform(orc.Gray(w, h), 0, 50))
    exp = orc.hessian(ii, skip, size).array()
    out = api.GrayF32(w // skip, h // skip)
    api.IntegralImageFeatureIntensity.hessian(G(api, ii), skip, size, out)
    assert np.array_equal(bits(out.array()), bits(exp))
    # reference test tolerance vs the naive implementation (TestIntegralImageFeatureIntensity.java:45-65)
    naive = orc.hessian(ii, skip, size, naive=True).array()
    assert np.max(np.abs(out.array() - naive)) <= 1e-4 * max(1.0, float(np.max(np.abs(naive))))


def test_hessian_subimage(api, orc):
    ii = orc.integral(orc.noise_image(90, 80, 11))
    exp = orc.hessian(ii, 2, 15).array()
    big = api.GrayF32(45 + 4, 40 + 6)
    out = big.subimage(2, 3, 47, 43)
    api.IntegralImageFeatureIntensity.hessian(G(api, ii.sub_image_of(3, 2)), 2, 15, out)
    assert np.array_equal(bits(out.array()), bits(exp))


# ------------------------------------------------------------------------------------------------------------------ K3
def _nm(api, g, radius, thr, border):
    found = api.FactoryFeatureExtractor.nonmax(api.ConfigExtract(radius, thr, border, True)).process(G(api, g))
    return [(p.x, p.y) for p in found]


def test_nonmax_reference_cases(api, orc):
    NW, NH = 30, 40
    a = np.zeros((NH, NW), np.float32); a[1, 0] = 90; a[1, 1] = 30
    assert len(_nm(api, orc.Gray.from_array(a), 1, 5, 0)) == 1 and len(_nm(api, orc.Gray.from_array(a), 1, 5, 1)) == 0
    a = np.zeros((NH, NW), np.float32)
    a[0, NW // 2] = 90; a[NH - 1, NW // 2] = 90; a[NH // 2, 0] = 90; a[NH // 2, NW - 1] = 90
    assert len(_nm(api, orc.Gray.from_array(a), 2, 5, 0)) == 4
    a = np.zeros((NH, NW), np.float32); a[5, 3] = 30; a[7, 5] = 30; a[7, 7] = 30
    assert len(_nm(api, orc.Gray.from_array(a), 2, 5, 0)) == 0
    a = np.zeros((NH, NW), np.float32); a[10, 10] = orc.MAX_VALUE_F32; a[20, 20] = 50
    assert _nm(api, orc.Gray.from_array(a), 2, 5, 0) == [(20, 20)]


def test_nonmax_equals_oracle_in_block_raster_order(api, orc):
    rand = orc.JavaRandom(2134)
    for use_sub in (False, True):
        for radius in (1, 2, 3, 4):
            for border in (0, 3):
                img = rand.fillGaussian(orc.Gray(30, 40), 0, 3, -100, 100)
                if use_sub:
                    img = img.sub_image_of(5, 4)
                exp = [tuple(p) for p in orc.nonmax(img, radius, 0.6, border)]
                assert _nm(api, img, radius, 0.6, border) == exp
    img = orc.noise_image(333, 217, 8)
    assert _nm(api, img, 2, 50.0, 7) == [tuple(p) for p in orc.nonmax(img, 2, 50.0, 7)]


def test_nonmax_rejects_unsupported_config(api):
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryFeatureExtractor.nonmax(api.ConfigExtract(0, 1.0))
    with pytest.raises(RuntimeError):  # BOverride convention: not handled -> Java path
        api.FactoryFeatureExtractor.nonmax(api.ConfigExtract(2, 1.0, 0, False))


# ------------------------------------------------------------------------------------------------------------------ detector
@pytest.mark.parametrize("w,h,seed", [(80, 90, 1), (100, 120, 234), (400, 300, 234), (640, 480, 234), (57, 301, 7), (400, 300, 6), (402, 302, 6),
                                      (403, 301, 8), (1001, 703, 9), (1918, 1078, 10)])
def test_fast_hessian_points_bit_exact(api, orc, w, h, seed):
    ii = orc.integral(orc.noise_image(w, h, seed))
    exp = orc.fh_detect(ii)
    det = api.FastHessianFeatureDetector()
    det.detect(G(api, ii))
    got = det.getFoundPoints()
    assert got.shape == exp.shape and np.array_equal(got, exp)  # same points, same order, same bits


def test_fast_hessian_config_variants(api, orc):
    ii = orc.integral(orc.noise_image(300, 260, 21))
    for cfg in [dict(extractRadius=1), dict(detectThreshold=20.0), dict(initialSampleSize=2), dict(numberOfOctaves=2),
                dict(numberScalesPerOctave=5), dict(initialSize=15, numberScalesPerOctave=5), dict(scaleStepSize=8)]:
        exp = orc.fh_detect(ii, orc.FhCfg(**cfg))
        det = api.FastHessianFeatureDetector(api.ConfigFastHessian(**cfg))
        det.detect(G(api, ii))
        assert np.array_equal(det.getFoundPoints(), exp), cfg


@pytest.mark.parametrize("w,h,seed,nbest", [(300, 260, 21, 10), (300, 260, 21, 1), (640, 480, 234, 100), (400, 300, 5, 100000), (402, 301, 8, 100000),
                                            (407, 303, 9, 100000), (1920, 1080, 7, 300)])
def test_fast_hessian_max_features_per_scale(api, orc, w, h, seed, nbest):
    """SelectNBestFeatures between the NMS and the scale-space test (FastHessianFeatureDetector.java:255-262).  The GPU runs the
    same sequential QuickSelect exchange sequence as the oracle, so order and tie survivors agree bit for bit; against the real ddogleg
    build the order is unpinned (the library is not in the reference tree), the kept *set* is not."""
    img = orc.noise_image(w, h, seed)
    ii = orc.integral(img)
    exp = orc.fh_detect(ii, orc.FhCfg(maxFeaturesPerScale=nbest), threads=8)
    det = api.FastHessianFeatureDetector(api.ConfigFastHessian(maxFeaturesPerScale=nbest))
    det.detect(G(api, ii))
    got = det.getFoundPoints()
    assert len(exp) > 0 and got.shape == exp.shape and np.array_equal(got, exp)
    full = orc.fh_detect(ii, threads=8)
    assert {tuple(p) for p in got.tolist()} <= {tuple(p) for p in full.tolist()}
    if nbest >= 100000:
        assert np.array_equal(got, full)   # N above every list length: nothing is pruned, original order
    # detect + describe with the limit, batched (two different frames): same key points per frame, descriptors within tolerance
    if w <= 640:
        cfg = api.ConfigFastHessian(maxFeaturesPerScale=nbest)
        dd = api.FactoryDetectDescribe.surfStable(cfg, None, None, api.GrayF32)
        ref = orc.Surf(True, fh=orc.FhCfg(maxFeaturesPerScale=nbest))
        img2 = orc.noise_image(w, h, seed + 1)
        dd.detectBatch([G(api, img), G(api, img2)])
        for k, im in enumerate((img, img2)):
            _compare_surf(api, orc, dd, ref, im, k)


def test_fast_hessian_random_shapes_and_configs(api, orc):
    """Seeded sweep over frame shapes (every residue of W, H modulo the octave steps moves the inner / border split of the Hessian forms and
    the NMS block grid) and detector configurations, key points bit-exact and in order.  Noise frames put key points right up to the borders."""
    rng = np.random.default_rng(20240607)
    checked = 0
    for k in range(24):
        w, h = int(rng.integers(60, 520)), int(rng.integers(60, 420))
        cfg = {}
        if k % 3 == 1:
            cfg = dict(extractRadius=int(rng.integers(1, 4)), detectThreshold=float(rng.choice([0.5, 1.0, 10.0])))
        elif k % 3 == 2:
            cfg = dict(initialSampleSize=int(rng.integers(1, 3)), numberScalesPerOctave=int(rng.integers(3, 6)), numberOfOctaves=int(rng.integers(1, 5)),
                       initialSize=int(rng.choice([9, 15])), scaleStepSize=int(rng.choice([6, 8])))
        if k % 4 == 3:
            cfg["maxFeaturesPerScale"] = int(rng.choice([5, 50, 500]))
        ii = orc.integral(orc.noise_image(w, h, 1000 + k))
        exp = orc.fh_detect(ii, orc.FhCfg(**cfg), threads=8)
        det = api.FastHessianFeatureDetector(api.ConfigFastHessian(**cfg))
        det.detect(G(api, ii))
        assert np.array_equal(det.getFoundPoints(), exp), (w, h, cfg)
        checked += len(exp)
    assert checked > 5000


def test_fast_hessian_image_smaller_than_kernel(api, orc):
    ii = orc.integral(orc.noise_image(20, 20, 3))  # 27 > 20: no octave runs (FastHessianFeatureDetector.java:178)
    det = api.FastHessianFeatureDetector(); det.detect(G(api, ii))
    assert len(det.getFoundPoints()) == 0 and len(orc.fh_detect(ii)) == 0


# ------------------------------------------------------------------------------------------------------------------ detect + describe
def _compare_surf(api, orc, dd, ref, img, image_index=0):
    n = ref.detect(img)
    xys, ang, white, desc = ref.fetch()
    dd.selectImage(image_index)
    got = dd._results()
    assert dd.getNumberOfFeatures() == n
    assert np.array_equal(got[0], xys)          # location + scale: bit exact, reference order
    assert np.array_equal(got[2], white)        # Laplacian sign
    if n:
        # No exception list: with the wave-parallel window sweep handing every trailing-side window to the serial reference sweep, every
        # orientation agrees with the oracle to a few ulp (measured max 2.2e-15 rad over 110 k key points) and every descriptor value to
        # ~5e-16.  The north-star bar is 1e-5; the orientation bar below is 1e-12 rad for EVERY key point.
        dang = np.abs(np.angle(np.exp(1j * (got[1] - ang))))
        derr = np.max(np.abs(got[3] - desc), axis=1)
        nout = int((derr > DESC_TOL).sum())
        assert nout == 0, "descriptors outside 1e-5: %d of %d, max err %.3g, their angle errors %s" % (nout, n, derr.max(), dang[derr > DESC_TOL][:5])
        assert dang.max() < 1e-12, "orientation max err %.3g rad at key point %d" % (dang.max(), int(dang.argmax()))
        assert np.allclose(np.linalg.norm(got[3], axis=1), 1, atol=1e-12)
    return n


@pytest.mark.parametrize("stable", [True, False])
def test_surf_detect_describe_parity(api, orc, stable):
    dd = (api.FactoryDetectDescribe.surfStable if stable else api.FactoryDetectDescribe.surfFast)(None, None, None, api.GrayF32)
    ref = orc.Surf(stable)
    rand = orc.JavaRandom(234)
    for _ in range(4):  # GenericTestsDetectDescribePoint: 100x120 noise, N > 5
        img = rand.fillUniform(orc.Gray(100, 120), 0, 100)
        dd.detect(G(api, img))
        assert _compare_surf(api, orc, dd, ref, img) > 5
    # sub-image == full image ; repeated call == first call
    full = dd._results()
    dd.detect(G(api, img.sub_image_of()))
    sub = dd._results()
    assert all(np.array_equal(a, b) for a, b in zip(full, sub))
    # TestWrapDetectDescribeSurf_MT: 400x300 noise -> > 200 features
    img = orc.JavaRandom(234).fillUniform(orc.Gray(400, 300), 0, 100)
    dd.detect(G(api, img))
    assert _compare_surf(api, orc, dd, ref, img) > 200
    # interface odds and ends
    assert dd.hasScale() and dd.hasOrientation() and dd.createDescription().size() == 64
    p = dd.getLocation(0); d = dd.getDescription(0)
    assert isinstance(d, api.BrightFeature) and dd.getRadius(0) == dd._results()[0][0][2] * 2.0 and p.x == dd._results()[0][0][0]


@pytest.mark.parametrize("stable", [True, False])
def test_surf_random_shapes_batched(api, orc, stable):
    """Seeded sweep of frame shapes through detect + describe, several frames per batch: key points bit-exact, descriptors within
    tolerance.  Blob frames (S-blobs of SURVEY 8d, scaled down) put large-scale key points next to the borders, where the descriptor
    and orientation samplers switch to their bounds-checked forms."""
    rng = np.random.default_rng(77 if stable else 78)
    ref = orc.Surf(stable)
    for k in range(3):
        w, h = int(rng.integers(150, 420)), int(rng.integers(120, 330))
        dd = (api.FactoryDetectDescribe.surfStable if stable else api.FactoryDetectDescribe.surfFast)(None, None, None, api.GrayF32)
        frames = []
        for j in range(3):
            yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
            a = np.full((h, w), 50.0)
            for _ in range(max(4, w * h // 2500)):
                cx, cy = rng.uniform(0, w), rng.uniform(0, h)
                sg = float(rng.choice([2, 3, 5, 8, 13]))
                amp = float(rng.uniform(40, 100) * rng.choice([-1, 1]))
                a += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sg * sg))
            a += rng.uniform(0, 2, (h, w))
            frames.append(orc.Gray.from_array(a.astype(np.float32)))
        dd.detectBatch([G(api, f) for f in frames])
        total = sum(_compare_surf(api, orc, dd, ref, f, j) for j, f in enumerate(frames))
        assert total > 30, (w, h)


def test_surf_batch_equals_single(api, orc):
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    ref = orc.Surf(True)
    imgs = [orc.noise_image(320, 200, 1000 + i) for i in range(5)]
    dd.detectBatch([G(api, im) for im in imgs])
    total = 0
    for i, im in enumerate(imgs):
        total += _compare_surf(api, orc, dd, ref, im, i)
    assert dd.totalFeatures() == total


def test_surf_describe_points_edge_cases(api, orc):
    """BaseTestDescribeSurf: constant image, ramps, border points, fractional scale -- through describePoints"""
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    ref = orc.Surf(True)
    img = orc.noise_image(120, 100, 5)
    dd.detect(G(api, img))
    pts = np.array([[0, 0, 1.0], [119, 99, 1.0], [60.3, 50.7, 1.5], [3.2, 96.1, 2.2], [117.9, 2.5, 4.0], [60, 50, 9.7], [25, 25, 1.2]])
    ang, white, desc = dd.describePoints(pts)
    ref.describe_points(pts, img)
    _, rang, rwhite, rdesc = ref.fetch()
    assert np.array_equal(white, rwhite)
    assert np.max(np.abs(desc - rdesc)) <= DESC_TOL and np.max(np.abs(np.angle(np.exp(1j * (ang - rang))))) < 1e-9


def test_surf_config_variants(api, orc):
    img = orc.noise_image(240, 200, 17)
    cases = [
        (True, dict(fh=orc.FhCfg(detectThreshold=5.0, extractRadius=1)), dict(configDetector=dict(detectThreshold=5.0, extractRadius=1))),
        (True, dict(ori=orc.OriCfg.sliding(samplePeriod=1.0, radius=6, weightSigma=0.0, sampleWidth=4)),
         dict(configOrientation=dict(samplePeriod=1.0, radius=6, weightSigma=0.0, sampleWidth=4))),
        (False, dict(ori=orc.OriCfg.average(radius=4, weightSigma=0.0)), dict(configOrientation=dict(radius=4, weightSigma=0.0))),
    ]
    for stable, okw, akw in cases:
        ref = orc.Surf(stable, **okw)
        kw = {}
        if "configDetector" in akw:
            kw["configDetector"] = api.ConfigFastHessian(**akw["configDetector"])
        if "configOrientation" in akw:
            kw["configOrientation"] = (api.ConfigSlidingIntegral if stable else api.ConfigAverageIntegral)(**akw["configOrientation"])
        if stable:
            dd = api.FactoryDetectDescribe.surfStable(kw.get("configDetector"), None, kw.get("configOrientation"), api.GrayF32)
        else:
            dd = api.FactoryDetectDescribe.surfFast(kw.get("configDetector"), None, kw.get("configOrientation"), api.GrayF32)
        dd.detect(G(api, img))
        assert _compare_surf(api, orc, dd, ref, img) > 10


def test_integral_from_detect_is_bit_exact(api, orc):
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    img = orc.noise_image(333, 111, 3)
    dd.detect(G(api, img))
    assert np.array_equal(bits(dd.fetchIntegral(0, 333, 111)), bits(orc.integral(img).array()))


@pytest.mark.parametrize("w,h,batch", [(100, 130, 128), (33, 65, 130), (700, 1100, 128), (513, 64, 129), (1920, 1080, 128), (1921, 1081, 128), (64, 2100, 128)])
def test_integral_single_pass_batched(api, orc, w, h, batch):
    """Batches of 128+ frames take the single-pass integral kernel (one workgroup per image, row and column chains both sequential): every
    frame's integral image is bit-exact.  Shapes cover fewer than / more than 16 column tiles, more than 16 row bands (a wave takes a second
    band), ragged last tiles and bands.  Large values (up to 1e4 per pixel) make every addition round."""
    dd = api.FactoryDetectDescribe.surfFast(api.ConfigFastHessian(detectThreshold=1e12), None, None, api.GrayF32)   # no key points: integral only
    rng = np.random.default_rng(w * 7 + h)
    frames = [(rng.uniform(0, 1e4, (h, w))).astype(np.float32) for _ in range(3)]
    idx = [int(k) for k in rng.integers(0, 3, batch)]
    dd.detectBatch([api.GrayF32.wrap(frames[k]) for k in idx])
    want = [orc.integral(orc.Gray.from_array(f)).array() for f in frames]
    for pos in sorted({0, 1, batch // 2, batch - 1}):
        assert np.array_equal(bits(dd.fetchIntegral(pos, w, h)), bits(want[idx[pos]])), pos


@pytest.mark.parametrize("w,h", [(333, 217), (200, 1100), (517, 1200), (96, 1080)])
def test_integral_single_pass_band_heights(api, orc, w, h):
    """The single-pass integral kernel runs bands of 64, 68 or 72 rows (the launch picks the height with the fewest rounds of 16 bands: 68 for
    1080 rows); lanes of a taller band carry a second row chain.  Device batches of 130 frames (host batches are chunked and take the
    streaming passes): every band height must give the oracle's integral image bit for bit -- ragged last band and tile, more than 16 bands
    (second round + wrap row), one round of tall bands."""
    torch = pytest.importorskip("torch")
    import os
    rng = np.random.default_rng(w * 5 + h)
    B = 130
    base = [(rng.uniform(0, 1e4, (h, w))).astype(np.float32) for _ in range(3)]
    idx = [int(k) for k in rng.integers(0, 3, B)]
    frames = torch.from_numpy(np.stack([base[k] for k in idx])).cuda()
    want = [orc.integral(orc.Gray.from_array(f)).array() for f in base]
    for band in (None, "64", "68", "72"):
        if band:
            os.environ["BHIP_INTEGRAL_BAND"] = band
        try:
            ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
            dd = api.FactoryDetectDescribe.surfFast(api.ConfigFastHessian(detectThreshold=1e12), None, None, api.GrayF32, ctx=ctx)   # no key points: integral only
            dd.detectDevice(frames.data_ptr(), h * w, w, w, h, B)
            for pos in (0, 1, B // 2, B - 1):
                assert np.array_equal(bits(dd.fetchIntegral(pos, w, h)), bits(want[idx[pos]])), (band, pos)
        finally:
            os.environ.pop("BHIP_INTEGRAL_BAND", None)


# ------------------------------------------------------------------------------------------------------------------ association
def _col(*v):
    return np.array(v, np.float64).reshape(-1, 1)


def _greedy(api, score, maxErr, backwards, src, dst):
    alg = api.FactoryAssociation.greedy(score, maxErr, backwards)
    alg.setSource(src); alg.setDestination(dst); alg.associate()
    return alg


def test_greedy_reference_literals(api):  # FT:alg/feature/associate/TestAssociateGreedy.java:38-105
    S = api.ScoreAssociateEuclidean_F64()
    a = _greedy(api, S, 0.5, False, _col(1, 2, 3, 4), _col(3, 4, 1, 40))
    assert a.getPairs().tolist() == [2, -1, 0, 1] and a.getFitQuality()[[0, 2, 3]].tolist() == [0, 0, 0]
    assert _greedy(api, S, 10, False, _col(1, 2, 3, 4), _col(3, 4, 1.1, 40)).getPairs()[1] == 2
    assert _greedy(api, S, 0.1, False, _col(1, 2, 3, 4), _col(3, 4, 1.1, 40)).getPairs()[1] == -1
    a = _greedy(api, S, 10, True, _col(1, 2, 3, 8), _col(3, 4, 1, 10))
    assert a.getPairs().tolist() == [2, -1, 0, 3] and a.getFitQuality()[3] == 2 and a.getFitQuality()[1] == api.Double_MAX_VALUE


def test_associate_description_standard_checks(api):  # FT:abst/feature/associate/StandardAssociateDescriptionChecks.java:76-240
    S = api.ScoreAssociateEuclidean_F64()
    c = lambda v: api.TupleDesc_F64(1, [v])
    for n in (20, 40):
        alg = _greedy(api, S, 0.01, True, [c(i + 1) for i in range(n)], [c(i + 1 + 0.001) for i in range(n)])
        m = alg.getMatches()
        assert len(m) == n and all(x.src == x.dst and x.fitScore != 0 for x in m)
        assert alg.getUnassociatedSource() == [] and alg.getUnassociatedDestination() == []
    assert len(_greedy(api, S, api.Double_MAX_VALUE, True, [c(1)], [c(100)]).getMatches()) == 1  # checkDefaultThreshold
    alg = api.FactoryAssociation.greedy(S, api.Double_MAX_VALUE, True)
    alg.setSource([c(1)]); alg.setDestination([c(1 + 0.1)])
    for thr, exp in [(0.01, 0), (1.1 - 1, 1), (0.2, 1), (api.Double_MAX_VALUE, 1)]:  # inclusive threshold edge
        alg.setMaxScoreThreshold(thr); alg.associate()
        assert len(alg.getMatches()) == exp
    alg = _greedy(api, S, 0.07, True, [c(1), c(2), c(3)], [c(1.1), c(2.05), c(3.05), c(20)])  # checkUnassociatedLists
    assert len(alg.getMatches()) == 2 and len(alg.getUnassociatedSource()) == 1 and len(alg.getUnassociatedDestination()) == 2
    alg = _greedy(api, S, api.Double_MAX_VALUE, True, [c(1)], [c(1), c(1.001)])
    assert alg.uniqueSource() and sum(1 for x in alg.getMatches() if x.src == 0) == 1
    alg = _greedy(api, S, api.Double_MAX_VALUE, True, [c(1), c(1.001)], [c(1)])
    assert alg.uniqueDestination() and sum(1 for x in alg.getMatches() if x.dst == 0) == 1
    assert alg.getScoreType() == api.MatchScoreType.NORM_ERROR
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryAssociation.greedy(S, 1, True).associate()


def _surf_like(rng, n, dof=64):
    a = rng.normal(size=(n, dof)); a /= np.linalg.norm(a, axis=1, keepdims=True)
    return a


@pytest.mark.parametrize("ns,nd,dof", [(200, 180, 64), (1, 1, 64), (3, 500, 64), (700, 2, 64), (257, 255, 64), (100, 90, 7), (64, 64, 128), (50, 40, 1)])
@pytest.mark.parametrize("backwards", [False, True])
def test_l2_association_bit_exact(api, orc, ns, nd, dof, backwards):
    rng = np.random.default_rng(ns * 1000 + nd)
    src = _surf_like(rng, ns, dof); dst = _surf_like(rng, nd, dof)
    k = min(ns, nd) // 2
    dst[:k] = src[:k] + rng.normal(scale=0.05, size=(k, dof))
    for maxErr in (api.Double_MAX_VALUE, 0.5):
        a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), maxErr, backwards, src, dst)
        p, f = orc.associate_l2(src, dst, maxErr, backwards)
        assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)


def test_l2_association_ties_duplicates_nan(api, orc):
    rng = np.random.default_rng(3)
    base = _surf_like(rng, 40)
    src = np.concatenate([base, base[:10], base[5:15]])          # duplicate sources -> column ties
    dst = np.concatenate([base[::-1], base[:7], base[:7]])        # duplicate destinations -> row ties (largest index wins)
    for backwards in (False, True):
        a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, backwards, src, dst)
        p, f = orc.associate_l2(src, dst, api.Double_MAX_VALUE, backwards)
        assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)
    src2 = src.copy(); src2[3, 5] = np.nan; dst2 = dst.copy(); dst2[8, 1] = np.nan
    a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True, src2, dst2)
    p, f = orc.associate_l2(src2, dst2, api.Double_MAX_VALUE, True)
    assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)
    # empty sets
    a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), 1.0, True, src, np.zeros((0, 64)))
    assert a.getPairs().tolist() == [-1] * len(src) and np.all(a.getFitQuality() == 1.0) and a.getMatches() == []
    a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), 1.0, True, np.zeros((0, 64)), dst)
    assert len(a.getPairs()) == 0 and a.getUnassociatedDestination() == list(range(len(dst)))


@pytest.mark.parametrize("ns,nd,words", [(300, 280, 16), (1, 5, 16), (129, 64, 16), (90, 100, 8), (60, 60, 1), (40, 50, 3)])
@pytest.mark.parametrize("backwards", [False, True])
def test_hamming_association_bit_exact(api, orc, ns, nd, words, backwards):
    rng = np.random.default_rng(ns + nd + words)
    src = rng.integers(-2**31, 2**31, size=(ns, words), dtype=np.int64).astype(np.int32)
    dst = rng.integers(-2**31, 2**31, size=(nd, words), dtype=np.int64).astype(np.int32)
    k = min(ns, nd) // 2
    flips = (rng.integers(0, 2**31, size=(k, words), dtype=np.int64) & rng.integers(0, 2**31, size=(k, words), dtype=np.int64)
             & rng.integers(0, 2**31, size=(k, words), dtype=np.int64)).astype(np.int32)
    dst[:k] = src[:k] ^ flips
    dst[k // 2] = dst[0]  # exact duplicate destination
    for maxErr in (api.Double_MAX_VALUE, 40.0):
        a = _greedy(api, api.ScoreAssociateHamming_B(), maxErr, backwards, src, dst)
        p, f = orc.associate_hamming(src, dst, maxErr, backwards)
        assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)


# ------------------------------------------------------------------------------------------------------------------ ip front end
def test_convolution_and_blur_bit_exact(api, orc):
    rand = orc.JavaRandom(234)
    for (w, h) in [(35, 28), (200, 150), (7, 9)]:
        img = rand.fillUniform(orc.Gray(w, h), 0, 50)
        for r in (1, 2, 3, 5, 6, 8):
            k = orc.gaussian1d_f32(-1, r)
            K = api.Kernel1D_F32(k)
            for kind, cls, fn in [("h", api.ConvolveImageNoBorder, "horizontal"), ("v", api.ConvolveImageNoBorder, "vertical"),
                                  ("norm_h", api.ConvolveImageNormalized, "horizontal"), ("norm_v", api.ConvolveImageNormalized, "vertical")]:
                if not kind.startswith("norm") and len(k) > min(w, h):
                    continue
                out = api.GrayF32(w, h)
                getattr(cls, fn)(K, G(api, img), out)
                assert np.array_equal(bits(out.array()), bits(orc.conv(kind, k, r, img).array())), (w, h, r, kind)
        for sigma, radius in [(-1, 2), (2.0, -1), (1.5, 4), (-1, 1)]:
            if 2 * max(radius, 1) + 1 > 2 * min(w, h):
                continue
            out = api.BlurImageOps.gaussian(G(api, img), None, sigma, radius)
            assert np.array_equal(bits(out.array()), bits(orc.gaussian_blur(img, sigma, radius).array())), (w, h, sigma, radius)
    # asymmetric kernel with an off-centre origin goes through the standard (not unrolled) form
    img = rand.fillUniform(orc.Gray(40, 30), -5, 5)
    k = np.array([0.1, 0.5, -0.2, 0.3], np.float32)
    for kind, cls, fn in [("h", api.ConvolveImageNoBorder, "horizontal"), ("v", api.ConvolveImageNoBorder, "vertical"),
                          ("norm_h", api.ConvolveImageNormalized, "horizontal"), ("norm_v", api.ConvolveImageNormalized, "vertical")]:
        out = api.GrayF32(40, 30)
        getattr(cls, fn)(api.Kernel1D_F32(k, offset=1), G(api, img), out)
        assert np.array_equal(bits(out.array()), bits(orc.conv(kind, k, 1, img).array())), kind
    # sub-image views in and out
    sub = img.sub_image_of(4, 3)
    big = api.GrayF32(46, 38); out = big.subimage(2, 5, 42, 35)
    api.ConvolveImageNormalized.horizontal(api.Kernel1D_F32(orc.gaussian1d_f32(-1, 2)), G(api, sub), out)
    assert np.array_equal(bits(out.array()), bits(orc.conv("norm_h", orc.gaussian1d_f32(-1, 2), 2, img).array()))


def test_one_pass_gaussian_blur_bit_exact(api, orc, monkeypatch):
    """BlurImageOps.gaussian for the unrolled widths runs as ONE kernel (horizontal filter in registers, vertical filter from a register
    ring): bit-exact against the oracle's two passes and against the library's own two-pass form (BHIP_BLUR_TWO_PASS=1) on shapes that
    exercise every position class -- widths that are no multiple of 4 or of 256, strips shorter than the kernel reach, images barely larger
    than the kernel, several strips per column, device batches"""
    import torch
    from boofcv_amd import device as dv
    rand = orc.JavaRandom(77)
    shapes = [(12, 12), (13, 70), (70, 13), (259, 40), (300, 131), (517, 65), (64, 200)]
    for (w, h) in shapes:
        img = rand.fillUniform(orc.Gray(w, h), 0, 255)
        for radius in (1, 2, 3, 4, 5):
            if 2 * radius + 1 >= min(w, h):
                continue
            ref = bits(orc.gaussian_blur(img, -1, radius).array())
            out = api.BlurImageOps.gaussian(G(api, img), None, -1, radius)
            assert np.array_equal(bits(out.array()), ref), (w, h, radius)
            monkeypatch.setenv("BHIP_BLUR_TWO_PASS", "1")
            out2 = api.BlurImageOps.gaussian(G(api, img), None, -1, radius)
            monkeypatch.delenv("BHIP_BLUR_TWO_PASS")
            assert np.array_equal(bits(out2.array()), ref), (w, h, radius, "two pass")
    # a kernel whose fp32 sum is off by more than 1e-4 is re-normalised by both passes (sigma given, radius given)
    img = rand.fillUniform(orc.Gray(90, 77), -20, 20)
    for sigma, radius in [(3.0, 2), (0.7, 3), (5.0, 5)]:
        out = api.BlurImageOps.gaussian(G(api, img), None, sigma, radius)
        assert np.array_equal(bits(out.array()), bits(orc.gaussian_blur(img, sigma, radius).array())), (sigma, radius)
    # device batch, on torch's stream: every image equals its single-image result
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    ops = dv.DeviceImageOps(ctx)
    imgs = [rand.fillUniform(orc.Gray(324, 100), 0, 100) for _ in range(3)]
    t = torch.from_numpy(np.stack([g.array() for g in imgs])).to("cuda:0")
    for radius in (2, 5):
        got = ops.gaussian(t, -1, radius).cpu().numpy()
        for i, g in enumerate(imgs):
            assert np.array_equal(bits(got[i]), bits(orc.gaussian_blur(g, -1, radius).array())), (radius, i)
    ctx.close()


def test_one_pass_pyramid_layer_bit_exact(api, orc, monkeypatch):
    """PyramidDiscreteSampleBlur's layer step (skip 2, widths 3 / 5) runs as ONE kernel per layer: bit-exact against the oracle's two passes
    through `temp` and against the library's own two-pass form (BHIP_PYRAMID_TWO_PASS=1) -- even and odd sizes (the last output column /
    row is a border output or does not exist), sizes barely above the kernel, several layers, device batches"""
    import torch
    from boofcv_amd import device as dv
    rand = orc.JavaRandom(91)
    for (w, h) in [(64, 48), (66, 50), (65, 49), (131, 77), (260, 38), (16, 16), (20, 12), (517, 130)]:
        img = rand.fillUniform(orc.Gray(w, h), 0, 200)
        for radius in (1, 2):
            ker = orc.gaussian1d_f32(-1, radius)
            for scales in ([2], [1, 2], [1, 2, 4], [2, 4, 8]):
                try:
                    exp, _ = orc.pyramid(ker, -1, scales, img)
                except ValueError:
                    continue   # a shape the reference rejects (covered by the acceptance tests)
                for two_pass in (False, True):
                    if two_pass:
                        monkeypatch.setenv("BHIP_PYRAMID_TWO_PASS", "1")
                    pyr = api.PyramidDiscreteSampleBlur(api.Kernel1D_F32(ker), -1, False, scales).process(G(api, img))
                    if two_pass:
                        monkeypatch.delenv("BHIP_PYRAMID_TWO_PASS")
                    for i, e in enumerate(exp):
                        assert np.array_equal(bits(pyr.getLayer(i).array()), bits(e)), (w, h, radius, scales, i, two_pass)
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    ops = dv.DeviceImageOps(ctx)
    imgs = [rand.fillUniform(orc.Gray(328, 122), 0, 100) for _ in range(3)]
    t = torch.from_numpy(np.stack([g.array() for g in imgs])).to("cuda:0")
    ker = orc.gaussian1d_f32(-1, 2)
    layers = ops.pyramid(ker, [1, 2, 4], t)
    for b, g in enumerate(imgs):
        exp, _ = orc.pyramid(ker, -1, [1, 2, 4], g)
        for i, e in enumerate(exp):
            assert np.array_equal(bits(layers[i][b].cpu().numpy()), bits(e)), (b, i)
    ctx.close()


def test_gradients_bit_exact(api, orc):
    rand = orc.JavaRandom(234)
    for (w, h) in [(31, 26), (200, 100), (3, 3), (5, 4)]:
        img = rand.fillUniform(orc.Gray(w, h), 0, 50)
        for kind, cls in [("sobel", api.GradientSobel), ("three", api.GradientThree)]:
            for border in (None, 0):
                dx, dy = api.GrayF32(w, h), api.GrayF32(w, h)
                dx.data[:] = 7; dy.data[:] = 7  # untouched frame must stay
                cls.process(G(api, img), dx, dy, border)
                ex, ey = orc.gradient(kind, img, border_zero=border is not None)
                if border is None:
                    ex.array()[[0, -1], :] = 7; ex.array()[:, [0, -1]] = 7; ey.array()[[0, -1], :] = 7; ey.array()[:, [0, -1]] = 7
                assert np.array_equal(bits(dx.array()), bits(ex.array())) and np.array_equal(bits(dy.array()), bits(ey.array())), (w, h, kind, border)


def test_down_convolution_bit_exact(api, orc):
    """ConvolveImageDownNormalized.horizontal/vertical: every (size, radius, skip) class incl. the naive form, the off-grid skip>=3
    quirk (untouched column keeps the caller's value) and the shapes the reference rejects."""
    rand = orc.JavaRandom(99)
    cases = 0
    for (w, h) in [(15, 20), (16, 21), (80, 120), (41, 27), (201, 133), (9, 64)]:
        img = rand.fillUniform(orc.Gray(w, h), 1, 10)
        for r in (1, 2, 3, 4, 5, 7, 10):
            k = orc.gaussian1d_f32(-1, r)
            for skip in (1, 2, 3, 4, 5):
                for kind in ("h", "v"):
                    ow, oh = (w // skip, h) if kind == "h" else (w, h // skip)
                    if ow == 0 or oh == 0:
                        continue
                    exp = orc.Gray(ow, oh); exp.buf[:] = -3.0
                    try:
                        orc.conv_down(kind, k, img, skip, out=exp)
                    except ValueError:
                        exp = None
                    out = api.GrayF32(ow, oh); out.data[:] = -3.0
                    fn = api.ConvolveImageDownNormalized.horizontal if kind == "h" else api.ConvolveImageDownNormalized.vertical
                    if exp is None:
                        with pytest.raises(api.IllegalArgumentException):
                            fn(api.Kernel1D_F32(k), G(api, img), out, skip)
                    else:
                        fn(api.Kernel1D_F32(k), G(api, img), out, skip)
                        assert np.array_equal(bits(out.array()), bits(exp.array())), (w, h, r, skip, kind)
                        cases += 1
    assert cases > 300
    # kernel that does not sum to one (interior plain sum vs normalised border), even width, sub-images, larger output
    img = rand.fillUniform(orc.Gray(64, 48), -5, 5)
    k = np.array([1, 2, 3, 2, 1], np.float32)
    sub = img.sub_image_of(4, 3)
    for kind in ("h", "v"):
        ow, oh = (40, 50) if kind == "h" else (70, 30)
        exp = orc.Gray(ow, oh).sub_image_of(2, 2, fill=9.0); exp.array()[:, :] = 4.0
        orc.conv_down(kind, k, sub, 2, out=exp)
        big = api.GrayF32(ow + 4, oh + 4); big.data[:] = 9.0
        out = big.subimage(2, 2, 2 + ow, 2 + oh); out.array()[:, :] = 4.0
        fn = api.ConvolveImageDownNormalized.horizontal if kind == "h" else api.ConvolveImageDownNormalized.vertical
        fn(api.Kernel1D_F32(k), G(api, sub), out, 2)
        assert np.array_equal(bits(big.data), bits(exp.buf)), kind
    for bad_skip, shape in [(0, (32, 48)), (2, (31, 48)), (2, (32, 47))]:
        with pytest.raises(api.IllegalArgumentException):
            api.ConvolveImageDownNormalized.horizontal(api.Kernel1D_F32(k), G(api, img), api.GrayF32(*shape), bad_skip)
    with pytest.raises(api.IllegalArgumentException):  # even kernel on the non-naive path
        api.ConvolveImageDownNormalized.horizontal(api.Kernel1D_F32(np.ones(4, np.float32)), G(api, img), api.GrayF32(32, 48), 2)


@pytest.mark.parametrize("w,h,scales,sigma,radius", [
    (80, 120, [1, 2, 4], -1, 3),        # TestPyramidDiscreteSampleBlur._update
    (41, 27, [1, 2, 4], -1, 3),         # odd sizes: ceil layer dims, last row/column stays 0
    (41, 27, [2, 4, 8], -1, 3),         # scale[0] != 1: layer 0 is convolved too
    (640, 480, [1, 2, 4, 8], -1, 2),    # FactoryPyramid.discreteGaussian(-1, 2) as the trackers configure it
    (333, 251, [1, 3, 6], 1.5, -1),
    (64, 64, [1, 1, 2], -1, 1),         # repeated scale: skip == 1 layer
    (1920, 1080, [1, 2, 4, 8, 16], -1, 2),
])
def test_pyramid_bit_exact(api, orc, w, h, scales, sigma, radius):
    img = orc.noise_image(w, h, 31, 0, 255)
    ker = orc.gaussian1d_f32(sigma, radius)
    exp_layers, exp_sig = orc.pyramid(ker, sigma, scales, img)
    pyr = api.FactoryPyramid.discreteGaussian(scales, sigma, radius)
    assert np.array_equal(bits(pyr.kernel.data), bits(ker))
    pyr.process(G(api, img))
    assert pyr.getNumLayers() == len(scales)
    for i, e in enumerate(exp_layers):
        got = pyr.getLayer(i)
        assert (got.height, got.width) == e.shape and (pyr.getWidth(i), pyr.getHeight(i)) == (e.shape[1], e.shape[0])
        assert np.array_equal(bits(got.array()), bits(e)), i
        assert pyr.getSigma(i) == exp_sig[i] and pyr.getSampleOffset(i) == 0 and pyr.getScale(i) == scales[i]
    # saveOriginalReference: layer 0 IS the input object
    if scales[0] == 1:
        inp = G(api, img)
        p2 = api.PyramidDiscreteSampleBlur(api.Kernel1D_F32(ker), sigma, True, scales).process(inp)
        assert p2.getLayer(0) is inp
        assert np.array_equal(bits(p2.getLayer(len(scales) - 1).array()), bits(exp_layers[-1]))


def test_pyramid_rejects_bad_scales(api, orc):
    ker = api.FactoryKernelGaussian.gaussian1D_F32(-1, 2)
    with pytest.raises(api.IllegalArgumentException):
        api.PyramidDiscreteSampleBlur(ker, 1.0, False, [2, 1])
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryKernelGaussian.gaussian1D_F32(-1, -1)


def test_pyramid_batched_device_equals_single(api, orc):
    """bhip_pyramid_dev_f32 over a batch of device frames == bhip_pyramid_f32 frame by frame (same stream, no host hop)."""
    torch = pytest.importorskip("torch")
    import ctypes as C
    from boofcv_amd import _lib
    L = _lib.load()
    ctx = api.Context.default()
    w, h, B, scales = 321, 200, 3, np.array([1, 2, 4, 8], np.int32)
    frames = np.stack([orc.noise_image(w, h, 50 + b, 0, 255).array() for b in range(B)])
    ker = api.FactoryKernelGaussian.gaussian1D_F32(-1, 2)
    dims = np.zeros(8, np.int32); offs = np.zeros(4, np.int64); total = C.c_longlong()
    assert L.bhip_pyramid_layout(w, h, scales.ctypes.data_as(_lib._ip), 4, dims.ctypes.data_as(_lib._ip), offs.ctypes.data_as(_lib._llp), C.byref(total)) == 0
    d_in = torch.from_numpy(frames).cuda()
    d_out = torch.full((B, total.value), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = L.bhip_pyramid_dev_f32(ctx._h, ker.data.ctypes.data_as(_lib._fp), ker.width, scales.ctypes.data_as(_lib._ip), 4, d_in.data_ptr(), w * h, w, w, h, B,
                                d_out.data_ptr())
    assert rc == 0, ctx.lastError()
    ctx.synchronize()
    got = d_out.cpu().numpy()
    for b in range(B):
        exp_layers, _ = orc.pyramid(ker.data, -1, scales, orc.Gray.from_array(frames[b]))
        for i, e in enumerate(exp_layers):
            assert np.array_equal(bits(got[b, offs[i]:offs[i] + e.size].reshape(e.shape)), bits(e)), (b, i)


def test_mean_median_conv2d_bit_exact(api, orc):
    """The remaining BOverride hooks: BlurImageOps.mean (float running sums in the reference's order), BlurImageOps.median (order
    statistic), ConvolveImageNoBorder.convolve (unrolled and standard 2-D forms); sub-images; argument checks."""
    rand = orc.JavaRandom(77)
    for (w, h) in [(25, 20), (200, 150), (640, 480), (5, 4)]:
        img = rand.fillUniform(orc.Gray(w, h), 0, 20)
        for radius in (1, 2, 3, 4):
            out = api.BlurImageOps.mean(G(api, img), None, radius)
            assert np.array_equal(bits(out.array()), bits(orc.blur_mean(img, radius).array())), (w, h, radius, "mean")
            if radius <= 3 or w * h < 50000:
                out = api.BlurImageOps.median(G(api, img), None, radius)
                assert np.array_equal(bits(out.array()), bits(orc.blur_median(img, radius).array())), (w, h, radius, "median")
        out = api.BlurImageOps.mean(G(api, img), None, 2, 1)
        assert np.array_equal(bits(out.array()), bits(orc.blur_mean(img, 2, 1).array()))
        for kw, off in [(3, 1), (5, 2), (7, 3), (4, 1), (2, 0)]:
            if kw > min(w, h):
                continue
            k = (np.arange(kw * kw, dtype=np.float32).reshape(kw, kw) - 3.5) / 11
            exp = orc.Gray(w, h); exp.buf[:] = 5.0
            orc.conv2d(k, off, img, exp)
            o = api.GrayF32(w, h); o.data[:] = 5.0
            api.ConvolveImageNoBorder.convolve(api.Kernel2D_F32(k, offset=off), G(api, img), o)
            assert np.array_equal(bits(o.array()), bits(exp.array())), (w, h, kw)
    sub = img.sub_image_of(3, 2)
    big = api.GrayF32(w + 8, h + 6); view = big.subimage(4, 3, 4 + w, 3 + h)
    api.BlurImageOps.mean(G(api, sub), view, 1)
    assert np.array_equal(bits(view.array()), bits(orc.blur_mean(img, 1).array())) and big.data[0] == 0
    for bad in (lambda: api.BlurImageOps.mean(G(api, img), None, 0), lambda: api.BlurImageOps.median(G(api, img), None, 0)):
        with pytest.raises(api.IllegalArgumentException):
            bad()


def test_brief_bit_exact(api, orc):
    sp, cp = orc.brief_definition()  # FactoryBriefDefinition.gaussian2(new Random(123), 16, 512), generated on the host side
    img = orc.noise_image(160, 120, 77)
    rng = np.random.default_rng(1)
    xy = np.concatenate([rng.uniform(0, 160, size=(200, 1)), rng.uniform(0, 120, size=(200, 1))], axis=1)
    xy = np.concatenate([xy, [[0, 0], [159.9, 119.9], [16, 16], [15.9, 50], [143, 103], [144, 104]]])
    b = api.DescribePointBrief(16, sp, cp); b.setImage(G(api, img))
    assert np.array_equal(b.processAll(xy), orc.brief_describe(img, xy, 16, sp, cp))
    f = api.TupleDesc_B(512); b.process(80.5, 60.2, f)
    assert np.array_equal(f.data, orc.brief_describe(img, [[80.5, 60.2]], 16, sp, cp)[0])


# ------------------------------------------------------------------------------------------------------------------ MFMA association path
def _assoc_exact_only(api, src, dst, maxErr, backwards):
    """the exact fp64 VALU kernels, reached through a non-64 code path: sqrtScore=0 but forced by a private context flag"""
    import os
    os.environ["BHIP_ASSOC_EXACT"] = "1"
    try:
        ctx = api.Context(0)
        a = api.FactoryAssociation.greedy(api.ScoreAssociateEuclideanSq_F64(), maxErr, backwards, ctx=ctx)
        a.setSource(src); a.setDestination(dst); a.associate()
        return a.getPairs().copy(), a.getFitQuality().copy()
    finally:
        del os.environ["BHIP_ASSOC_EXACT"]


def test_mfma_association_config3_and_tie_stress(api, orc):
    """BASELINE config 3: two 4096-key-point SURF-64 sets; B = A permuted + N(0,0.05) for 3072 rows, fresh for 1024."""
    rng = np.random.default_rng(1)
    A = _surf_like(rng, 4096)
    perm = rng.permutation(4096)
    Bm = A[perm].copy()
    Bm[:3072] += np.random.default_rng(2).normal(scale=0.05, size=(3072, 64))
    Bm[3072:] = _surf_like(np.random.default_rng(3), 1024)
    Bm /= np.linalg.norm(Bm, axis=1, keepdims=True)
    a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True, A, Bm)
    p, f = orc.associate_l2(A, Bm, api.Double_MAX_VALUE, True, threads=8)
    assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)
    assert (p >= 0).sum() > 2500
    pe, fe = _assoc_exact_only(api, A, Bm, api.Double_MAX_VALUE, True)
    assert np.array_equal(pe, p) and np.array_equal(fe, f)  # exact VALU path == MFMA path == oracle
    # tie stress: exact duplicates on both sides, near-duplicates one ulp apart
    A2 = A[:1500].copy(); A2[100:200] = A2[0:100]
    B2 = np.concatenate([A2[::-1], A2[:300]]); B2[5] = np.nextafter(B2[5], 2.0)
    for backwards in (False, True):
        for maxErr in (api.Double_MAX_VALUE, 1e-3):
            a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), maxErr, backwards, A2, B2)
            p, f = orc.associate_l2(A2, B2, maxErr, backwards, threads=8)
            assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)


def test_mfma_association_long_sweeps(api, orc, tmp_path):
    """The matrix-core filter keeps one column strip of a problem in LDS and walks the rows in wave tiles; a single problem normally has
    its rows split into chunks (to fill the chip), a batch does not.  Both plans are forced in child processes (BHIP_ASSOC_ROWSPLIT = 1:
    every block walks all rows of its strip; = 5: row chunks that meet in the global atomics) and compared with the oracle."""
    import os, subprocess, sys
    rng = np.random.default_rng(3)
    src = _surf_like(rng, 1500); dst = _surf_like(rng, 1300)
    dst[:800] = src[100:900] + rng.normal(scale=0.02, size=(800, 64)); dst[900] = dst[10]
    np.save(tmp_path / "s.npy", src); np.save(tmp_path / "d.npy", dst)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from boofcv_amd import api; "
            "a = api.FactoryAssociation.greedy(api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True); "
            "a.setSource(np.load(%r)); a.setDestination(np.load(%r)); a.associate(); np.save(%r, a.getPairs()); np.save(%r, a.getFitQuality())")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ep, ef = orc.associate_l2(src, dst, orc.MAX_VALUE_F64, True, threads=8)
    assert (ep >= 0).sum() > 700
    for split in ("1", "5"):
        e = dict(os.environ); e["BHIP_ASSOC_ROWSPLIT"] = split
        subprocess.run([sys.executable, "-c", code % (root, str(tmp_path / "s.npy"), str(tmp_path / "d.npy"), str(tmp_path / "p.npy"), str(tmp_path / "f.npy"))],
                       check=True, env=e, timeout=300)
        assert np.array_equal(np.load(tmp_path / "p.npy"), ep) and np.array_equal(np.load(tmp_path / "f.npy"), ef), split


def test_mfma_association_degenerate_inputs_fall_back(api, orc):
    z = np.zeros((300, 64)); one = np.tile(_surf_like(np.random.default_rng(0), 1), (260, 1))
    for src, dst in [(z, z), (one, one), (z, one)]:  # every pair is a candidate: list overflow -> exact path
        a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True, src, dst)
        p, f = orc.associate_l2(src, dst, api.Double_MAX_VALUE, True)
        assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)
    big = _surf_like(np.random.default_rng(4), 100) * 1e200  # norms overflow fp32: exact path
    a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True, big, big[::-1].copy())
    p, f = orc.associate_l2(big, big[::-1].copy(), api.Double_MAX_VALUE, True)
    assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)
    unnorm = np.random.default_rng(5).normal(size=(500, 64)) * np.random.default_rng(6).uniform(0.01, 100, size=(500, 1))  # wildly different norms
    a = _greedy(api, api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True, unnorm, unnorm[::-1] * 1.0000001)
    p, f = orc.associate_l2(unnorm, unnorm[::-1] * 1.0000001, api.Double_MAX_VALUE, True)
    assert np.array_equal(a.getPairs(), p) and np.array_equal(a.getFitQuality(), f)


def test_batched_device_association(api, orc):
    """bhip_assoc_l2_dev_batched: several (src,dst) problems that share one descriptor buffer, as bench.py uses it."""
    import ctypes as C
    import torch
    from boofcv_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(9)
    sizes = [700, 1, 350, 64, 129]
    sets = [_surf_like(rng, n) for n in sizes]
    sets[2][:300] = sets[0][:300] + rng.normal(scale=0.02, size=(300, 64))
    allrows = np.concatenate(sets)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    dev = torch.from_numpy(allrows).cuda()
    n = len(sizes)
    src_off = np.ascontiguousarray(starts[:n]); dst_idx = (np.arange(n) + 2) % n
    dst_off = np.ascontiguousarray(starts[dst_idx]); ns = np.array(sizes, np.int32); nd = np.ascontiguousarray(ns[dst_idx])
    pairs = torch.full((len(allrows),), -7, dtype=torch.int32, device="cuda"); fit = torch.zeros(len(allrows), dtype=torch.float64, device="cuda")
    ctx = api.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    LL, I = C.POINTER(C.c_longlong), C.POINTER(C.c_int)
    st = L.bhip_assoc_l2_dev_batched(ctx._h, C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr()), 64, n, src_off.ctypes.data_as(LL), ns.ctypes.data_as(I),
                                     dst_off.ctypes.data_as(LL), nd.ctypes.data_as(I), api.Double_MAX_VALUE, 1, C.c_void_p(pairs.data_ptr()),
                                     C.c_void_p(fit.data_ptr()))
    assert st == 0, L.bhip_last_error(ctx._h)
    torch.cuda.synchronize()
    pairs, fit = pairs.cpu().numpy(), fit.cpu().numpy()
    for k in range(n):
        p, f = orc.associate_l2(sets[k], sets[dst_idx[k]], api.Double_MAX_VALUE, True)
        assert np.array_equal(pairs[starts[k]:starts[k + 1]], p) and np.array_equal(fit[starts[k]:starts[k + 1]], f), k


def test_orientation_degenerate_regimes(api, orc):
    """Planar ramps (all gradients parallel: the sliding window wraps the full circle), flat patches (all angles equal) and points
    whose sample grid leaves the image (zero gradients) -- GenericOrientationIntegralTests.java:98-170 through the full pipeline."""
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    ref = orc.Surf(True)
    yy, xx = np.mgrid[0:100, 0:120]
    for k, theta in enumerate([0.0, 0.5, math.pi / 2, 2.0, -1.2, 3.0, -3.1]):
        a = (10 * (xx * math.cos(theta) + yy * math.sin(theta))).astype(np.float32)
        img = orc.Gray.from_array(a + 500.0)
        dd.detect(G(api, img))
        pts = np.array([[60, 50, 2.0], [60.5, 50.25, 3.7], [30, 70, 1.2], [2, 2, 2.0], [118, 97, 2.5], [60, 3, 5.0]])
        ang, white, desc = dd.describePoints(pts)
        ref.describe_points(pts, img)
        _, rang, rwhite, rdesc = ref.fetch()
        assert np.max(np.abs(np.angle(np.exp(1j * (ang - rang))))) < 1e-9, theta
        assert np.max(np.abs(desc - rdesc)) <= DESC_TOL and np.array_equal(white, rwhite)
        assert abs(np.angle(np.exp(1j * (ang[0] - theta)))) < math.pi / 9
    flat = orc.Gray.from_array(np.full((100, 120), 50, np.float32))
    dd.detect(G(api, flat))
    ang, white, desc = dd.describePoints(pts)
    ref.describe_points(pts, flat)
    _, rang, rwhite, rdesc = ref.fetch()
    assert np.array_equal(ang, rang) and np.array_equal(desc, rdesc) and np.all(desc == 0)


@pytest.mark.parametrize("w,h,seed,hi", [(700, 520, 21, 255), (400, 300, 6, 100), (403, 301, 8, 100)])
def test_detector_plans_agree(api, orc, tmp_path, w, h, seed, hi):
    """The detector's execution plans must give the same key points bit for bit: fused octaves + levels shared between octaves + outer
    levels of the stand-alone octaves evaluated on demand (default), no sharing (BHIP_DETECT_NOSHARE=1), the stand-alone kernels for every
    octave (BHIP_DETECT_UNFUSED=1, with and without sharing), and every level computed densely (BHIP_DETECT_DENSE=1).  The switches are
    read by the child processes the variants run in."""
    import os, subprocess, sys
    # (400, 300, 6): a key point next to the column where octave 1 evaluates size 27 with the border form and octave 0 with the inner form
    img = orc.noise_image(w, h, seed, 0, hi)
    np.save(tmp_path / "img.npy", img.array())
    fh = api.FastHessianFeatureDetector(api.ConfigFastHessian(1, 2, -1, 1, 9, 4, 4))
    ii = api.IntegralImageOps.transform(G(api, img))
    fh.detect(ii)
    base = fh.getFoundPoints().copy()
    assert len(base) > 500 and np.array_equal(base, orc.fh_detect(orc.integral(img), orc.FhCfg()))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from boofcv_amd import api; "
            "a = np.load(%r); fh = api.FastHessianFeatureDetector(api.ConfigFastHessian(1, 2, -1, 1, 9, 4, 4)); "
            "fh.detect(api.IntegralImageOps.transform(api.GrayF32.wrap(a))); "
            "np.save(%r, fh.getFoundPoints())")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for k, env in enumerate([{"BHIP_DETECT_NOSHARE": "1"}, {"BHIP_DETECT_UNFUSED": "1"}, {"BHIP_DETECT_UNFUSED": "1", "BHIP_DETECT_NOSHARE": "1"},
                             {"BHIP_DETECT_DENSE": "1"}, {"BHIP_DETECT_UNFUSED": "1", "BHIP_DETECT_DENSE": "1"}]):
        out = str(tmp_path / ("kp%d.npy" % k))
        e = dict(os.environ); e.update(env)
        subprocess.run([sys.executable, "-c", code % (root, str(tmp_path / "img.npy"), out)], check=True, env=e, timeout=300)
        assert np.array_equal(np.load(out), base), env


@pytest.mark.parametrize("stable", [True, False])
def test_surf_color_planar_parity(api, orc, stable):
    """FactoryDetectDescribe.surfColorStable / surfColorFast on Planar<GrayF32>: key points from the band average bit-exact,
    192-value descriptors inside the 1e-5 bar, Laplacian sign from the average, getRadius == scale; sub-image bands; band-count check."""
    rand = orc.JavaRandom(234)
    for (w, h, nb) in [(150, 120, 3), (200, 160, 3), (120, 100, 2), (90, 80, 4)]:
        bands = [rand.fillUniform(orc.Gray(w, h), 0, 200) for _ in range(nb)]
        ref = orc.Surf(stable)
        n = ref.detect_planar(bands, threads=4)
        pts, ang, white, desc = ref.fetch()
        fac = api.FactoryDetectDescribe.surfColorStable if stable else api.FactoryDetectDescribe.surfColorFast
        dd = fac(None, None, None, api.PlanarType(nb))
        dd.detect(api.Planar.wrap([G(api, b) for b in bands]))
        got = dd._results()
        assert n > 10 and dd.getNumberOfFeatures() == n and dd.createDescription().size() == 64 * nb
        assert np.array_equal(got[0], pts) and np.array_equal(got[2], white)
        assert np.max(np.abs(np.angle(np.exp(1j * (got[1] - ang))))) < 1e-9
        derr = np.max(np.abs(got[3] - desc), axis=1)
        assert int((derr > DESC_TOL).sum()) == 0, (w, h, nb, int((derr > DESC_TOL).sum()), derr.max())
        assert dd.getRadius(0) == pts[0, 2] and dd.getOrientation(0) == got[1][0]
        # sub-image bands (shared startIndex / stride)
        dd.detect(api.Planar.wrap([G(api, b.sub_image_of()) for b in bands]))
        sub = dd._results()
        assert all(np.array_equal(a, b) for a, b in zip(got, sub))
    with pytest.raises(api.IllegalArgumentException):
        dd.detect(api.Planar.wrap([G(api, bands[0])]))
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryDetectDescribe.surfColorStable(None, None, None, api.GrayF32)


def test_select_nbest_reference_literals(api):  # FT:alg/feature/detect/extract/TestSelectNBestFeatures.java:36-93
    a = np.zeros((20, 10), np.float32)
    a[10, 5] = -3; a[10, 4] = -3.5; a[11, 5] = 0; a[8, 8] = 10
    corners = [api.Point2D_I16(5, 10), api.Point2D_I16(4, 10), api.Point2D_I16(5, 11), api.Point2D_I16(8, 8)]
    alg = api.SelectNBestFeatures(20)
    alg.setN(3)
    alg.process(api.GrayF32.wrap(a), corners, True)
    found = alg.getBestCorners()
    assert len(found) == 3 and (found[0].x, found[0].y) == (8, 8)
    alg.process(api.GrayF32.wrap(a), corners, False)
    found = alg.getBestCorners()
    assert len(found) == 3 and (found[0].x, found[0].y) == (4, 10)
    alg.setN(20)   # testTooLittle: fewer corners than N, all are returned
    alg.process(api.GrayF32.wrap(a), corners, True)
    assert [(p.x, p.y) for p in alg.getBestCorners()] == [(5, 10), (4, 10), (5, 11), (8, 8)]
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayF32.wrap(a), [api.Point2D_I16(10, 3)], True)   # outside the image


@pytest.mark.parametrize("w,h", [(40, 50), (320, 240), (1920, 1080), (7, 9)])
def test_corner_intensity_and_general_detector(api, orc, w, h):
    """Shi-Tomasi / Harris gradient corner intensity (running box sums in the reference's order: bit-exact), then
    GeneralFeatureDetector = intensity -> strict non-maximum suppression."""
    img = orc.noise_image(w, h, 234)
    dxo, dyo = orc.gradient("sobel", img, border_zero=True)
    dx, dy = api.GrayF32(w, h), api.GrayF32(w, h)
    api.GradientSobel.process(G(api, img), dx, dy, 0)
    for radius in (1, 2, 3):
        if 2 * radius + 1 > min(w, h):
            continue
        for alg, kind, kappa in [(api.FactoryIntensityPointAlg.shiTomasi(radius, False, api.GrayF32), "shitomasi", 0.0),
                                 (api.FactoryIntensityPointAlg.harris(radius, 0.04, False, api.GrayF32), "harris", 0.04)]:
            inten = api.GrayF32(1, 1)
            alg.process(dx, dy, inten)
            exp = orc.corner_intensity(dxo, dyo, radius, kind, kappa)
            assert np.array_equal(bits(inten.array()), bits(exp)), (radius, kind)
            assert alg.getRadius() == radius and alg.getIgnoreBorder() == radius
    if min(w, h) >= 40:
        cfg = api.ConfigExtract(radius=2, threshold=1.0, ignoreBorder=0)
        det = api.GeneralFeatureDetector(api.FactoryIntensityPointAlg.shiTomasi(2, False, api.GrayF32), api.FactoryFeatureExtractor.nonmax(cfg))
        det.process(G(api, img), dx, dy)
        got = [(p.x, p.y) for p in det.getMaximums()]
        exp = orc.nonmax(orc.Gray.from_array(orc.corner_intensity(dxo, dyo, 2, "shitomasi")), 2, 1.0, 2)
        assert len(got) > 5 and got == [(int(x), int(y)) for x, y in exp]
        # maxFeatures > 0: SelectNBestFeatures on the maxima (GeneralFeatureDetector.java:143-160); same QuickSelect exchange sequence as the oracle
        inten_o = orc.Gray.from_array(orc.corner_intensity(dxo, dyo, 2, "shitomasi"))
        for nmax in (1, 10, len(exp) - 1, len(exp), len(exp) + 5):
            det.setMaxFeatures(nmax)
            det.process(G(api, img), dx, dy)
            got = [(p.x, p.y) for p in det.getMaximums()]
            want = orc.select_nbest(inten_o, exp, nmax, positive=True)
            assert got == [(int(x), int(y)) for x, y in want], nmax
        sel = api.SelectNBestFeatures(3)
        sel.process(det.getIntensity(), [api.Point2D_I16(int(x), int(y)) for x, y in exp], False)   # negative: the least intense
        assert [(p.x, p.y) for p in sel.getBestCorners()] == [(int(x), int(y)) for x, y in orc.select_nbest(inten_o, exp, 3, positive=False)]
    with pytest.raises(api.IllegalArgumentException):
        api.FactoryIntensityPointAlg.shiTomasi(5, False, api.GrayF32).process(api.GrayF32(6, 6), api.GrayF32(6, 6), api.GrayF32(1, 1))


def test_integer_variants_stage_level(api, orc):
    """SURVEY 8f-4 at stage level: GrayU8 -> GrayS32 integral image (exact), Hessian intensity from the S32 integral image (bit-exact),
    BRIEF-512 on GrayU8 (inside and border forms)."""
    rng = np.random.default_rng(12)
    for (w, h) in [(60, 70), (640, 480), (1920, 1080), (1, 1), (65, 3), (130, 200)]:
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        ii = api.IntegralImageOps.transform(api.GrayU8.wrap(img))
        assert isinstance(ii, api.GrayS32) and np.array_equal(ii.array(), orc.integral_u8(img))
        if w >= 60 and h >= 70:
            for skip, size in [(1, 9), (1, 27), (2, 15), (2, 51), (4, 27), (3, 9)]:
                if size > min(w, h):
                    continue
                inten = api.GrayF32(w // skip, h // skip)
                api.IntegralImageFeatureIntensity.hessian(ii, skip, size, inten)
                assert np.array_equal(bits(inten.array()), bits(orc.hessian_s32(ii.array(), skip, size))), (w, h, skip, size)
    # sub-image views
    img = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    big = np.zeros((60, 80), np.uint8); big[5:53, 7:71] = img
    sub = api.GrayU8(64, 48, big.reshape(-1), 5 * 80 + 7, 80)
    out = api.GrayS32(70, 50).subimage(3, 1, 67, 49)
    api.IntegralImageOps.transform(sub, out)
    assert np.array_equal(out.array(), orc.integral_u8(img))
    # BRIEF on GrayU8
    sp, cp = orc.brief_definition()
    img = rng.integers(0, 256, (120, 160), dtype=np.uint8)
    xy = np.concatenate([rng.uniform(0, 160, (200, 1)), rng.uniform(0, 120, (200, 1))], axis=1)
    xy = np.concatenate([xy, [[0, 0], [159.9, 119.9], [16, 16], [15.9, 50], [143, 103], [144, 104]]])
    b = api.DescribePointBrief(16, sp, cp); b.setImage(api.GrayU8.wrap(img))
    assert np.array_equal(b.processAll(xy), orc.brief_describe_u8(img, xy, 16, sp, cp))


@pytest.mark.parametrize("w,h,seed", [(100, 120, 1), (400, 300, 2), (641, 479, 3), (1920, 1080, 4)])
def test_fast_hessian_on_s32_integral(api, orc, w, h, seed):
    """FastHessianFeatureDetector<GrayS32> on the integral image of a GrayU8 frame: fused octaves on integer taps, the
    shared levels, the stand-alone kernels -- key points bit-exact and in the reference's order."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = (127 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 25, (h, w))).clip(0, 255).astype(np.uint8)
    ii = api.IntegralImageOps.transform(api.GrayU8.wrap(img))
    for cfg, ocfg in [(api.ConfigFastHessian(), orc.FhCfg()),
                      (api.ConfigFastHessian(detectThreshold=20.0, extractRadius=1, initialSize=9, numberScalesPerOctave=4, numberOfOctaves=3),
                       orc.FhCfg(20.0, 1, -1, 1, 9, 4, 3, 6))]:
        fh = api.FastHessianFeatureDetector(cfg)
        fh.detect(ii)
        exp = orc.fh_detect_s32(ii.array(), ocfg, threads=8)
        assert len(exp) > 10 and np.array_equal(fh.getFoundPoints(), exp), (w, h)


@pytest.mark.parametrize("stable", [True, False])
def test_surf_on_gray_u8(api, orc, stable):
    """FactoryDetectDescribe.surfStable / surfFast(..., GrayU8): GrayS32 integral image, every stage on integer taps.
    Key points and Laplacian signs bit-exact, descriptors inside the 1e-5 bar; a batch equals frame by frame; sub-image frames; and on a
    frame small enough for a float integral image to be exact, the GrayU8 and the GrayF32 pipelines agree."""
    rng = np.random.default_rng(31)
    frames = []
    for (w, h) in [(240, 200), (640, 480), (1920, 1080)]:
        yy, xx = np.mgrid[0:h, 0:w]
        frames.append((127 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 25, (h, w))).clip(0, 255).astype(np.uint8))
    fac = api.FactoryDetectDescribe.surfStable if stable else api.FactoryDetectDescribe.surfFast
    dd = fac(None, None, None, api.GrayU8)
    ref = orc.Surf(stable)
    for img in frames:
        dd.detect(api.GrayU8.wrap(img))
        got = dd._results()
        n = ref.detect_u8(img, threads=8)
        pts, ang, white, desc = ref.fetch()
        assert n > 100 and np.array_equal(got[0], pts) and np.array_equal(got[2], white)
        assert np.abs(np.angle(np.exp(1j * (got[1] - ang)))).max() < 1e-12
        derr = np.max(np.abs(got[3] - desc), axis=1)
        assert int((derr > DESC_TOL).sum()) == 0, (img.shape, int((derr > DESC_TOL).sum()), derr.max())
    # batch of equal-sized frames == frame by frame; sub-image input
    a, b = frames[0], np.ascontiguousarray(frames[1][:200, :240])
    dd.detectBatch([api.GrayU8.wrap(a), api.GrayU8.wrap(b)])
    batch = [tuple(np.array(x) for x in dd._results(i)) for i in range(2)]
    big = np.zeros((220, 260), np.uint8); big[10:210, 12:252] = a
    for i, im in enumerate([api.GrayU8(240, 200, big.reshape(-1), 10 * 260 + 12, 260), api.GrayU8.wrap(b)]):
        dd.detect(im)
        assert all(np.array_equal(x, y) for x, y in zip(dd._results(), batch[i]))
    # 240 x 200 x 255 < 2^24: the float integral image is exact, so the float pipeline on the same pixel values gives the same features
    ddf = fac(None, None, None, api.GrayF32)
    ddf.detect(api.GrayF32.wrap(a.astype(np.float32)))
    f = ddf._results()
    assert np.array_equal(f[0], batch[0][0]) and np.array_equal(f[2], batch[0][2]) and np.max(np.abs(f[3] - batch[0][3])) < 1e-12


def test_associate_surf_basic(api, orc):
    """AssociateSurfBasic / WrapAssociateSurfBasic (TestAssociateSurfBasic.java literals + detected SURF features of two noise images)."""
    def feats(desc, white):
        return [api.BrightFeature(64, np.asarray(d, dtype=np.float64), bool(w)) for d, w in zip(desc, white)]

    def run(sd, sw, dd, dw, score, maxErr, backwards):
        alg = api.WrapAssociateSurfBasic(api.AssociateSurfBasic(api.FactoryAssociation.greedy(score, maxErr, backwards)))
        alg.setSource(feats(sd, sw)); alg.setDestination(feats(dd, dw)); alg.associate()
        return [(m.src, m.dst, m.fitScore) for m in alg.getMatches()], list(alg.getUnassociatedSource()), list(alg.getUnassociatedDestination())

    d = lambda vals: np.pad(np.asarray(vals, dtype=np.float64)[:, None], ((0, 0), (0, 63)))
    eu = api.ScoreAssociateEuclidean_F64()
    m, us, ud = run(d([10]), [True], d([0, 10]), [True, False], eu, 20, True)
    assert [(a, b) for a, b, _ in m] == [(0, 0)] and us == [] and ud == [1]
    sd, sw, dd, dw = d([10, 12, 5, 2344, 1000]), [True, True, False, False, False], d([0, 10.1, 13, 0.1, 7]), [True, True, True, False, False]
    m, us, ud = run(sd, sw, dd, dw, eu, 20, True)
    em, eus = orc.associate_surf_basic(sd, sw, dd, dw, 20, True, sqrt_score=True)
    assert m == em and us == eus and [(a, b) for a, b, _ in m] == [(0, 1), (1, 2), (2, 4)]
    assert run(np.zeros((0, 64)), [], d([10]), [True], eu, 20, True)[0] == []
    # real features
    dd_ = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    sets = []
    for seed in (5, 6):
        dd_.detect(G(api, orc.noise_image(240, 180, seed)))
        n = dd_.getNumberOfFeatures()
        sets.append((np.array([dd_.getDescription(i).value for i in range(n)]), [dd_.getDescription(i).white for i in range(n)]))
    (a, aw), (b, bw) = sets
    for backwards in (True, False):
        m, us, ud = run(a, aw, b, bw, api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, backwards)
        em, eus = orc.associate_surf_basic(a, aw, b, bw, orc.MAX_VALUE_F64, backwards)
        assert m == em and us == eus and len(m) > 50
        assert all(aw[i] == bw[j] for i, j, _ in m)


def test_describe_internal_paths_agree(api, orc):
    """The 32-bit-key sort (with its fp64 check and fallback) must order exactly like the fp64 (angle, index) sort, and the parallel
    window enumeration must pick the reference's window: angles and descriptors with BHIP_DESCRIBE_SORT64 / BHIP_DESCRIBE_SERIAL are
    compared against the default path.  Includes images built to produce many equal / nearly equal gradient directions."""
    import os
    rng = np.random.default_rng(5)
    imgs = [orc.noise_image(320, 240, 11)]
    yy, xx = np.mgrid[0:240, 0:320]
    imgs.append(orc.Gray.from_array((np.round(20 * np.sin(xx / 7.0) + 20 * np.cos(yy / 5.0)) * 4 + 100).astype(np.float32)))  # quantised: many exact ties
    imgs.append(orc.Gray.from_array((rng.integers(0, 4, (240, 320)) * 25).astype(np.float32)))                                  # 4 grey levels
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    for img in imgs:
        dd.detect(G(api, img))
        n = dd.getNumberOfFeatures()
        pts = np.array([[dd.getLocation(i).x, dd.getLocation(i).y, dd.getRadius(i) / 2.0] for i in range(min(n, 400))])
        if len(pts) == 0:
            continue
        base = dd.describePoints(pts)
        for var in ("BHIP_DESCRIBE_SORT64", "BHIP_DESCRIBE_SERIAL"):
            os.environ[var] = "1"
            try:
                other = dd.describePoints(pts)
            finally:
                del os.environ[var]
            if var == "BHIP_DESCRIBE_SORT64":
                assert np.array_equal(base[0], other[0]) and np.array_equal(base[2], other[2]), var   # same order -> same bits
            else:
                assert np.max(np.abs(np.angle(np.exp(1j * (base[0] - other[0]))))) < 1e-9 and np.max(np.abs(base[2] - other[2])) <= 1e-9, var
            assert np.array_equal(base[1], other[1])


def test_page_locked_boundary_arrays(api, orc):
    """bhip_host_alloc / bhip_host_free and the pool the Python mirror builds on them: the arrays _results() and associate() hand out live in
    page-locked blocks that are recycled when the arrays die, stay readable after their context is closed, and give the same numbers as
    ordinary (pageable) arrays."""
    import ctypes as C
    import gc
    from boofcv_amd import _lib
    L = _lib.load()
    ctx = api.Context(0)
    p = C.c_void_p()
    assert L.bhip_host_alloc(ctx._h, 0, C.byref(p)) == _lib.BHIP_ERR_INVALID and not p.value
    assert L.bhip_host_alloc(ctx._h, 1 << 20, C.byref(p)) == _lib.BHIP_OK and p.value
    a = np.frombuffer((C.c_uint8 * (1 << 20)).from_address(p.value), dtype=np.float64)
    a[:] = 3.0
    assert a.sum() == 3.0 * a.size
    del a
    assert L.bhip_host_free(p) == _lib.BHIP_OK and L.bhip_host_free(None) == _lib.BHIP_OK
    img = orc.noise_image(320, 240, 77)
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32, ctx=ctx)
    dd.detect(G(api, img))
    xys, ang, white, desc = dd._results(0)
    n = len(xys)
    assert n > 50 and desc.shape == (n, 64)
    addr = desc.ctypes.data
    pageable = np.array(desc)             # an ordinary copy
    assoc = api.FactoryAssociation.greedy(api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True, ctx=ctx)
    assoc.setSource(desc); assoc.setDestination(desc[::-1].copy()); assoc.associate()
    pinned_pairs = np.array(assoc.getPairs())
    assoc.setSource(pageable); assoc.setDestination(pageable[::-1].copy()); assoc.associate()
    assert np.array_equal(pinned_pairs, assoc.getPairs()) and np.array_equal(pinned_pairs, np.arange(n)[::-1])
    assert [m.src for m in assoc.getMatches()] == list(range(n)) and assoc.getUnassociatedSource() == []
    # the block goes back to the pool when the last array on it dies, and the next fetch of the same size takes it again
    del xys, ang, white, desc
    dd._cache.clear()
    gc.collect()
    again = dd._results(0)
    assert again[3].ctypes.data == addr and np.array_equal(again[3], pageable)
    keep = again[3]
    ctx.close()                            # the arrays outlive the context
    assert np.array_equal(keep, pageable)


@pytest.mark.parametrize("kind", ["l2", "hamming"])
def test_sharded_association_single_process_ranks(api, orc, kind):
    """SURVEY 8e on one GPU: R simulated ranks run phase 1 on their row slices, the column records are concatenated exactly as
    all_gather_into_tensor would, and phase 2 must reproduce the slices of the unsharded result (the gloo test covers the collective)."""
    import torch
    from boofcv_amd import sharded
    rng = np.random.default_rng(11)
    ns, nd = 1000, 900
    if kind == "l2":
        src = _surf_like(rng, ns); dst = _surf_like(rng, nd)
        dst[:500] = src[100:600] + rng.normal(scale=0.03, size=(500, 64)); src[900:950] = src[0:50]; dst[800:820] = dst[0:20]
        full_p, full_f = orc.associate_l2(src, dst, api.Double_MAX_VALUE, True, threads=8)
    else:
        src = rng.integers(-2**31, 2**31, size=(ns, 16), dtype=np.int64).astype(np.int32)
        dst = rng.integers(-2**31, 2**31, size=(nd, 16), dtype=np.int64).astype(np.int32)
        dst[:400] = src[200:600]; dst[5] ^= 9; src[990] = src[250]
        full_p, full_f = orc.associate_hamming(src, dst, api.Double_MAX_VALUE, True, threads=8)
    eng = sharded.GpuEngine(device=0)
    ts, td = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    for R in (1, 2, 3, 8):
        part = sharded.row_partition(ns, R)
        locals_ = [eng.phase1(kind, ts[b:b + c].contiguous(), b, td, api.Double_MAX_VALUE) for b, c in part]
        col_all = torch.cat([l[2] for l in locals_])
        for (b, c), (p, f, _) in zip(part, locals_):
            p2, f2 = eng.phase2(col_all, R, nd, p.clone(), f.clone(), b)
            torch.cuda.synchronize()
            assert np.array_equal(p2.cpu().numpy(), full_p[b:b + c]) and np.array_equal(f2.cpu().numpy(), full_f[b:b + c]), (kind, R, b)


# ------------------------------------------------------------------------------------------------------------------ device-batched ip front end
@pytest.mark.parametrize("w,h,B", [(64, 40, 3), (260, 70, 2), (257, 33, 2), (1024, 37, 1), (31, 29, 2)])
def test_device_batched_ip_ops(api, orc, w, h, B):
    """bhip_*_dev_f32 on [B,H,W] device batches == the oracle image by image, bit for bit: tiled (16-byte aligned rows) and general
    kernels, strided views, every border class of the normalised convolution, both gradient border policies, NMS lists in block order."""
    torch = pytest.importorskip("torch")
    from boofcv_amd import device as dv
    ops = dv.DeviceImageOps(api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream))   # same stream as the torch fills below
    frames = [orc.noise_image(w, h, 900 + b, 0, 255) for b in range(B)]
    host = np.stack([f.array() for f in frames])
    dense = torch.from_numpy(host).cuda()
    # a strided view: rows padded to a multiple of 4 floats (tiled kernels) or to an odd pitch (general kernels)
    views = [dense]
    for pitch in ((w + 3) // 4 * 4 + 8, w + 3):
        big = torch.full((B, h + 2, pitch), -7.0, dtype=torch.float32, device="cuda")
        big[:, 1:h + 1, :w] = dense
        views.append(big[:, 1:h + 1, :w])
    torch.cuda.synchronize()
    for src in views:
        for r in (1, 2, 5, 6, 20):
            k = orc.gaussian1d_f32(-1, r)
            for kind, fn in [("h", ops.convolveHorizontal), ("v", ops.convolveVertical), ("norm_h", ops.convolveNormalizedHorizontal),
                             ("norm_v", ops.convolveNormalizedVertical)]:
                if not kind.startswith("norm") and len(k) > min(w, h):
                    continue
                out = torch.full_like(dense, 3.0)
                fn(k, r, src, out)
                ops.ctx.synchronize()
                got = out.cpu().numpy()
                for b in range(B):
                    exp = orc.conv(kind, k, r, frames[b]).array().copy()
                    if not kind.startswith("norm"):   # the frame keeps the caller's pixels
                        keep = np.ones((h, w), bool)
                        if kind == "h":
                            keep[:, r:w - r] = False
                        else:
                            keep[r:h - r, :] = False
                        exp[keep] = 3.0
                    assert np.array_equal(bits(got[b]), bits(exp)), (kind, r, b, tuple(src.stride()))
        k4 = np.array([0.1, 0.5, -0.2, 0.3], np.float32)   # even width, off-centre origin: the standard (not unrolled) form
        for kind, fn in [("norm_h", ops.convolveNormalizedHorizontal), ("norm_v", ops.convolveNormalizedVertical)]:
            got = fn(k4, 1, src)
            ops.ctx.synchronize()
            for b in range(B):
                assert np.array_equal(bits(got[b].cpu().numpy()), bits(orc.conv(kind, k4, 1, frames[b]).array())), kind
        for sigma, radius in [(-1, 2), (2.0, -1)]:
            got = ops.gaussian(src, sigma, radius)
            ops.ctx.synchronize()
            for b in range(B):
                assert np.array_equal(bits(got[b].cpu().numpy()), bits(orc.gaussian_blur(frames[b], sigma, radius).array())), (sigma, radius, b)
        for kind, fn in [("sobel", ops.sobel), ("three", ops.three)]:
            for border in (None, 0):
                dx = torch.full_like(dense, 7.0); dy = torch.full_like(dense, 7.0)
                fn(src, border, dx, dy)
                ops.ctx.synchronize()
                for b in range(B):
                    ex, ey = orc.gradient(kind, frames[b], border_zero=border is not None)
                    ex, ey = ex.array().copy(), ey.array().copy()
                    if border is None:
                        for e in (ex, ey):
                            e[[0, -1], :] = 7; e[:, [0, -1]] = 7
                    assert np.array_equal(bits(dx[b].cpu().numpy()), bits(ex)) and np.array_equal(bits(dy[b].cpu().numpy()), bits(ey)), (kind, border, b)
    # gradient magnitude images + strict NMS lists (block-raster order) + corner intensity, per image
    dx, dy = ops.sobel(dense, 0)
    for kind in (dv.INTENSITY_E, dv.INTENSITY_ABS, dv.INTENSITY_SQ):
        inten = ops.intensity(kind, dx, dy)
        ops.ctx.synchronize()
        gx, gy = dx.cpu().numpy(), dy.cpu().numpy()
        exp = [np.sqrt(gx * gx + gy * gy), np.abs(gx) + np.abs(gy), gx * gx + gy * gy][kind]
        assert np.array_equal(bits(inten.cpu().numpy()), bits(exp.astype(np.float32))), kind
        for radius, thr, border in [(2, 100.0, 0), (1, 0.0, 3), (3, 2000.0, 1)]:
            xy, n = ops.nonmax(inten, radius, thr, border)
            ops.ctx.synchronize()
            xy, n = xy.cpu().numpy(), n.cpu().numpy()
            for b in range(B):
                e = orc.nonmax(orc.Gray.from_array(exp[b].astype(np.float32)), radius, thr, border)
                assert n[b] == len(e) and np.array_equal(xy[b, :n[b]], np.asarray(e, np.int16).reshape(-1, 2)), (kind, radius, b)
    if w > 8 and h > 8:
        for kname, kind, kappa in [("shitomasi", 0, 0.0), ("harris", 1, 0.04)]:
            got = ops.cornerIntensity(kind, 2, kappa, dx, dy)
            ops.ctx.synchronize()
            for b in range(B):
                e = orc.corner_intensity(orc.Gray.from_array(dx[b].cpu().numpy()), orc.Gray.from_array(dy[b].cpu().numpy()), 2, kname, kappa)
                assert np.array_equal(bits(got[b].cpu().numpy()), bits(e)), (kname, b)
    # BRIEF over the batch == per image
    sp, cp = orc.brief_definition()
    rng = np.random.default_rng(w * 1000 + h)
    counts = [int(c) for c in rng.integers(0, 40, B)]
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    pts = np.stack([rng.uniform(-2, w + 2, start[-1]), rng.uniform(-2, h + 2, start[-1])], axis=1)
    if start[-1] > 0:
        words = ops.brief(dense, 16, sp, cp, torch.from_numpy(pts).cuda(), start).cpu().numpy()
        for b in range(B):
            if counts[b]:
                assert np.array_equal(words[start[b]:start[b + 1]], orc.brief_describe(frames[b], pts[start[b]:start[b + 1]], 16, sp, cp)), b


def test_batch_level_fetch_and_resident_association(api, orc):
    """bhip_surf_fetch_all == the per-image bhip_surf_fetch slices; bhip_assoc_l2_surf (descriptors still resident from the detect) ==
    bhip_assoc_l2_f64 on the fetched descriptors == the oracle's greedy association, pairs and scores identical."""
    frames = [orc.noise_image(200, 150, 40 + i) for i in range(4)] + [orc.Gray(200, 150)]   # the last frame is blank: no key points
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    dd.detectBatch([G(api, f) for f in frames])
    xys, ang, white, desc, starts = dd.fetchAll()
    assert starts[-1] == dd.totalFeatures() and starts[-1] == starts[-2]
    for i in range(len(frames)):
        one = dd._results(i)
        sl = slice(int(starts[i]), int(starts[i + 1]))
        assert np.array_equal(xys[sl], one[0]) and np.array_equal(ang[sl], one[1]) and np.array_equal(white[sl], one[2]) and np.array_equal(desc[sl], one[3])
    src = np.array([0, 1, 2, 3, 4], np.int32)
    dst = np.array([1, 2, 3, 4, 0], np.int32)
    for backwards in (True, False):
        for maxErr in (api.Double_MAX_VALUE, 0.2):
            pairs, fit = dd.associateImages(src, dst, maxErr, backwards)
            for a, b in zip(src, dst):
                sa = slice(int(starts[a]), int(starts[a + 1]))
                db = desc[int(starts[b]):int(starts[b + 1])]
                ep, ef = orc.associate_l2(desc[sa], db, maxErr, backwards)
                assert np.array_equal(pairs[sa], ep) and np.array_equal(fit[sa], ef), (a, b, backwards, maxErr)
    # images that are the source of no problem read "no match" (-1, 0.0), whatever an earlier call left in the library's scratch
    pairs, fit = dd.associateImages([1, 3], [2, 4])
    for a in (0, 2, 4):
        sa = slice(int(starts[a]), int(starts[a + 1]))
        assert np.all(pairs[sa] == -1) and np.all(fit[sa] == 0.0), a
    for a, b in ((1, 2), (3, 4)):
        sa = slice(int(starts[a]), int(starts[a + 1]))
        ep, ef = orc.associate_l2(desc[sa], desc[int(starts[b]):int(starts[b + 1])], api.Double_MAX_VALUE, True)
        assert np.array_equal(pairs[sa], ep) and np.array_equal(fit[sa], ef)
    with pytest.raises(api.IllegalArgumentException):
        dd.associateImages([0, 0], [1, 2])       # an image may be the source of one problem per call
    with pytest.raises(api.IllegalArgumentException):
        dd.associateImages([0], [7])


@pytest.mark.parametrize("u8", [False, True])
def test_chunked_host_batch_equals_plain(api, orc, tmp_path, u8):
    """bhip_surf_detect_f32 / _u8 process large host batches in chunks (upload of chunk k+1 under the kernels of chunk k, results appended).
    A 7-frame batch is far below the chunking threshold, so a child process with BHIP_SURF_CHUNK=2 (chunks 2,2,2,1) is compared, array by
    array, with the plain path of this process and with the oracle."""
    import os, subprocess, sys
    frames = []
    for k in range(7):
        g = orc.noise_image(200, 150, 300 + k, 0, 255).array().astype(np.float32)
        frames.append(np.floor(g).astype(np.uint8) if u8 else g)
    np.save(tmp_path / "frames.npy", np.stack(frames))
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayU8 if u8 else api.GrayF32)
    Img = api.GrayU8 if u8 else api.GrayF32
    dd.detectBatch([Img(200, 150, f.reshape(-1)) for f in frames])
    base = dd.fetchAll()
    pairs, fit = dd.associateImages(np.arange(7), (np.arange(7) + 1) % 7)
    assert base[4][-1] > 300
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from boofcv_amd import api; fr = np.load(%r); u8 = %r; "
            "Img = api.GrayU8 if u8 else api.GrayF32; dd = api.FactoryDetectDescribe.surfStable(None, None, None, Img); "
            "dd.detectBatch([Img(200, 150, f.reshape(-1)) for f in fr]); o = dd.fetchAll(); "
            "p, f = dd.associateImages(np.arange(7), (np.arange(7) + 1) %% 7); "
            "np.savez(%r, xys=o[0], ang=o[1], white=o[2], desc=o[3], starts=o[4], pairs=p, fit=f, one=dd._results(5)[3])")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "chunked.npz")
    e = dict(os.environ); e["BHIP_SURF_CHUNK"] = "2"
    subprocess.run([sys.executable, "-c", code % (root, str(tmp_path / "frames.npy"), u8, out)], check=True, env=e, timeout=300)
    got = np.load(out)
    for k, name in enumerate(["xys", "ang", "white", "desc", "starts"]):
        assert np.array_equal(got[name], base[k]), name
    assert np.array_equal(got["pairs"], pairs) and np.array_equal(got["fit"], fit)
    assert np.array_equal(got["one"], dd._results(5)[3])   # per-image fetch after a chunked detect
    if not u8:   # and the oracle, frame 3
        ref = orc.Surf(True)
        ref.detect(orc.Gray.from_array(frames[3]), threads=4)
        rp = ref.fetch()
        s0, s1 = int(base[4][3]), int(base[4][4])
        assert np.array_equal(base[0][s0:s1], rp[0]) and np.array_equal(base[2][s0:s1], rp[2])


@pytest.mark.parametrize("batch", [3, 130])
@pytest.mark.parametrize("kind", ["surfStable", "brief"])
def test_detect_device_padded_rows_equals_dense_host_batch(api, orc, kind, batch):
    """bhip_surf_detect_dev_f32 on a device batch whose rows and images are padded (160x120 frames, row stride 176, image stride 176*125,
    every padding element 1e6) gives, array for array, what detectBatch gives on the same frames as dense host images -- for a surfStable
    object and for Fast-Hessian + BRIEF (key points and words; BRIEF samples the strided frames themselves).  130 frames are above the
    single-pass integral kernel's batch threshold (128), so that kernel reads the strided input too."""
    torch = pytest.importorskip("torch")
    w, h, stride, rows = 160, 120, 176, 125
    base = [orc.noise_image(w, h, 234 + k) for k in range(5)]
    idx = [k % 5 for k in range(batch)]

    def make(ctx=None):
        if kind == "surfStable":
            return api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32, ctx=ctx)
        brief = api.FactoryDescribeRegionPoint.brief(None, api.GrayF32, ctx=ctx)
        return api.FactoryDetectDescribe.fuseTogether(api.FactoryInterestPoint.fastHessian(None), None, brief, ctx=ctx)

    host = make()
    host.detectBatch([G(api, base[k]) for k in idx])
    want = host.fetchAll()
    padded = np.full((batch, rows, stride), 1e6, dtype=np.float32)
    for b, k in enumerate(idx):
        padded[b, :h, :w] = base[k].array()
    frames = torch.from_numpy(padded).cuda()
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    dev = make(ctx)
    dev.detectDevice(frames.data_ptr(), stride * rows, stride, w, h, batch)
    got = dev.fetchAll()
    assert len(got) == len(want) and want[-1][-1] > 20 * batch
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (kind, batch, k)
    dev.close(); ctx.close()
