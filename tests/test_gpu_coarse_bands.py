"""The coarse Fast-Hessian octaves of the default schedule (size 75 at step 4, sizes 99 and 147 at step 8): the compile-time-geometry rows
kernel with its row bands (k_hessian_rows_fixed), the merged rows launch of the two octaves and the merged NMS launch of their four middle
levels, against the run-time rows kernel (BHIP_HESSIAN_ROWS_GENERIC=1), the gather plan (BHIP_DETECT_GATHER=1) and the CPU oracle.
Everything is bit-exact: no tolerances.  Run with `pytest -m gpu` on an MI355X.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a detector run in a child process: the plan switches are read from the environment of the process that calls the library
CHILD = ("import sys, numpy as np; sys.path.insert(0, %r); from boofcv_amd import api; "
         "a = np.load(%r); fh = api.FastHessianFeatureDetector(api.ConfigFastHessian(1, 2, -1, 1, 9, 4, 4)); "
         "fh.detect(api.IntegralImageOps.transform(api.GrayF32.wrap(a))); "
         "np.save(%r, fh.getFoundPoints())")


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()  # fails loudly without a GPU / without libboofhip.so
    return a


def G(api, g):
    return api.GrayF32(g.width, g.height, g.buf, g.startIndex, g.stride)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def child_points(tmp_path, img, env):
    src, out = str(tmp_path / "img.npy"), str(tmp_path / ("kp_%s.npy" % "_".join(sorted(env))))
    np.save(src, img.array())
    e = dict(os.environ)
    e.update(env)
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, src, out)], check=True, env=e, timeout=300)
    return np.load(out)


# 256 x 200: the inner region of size 147 is 5 rows high, and a row has 32 outputs at step 8 (less than a wave).  403 x 301: odd width, rows
# not 16-byte aligned.  2100 x 210: three x-tiles at step 4, and at step 8 the 6 inner rows of size 147 end in a partial band.  300 x 212:
# 33 inner rows at step 4, so a band of 2, 4 or 8 rows leaves a last band of exactly one row.
@pytest.mark.parametrize("w,h,seed", [(256, 200, 3), (403, 301, 8), (2100, 210, 5), (300, 212, 13)])
def test_three_plans_agree_and_match_oracle(api, orc, tmp_path, w, h, seed):
    img = orc.noise_image(w, h, seed, 0, 255)
    fh = api.FastHessianFeatureDetector(api.ConfigFastHessian(1, 2, -1, 1, 9, 4, 4))
    fh.detect(api.IntegralImageOps.transform(G(api, img)))
    base = fh.getFoundPoints().copy()
    assert len(base) > 100
    assert np.array_equal(base, child_points(tmp_path, img, {"BHIP_HESSIAN_ROWS_GENERIC": "1"}))
    assert np.array_equal(base, child_points(tmp_path, img, {"BHIP_DETECT_GATHER": "1"}))
    assert np.array_equal(base, orc.fh_detect(orc.integral(img), orc.FhCfg()))


def test_rows_launched_before_an_octave_that_copies_them(api, orc, tmp_path):
    """BHIP_DETECT_DENSE=1: size 99 is computed densely at step 4 and copied by the octave at step 8, so the queued rows of the step-4 octave
    cannot wait for the merged launch."""
    img = orc.noise_image(403, 301, 8, 0, 255)
    exp = orc.fh_detect(orc.integral(img), orc.FhCfg())
    assert len(exp) > 100 and np.array_equal(child_points(tmp_path, img, {"BHIP_DETECT_DENSE": "1"}), exp)


# (27, 4) is not one of the compile-time geometries: it still goes through the run-time rows kernel
@pytest.mark.parametrize("w,h", [(403, 301), (2100, 210)])
@pytest.mark.parametrize("size,skip", [(75, 4), (99, 8), (147, 8), (27, 4)])
def test_single_levels(api, orc, size, skip, w, h):
    ii = orc.integral(orc.noise_image(w, h, 8, 0, 255))
    out = api.GrayF32(w // skip, h // skip)
    api.IntegralImageFeatureIntensity.hessian(G(api, ii), skip, size, out)
    assert np.array_equal(bits(out.array()), bits(orc.hessian(ii, skip, size).array()))
    frame = np.random.default_rng(size).integers(0, 256, (h, w), dtype=np.uint8)
    iis = api.IntegralImageOps.transform(api.GrayU8.wrap(frame))
    out = api.GrayF32(w // skip, h // skip)
    api.IntegralImageFeatureIntensity.hessian(iis, skip, size, out)
    assert np.array_equal(bits(out.array()), bits(orc.hessian_s32(iis.array(), skip, size)))


@pytest.mark.parametrize("u8", [False, True])
def test_batch_of_eleven_equals_single_frames(api, u8):
    """More frames than XCDs and not a multiple of 8: the merged launches take every (octave, level, band, tile, image) to its place, so
    every frame of the batch gives what it gives alone (GrayF32, and GrayU8 for the integer taps)."""
    rng = np.random.default_rng(78)
    frames = [rng.integers(0, 256, (240, 320), dtype=np.uint8) for _ in range(11)]
    wrap = (lambda f: api.GrayU8.wrap(f)) if u8 else (lambda f: api.GrayF32.wrap(f.astype(np.float32)))
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayU8 if u8 else api.GrayF32)
    dd.detectBatch([wrap(f) for f in frames])
    batch = [np.array(dd._results(i)[0]) for i in range(11)]
    for i, f in enumerate(frames):
        dd.detect(wrap(f))
        single = np.array(dd._results()[0])
        assert len(single) > 100 and np.array_equal(batch[i], single), i


def test_other_schedules_keep_their_launches(api, orc):
    """N-best selection (per-level NMS lists) and a schedule that starts at step 2 (no compile-time geometry fits its levels)."""
    ii = orc.integral(orc.noise_image(403, 301, 8, 0, 255))
    fh = api.FastHessianFeatureDetector(api.ConfigFastHessian(1, 2, 50, 1, 9, 4, 4))
    fh.detect(G(api, ii))
    nbest = orc.fh_detect(ii, orc.FhCfg(maxFeaturesPerScale=50), threads=8)
    assert len(nbest) > 100 and np.array_equal(fh.getFoundPoints(), nbest)
    fh = api.FastHessianFeatureDetector(api.ConfigFastHessian(1, 2, -1, 2, 9, 4, 4))
    fh.detect(G(api, ii))
    coarse = orc.fh_detect(ii, orc.FhCfg(initialSampleSize=2))
    assert len(coarse) > 50 and np.array_equal(fh.getFoundPoints(), coarse)
