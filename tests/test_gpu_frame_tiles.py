"""Frame tiles of the fused Fast-Hessian octaves (step 1 and 2 in the default schedule): tiles whose halo touches the ring where the
reference switches from hessianInner to the clamped hessianBorder form.  Such a tile runs its inner rectangle through the inline inner
forms and the strips around it through the clamped form; the shapes below put the rectangle's edges on every kind of position (empty,
one pixel wide, odd starts and ends, the whole tile) on small images, where nearly every tile is a frame tile.
Everything is bit-exact: no tolerances.  Run with `pytest -m gpu` on an MI355X.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every fixed shape in one child process: the plan switches are read from the environment of the process that calls the library
CHILD = ("import sys, numpy as np; sys.path.insert(0, %r); from boofcv_amd import api; "
         "z = np.load(%r); fh = api.FastHessianFeatureDetector(api.ConfigFastHessian()); out = {}\n"
         "for k in z.files:\n"
         "    fh.detect(api.IntegralImageOps.transform(api.GrayF32.wrap(z[k]))); out[k] = fh.getFoundPoints().copy()\n"
         "np.savez(%r, **out)")

# (w, h, seed, key points the CPU oracle finds on noise_image(w, h, seed, 0, 255))
#  57 x 57:   every tile is a frame tile; the third tile column and row are 1 px wide
#  30 x 200:  one tile column is both the left and the right frame
#  200 x 30:  one tile row is both the top and the bottom frame
#  85 x 121:  inner rectangles with odd starts and ends (14 points above octave 0)
#  113 x 161: every octave-1 tile is a frame tile (38 points above octave 0)
#  403 x 301: frame and interior tiles mixed
FIXED = [(57, 57, 1, 13), (30, 200, 2, 21), (200, 30, 3, 18), (85, 121, 4, 83), (113, 161, 5, 220), (403, 301, 8, 2002)]
IDS = ["%dx%d" % (w, h) for w, h, _, _ in FIXED]

SWEEP_SEED, SWEEP_N = 20, 40


def sweep_sizes():
    rng = np.random.default_rng(SWEEP_SEED)
    return [(int(w), int(h)) for w, h in rng.integers(40, 221, (SWEEP_N, 2))]


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()  # fails loudly without a GPU / without libboofhip.so
    return a


def G(api, g):
    return api.GrayF32(g.width, g.height, g.buf, g.startIndex, g.stride)


def gpu_points(api, img):
    fh = api.FastHessianFeatureDetector(api.ConfigFastHessian())
    fh.detect(api.IntegralImageOps.transform(G(api, img)))
    return fh.getFoundPoints().copy()


@pytest.fixture(scope="module")
def fixed(orc):
    """image and oracle key points of every fixed shape, computed once"""
    out = {}
    for w, h, seed, _ in FIXED:
        img = orc.noise_image(w, h, seed, 0, 255)
        out[(w, h)] = (img, orc.fh_detect(orc.integral(img), orc.FhCfg()))
    return out


@pytest.fixture(scope="module")
def unfused(fixed, tmp_path_factory):
    """key points of every fixed shape from the stand-alone kernels (BHIP_DETECT_UNFUSED=1), one child process for all of them"""
    d = tmp_path_factory.mktemp("frame_tiles")
    src, out = str(d / "img.npz"), str(d / "kp.npz")
    np.savez(src, **{"%dx%d" % k: img.array() for k, (img, _) in fixed.items()})
    e = dict(os.environ)
    e["BHIP_DETECT_UNFUSED"] = "1"
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, src, out)], check=True, env=e, timeout=300)
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("w,h,seed,count", FIXED, ids=IDS)
def test_fixed_shapes_match_oracle_and_unfused_plan(api, fixed, unfused, w, h, seed, count):
    img, exp = fixed[(w, h)]
    got = gpu_points(api, img)
    print("%d x %d: %d key points (oracle %d)" % (w, h, len(got), len(exp)))
    assert len(exp) == count and count >= 10
    assert len(got) >= 10
    assert np.array_equal(got, exp)
    assert np.array_equal(got, unfused["%dx%d" % (w, h)])


def test_seeded_sweep_matches_oracle(api, orc):
    """40 sizes with w, h in [40, 220]; at most a tenth of them may have fewer than 10 key points (they are compared all the same)."""
    sparse = 0
    for w, h in sweep_sizes():
        img = orc.noise_image(w, h, 1000 + w * 256 + h, 0, 255)
        exp = orc.fh_detect(orc.integral(img), orc.FhCfg())
        sparse += len(exp) < 10
        assert np.array_equal(gpu_points(api, img), exp), (w, h)
    assert sparse <= SWEEP_N // 10, sparse


@pytest.mark.parametrize("w,h,seed,count", FIXED, ids=IDS)
def test_u8_batch_of_eleven_equals_single_frames(api, orc, w, h, seed, count):
    """GrayU8 frames (integer taps; the one-by-one inner form at step 1), more frames than XCDs so that tiles of several images are in
    flight at once: every frame of the batch gives what it gives alone, and what the oracle gives."""
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(11)]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayU8)
    dd.detectBatch([api.GrayU8.wrap(f) for f in frames])
    batch = [np.array(dd._results(i)[0]) for i in range(11)]
    ref = orc.Surf(True)
    for i, f in enumerate(frames):
        dd.detect(api.GrayU8.wrap(f))
        single = np.array(dd._results()[0])
        assert len(single) >= 10 and np.array_equal(batch[i], single), i
        ref.detect_u8(f)
        assert np.array_equal(single, ref.fetch()[0]), i
