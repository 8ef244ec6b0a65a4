"""Tail of the fused Fast-Hessian octaves (step 1 and 2 in the default schedule): behind the candidate list, a group of 16 lanes takes one
candidate through the window test, the ignore border, the scale-space test and the emission, 16 candidates per round at 256 threads
(step 1) and 64 at 1024 (step 2), rounds until the list is done; the levels that the next octave shares are exported slot by slot behind
the dense phase.  Noise images make crowded tiles, which is what the round loop and the groups have to survive.
Everything is bit-exact: no tolerances.  Run with `pytest -m gpu` on an MI355X.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every shape and both configurations in one child process: the plan switches are read from the environment of the process that calls the library
CHILD = ("import sys, numpy as np; sys.path.insert(0, %r); from boofcv_amd import api; z = np.load(%r); out = {}\n"
         "for octaves in (4, 2):\n"
         "    fh = api.FastHessianFeatureDetector(api.ConfigFastHessian(numberOfOctaves=octaves))\n"
         "    for k in z.files:\n"
         "        fh.detect(api.IntegralImageOps.transform(api.GrayF32.wrap(z[k]))); out['%%s/%%d' %% (k, octaves)] = fh.getFoundPoints().copy()\n"
         "np.savez(%r, **out)")

# (w, h, seed, key points the CPU oracle finds on noise_image(w, h, seed, 0, 255), of those with scale > 3.3, i.e. above octave 0)
FIXED = [(113, 161, 5, 220, 28), (120, 200, 32, 304, 46), (176, 176, 33, 404, 59), (230, 170, 31, 537, 101), (403, 301, 8, 2002, 409)]
IDS = ["%dx%d" % (w, h) for w, h, _, _, _ in FIXED]
OCTAVE0_MAX_SCALE = 3.3   # octave 0 interpolates kernel sizes between 9 and 27: scale = 1.2 * size / 9 <= 3.6, and its mid levels are 15 and 21
TILE = 28                 # core columns of a tile at both steps, core rows at step 1
TILE_ROWS_STEP2 = 40      # core rows of a tile at step 2
EXPORT_SHAPE = (230, 170)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()  # fails loudly without a GPU / without libboofhip.so
    return a


def G(api, g):
    return api.GrayF32(g.width, g.height, g.buf, g.startIndex, g.stride)


def gpu_points(api, img, octaves=4):
    fh = api.FastHessianFeatureDetector(api.ConfigFastHessian(numberOfOctaves=octaves))
    fh.detect(api.IntegralImageOps.transform(G(api, img)))
    return fh.getFoundPoints().copy()


@pytest.fixture(scope="module")
def fixed(orc):
    """image and oracle key points of every fixed shape, computed once"""
    out = {}
    for w, h, seed, _, _ in FIXED:
        img = orc.noise_image(w, h, seed, 0, 255)
        out[(w, h)] = (img, orc.fh_detect(orc.integral(img), orc.FhCfg()))
    return out


@pytest.fixture(scope="module")
def unfused(fixed, tmp_path_factory):
    """key points of every fixed shape from the stand-alone kernels (BHIP_DETECT_UNFUSED=1), four and two octaves, one child process for all"""
    d = tmp_path_factory.mktemp("fused_tail")
    src, out = str(d / "img.npz"), str(d / "kp.npz")
    np.savez(src, **{"%dx%d" % k: img.array() for k, (img, _) in fixed.items()})
    e = dict(os.environ)
    e["BHIP_DETECT_UNFUSED"] = "1"
    subprocess.run([sys.executable, "-c", CHILD % (ROOT, src, out)], check=True, env=e, timeout=300)
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("w,h,seed,count,above", FIXED, ids=IDS)
def test_fixed_shapes_match_oracle_and_unfused_plan(api, fixed, unfused, w, h, seed, count, above):
    img, exp = fixed[(w, h)]
    got = gpu_points(api, img)
    print("%d x %d: %d key points (oracle %d), %d above octave 0" % (w, h, len(got), len(exp), int((exp[:, 2] > OCTAVE0_MAX_SCALE).sum())))
    assert len(exp) == count and int((exp[:, 2] > OCTAVE0_MAX_SCALE).sum()) == above
    assert np.array_equal(got, exp)
    assert np.array_equal(got, unfused["%dx%d/4" % (w, h)])


def test_crowded_tiles_and_tile_edges_are_in_the_fixed_shapes(fixed):
    """What 403 x 301 / seed 8 is there for, asserted from the oracle's points so that a change of the noise generator cannot silently empty
    the case.  Octave 0: 19 key points in one 28 x 28-pixel tile region, more than the 16 candidates one round serves at 256 threads, so the
    round loop runs.  Above octave 0: 27 in one 56 x 80-pixel region, the footprint of a step-2 tile -- candidates are at least as many as
    key points, so this is a lower bound on how full that tile's round gets, not a proof that it loops.  Tile edges: key points on the
    first and last core column and row of a tile of each step (their window and 3 x 3 neighbours lie in the halo)."""
    _, exp = fixed[(403, 301)]
    lo, hi = exp[exp[:, 2] <= OCTAVE0_MAX_SCALE], exp[exp[:, 2] > OCTAVE0_MAX_SCALE]
    px, py = np.rint(lo[:, 0]).astype(int), np.rint(lo[:, 1]).astype(int)
    crowd0 = int(np.bincount((py // TILE) * 1000 + px // TILE).max())
    qx, qy = np.rint(hi[:, 0]).astype(int), np.rint(hi[:, 1]).astype(int)
    crowd1 = int(np.bincount((qy // (2 * TILE_ROWS_STEP2)) * 1000 + qx // (2 * TILE)).max())
    print("most key points in one tile region: %d at step 1, %d above octave 0 in a step-2 footprint" % (crowd0, crowd1))
    assert crowd0 == 19 and crowd0 > 16
    assert crowd1 == 27 and crowd1 >= 16
    edge = {"step 1 columns": np.isin(px % TILE, (0, TILE - 1)).sum(), "step 1 rows": np.isin(py % TILE, (0, TILE - 1)).sum(),
            "step 2 columns": np.isin(np.rint(hi[:, 0] / 2).astype(int) % TILE, (0, TILE - 1)).sum(),
            "step 2 rows": np.isin(np.rint(hi[:, 1] / 2).astype(int) % TILE_ROWS_STEP2, (0, TILE_ROWS_STEP2 - 1)).sum()}
    print(edge)
    assert all(n >= 1 for n in edge.values()), edge


@pytest.mark.parametrize("octaves", [2, 4])
def test_export_on_and_off(api, orc, fixed, unfused, octaves):
    """Two octaves: both fused, no level is exported.  Four: step 2 exports its levels 1 and 3 to octave 2, which copies them instead of
    evaluating them -- a wrong plane shows up as wrong coarse key points."""
    img, exp4 = fixed[EXPORT_SHAPE]
    exp = exp4 if octaves == 4 else orc.fh_detect(orc.integral(img), orc.FhCfg(numberOfOctaves=2))
    got = gpu_points(api, img, octaves)
    coarse = int((exp[:, 2] > 2 * OCTAVE0_MAX_SCALE).sum())
    print("%d octaves: %d key points, %d above octave 1" % (octaves, len(exp), coarse))
    assert len(exp) >= 100 and (coarse >= 3) == (octaves == 4)
    assert np.array_equal(got, exp)
    assert np.array_equal(got, unfused["%dx%d/%d" % (EXPORT_SHAPE + (octaves,))])


@pytest.mark.parametrize("w,h,seed,count,above", FIXED, ids=IDS)
def test_u8_batch_of_eleven_equals_single_frames(api, orc, w, h, seed, count, above):
    """GrayU8 frames (integer taps), more frames than XCDs so that tiles of several images are in flight at once: every frame of the batch
    gives what it gives alone, and what the oracle gives."""
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
