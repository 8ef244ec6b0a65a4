"""k_describe keeps its constant tables off the vector load path (describe.hip, header comment and "the wave's copy"): the surfStable
kernels copy weightSub and weightGrid into the wave's LDS slice once per key point and issue the orientation weights' loads ahead of the
orientation taps.  BHIP_DESCRIBE_TABLEPTR=1 reads every table through its device pointer at the point of use, as the generic kernels do.

What can go wrong is in the copy, not in the arithmetic: a table value read before it is stored or after the slice was overwritten (by the
samples, by feat of a later band, by the next key point's orientation phase), a lane that loads the wrong element, a clamped index that
reads past the table.  A wrong weight moves a descriptor by far more than the bar.  Every case compares with the CPU oracle under the bars
of tests/test_gpu_parity.py::_compare_surf (restated in tests/test_gpu_surf_configs.py::_compare: key points and Laplacian sign bit for bit,
every descriptor value within 1e-5, every orientation within 1e-12 rad, norms 1 within 1e-12), and the two table paths must agree
array_equal: they multiply the same doubles in the same order.

Shapes: 96 x 80 and 160 x 120 frames with three to six Gaussian blobs of sigma 2, 3, 5 and 8, so key points of several scales exist and some
descriptor grids leave the image; batches of three with a flat frame in the middle (no key point: the order records of the third frame
follow the first's); supplied points in each corner region whose orientation and descriptor samples are partly outside the image.  Blob
frames this small have one to ten key points each, fewer than there are waves, so one case describes more supplied points than the device
has wave slots: every wave then makes its copy again and again, each time over what the orientation phase left in the slice.

The describe entry takes no caller-supplied angles (every caller of bhip_launch_describe_ex passes anglesIn = nullptr), so that switch has
no case here; the describe-only call is describePoints (a flat list, no order record).
"""
import os

import numpy as np
import pytest

from test_gpu_surf_configs import G, _compare, make, make_ref

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (160, 120)]
SIGMAS = (2.0, 3.0, 5.0, 8.0)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()  # fails loudly without a GPU / without libboofhip.so
    return a


def blob_frame(w, h, seed, nblobs):
    """background 50 + nblobs Gaussian blobs (sigma from SIGMAS in turn, starting at `seed`, so every sigma occurs in a batch) + U[0,2) noise
    -> (h, w) float32 in [0, 255)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.full((h, w), 50.0)
    for k in range(nblobs):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        sg = SIGMAS[(seed + k) % 4]
        amp = float(rng.uniform(40, 100) * (1 if k % 2 else -1))
        a += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sg * sg))
    a += rng.uniform(0, 2, (h, w))
    return np.clip(a, 0, 254.9).astype(np.float32)


@pytest.fixture(scope="module")
def frames():
    """(w, h) -> [blobs, flat, blobs]; read only"""
    return {(w, h): [blob_frame(w, h, 10 + w, 6), np.full((h, w), 50.0, dtype=np.float32), blob_frame(w, h, 11 + w, 3 if w < 100 else 5)] for w, h in SIZES}


def corner_points(w, h):
    """one point in each corner region (small and large scales: the 17 x 17 orientation grid and the 24 x 24 descriptor grid of a point at
    scale s reach 16 s and 12 s pixels out, so all of them sample outside), the corners themselves, and one whose grid covers the frame"""
    return np.array([[0, 0, 1.0], [w - 1, h - 1, 1.0], [3.2, 2.6, 1.2], [w - 4.5, 3.3, 2.5], [2.4, h - 3.7, 4.0], [w - 2.1, h - 2.2, 1.6],
                     [6.0, 5.0, 6.3], [w / 2 + 0.3, h / 2 + 0.7, 9.7], [w / 2, h / 2, 1.5]])


def _gray(orc, a):
    return orc.Gray.from_array(a)


def _pointer_path(fn):
    """fn() with every table read through its device pointer"""
    os.environ["BHIP_DESCRIBE_TABLEPTR"] = "1"
    try:
        return fn()
    finally:
        del os.environ["BHIP_DESCRIBE_TABLEPTR"]


def _all(dd, n):
    return [tuple(np.array(x) for x in dd._results(i)) for i in range(n)]


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), "%s: the table paths differ on item %d" % (what, i)


def _batch_case(api, orc, dd, ref, arrays, wrap, detect_ref, what):
    """detectBatch against the oracle frame by frame, then once more on the pointer path: array_equal -> per-frame counts"""
    run = lambda: (dd.detectBatch([wrap(a) for a in arrays]), _all(dd, len(arrays)))[1]
    got = run()
    counts = []
    for i, a in enumerate(arrays):
        detect_ref(ref, a)
        counts.append(_compare(got[i], ref.fetch(), "%s frame %d" % (what, i))[0])
    _same(got, _pointer_path(run), what)
    return counts


def _points_case(api, orc, dd, ref, pts, describe_ref, what):
    """describePoints on the integral image of the last detect (image 0), both table paths"""
    run = lambda: dd.describePoints(pts, image=0)
    ang, white, desc = run()
    describe_ref(ref)
    _, rang, rwhite, rdesc = ref.fetch()
    _compare((pts, ang, white, desc), (pts, rang, rwhite, rdesc), what)
    assert np.any(desc[0]) and np.any(desc[1])   # the corner points still have samples inside
    _same([(ang, white, desc)], [_pointer_path(run)], what)


# ------------------------------------------------------------------------------------------------------------------ surfStable (CFG 1)
@pytest.mark.parametrize("w,h", SIZES)
def test_stable_f32_batch(api, orc, frames, w, h):
    arrays = frames[(w, h)]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    ref = orc.Surf(True)
    counts = _batch_case(api, orc, dd, ref, arrays, api.GrayF32.wrap, lambda r, a: r.detect(_gray(orc, a)), "stable F32 %dx%d" % (w, h))
    assert counts[1] == 0 and counts[0] >= 1 and counts[2] >= 1, counts
    scales = np.concatenate([np.array(dd._results(i)[0])[:, 2] for i in (0, 2)])
    assert scales.max() > 1.25 * scales.min(), scales     # key points of several scales (4.7 and 6.0 at 96 x 80; 2.2 to 6.6 at 160 x 120)
    first = _gray(orc, arrays[0])
    _points_case(api, orc, dd, ref, corner_points(w, h), lambda r: r.describe_points(corner_points(w, h), first), "stable F32 %dx%d corners" % (w, h))


@pytest.mark.parametrize("w,h", SIZES)
def test_stable_u8_batch(api, orc, frames, w, h):
    """integer taps: the GrayS32 integral image of a GrayU8 frame"""
    arrays = [np.floor(a).astype(np.uint8) for a in frames[(w, h)]]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayU8)
    ref = orc.Surf(True)
    counts = _batch_case(api, orc, dd, ref, arrays, api.GrayU8.wrap, lambda r, a: r.detect_u8(a), "stable U8 %dx%d" % (w, h))
    assert counts[1] == 0 and counts[0] >= 1 and counts[2] >= 1, counts
    ref.detect_u8(arrays[0])   # the oracle describes a caller's points on the integral image of its last detect
    _points_case(api, orc, dd, ref, corner_points(w, h), lambda r: r.describe_points(corner_points(w, h)), "stable U8 %dx%d corners" % (w, h))


@pytest.mark.parametrize("w,h", SIZES)
def test_stable_colour_bands(api, orc, frames, w, h):
    """colour SURF on the default grid, three bands: feat grows to three bands' sums and the tables sit behind it; the band loop runs between
    the copy and its last reader"""
    base = frames[(w, h)]
    bands = [base[0], base[2], (0.5 * (base[0] + base[2])).astype(np.float32)]
    # (at the default threshold the band average of the 96 x 80 frames has no key point)
    dd = api.FactoryDetectDescribe.surfColorStable(api.ConfigFastHessian(detectThreshold=0.5), None, None, api.PlanarType(3))
    ref = orc.Surf(True, fh=orc.FhCfg(detectThreshold=0.5))
    n = ref.detect_planar([_gray(orc, b) for b in bands])
    want = ref.fetch()
    run = lambda: (dd.detect(api.Planar.wrap([api.GrayF32.wrap(b) for b in bands])), tuple(np.array(x) for x in dd._results()))[1]
    got = run()
    assert got[3].shape[1] == 192
    assert _compare(got, want, "stable colour %dx%d" % (w, h))[0] == n and n >= 2
    _same([got], [_pointer_path(run)], "stable colour")


def test_more_points_than_wave_slots(api, orc, frames):
    """supplied points, 3 per wave slot of an MI355X and a few over (256 CUs, 16 slots each), seeded positions up to the frame's edges and scales
    1 to 8: a wave's second and third key point find the previous one's orientation data where the tables go"""
    w, h = SIZES[1]
    n = 3 * 16 * 256 + 7
    rng = np.random.default_rng(20261020)
    pts = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n), rng.uniform(1.0, 8.0, n)], axis=1)
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    dd.detect(api.GrayF32.wrap(frames[(w, h)][0]))
    ref = orc.Surf(True)
    run = lambda: dd.describePoints(pts)
    ang, white, desc = run()
    ref.describe_points(pts, _gray(orc, frames[(w, h)][0]), threads=max(1, min(16, os.cpu_count() or 1)))
    _, rang, rwhite, rdesc = ref.fetch()
    _compare((pts, ang, white, desc), (pts, rang, rwhite, rdesc), "%d supplied points" % n)
    _same([(ang, white, desc)], [_pointer_path(run)], "supplied points")


# ------------------------------------------------------------------------------------------------------------------ the kernels beside it
@pytest.mark.parametrize("w,h", SIZES)
def test_fast_defaults(api, orc, frames, w, h):
    """surfFast defaults (CFG 2): weightFast and the average orientation's weights stay on the pointer path"""
    arrays = frames[(w, h)]
    dd = api.FactoryDetectDescribe.surfFast(None, None, None, api.GrayF32)
    ref = orc.Surf(False)
    counts = _batch_case(api, orc, dd, ref, arrays, api.GrayF32.wrap, lambda r, a: r.detect(_gray(orc, a)), "fast %dx%d" % (w, h))
    assert counts[1] == 0 and counts[0] >= 1 and counts[2] >= 1, counts
    first = _gray(orc, arrays[0])
    _points_case(api, orc, dd, ref, corner_points(w, h), lambda r: r.describe_points(corner_points(w, h), first), "fast %dx%d corners" % (w, h))


@pytest.mark.parametrize("name", ["s-4-6-3", "s-3-5-2"])
def test_generic_grid(api, orc, frames, name):
    """non-default grids run the generic instantiations (<8,16,T,0> and <5,9,T,0>): every table by pointer, 8-byte samples, no room reserved"""
    w, h = SIZES[1]
    arrays = frames[(w, h)]
    dd = make(api, name)
    ref = make_ref(orc, name)
    counts = _batch_case(api, orc, dd, ref, arrays, api.GrayF32.wrap, lambda r, a: r.detect(_gray(orc, a)), name)
    assert counts[1] == 0 and counts[0] >= 1 and counts[2] >= 1, counts
    first = _gray(orc, arrays[0])
    _points_case(api, orc, dd, ref, corner_points(w, h), lambda r: r.describe_points(corner_points(w, h), first), name + " corners")
