"""k_describe hands its key points out through per-XCD queues: persistent waves take slot after slot (describe.hip, "Hand-out of the key points").

What can go wrong is in the hand-out, not in the arithmetic: a slot taken twice or never, a wave that starts its next key point before its
LDS slice is free, an order record that names the wrong image, counters left over from the launch before.  Every case compares with the CPU
oracle under the bars of tests/test_gpu_parity.py and tests/test_gpu_surf_configs.py (key points, Laplacian sign bit for bit; descriptors
1e-5 with no exception; orientations 1e-12 rad), so a key point that was skipped (stale output) or described from another image shows.

Shapes: totals of 0, 1, 3, 4, 5, 7 and 30 key points (below the wave count, the first and second workgroup of the order, not a multiple of
four), a flat frame in the middle of a batch, one batch with more than three key points per persistent wave (48 x CUs, from the device's
properties), a batch whose key points sit in its first frames, and one small shape for each path that shares the kernel.
"""
import math
import os

import numpy as np
import pytest

from test_gpu_fullsize import blobs
from test_gpu_surf_configs import ANG_TOL, DESC_TOL, POINTS, G, _adiff, _compare, make, make_ref

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, os.cpu_count() or 1))
SMALL_TOTALS = (0, 1, 3, 4, 5, 7, 30)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()  # fails loudly without a GPU / without libboofhip.so
    return a


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev_ctx(api, torch):
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    yield ctx
    ctx.close()


def _detect_device(api, torch, dd, arrays):
    """(H, W) float32 arrays of one shape -> detectDevice on a dense device batch"""
    t = torch.from_numpy(np.stack(arrays)).cuda()
    b, h, w = t.shape
    dd.detectDevice(t.data_ptr(), h * w, w, w, h, b)
    return t   # keep alive until the results are fetched


def _flat(w, h, value=50.0):
    return np.full((h, w), value, dtype=np.float32)


def _check_batch(api, orc, dd, ref, arrays, what):
    """every frame of the batch against the oracle; -> per-frame counts"""
    counts = []
    for i, a in enumerate(arrays):
        ref.detect(orc.Gray.from_array(a))
        counts.append(_compare(dd._results(i), ref.fetch(), "%s frame %d" % (what, i))[0])
    assert dd.totalFeatures() == sum(counts), what
    return counts


@pytest.fixture(scope="module")
def thresholds(orc):
    """detectThreshold values at which the 160x120 noise frame (seed 5) has exactly k key points, k in SMALL_TOTALS: bisection on the oracle's
    detector (the count falls as the threshold rises)"""
    img = orc.noise_image(160, 120, 5)
    ii = orc.integral(img)
    count = lambda t: len(orc.fh_detect(ii, orc.FhCfg(detectThreshold=t)))
    out = {}
    for k in SMALL_TOTALS:
        lo, hi = 1.0, 1.0e9     # count(lo) = 218 > k >= count(hi) = 0
        assert count(lo) > k and count(hi) == 0
        for _ in range(200):
            mid = math.sqrt(lo * hi)
            c = count(mid)
            if c == k:
                out[k] = float(np.float32(mid))
                break
            if c > k:
                lo = mid
            else:
                hi = mid
        assert k in out and count(out[k]) == k, "no threshold leaves exactly %d key points" % k
    return img, out


# ------------------------------------------------------------------------------------------------------------------ 1. scheduling edges
@pytest.mark.parametrize("k", SMALL_TOTALS)
def test_small_totals(api, orc, torch, dev_ctx, thresholds, k):
    img, thr = thresholds
    dd = api.FactoryDetectDescribe.surfStable(api.ConfigFastHessian(detectThreshold=thr[k]), None, None, api.GrayF32, ctx=dev_ctx)
    ref = orc.Surf(True, fh=orc.FhCfg(detectThreshold=thr[k]))
    arrays = [img.array().copy()]
    keep = _detect_device(api, torch, dd, arrays)
    assert _check_batch(api, orc, dd, ref, arrays, "total %d" % k) == [k]
    del keep


def test_flat_frame_in_the_middle(api, orc, torch, dev_ctx):
    """320x240: noise, flat, noise -- the flat frame has no key point, the order records of the third frame follow those of the first; the total
    is chosen (by the oracle's counts) not to be a multiple of four"""
    ref = orc.Surf(True)
    first = orc.noise_image(320, 240, 40).array().copy()
    n_first = ref.detect(orc.Gray.from_array(first))
    for seed in range(41, 60):
        last = orc.noise_image(320, 240, seed).array().copy()
        if (n_first + ref.detect(orc.Gray.from_array(last))) % 4:
            break
    arrays = [first, _flat(320, 240), last]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32, ctx=dev_ctx)
    keep = _detect_device(api, torch, dd, arrays)
    counts = _check_batch(api, orc, dd, ref, arrays, "flat in the middle")
    assert counts[1] == 0 and counts[0] > 300 and counts[2] > 300 and sum(counts) % 4 != 0
    del keep


# ------------------------------------------------------------------------------------------------------------------ 2. every wave loops
def test_more_than_three_key_points_per_wave(api, orc, torch, dev_ctx):
    """1080p S-blob frames, as many as put more than 48 key points on every CU's sixteen wave slots (a frame has about 2150): all per-frame
    counts and key points, a seeded sample of 2048 descriptors and orientations against the oracle, and the whole batch array_equal to the
    same frames described one image per call"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    need = 3 * 16 * cus
    B = max(8, need // 1800 + 2)
    arrays = [blobs(orc, 1920, 1080, 3000 + i).array().copy() for i in range(B)]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32, ctx=dev_ctx)
    keep = _detect_device(api, torch, dd, arrays)
    got = [tuple(np.array(x) for x in dd._results(i)) for i in range(B)]
    del keep
    total = dd.totalFeatures()
    assert total > need, (total, need)
    ref = orc.Surf(True)
    rng = np.random.default_rng(20260101)
    pick = np.sort(rng.choice(total, 2048, replace=False))
    base = 0
    checked = 0
    for i, a in enumerate(arrays):
        n = ref.detect(orc.Gray.from_array(a), threads=THREADS)
        xys, ang, white, desc = ref.fetch()
        assert len(got[i][0]) == n and np.array_equal(got[i][0], xys) and np.array_equal(got[i][2], white), i
        rows = pick[(pick >= base) & (pick < base + n)] - base
        derr = np.max(np.abs(got[i][3][rows] - desc[rows]), axis=1)
        assert int((derr > DESC_TOL).sum()) == 0, (i, derr.max())
        assert _adiff(got[i][1][rows], ang[rows]).max() < ANG_TOL, i
        checked += len(rows)
        base += n
    assert base == total and checked == 2048
    one = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    for i, a in enumerate(arrays):
        one.detect(api.GrayF32.wrap(a))
        assert all(np.array_equal(x, y) for x, y in zip(one._results(), got[i])), i


# ------------------------------------------------------------------------------------------------------------------ 3. uneven chunks
def test_key_points_in_the_first_frames(api, orc, torch, dev_ctx):
    """two 640x480 S-blob frames followed by six flat ones: every order record names one of the first two images, the eight chunks of the
    order are short against the wave count, and waves whose chunk is used up take slots of the others"""
    arrays = [blobs(orc, 640, 480, 4000 + i).array().copy() for i in range(2)] + [_flat(640, 480, 10.0 * i) for i in range(6)]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32, ctx=dev_ctx)
    keep = _detect_device(api, torch, dd, arrays)
    counts = _check_batch(api, orc, dd, orc.Surf(True), arrays, "first frames")
    assert counts[0] > 200 and counts[1] > 200 and counts[2:] == [0] * 6
    del keep


# ------------------------------------------------------------------------------------------------------------------ 4. paths that share the kernel
def test_describe_only_entry(api, orc):
    """describePoints: a flat list for one image, no processing order (the image comes from the call, not from an order record)"""
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    ref = orc.Surf(True)
    imgs = [orc.noise_image(160, 120, 5 + k) for k in range(2)]
    dd.detectBatch([G(api, im) for im in imgs])
    for i, im in enumerate(imgs):
        ang, white, desc = dd.describePoints(POINTS, image=i)
        ref.describe_points(POINTS, im)
        _, rang, rwhite, rdesc = ref.fetch()
        _compare((POINTS, ang, white, desc), (POINTS, rang, rwhite, rdesc), "describePoints image %d" % i)


def test_surf_fast(api, orc, torch, dev_ctx):
    arrays = [orc.noise_image(160, 120, 5 + k).array().copy() for k in range(3)]
    dd = api.FactoryDetectDescribe.surfFast(None, None, None, api.GrayF32, ctx=dev_ctx)
    keep = _detect_device(api, torch, dd, arrays)
    assert sum(_check_batch(api, orc, dd, orc.Surf(False), arrays, "surfFast")) > 500
    del keep


def test_generic_grid(api, orc, torch, dev_ctx):
    """s-4-6-3: sub-region rows of 12 samples, the <8,16> instantiation with 8-byte samples (59 648 bytes of LDS: two workgroups per CU)"""
    arrays = [orc.noise_image(160, 120, 5 + k).array().copy() for k in range(3)]
    dd = make(api, "s-4-6-3", ctx=dev_ctx)
    keep = _detect_device(api, torch, dd, arrays)
    assert sum(_check_batch(api, orc, dd, make_ref(orc, "s-4-6-3"), arrays, "s-4-6-3")) > 500
    del keep


def test_gray_u8(api, orc):
    """integer taps: the GrayS32 integral image of a GrayU8 frame"""
    imgs = [np.floor(orc.noise_image(160, 120, 5 + k, 0, 255).array()).astype(np.uint8) for k in range(2)]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayU8)
    ref = orc.Surf(True)
    dd.detectBatch([api.GrayU8.wrap(im) for im in imgs])
    for i, im in enumerate(imgs):
        ref.detect_u8(im)
        assert _compare(dd._results(i), ref.fetch(), "GrayU8 frame %d" % i)[0] > 100


@pytest.mark.parametrize("w,h", [(150, 120), (640, 480)])
def test_colour_band_loop(api, orc, w, h):
    """colour SURF, three bands: the band loop runs inside the key-point loop; at 640x480 there are more key points than waves"""
    rand = orc.JavaRandom(234)
    bands = [rand.fillUniform(orc.Gray(w, h), 0, 200) for _ in range(3)]
    ref = make_ref(orc, "s-3-5-2")
    n = ref.detect_planar(bands, threads=THREADS)
    want = ref.fetch()
    dd = make(api, "s-3-5-2", bands=3)
    dd.detect(api.Planar.wrap([G(api, b) for b in bands]))
    assert _compare(dd._results(), want, "colour %dx%d" % (w, h))[0] == n and n > 10


# ------------------------------------------------------------------------------------------------------------------ 5. repeatability
def test_successive_batches_on_one_object(api, orc, torch, dev_ctx):
    """the counters are cleared for every launch: a large batch, then a small one, then the large one again, each against the oracle"""
    big = [orc.noise_image(320, 240, 70 + k).array().copy() for k in range(3)]
    small = [orc.noise_image(320, 240, 80).array().copy(), _flat(320, 240)]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32, ctx=dev_ctx)
    ref = orc.Surf(True)
    first = None
    for arrays, what in ((big, "big"), (small, "small"), (big, "big again")):
        keep = _detect_device(api, torch, dd, arrays)
        counts = _check_batch(api, orc, dd, ref, arrays, what)
        del keep
        if what == "big":
            first = (counts, [tuple(np.array(x) for x in dd._results(i)) for i in range(len(arrays))])
        if what == "big again":
            assert counts == first[0]
            for i in range(len(arrays)):
                assert all(np.array_equal(x, y) for x, y in zip(dd._results(i), first[1][i])), i
