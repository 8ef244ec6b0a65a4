"""GPU: FhDetector::run (csrc/cabi.hip) launches k_rank_scatter before it has read the candidate counts back, so after a list overflow the
kernel ranks an incomplete list once (its store is guarded) and the detector runs again with a longer list.

The overflow is forced the way tests/test_gpu_surf_regrow.py forces it: ConfigFastHessian(detectThreshold=0, extractRadius=1) on a
720x540 noise frame, whose key points exceed BHIP_SURF_INITIAL_CAPACITY (a 160x120 frame has fewer blocks than the list has slots and
cannot overflow it); its two neighbours in the batch stay far below the capacity.  The run that overflowed must leave what a run on the
grown object leaves, array for array, and the big frame's key points are the oracle's.  The plain case is three 160x120 frames against
the oracle's detect + describe.  Run with `pytest -m gpu` on an MI355X."""
import os

import numpy as np
import pytest

from boofcv_amd import _lib

pytestmark = pytest.mark.gpu

W, H = 720, 540
CAP = _lib.BHIP_SURF_INITIAL_CAPACITY
FH = dict(detectThreshold=0, extractRadius=1)
THREADS = min(os.cpu_count() or 1, 8)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()
    return a


def _copy(arrays):
    return tuple(np.array(a) for a in arrays)


def _scatter_launches(dd, images):
    """detectBatch under the per-kernel profile -> (fetchAll arrays, launches of k_rank_scatter): one per run of the detector"""
    ctx = dd.ctx
    ctx.profile(True)
    ctx.profileReset()
    try:
        dd.detectBatch(images)
        return _copy(dd.fetchAll()), ctx.profileReport().get("k_rank_scatter", {}).get("launches", 0)
    finally:
        ctx.profile(False)


def test_overflow_seen_by_the_early_scatter(api, orc):
    """[quarter noise, full noise, zeros]: the first call overflows on the middle frame, after k_rank_scatter has already been launched on
    the short list, and reruns (two launches); the second call on the grown object does not (one launch).  Same key points, counts,
    orientations, Laplacian signs and descriptors."""
    full = orc.noise_image(W, H, 5).array().copy()
    quarter = np.full((H, W), 50.0, np.float32)
    quarter[:270, :360] = orc.noise_image(360, 270, 11).array()
    frames = [quarter, np.ascontiguousarray(full, np.float32), np.zeros((H, W), np.float32)]
    want_full = orc.fh_detect(orc.integral(orc.Gray.from_array(frames[1])), orc.FhCfg(**FH), threads=THREADS)
    assert len(want_full) > CAP, (len(want_full), CAP)        # the precondition: this frame alone overflows the list
    images = [api.GrayF32.wrap(f) for f in frames]
    dd = api.FactoryDetectDescribe.surfStable(api.ConfigFastHessian(**FH), None, None, api.GrayF32)
    first, n1 = _scatter_launches(dd, images)
    again, n2 = _scatter_launches(dd, images)
    assert (n1, n2) == (2, 1), (n1, n2)
    counts = [int(c) for c in np.diff(first[4])]
    assert counts[1] == len(want_full) and 1000 <= counts[0] <= CAP // 2 and counts[2] == 0, counts
    assert len(first) == len(again)
    for k, (a, b) in enumerate(zip(first, again)):
        assert a.shape == b.shape and np.array_equal(a, b), k
    assert np.array_equal(np.array(dd._results(1)[0]), want_full)
    dd.close()


def test_plain_batch_without_overflow(api, orc):
    """three 160x120 noise frames with the default configuration: one run of the detector, key points bit for bit, descriptors within 1e-5"""
    ims = [orc.noise_image(160, 120, 234 + k) for k in range(3)]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32)
    got_all, n = _scatter_launches(dd, [api.GrayF32(im.width, im.height, im.buf) for im in ims])
    assert n == 1
    ref = orc.Surf(True)
    for i, im in enumerate(ims):
        cnt = ref.detect(im)
        xys, ang, white, desc = ref.fetch()
        got = _copy(dd._results(i))
        assert cnt > 20 and len(got[0]) == cnt
        assert np.array_equal(got[0], xys) and np.array_equal(got[2], white)
        assert np.max(np.abs(np.angle(np.exp(1j * (got[1] - ang))))) < 1e-12
        assert np.max(np.abs(got[3] - desc)) < 1e-5
    assert int(got_all[4][-1]) == dd.totalFeatures()
    dd.close()
