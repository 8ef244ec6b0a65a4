"""SURF describe on non-default sample grids: the generic k_describe instantiations, the LDS limits, and every host path that carries dof.

Every other descriptor test runs ConfigSurfDescribe's defaults, i.e. the two compile-time kernels k_describe<5,9,T,1> and <3,5,T,2>.  Here
each geometry goes through detect and describePoints against the CPU oracle (which tests/test_surf_reference.py pins, bit for bit, to a
numpy restatement of the Java on the same geometries), and a subset goes through detectBatch, detectDevice, the chunked host batch,
GrayU8 frames, colour SURF, fetchAll / getDescription and resident association.

The bars are the project's own (tests/test_gpu_parity.py::_compare_surf, restated in _compare): key points and Laplacian signs bit-exact,
every descriptor value within DESC_TOL = 1e-5, every orientation within 1e-12 rad, norms 1 within 1e-12.

Dynamic LDS = 4 * bhip_describe_lds_bytes (describe.hip): per wave max(orientation, descriptor), rounded up to 16, with n = oriWidth^2,
  orientation = max(32 n + 16, align16(28 n) + 2048)      sliding radius 8: n = 289 -> 10144;  average radius 6: n = 169 -> 6784
  descriptor  = 2 * gridW^2 * (8 generic | 4 default-config) + 8 * dof * bands
Kernel choice (bhip_launch_describe_ex): CFG 1 / 2 for the default grid + overlap + orientation width; else <5,9,T,0> when EPL = ceil(n / 64)
is 5 and tw = widthSubRegion + 2 overLap is 9; else <3,5,T,0> when EPL is 3 and tw is 5; else <8,16,T,0>.  T = float for GrayF32 frames,
int for GrayU8 frames.  The sampling loop of the generic kernels walks ceil(gridW / 8)^2 blocks in batches of three.

surfFast on (3, 5) is not a geometry: widthLargeGrid * widthSubRegion is odd, DescribePointSurf.features throws "Weighting kernel has an
unexpected size" (DescribePointSurf.java:122-123, 241-243) and bhip_surf_create answers BHIP_ERR_INVALID.  It is with the refusals; fast
(2, 5) and (6, 5) are the grids that reach <3,5,T,0>.

Measured on an MI355X, detect on the 160x120 noise frame and the 200x160 blob frame together (per geometry in MEASURED below): descriptor
error at most 4.4e-16 (stable) / 3.1e-16 (fast) against the 1e-5 bar, orientation error at most 1.33e-15 rad (sliding, radius 8 and 10)
/ 4.4e-16 rad (average, and sliding radius 1) against 1e-12, |norm - 1| at most 2.2e-16.  The other paths (describePoints, GrayU8, colour)
stay below 4.5e-16 and 1.4e-15 rad as well.  Dynamic LDS above 64 KiB (the hipFuncSetAttribute branch): s-6-5-2, s-8-5-2, f-2-16,
s-r10-6-5-2, and colour SURF on s-6-5-2.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DESC_TOL = 1e-5   # north star: SURF descriptors within 1e-5 (unit vectors)
ANG_TOL = 1e-12   # every orientation, rad
NORM_TOL = 1e-12

# name -> (stable, describe fields, orientation radius or None)            gridW dof kernel      dynamic LDS   why
GEOMETRIES = {
    # stable: sliding orientation, radius 8, n = 289, EPL 5
    "s-3-5-2": (True, dict(widthLargeGrid=3, widthSubRegion=5, overLap=2), None),      # 19  36  <5,9,0>    40 576  odd grid width, 9 blocks, dof 36
    "s-4-7-1": (True, dict(widthLargeGrid=4, widthSubRegion=7, overLap=1), None),      # 30  64  <5,9,0>    59 648  16 blocks, the 4x4 lane layout at run-time sizes
    "s-4-6-3": (True, dict(widthLargeGrid=4, widthSubRegion=6, overLap=3), None),      # 30  64  <8,16,0>   59 648  tw 12
    "s-2-12-2": (True, dict(widthLargeGrid=2, widthSubRegion=12, overLap=2), None),    # 28  16  <8,16,0>   50 688  tw 16 = DESC_ROW_MAX, accepted
    "s-6-5-2": (True, dict(widthLargeGrid=6, widthSubRegion=5, overLap=2), None),      # 34 144  <5,9,0>    78 592  above 64 KiB: the attribute branch; 25 blocks
    "s-8-5-2": (True, dict(widthLargeGrid=8, widthSubRegion=5, overLap=2), None),      # 44 256  <5,9,0>   132 096  largest accepted; one workgroup per CU
    "s-sigmas": (True, dict(widthSample=5, sigmaLargeGrid=1.0, sigmaSubRegion=4.0), None),   # 24 64 CFG 1  40 576  the kernel must still honour the tables
    # fast: average orientation, radius 6, n = 169, EPL 3
    "f-2-5": (False, dict(widthLargeGrid=2, widthSubRegion=5), None),                  # 10  16  <3,5,0>    27 136  4 blocks
    "f-6-5": (False, dict(widthLargeGrid=6, widthSubRegion=5), None),                  # 30 144  <3,5,0>    62 208  16 blocks, dof 144
    "f-4-3": (False, dict(widthLargeGrid=4, widthSubRegion=3), None),                  # 12  64  <8,16,0>   27 136  tw 3
    "f-2-8": (False, dict(widthLargeGrid=2, widthSubRegion=8, weightSigma=2.0), None),  # 16 16  <8,16,0>   27 136  4 blocks
    "f-2-16": (False, dict(widthLargeGrid=2, widthSubRegion=16), None),                # 32  16  <8,16,0>   66 048  just above 64 KiB; tw 16
    "f-1-4": (False, dict(widthLargeGrid=1, widthSubRegion=4), None),                  #  4   4  <8,16,0>   27 136  one partly filled block (oracle: finite, unit norm)
    "f-sigma": (False, dict(widthSample=2, weightSigma=2.0), None),                    # 20  64  CFG 2      27 136  the kernel must still honour the tables
    # orientation extremes, alone (default grid, so <8,16,0> with 8-byte samples) and with one non-default grid each
    "s-r10": (True, dict(), 10),                                                       # 24  64  <8,16,0>   57 600  n = 441, EPL 7, the largest accepted
    "s-r1": (True, dict(), 1),                                                         # 24  64  <8,16,0>   38 912  n = 9
    "f-r10": (False, dict(), 10),                                                      # 20  64  <8,16,0>   57 600
    "f-r1": (False, dict(), 1),                                                        # 20  64  <8,16,0>   27 648
    "s-r10-6-5-2": (True, dict(widthLargeGrid=6, widthSubRegion=5, overLap=2), 10),    # 34 144  <8,16,0>   78 592
    "s-r1-3-5-2": (True, dict(widthLargeGrid=3, widthSubRegion=5, overLap=2), 1),      # 19  36  <8,16,0>   24 256
    "f-r10-2-8": (False, dict(widthLargeGrid=2, widthSubRegion=8, weightSigma=2.0), 10),   # 16 16 <8,16,0> 57 600
    "f-r1-6-5": (False, dict(widthLargeGrid=6, widthSubRegion=5), 1),                  # 30 144  <8,16,0>   62 208
}
# the geometries that go through every other path that carries dof or the config
SUBSET = ["s-3-5-2", "s-6-5-2", "f-6-5", "f-2-8"]

# name -> (max descriptor error, max orientation error in rad, max |norm - 1|) over detect on both frames, as test_detect_and_describe_points
# prints them.  A record of one MI355X run, not a bar: the bars are DESC_TOL, ANG_TOL and NORM_TOL.
MEASURED = {
    "s-3-5-2": (2.5e-16, 1.33e-15, 2.22e-16), "s-4-7-1": (3.33e-16, 1.33e-15, 2.22e-16), "s-4-6-3": (4.44e-16, 1.33e-15, 2.22e-16),
    "s-2-12-2": (3.33e-16, 1.33e-15, 2.22e-16), "s-6-5-2": (1.94e-16, 1.33e-15, 2.22e-16), "s-8-5-2": (1.94e-16, 1.33e-15, 2.22e-16),
    "s-sigmas": (4.44e-16, 1.33e-15, 2.22e-16), "f-2-5": (1.67e-16, 4.44e-16, 2.22e-16), "f-6-5": (2.22e-16, 4.44e-16, 2.22e-16),
    "f-4-3": (1.67e-16, 4.44e-16, 2.22e-16), "f-2-8": (2.22e-16, 4.44e-16, 2.22e-16), "f-2-16": (1.67e-16, 4.44e-16, 2.22e-16),
    "f-1-4": (3.05e-16, 4.44e-16, 2.22e-16), "f-sigma": (2.78e-16, 4.44e-16, 2.22e-16), "s-r10": (3.33e-16, 1.33e-15, 2.22e-16),
    "s-r1": (2.78e-16, 4.44e-16, 2.22e-16), "f-r10": (2.78e-16, 4.44e-16, 2.22e-16), "f-r1": (2.78e-16, 4.44e-16, 2.22e-16),
    "s-r10-6-5-2": (2.22e-16, 1.33e-15, 2.22e-16), "s-r1-3-5-2": (2.22e-16, 4.44e-16, 2.22e-16), "f-r10-2-8": (2.22e-16, 4.44e-16, 2.22e-16),
    "f-r1-6-5": (2.78e-16, 4.44e-16, 2.22e-16),
}


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api as a
    a.Context.default()  # fails loudly without a GPU / without libboofhip.so
    return a


def G(api, g):
    return api.GrayF32(g.width, g.height, g.buf, g.startIndex, g.stride)


def make(api, name, imageType=None, ctx=None, bands=0):
    stable, g, radius = GEOMETRIES[name]
    F = api.FactoryDetectDescribe
    if stable:
        cfg = api.ConfigSurfDescribe.Stability(**g)
        ori = api.ConfigSlidingIntegral(radius=radius) if radius else None
        fac = F.surfColorStable if bands else F.surfStable
    else:
        cfg = api.ConfigSurfDescribe.Speed(**g)
        ori = api.ConfigAverageIntegral(radius=radius) if radius else None
        fac = F.surfColorFast if bands else F.surfFast
    return fac(None, cfg, ori, api.PlanarType(bands) if bands else (imageType or api.GrayF32), ctx=ctx)


def make_ref(orc, name):
    stable, g, radius = GEOMETRIES[name]
    ori = None
    if radius:
        ori = orc.OriCfg.sliding(radius=radius) if stable else orc.OriCfg.average(radius=radius)
    return orc.Surf(stable, sd=orc.SurfCfg(**g), ori=ori)


def dof_of(name):
    return GEOMETRIES[name][1].get("widthLargeGrid", 4) ** 2 * 4


def _adiff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def _compare(got, want, what):
    """tests/test_gpu_parity.py::_compare_surf's rules on (xys, angle, white, desc) tuples -> (n, max desc err, max angle err, max |norm-1|)"""
    xys, ang, white, desc = want
    n = len(xys)
    assert len(got[0]) == n, what
    assert np.array_equal(got[0], xys), what          # location + scale: bit exact, reference order
    assert np.array_equal(got[2], white), what        # Laplacian sign
    if not n:
        return 0, 0.0, 0.0, 0.0
    assert got[3].shape == desc.shape, (what, got[3].shape, desc.shape)
    dang = _adiff(got[1], ang)
    derr = np.max(np.abs(got[3] - desc), axis=1)
    # UtilFeature.normalizeL2 leaves an all-zero descriptor (every sample box outside the image) as it is: such a row must be zero here
    # too, every other row has norm 1
    zero = ~np.any(desc, axis=1)
    assert not np.any(got[3][zero]), what
    nerr = np.where(zero, 0.0, np.abs(np.linalg.norm(got[3], axis=1) - 1))
    print("%s: n %d  max desc err %.3g  max angle err %.3g  max |norm-1| %.3g" % (what, n, derr.max(), dang.max(), nerr.max()))
    nout = int((derr > DESC_TOL).sum())
    assert nout == 0, "%s: descriptors outside 1e-5: %d of %d, max err %.3g, their angle errors %s" % (what, nout, n, derr.max(), dang[derr > DESC_TOL][:5])
    assert dang.max() < ANG_TOL, "%s: orientation max err %.3g rad at key point %d" % (what, dang.max(), int(dang.argmax()))
    assert nerr.max() <= NORM_TOL, (what, nerr.max())
    return n, float(derr.max()), float(dang.max()), float(nerr.max())


def _blob_frame(orc, w=200, h=160, seed=77):
    """S-blobs as in test_surf_random_shapes_batched: large-scale key points next to the borders"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.full((h, w), 50.0)
    for _ in range(max(4, w * h // 2500)):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        sg = float(rng.choice([2, 3, 5, 8, 13]))
        amp = float(rng.uniform(40, 100) * rng.choice([-1, 1]))
        a += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sg * sg))
    a += rng.uniform(0, 2, (h, w))
    return orc.Gray.from_array(a.astype(np.float32))


@pytest.fixture(scope="module")
def frames(orc):
    """160x120 noise frames (seed 5: 218 key points) and one 200x160 blob frame; read only"""
    return dict(noise=[orc.noise_image(160, 120, 5 + k) for k in range(5)], blob=_blob_frame(orc))


# border, fractional and large-scale points (the list of test_surf_describe_points_edge_cases on a 160x120 frame)
POINTS = np.array([[0, 0, 1.0], [159, 119, 1.0], [60.3, 50.7, 1.5], [3.2, 116.1, 2.2], [157.9, 2.5, 4.0], [60, 50, 9.7], [25, 25, 1.2]])


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_detect_and_describe_points(api, orc, frames, name):
    dd = make(api, name)
    ref = make_ref(orc, name)
    dof = dof_of(name)
    assert dd.createDescription().size() == dof == ref.dof
    worst = np.zeros(3)
    total = 0
    for label, img in (("noise", frames["noise"][0]), ("blob", frames["blob"])):
        dd.detect(G(api, img))
        ref.detect(img)
        want = ref.fetch()
        n, de, ae, ne = _compare(dd._results(), want, "%s detect %s" % (name, label))
        worst = np.maximum(worst, [de, ae, ne])
        total += n
        assert dd._results()[3].shape == (n, dof)
    assert total > 200
    print("%s: MEASURED %.3g %.3g %.3g" % (name, *worst))
    # describePoints on the noise frame
    img = frames["noise"][0]
    dd.detect(G(api, img))
    ang, white, desc = dd.describePoints(POINTS)
    ref.describe_points(POINTS, img)
    _, rang, rwhite, rdesc = ref.fetch()
    _compare((POINTS, ang, white, desc), (POINTS, rang, rwhite, rdesc), "%s describePoints" % name)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _default_detect_equals_oracle(api, orc, frames, ctx):
    img = frames["noise"][0]
    dd = api.FactoryDetectDescribe.surfStable(None, None, None, api.GrayF32, ctx=ctx)
    dd.detect(G(api, img))
    ref = orc.Surf(True)
    ref.detect(img)
    assert _compare(dd._results(), ref.fetch(), "default detect after a refusal")[0] > 100
    dd.close()


REFUSED_AT_DETECT = {
    "s-2-13-2": (True, dict(widthLargeGrid=2, widthSubRegion=13, overLap=2)),    # tw 17 > DESC_ROW_MAX
    "f-2-17": (False, dict(widthLargeGrid=2, widthSubRegion=17)),                # tw 17
    "s-9-5-2": (True, dict(widthLargeGrid=9, widthSubRegion=5, overLap=2)),      # gridW 49, dof 324: 4 * 41 008 = 164 032 > 163 840
    "s-4-12-2": (True, dict(widthLargeGrid=4, widthSubRegion=12, overLap=2)),    # tw 16 is allowed, 4 * 43 776 = 175 104 bytes of LDS are not
}


@pytest.mark.parametrize("name", list(REFUSED_AT_DETECT))
def test_refused_at_detect(api, orc, frames, name):
    stable, g = REFUSED_AT_DETECT[name]
    # the oracle takes the geometry: the refusal is the GPU path's own limit, not the reference's
    ref = orc.Surf(stable, sd=orc.SurfCfg(**g))
    assert ref.detect(frames["noise"][0]) > 100
    ctx = api.Context(0)
    cfg = (api.ConfigSurfDescribe.Stability if stable else api.ConfigSurfDescribe.Speed)(**g)
    dd = (api.FactoryDetectDescribe.surfStable if stable else api.FactoryDetectDescribe.surfFast)(None, cfg, None, api.GrayF32, ctx=ctx)
    for _ in range(2):   # refused every time, not only the first
        with pytest.raises(RuntimeError, match="status -2"):
            dd.detect(G(api, frames["noise"][0]))
        # nothing the caller can see: no batch, no counts, no features
        assert dd.totalFeatures() == 0 and len(dd.counts()) == 0
        with pytest.raises(api.IllegalArgumentException):
            dd._results(0)
        with pytest.raises(api.IllegalArgumentException):
            dd.describePoints(POINTS)
    _default_detect_equals_oracle(api, orc, frames, ctx)
    dd.close(); ctx.close()


def test_refused_at_create(api, orc, frames):
    ctx = api.Context(0)
    F = api.FactoryDetectDescribe
    with pytest.raises(RuntimeError, match="status -2"):     # orientation radius 11: n = 529 > 64 * ORI_EPL_MAX
        F.surfStable(None, None, api.ConfigSlidingIntegral(radius=11), api.GrayF32, ctx=ctx)
    with pytest.raises(RuntimeError, match="status -2"):
        F.surfFast(None, None, api.ConfigAverageIntegral(radius=11), api.GrayF32, ctx=ctx)
    # surfFast on an odd widthLargeGrid * widthSubRegion: the reference throws IllegalArgumentException, and so do the oracle and the GPU path
    with pytest.raises(api.IllegalArgumentException, match="unexpected size"):
        F.surfFast(None, api.ConfigSurfDescribe.Speed(widthLargeGrid=3, widthSubRegion=5), None, api.GrayF32, ctx=ctx)
    with pytest.raises(ValueError, match="unexpected size"):
        orc.Surf(False, sd=orc.SurfCfg(widthLargeGrid=3, widthSubRegion=5))
    _default_detect_equals_oracle(api, orc, frames, ctx)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ the other entry points
@pytest.mark.parametrize("name", SUBSET)
def test_detect_batch_fetch_all_and_getters(api, orc, frames, name):
    dd = make(api, name)
    ref = make_ref(orc, name)
    dof = dof_of(name)
    imgs = frames["noise"][:3]
    dd.detectBatch([G(api, im) for im in imgs])
    xys, ang, white, desc, starts = dd.fetchAll()
    assert desc.shape == (dd.totalFeatures(), dof) and starts[-1] == dd.totalFeatures()
    for i, im in enumerate(imgs):
        ref.detect(im)
        want = ref.fetch()
        dd.selectImage(i)
        one = dd._results()
        assert _compare(one, want, "%s detectBatch image %d" % (name, i))[0] > 100
        sl = slice(int(starts[i]), int(starts[i + 1]))
        assert np.array_equal(xys[sl], one[0]) and np.array_equal(ang[sl], one[1]) and np.array_equal(white[sl], one[2]) and np.array_equal(desc[sl], one[3])
        d = dd.getDescription(len(one[0]) - 1)
        assert isinstance(d, api.BrightFeature) and d.size() == dof == dd.createDescription().size()
        assert np.array_equal(np.asarray(d.value), one[3][-1]) and d.white == bool(one[2][-1])


@pytest.mark.parametrize("name", SUBSET)
def test_detect_device_padded_rows(api, orc, frames, name):
    """as test_detect_device_padded_rows_equals_dense_host_batch: rows and images padded with 1e6, against the dense host batch"""
    torch = pytest.importorskip("torch")
    w, h, stride, rows, batch = 160, 120, 176, 125, 3
    imgs = frames["noise"][:batch]
    host = make(api, name)
    host.detectBatch([G(api, im) for im in imgs])
    want = host.fetchAll()
    padded = np.full((batch, rows, stride), 1e6, dtype=np.float32)
    for b, im in enumerate(imgs):
        padded[b, :h, :w] = im.array()
    dev_frames = torch.from_numpy(padded).cuda()
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    dev = make(api, name, ctx=ctx)
    dev.detectDevice(dev_frames.data_ptr(), stride * rows, stride, w, h, batch)
    got = dev.fetchAll()
    assert want[-1][-1] > 100 * batch and got[3].shape == (want[-1][-1], dof_of(name))
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (name, k)
    dev.close(); ctx.close()


_CHUNK_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from boofcv_amd import api
import test_gpu_surf_configs as t
fr = np.load(%(frames)r)
out = {}
for name in t.SUBSET:
    dd = t.make(api, name)
    dd.detectBatch([api.GrayF32(fr.shape[2], fr.shape[1], f.reshape(-1)) for f in fr])
    o = dd.fetchAll()
    p, f = dd.associateImages(np.arange(5), (np.arange(5) + 1) %% 5)
    for k, a in zip(("xys", "ang", "white", "desc", "starts", "pairs", "fit", "one"), o + (p, f, dd._results(3)[3])):
        out[name + "/" + k] = a
np.savez(%(out)r, **out)
"""


def test_chunked_host_batch_equals_plain(api, orc, frames, tmp_path):
    """as tests/test_gpu_parity.py::test_chunked_host_batch_equals_plain: a child process with BHIP_SURF_CHUNK=2 takes a batch of 5 through
    chunks of 2, 2, 1 -- the worker object is created from the owner's describe config (surfRunChunked) and its descriptors are appended
    dof values at a time -- and is compared, array by array, with the plain path of this process."""
    fr = np.stack([im.array().copy() for im in frames["noise"]])
    np.save(tmp_path / "frames.npy", fr)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "chunked.npz")
    code = _CHUNK_CHILD % dict(root=root, tests=os.path.join(root, "tests"), frames=str(tmp_path / "frames.npy"), out=out)
    e = dict(os.environ); e["BHIP_SURF_CHUNK"] = "2"
    subprocess.run([sys.executable, "-c", code], check=True, env=e, timeout=120)
    got = np.load(out)
    for name in SUBSET:
        dd = make(api, name)
        dd.detectBatch([api.GrayF32(160, 120, f.reshape(-1)) for f in fr])
        base = dd.fetchAll()
        pairs, fit = dd.associateImages(np.arange(5), (np.arange(5) + 1) % 5)
        assert base[4][-1] > 500 and base[3].shape[1] == dof_of(name)
        for k, key in enumerate(["xys", "ang", "white", "desc", "starts"]):
            assert np.array_equal(got[name + "/" + key], base[k]), (name, key)
        assert np.array_equal(got[name + "/pairs"], pairs) and np.array_equal(got[name + "/fit"], fit), name
        assert np.array_equal(got[name + "/one"], dd._results(3)[3]), name


@pytest.mark.parametrize("name", SUBSET)
def test_gray_u8_frames(api, orc, frames, name):
    """GrayU8 frames: GrayS32 integral image, the `int` generic instantiations"""
    img = np.floor(orc.noise_image(160, 120, 5, 0, 255).array()).astype(np.uint8)
    dd = make(api, name, imageType=api.GrayU8)
    ref = make_ref(orc, name)
    dd.detect(api.GrayU8.wrap(img))
    ref.detect_u8(img)
    assert _compare(dd._results(), ref.fetch(), "%s GrayU8" % name)[0] > 100
    ang, white, desc = dd.describePoints(POINTS)
    # the oracle describes a caller's points on the integral image of its last detect
    ref.describe_points(POINTS)
    _, rang, rwhite, rdesc = ref.fetch()
    _compare((POINTS, ang, white, desc), (POINTS, rang, rwhite, rdesc), "%s GrayU8 describePoints" % name)


@pytest.mark.parametrize("name", ["s-3-5-2", "s-6-5-2"])
def test_color_surf_three_bands(api, orc, name):
    """colour SURF: dof * bands values per key point; s-6-5-2 needs 4 * (2 * 34^2 * 8 + 8 * 144 * 3) = 87 808 bytes of LDS, 432 values"""
    rand = orc.JavaRandom(234)
    w, h, nb = 150, 120, 3
    bands = [rand.fillUniform(orc.Gray(w, h), 0, 200) for _ in range(nb)]
    ref = make_ref(orc, name)
    n = ref.detect_planar(bands)
    want = ref.fetch()
    dd = make(api, name, bands=nb)
    dd.detect(api.Planar.wrap([G(api, b) for b in bands]))
    assert dd.createDescription().size() == dof_of(name) * nb == want[3].shape[1]
    assert _compare(dd._results(), want, "%s colour" % name)[0] == n and n > 10


def test_exact_scan_descriptor_length_limit(api, orc):
    """The scan's LDS tile is 64 descriptors: dof 320 is 163 840 bytes, a workgroup's whole LDS, and is accepted; dof 321 is refused.
    70 x 65 descriptors: more than one tile on either side, and a partly filled last tile."""
    rng = np.random.default_rng(9)
    for dof, ok in ((320, True), (321, False)):
        src = rng.normal(size=(70, dof)); dst = rng.normal(size=(65, dof))
        src /= np.linalg.norm(src, axis=1, keepdims=True); dst /= np.linalg.norm(dst, axis=1, keepdims=True)
        dst[:20] = src[5:25] + rng.normal(scale=1e-3, size=(20, dof))     # some true matches
        assoc = api.FactoryAssociation.greedy(api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True)
        assoc.setSource(src); assoc.setDestination(dst)
        if ok:
            assoc.associate()
            ep, ef = orc.associate_l2(src, dst)
            assert np.array_equal(assoc.getPairs(), ep) and np.array_equal(assoc.getFitQuality(), ef) and (ep >= 0).sum() >= 20
        else:
            with pytest.raises(RuntimeError, match="status -2"):
                assoc.associate()


@pytest.mark.parametrize("name", ["s-3-5-2", "s-6-5-2", "s-8-5-2"])
def test_resident_association_takes_the_exact_scan(api, orc, frames, name):
    """dof 36, 144 and 256: the fp16 matrix-core filter is built for 64 values, so resident association must answer from the exact
    L2ScorerDyn scan -- pairs and scores equal to the oracle's on the fetched descriptors, bit for bit.  The scan stages 64 descriptors
    per LDS tile: 73 728 bytes at dof 144 and 131 072 at dof 256, above the 64 KiB a kernel gets without asking (this was refused as
    "descriptor too long for the LDS tile" before the scan learnt to ask).  The host-list association takes the same scan."""
    ctx = api.Context(0)
    ctx.profile(True)
    dd = make(api, name, ctx=ctx)
    dd.detectBatch([G(api, im) for im in frames["noise"][:2]])
    xys, ang, white, desc, starts = dd.fetchAll()
    assert desc.shape[1] == dof_of(name) and starts[1] > 100 and starts[2] - starts[1] > 100
    for backwards in (True, False):
        for maxErr in (api.Double_MAX_VALUE, 0.2):
            ctx.profileReset()
            pairs, fit = dd.associateImages([0, 1], [1, 0], maxErr, backwards)
            rep = ctx.profileReport()
            assert "k_assoc_scan_rows" in rep and not any(k.startswith("k_assoc_mfma") for k in rep), sorted(rep)
            for a, b in ((0, 1), (1, 0)):
                sa = slice(int(starts[a]), int(starts[a + 1]))
                ep, ef = orc.associate_l2(desc[sa], desc[int(starts[b]):int(starts[b + 1])], maxErr, backwards)
                assert np.array_equal(pairs[sa], ep) and np.array_equal(fit[sa], ef), (name, a, b, backwards, maxErr)
    src, dst = desc[:int(starts[1])], desc[int(starts[1]):]
    ctx.profileReset()
    assoc = api.FactoryAssociation.greedy(api.ScoreAssociateEuclideanSq_F64(), api.Double_MAX_VALUE, True, ctx=ctx)
    assoc.setSource(src); assoc.setDestination(dst); assoc.associate()
    rep = ctx.profileReport()
    assert "k_assoc_scan_rows" in rep and not any(k.startswith("k_assoc_mfma") for k in rep), sorted(rep)
    ep, ef = orc.associate_l2(src, dst)
    assert np.array_equal(assoc.getPairs(), ep) and np.array_equal(assoc.getFitQuality(), ef), name
    dd.close(); ctx.close()
