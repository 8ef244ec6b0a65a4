"""GPU: the SIFT detector (FactoryInterestPoint.sift: SiftScaleSpace, SiftDetector, NonMaxLimiter, WrapSiftDetector), bit for bit against
tests/sift_ref.py through the device-batched API (device.py), the host mirror (boofcv_amd/sift.py) and the C ABI.  Scale and DoG images are
compared as bit patterns at every pixel of every octave; detections in every field (x, y, scale as float64 bit patterns, white, octave, DoG
index, pixel) and in order.

k_sift_level takes 64 x 64 tiles and odd kernels of 3 .. 27 taps narrower than the image over 16-byte aligned rows; everything else is two
normalised passes and a subtract, as is everything under BHIP_SIFT_TWO_PASS=1 (run in a child process through the host forms).
  80 x 70   the reference test's config (-1, 5, 3, 1.6), extractor radius 1: firstOctave -1, six octaves 160 x 140 .. 5 x 4, kernels as wide as
            the image from 20 x 17 on; noise for the detections, the reference's white and dark squares as well
  97 x 61   default config: odd sizes at every halving (97 x 61, 48 x 30, 24 x 15, 12 x 7, 6 x 3), 15- and 19-tap kernels against the small
            octaves; the rows of the first octave are not 16-byte aligned, so all of its levels take the two passes
  300 x 70  crosses tile edges of the fused kernel in x with a partial last tile (300 = 4 x 64 + 44); the rows of octave 1 (150) and below are
            not 16-byte aligned: fused and fallback in one call
  304 x 72  the aligned twin (304, 152, 76 fused; 38 x 9 not)
  128 x 64, 128 x 65   a height of exactly one tile, and a tile plus one row"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import sift_ref as sr
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# firstOctave, lastOctave, numScales, sigma0, extractor radius, edgeR, maxFeaturesPerScale
REF_CFG = (-1, 5, 3, 1.6, 1, 10.0, 1000)   # TestSiftDetector.createDetector
S0 = float(np.float32(2.75))
DEFAULT = (0, 5, 3, S0, 2, 10.0, 0)
# name -> (W, H, noise seed, config); the seeds were chosen on the CPU with sift_ref so that the assertions of _check_stats hold
CASES = {
    "80x70-ref": (80, 70, 1, REF_CFG),
    "97x61": (97, 61, 1, DEFAULT),
    "300x70": (300, 70, 2, DEFAULT),
    "304x72": (304, 72, 1, DEFAULT),
    "128x64": (128, 64, 1, DEFAULT),
    "128x65": (128, 65, 1, DEFAULT),
    "first1": (304, 200, 2, (1, 5, 3, 1.6, 2, 10.0, 0)),          # the blur-then-halve loop of initialize
    "scales1": (104, 72, 2, (0, 5, 1, 1.6, 3, 10.0, 0)),
    "scales5": (104, 72, 1, (0, 5, 5, S0, 1, 10.0, 0)),
    "sigma1.6-r3": (104, 72, 1, (0, 5, 3, 1.6, 3, 10.0, 0)),
}
# edgeR = 1: the threshold is (1+1)^2/1 = 4 and Tr^2 >= 4 det for every real xx, yy, xy, so the reference rejects every candidate that reaches
# the edge test; the case has no detections by construction and its precondition is on the rejections instead
EDGE1 = (104, 72, 1, (0, 5, 3, 1.6, 2, 1.0, 0))
SHAPES = ["80x70-ref", "97x61", "300x70", "304x72", "128x64", "128x65"]


def _configs(cfg, maxFeatures=None):
    fo, lo, ns, s0, radius, edgeR, limit = cfg
    return sr.ConfigSS(fo, lo, ns, s0), sr.ConfigDet(radius, 0.0, limit if maxFeatures is None else maxFeatures, edgeR)


def _mirror_configs(cfg, maxFeatures=None):
    """the same as objects of the mirror (sigma0 goes through the SiftScaleSpace constructor: a double)"""
    from boofcv_amd import sift
    from boofcv_amd.api.detect import ConfigExtract
    fo, lo, ns, s0, radius, edgeR, limit = cfg
    ss = sift.ConfigSiftScaleSpace(fo, lo, ns)
    ss.sigma0 = s0
    return ss, sift.ConfigSiftDetector(ConfigExtract(radius, 0.0, 1, True, True, True), limit if maxFeatures is None else maxFeatures, edgeR)


@functools.lru_cache(maxsize=None)
def _image(W, H, seed, u8=False):
    a = orc.noise_image(W, H, seed).array().copy()
    if u8:
        a = np.floor(a * np.float32(2.55)).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _reference(name, u8=False, maxFeatures=None):
    """(scale space, detections, stats) of sift_ref, computed once per case and shared by the tests that need it"""
    W, H, seed, cfg = EDGE1 if name == "edge1" else CASES[name]
    ss, det = _configs(cfg, maxFeatures)
    space = sr.scale_space(ss, _image(W, H, seed, u8))
    stats = {}
    found = sr.detect(ss, det, None, stats, space)
    return space, found, stats


def _check_stats(found, stats):
    """a vacuous input cannot pass: enough detections of both signs, and every test rejects something"""
    xy, scale, white, where = found
    assert len(scale) >= 20 and 0 < int(white.sum()) < len(white), (len(scale), int(white.sum()))
    assert stats["frame"] >= 1 and stats["extremum"] >= 1 and stats["edge"] >= 1, {k: v for k, v in stats.items() if k != "lists"}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _assert_space(got_scale, got_dog, dims, space, what):
    assert [(o[1][0].shape[1], o[1][0].shape[0]) for o in space] == list(dims), what
    for o, (octave, octv, dog) in enumerate(space):
        for i, img in enumerate(octv):
            assert _same(got_scale[o][i], img), "%s: scale image %d of octave %d" % (what, i, octave)
        for i, img in enumerate(dog):
            assert _same(got_dog[o][i], img), "%s: DoG image %d of octave %d" % (what, i, octave)


def _assert_detections(got, found, what, n=None):
    """got: (x, y, scale, white, where) arrays of one frame, already cut to the count"""
    xy, scale, white, where = found
    n = len(scale) if n is None else n
    assert _same(got[0], xy[:n, 0]) and _same(got[1], xy[:n, 1]), what + ": location"
    assert _same(got[2], scale[:n]), what + ": scale"
    assert _same(got[3], white[:n]) and _same(got[4], where[:n]), what + ": white / where"


@pytest.fixture(scope="module")
def lib():
    from boofcv_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _device_run(dev, frames, cfg, cap=4096, maxFeatures=None, space=True):
    ops, torch = dev
    ss, det = _mirror_configs(cfg, maxFeatures)
    t = frames if torch.is_tensor(frames) else torch.from_numpy(np.array(frames)).cuda()
    out = ops.siftDetect(t, ss, det, cap=cap)
    sp = ops.siftScaleSpace(t, ss) if space else None
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in out], sp


def _frame(out, b):
    x, y, scale, white, where, count = out
    n = int(count[b])
    return (x[b, :n], y[b, :n], scale[b, :n], white[b, :n], where[b, :n]), n


@pytest.mark.parametrize("name", list(CASES))
def test_scale_space_and_detections(dev, name):
    ops, torch = dev
    W, H, seed, cfg = CASES[name]
    space, found, stats = _reference(name)
    _check_stats(found, stats)
    ops.ctx.profileReset()
    ops.ctx.profile(True)
    try:
        out, (scale, dog, dims) = _device_run(dev, _image(W, H, seed)[None], cfg)
        launches = ops.ctx.profileReport()
    finally:
        ops.ctx.profile(False)
    ns = cfg[2]
    _assert_space(ops.siftImages(scale[0].cpu().numpy(), dims, ns + 3), ops.siftImages(dog[0].cpu().numpy(), dims, ns + 2), dims, space, name)
    got, n = _frame(out, 0)
    assert n == len(found[1])
    _assert_detections(got, found, name)
    # the path each level took: fused where the geometry allows it, twice (detector and scale space), the two passes elsewhere
    kws = [len(k) for k in sr.kernels(_configs(cfg)[0])[1]]
    fused = sum(1 for w, h in dims if w % 4 == 0 for kw in kws if 3 <= kw <= 27 and kw < w and kw < h)
    assert launches.get("k_sift_level", {"launches": 0})["launches"] == 2 * fused, (launches.get("k_sift_level"), fused)
    assert launches.get("k_sift_subtract", {"launches": 0})["launches"] == 2 * (len(dims) * len(kws) - fused)


def test_edge_r_of_one_rejects_every_candidate(dev):
    W, H, seed, cfg = EDGE1
    _, found, stats = _reference("edge1")
    assert len(found[1]) == 0 and stats["edge"] >= 20 and stats["extremum"] >= 1
    out, _ = _device_run(dev, _image(W, H, seed)[None], cfg, space=False)
    assert int(out[5][0]) == 0


def test_shapes_take_both_paths():
    """what the shapes above were chosen for, from the layout alone"""
    kws = {n: [len(k) for k in sr.kernels(_configs(CASES[n][3])[0])[1]] for n in SHAPES}
    assert kws["97x61"] == [9, 9, 13, 15, 19] and len(sr.kernels(_configs(DEFAULT)[0])[0]) == 15
    lay = {n: [(w, h) for _, w, h in sr.layout(_configs(CASES[n][3])[0], CASES[n][0], CASES[n][1])] for n in SHAPES}
    assert lay["80x70-ref"] == [(160, 140), (80, 70), (40, 35), (20, 17), (10, 8), (5, 4)]
    assert lay["97x61"][-1] == (6, 3) and lay["97x61"][0][0] % 4 and sum(1 for w, h in lay["97x61"][:4] if w % 2 or h % 2) == 3
    assert lay["300x70"][:2] == [(300, 70), (150, 35)] and 300 % 4 == 0 and 300 % 64 and 150 % 4 and lay["304x72"][:3] == [(304, 72), (152, 36), (76, 18)]
    assert lay["128x64"][0][1] == 64 and lay["128x65"][0][1] == 65


def test_reference_squares(dev):
    """TestSiftDetector.process: the white and dark squares of radius 2 and 5, scale space and detections"""
    ops, torch = dev
    ss, det = _configs(REF_CFG)
    frames = []
    for radius in (2, 5):
        for white in (True, False):
            img = np.zeros((70, 80), np.float32) if white else np.full((70, 80), 200, np.float32)
            img[42 - radius:43 + radius, 40 - radius:41 + radius] = 200 if white else 0
            frames.append(img)
    out, (scale, dog, dims) = _device_run(dev, np.stack(frames), REF_CFG)
    for b, img in enumerate(frames):
        space = sr.scale_space(ss, img)
        found = sr.detect(ss, det, None, None, space)
        assert len(found[1]) > 0
        _assert_space(ops.siftImages(scale[b].cpu().numpy(), dims, 6), ops.siftImages(dog[b].cpu().numpy(), dims, 5), dims, space, "square %d" % b)
        _assert_detections(_frame(out, b)[0], found, "square %d" % b)


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_sift as t
from boofcv_amd import sift
from boofcv_amd.api.image import GrayF32
out = {}
for name in t.CASES:
    W, H, seed, cfg = t.CASES[name]
    ss, det = t._mirror_configs(cfg)
    space = sift.SiftScaleSpace(ss.firstOctave, ss.lastOctave, ss.numScales, ss.sigma0)
    img = GrayF32.wrap(t._image(W, H, seed))
    space.initialize(img)
    o = 0
    while True:
        for i in range(ss.numScales + 3):
            out["%%s/s/%%d/%%d" %% (name, o, i)] = space.getImageScale(i).array().copy()
        for i in range(ss.numScales + 2):
            out["%%s/d/%%d/%%d" %% (name, o, i)] = space.getDifferenceOfGaussian(i).array().copy()
        o += 1
        if not space.computeNextOctave():
            break
    d = sift.SiftDetector(space, det.edgeR, sift.NonMaxLimiter(det.extract, det.maxFeaturesPerScale))
    d.process(img)
    for k in ("x", "y", "scale", "white", "where"):
        out["%%s/%%s" %% (name, k)] = getattr(d, k)
    out[name + "/launches"] = np.array([space.ctx.profileReport().get("k_sift_level", {"launches": 0})["launches"]])
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("flag", ["1", "0"], ids=["two-pass", "fused"])
def test_host_forms_with_and_without_the_two_pass_flag(tmp_path, flag):
    """the host mirror in a child process: under BHIP_SIFT_TWO_PASS=1 no level is fused, without it the fused levels run; both equal the
    reference (and so each other) on every case"""
    path = str(tmp_path / "sift.npz")
    env = dict(os.environ, BHIP_SIFT_TWO_PASS=flag)
    code = ("from boofcv_amd.api.core import Context\nContext.default().profile(True)\n" +
            _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    p = subprocess.run([sys.executable, "-c", code, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    got = np.load(path)
    total = 0
    for name in CASES:
        space, found, _ = _reference(name)
        ns = CASES[name][3][2]
        for o, (octave, octv, dog) in enumerate(space):
            for i in range(ns + 3):
                assert _same(got["%s/s/%d/%d" % (name, o, i)], octv[i]), (name, "scale", octave, i)
            for i in range(ns + 2):
                assert _same(got["%s/d/%d/%d" % (name, o, i)], dog[i]), (name, "dog", octave, i)
        assert "%s/s/%d/0" % (name, len(space)) not in got.files
        _assert_detections([got["%s/%s" % (name, k)] for k in ("x", "y", "scale", "white", "where")], found, name)
        total = int(got[name + "/launches"][0])   # the profile accumulates over the cases
    assert (total == 0) if flag == "1" else (total > 0)


def test_batch_of_three_in_strided_views(dev):
    """three different frames as views inside sentinel-filled parents (odd row and image strides, an offset start): every frame equals its own
    reference and nothing outside the views is touched"""
    ops, torch = dev
    W, H, _, cfg = CASES["304x72"]
    frames = [_image(W, H, s) for s in (1, 21, 3)]
    refs = []
    for f in frames:
        ss, det = _configs(cfg)
        space = sr.scale_space(ss, f)
        refs.append((space, sr.detect(ss, det, None, None, space)))
    for dtype, sentinel in ((np.float32, np.float32(-7777.0)),):
        parent = np.full((3, H + 5, W + 7), sentinel, dtype)
        parent[:, 2:2 + H, 3:3 + W] = np.stack(frames)
        t = torch.from_numpy(parent).cuda()
        view = t[:, 2:2 + H, 3:3 + W]
        out, (scale, dog, dims) = _device_run(dev, view, cfg)
        back = t.cpu().numpy()
        assert np.array_equal(back.view(np.uint32), parent.view(np.uint32)), "the input parent was written"
        for b in range(3):
            _assert_space(ops.siftImages(scale[b].cpu().numpy(), dims, 6), ops.siftImages(dog[b].cpu().numpy(), dims, 5), dims, refs[b][0], "frame %d" % b)
            got, n = _frame(out, b)
            assert n == len(refs[b][1][1])
            _assert_detections(got, refs[b][1], "frame %d" % b)
    assert len({len(r[1][1]) for r in refs}) == 3   # three different lists


def test_outputs_outside_the_records_are_not_written(dev):
    """cap smaller than the count: the count is reported in full, the first cap records are right, nothing beyond them is written; and the
    padding floats of the scale-space planes are left alone"""
    ops, torch = dev
    W, H, seed, cfg = CASES["97x61"]
    _, found, _ = _reference("97x61")
    n = len(found[1])
    cap = n - 7
    assert cap > 0
    ss, det = _mirror_configs(cfg)
    from boofcv_amd import sift
    c = sift._cfg(ss, det)
    src = torch.from_numpy(_image(W, H, seed).copy()).cuda()
    extra = 16
    x, y, scale = (torch.full((cap + extra,), -5.0, dtype=torch.float64, device="cuda") for _ in range(3))
    white = torch.full((cap + extra,), 77, dtype=torch.uint8, device="cuda")
    where = torch.full((cap + extra, 4), -3, dtype=torch.int16, device="cuda")
    count = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    p = lambda v: C.c_void_p(v.data_ptr())
    assert ops.L.bhip_sift_detect_dev_f32(ops.ctx._h, C.byref(c), p(src), W * H, W, W, H, 1, p(x), p(y), p(scale), p(white), p(where), p(count[1:]), cap) == 0
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [-9, n, -9]
    _assert_detections([v.cpu().numpy()[:cap] for v in (x, y, scale, white, where)], found, "cap", cap)
    assert (x[cap:] == -5).all() and (y[cap:] == -5).all() and (scale[cap:] == -5).all() and (white[cap:] == 77).all() and (where[cap:] == -3).all()
    # cap 0: only the count
    assert ops.L.bhip_sift_detect_dev_f32(ops.ctx._h, C.byref(c), p(src), W * H, W, W, H, 1, None, None, None, None, None, p(count[1:]), 0) == 0
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [-9, n, -9]
    # scale-space padding: 97 * 61 = 5917 pixels in a plane of 5920 floats
    dims, sf, df = ops.siftLayout(W, H, ss)
    sbuf = torch.full((sf + 8,), 123.0, dtype=torch.float32, device="cuda")
    dbuf = torch.full((df + 8,), 123.0, dtype=torch.float32, device="cuda")
    assert ops.L.bhip_sift_scale_space_dev_f32(ops.ctx._h, C.byref(c), p(src), W * H, W, W, H, 1, p(sbuf), p(dbuf)) == 0
    torch.cuda.synchronize()
    s = sbuf.cpu().numpy()
    assert (s[sf:] == 123).all() and (dbuf.cpu().numpy()[df:] == 123).all() and (s[5917:5920] == 123).all()
    assert _same(s[:5917].reshape(H, W), _reference("97x61")[0][0][1][0])


@pytest.mark.parametrize("name", ["97x61", "304x72"])
def test_uint8_frames_equal_float_frames_of_the_same_values(dev, name):
    ops, torch = dev
    W, H, seed, cfg = CASES[name]
    img = _image(W, H, seed, True)
    space, found, stats = _reference(name, True)
    _check_stats(found, stats)
    out8, (scale8, dog8, dims) = _device_run(dev, img[None], cfg)
    outf, (scalef, dogf, _) = _device_run(dev, img.astype(np.float32)[None], cfg)
    assert torch.equal(scale8.view(torch.int32), scalef.view(torch.int32)) and torch.equal(dog8.view(torch.int32), dogf.view(torch.int32))
    _assert_space(ops.siftImages(scale8[0].cpu().numpy(), dims, 6), ops.siftImages(dog8[0].cpu().numpy(), dims, 5), dims, space, name)
    for out in (out8, outf):
        got, n = _frame(out, 0)
        assert n == len(found[1])
        _assert_detections(got, found, name)


def test_max_features_per_scale(dev):
    """NonMaxLimiter's cut.  Precondition, on the reference's lists: at every scale that is cut, no two |value| around the cut are equal, so the
    kept set does not depend on how QuickSelect breaks ties; then the kept records and their order under the restated routine are compared"""
    W, H, seed, cfg = CASES["304x72"]
    limit = 40
    _, found, stats = _reference("304x72", False, limit)
    _, uncut, _ = _reference("304x72")
    cut = 0
    for full in stats["lists"]:
        if len(full) > limit:
            cut += 1
            v = np.sort(np.array([e[0] for e in full], np.float32))[::-1]
            assert v[limit - 1] > v[limit], "equal |value| across the cut"
    assert cut >= 2 and 20 <= len(found[1]) < len(uncut[1])
    out, _ = _device_run(dev, _image(W, H, seed)[None], cfg, maxFeatures=limit, space=False)
    got, n = _frame(out, 0)
    assert n == len(found[1])
    _assert_detections(got, found, "maxFeaturesPerScale")


def test_refusals(dev, lib):
    ops, torch = dev
    from boofcv_amd import sift
    from boofcv_amd.api.detect import ConfigExtract
    from boofcv_amd.api.image import GrayF32, GrayS16, PlanarType, InterleavedType
    IAE = sift.IllegalArgumentException
    W, H = 40, 30
    src = torch.zeros((1, H, W), dtype=torch.float32, device="cuda")
    keep = torch.full((4, 8), -1.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    p = lambda v: C.c_void_p(v.data_ptr())

    def detect(c, w=W, h=H, batch=1, stride=W, cap=8):
        wh = torch.zeros((8, 4), dtype=torch.int16, device="cuda")
        return ops.L.bhip_sift_detect_dev_f32(ops.ctx._h, C.byref(c), p(src), w * h, stride, w, h, batch, p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), p(wh), p(cnt), cap)

    def cfg(**kw):
        c = lib.SiftCfg()
        assert lib.load().bhip_sift_cfg_default(C.byref(c)) == 0
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    d = cfg()
    assert (d.firstOctave, d.lastOctave, d.numScales, d.sigma0) == (0, 5, 3, float(np.float32(2.75)))
    assert (d.extractRadius, d.extractThreshold, d.extractIgnoreBorder, d.extractUseStrictRule, d.extractDetectMin, d.extractDetectMax) == (2, 0.0, 1, 1, 1, 1)
    assert (d.maxFeaturesPerScale, d.edgeR) == (0, 10.0)
    INV, UNS = lib.BHIP_ERR_INVALID, lib.BHIP_ERR_UNSUPPORTED
    for bad in (dict(lastOctave=0), dict(firstOctave=2, lastOctave=1), dict(numScales=0), dict(edgeR=0.5), dict(extractIgnoreBorder=0), dict(extractIgnoreBorder=2),
                dict(extractDetectMin=0), dict(extractDetectMax=0), dict(extractRadius=0), dict(sigma0=0.0)):
        assert detect(cfg(**bad)) == INV, bad
    assert detect(cfg(), w=0) == INV and detect(cfg(), h=0) == INV and detect(cfg(), batch=0) == INV and detect(cfg(), stride=W - 1) == INV
    assert detect(cfg(), cap=-1) == INV
    assert detect(cfg(firstOctave=6, lastOctave=7)) == INV             # 40 x 30 halved six times: an octave of no pixels
    assert detect(cfg(extractUseStrictRule=0)) == UNS
    assert detect(cfg(sigma0=60.0)) == UNS                             # a 301-tap kernel
    assert detect(cfg(firstOctave=-1), w=16384, h=2) == UNS            # the first octave is 32768 wide
    assert detect(cfg(), w=32768, h=2, stride=32768) == UNS
    assert detect(cfg(), batch=65536) == UNS
    assert lib.load().bhip_sift_layout(C.byref(cfg(numScales=0)), W, H, None, 0, None, None) == INV
    assert lib.load().bhip_sift_layout(C.byref(cfg(edgeR=0.0)), W, H, None, 0, None, None) == 4   # the scale space does not read the detector's fields
    torch.cuda.synchronize()
    assert (keep == -1).all() and cnt.item() == -9                     # a refused call writes nothing
    # the mirror: the reference's exceptions
    with pytest.raises(IAE):
        sift.SiftScaleSpace(0, 0, 3, 1.6)
    with pytest.raises(IAE):
        sift.SiftScaleSpace(0, 5, 0, 1.6)
    space = sift.SiftScaleSpace(0, 5, 3, 1.6)
    ok = ConfigExtract(2, 0.0, 1, True, True, True)
    with pytest.raises(IAE):
        sift.SiftDetector(space, 0.5, sift.NonMaxLimiter(ok, 0))
    with pytest.raises(IAE):
        sift.SiftDetector(space, 10, sift.NonMaxLimiter(ConfigExtract(2, 0.0, 1, True, False, True), 0))
    with pytest.raises(RuntimeError):
        sift.SiftDetector(space, 10, sift.NonMaxLimiter(ConfigExtract(2, 0.0, 0, True, True, True), 0))
    with pytest.raises(RuntimeError):
        sift.SiftDetector(space, 10, sift.NonMaxLimiter(ConfigExtract(2, 0.0, 1, False, True, True), 0))
    for t in (GrayS16, PlanarType(3, GrayF32), InterleavedType(3)):
        with pytest.raises(RuntimeError):
            sift.FactoryInterestPointSift.sift(None, None, t)
    det = sift.FactoryInterestPointSift.sift(None, None, GrayF32)
    with pytest.raises(IAE):
        det.detect(sift.GrayU8(8, 8))


def test_factory_mirror(dev):
    """FactoryInterestPointSift.sift(null, null, type): the InterestPointDetector of WrapSiftDetector on GrayF32 and GrayU8"""
    from boofcv_amd import sift
    W, H, seed, cfg = CASES["97x61"]
    for u8 in (False, True):
        _, found, _ = _reference("97x61", u8)
        t = sift.GrayU8 if u8 else sift.GrayF32
        det = sift.FactoryInterestPointSift.sift(None, None, t)
        det.detect(t.wrap(_image(W, H, seed, u8)))
        n = det.getNumberOfFeatures()
        assert n == len(found[1]) and det.hasScale() and not det.hasOrientation() and det.getOrientation(0) == 0
        xy = np.array([(det.getLocation(i).x, det.getLocation(i).y) for i in range(n)])
        assert _same(xy, found[0]) and _same(np.array([det.getRadius(i) for i in range(n)]), found[1])
        pts = det.detector.getDetections()
        assert [p.white for p in pts] == [bool(w) for w in found[2]] and _same(det.detector.where, found[3])
