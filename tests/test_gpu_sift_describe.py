"""GPU: SIFT orientation and description (FactoryDetectDescribe.sift: CompleteSift, OrientationHistogramSift, DescribePointSift) against
tests/sift_describe_ref.py, through the device-batched call (DeviceImageOps.siftDetectDescribe), the host mirror (boofcv_amd/sift.py) and the
C ABI (bhip_csift_*).

Exact, as bit patterns where float: the feature count of every frame, the number of angles of every detection (hence which detection a feature
belongs to), x, y, scale, white and the order of features.  Every angle is within 1e-12 rad of the reference's (UtilAngle.dist: the bound the
project holds SURF orientations to) and every descriptor element within 1e-12 absolute: the only difference allowed is the last ulp of atan2 /
sin / cos between the C library and the device library.  An atan2 error of a few ulp of pi is about 1e-15 rad; it moves a histogram weight by
about 1e-15 / histogramBinWidth and an element of the unit-normalised descriptor by less than 1e-13; clipping and both normalisations are
continuous.

Preconditions, asserted on the reference alone before anything is compared (a failing one means the input is wrong):
  * no generic orientation sample (both gradient components non-zero, |dx| != |dy|) has theta / histAngleBin within 1e-9 of an integer, no
    descriptor sample has a pixel coordinate within 1e-9 of an integer, no peak other than the largest is within 1e-9 (relative) of the 0.8
    threshold.  The device's atan2 / sin / cos error moves a quotient by less than 1e-14 and a coordinate by less than 1e-12.
  * at least 20 features, detections with one and with two or more angles, descriptor samples inside and outside the image.
  * axis samples (dx == 0 or dy == 0: theta exactly on a bin edge) are asserted where they exist: on the two axis-aligned images every
    sample away from the squares is one (1870 of 6362 and 3432 of 8413 orientation samples).  The noise images have none under the
    reference's gradient (BorderType.EXTENDED: the frame of derivX / derivY is (a - b) / 2 of clamped reads, never 0); a gradient whose
    frame is left at zero would put 1.4 % of the samples on an axis, but that is not GradientThree's.  The count is printed for every case.
Every feature of every case is compared; none is left out.

Cases (seed 1; chosen on the CPU with the restatement so that the preconditions hold):
  304x72, 97x61, 128x65   default configs; 91 / 26 / 38 detections, 122 / 33 / 44 features; r up to 12
  80x70-ref               the reference test's detector config (-1, 5, 3, 1.6, radius 1, limit 1000): 535 detections, up to 6 angles a
                          detection (more than the BHIP_CSIFT_ANGLE_SLOTS kept beside a detection: the second orientation launch)
  large-r                 sigmaEnlarge = 5 on 128x65: r up to 28, windows of up to 57 x 57 samples = 13 chunks of 256 (sigma0 = 6 on this
                          image leaves 6 detections, too few for the assertions below)
  paper                   ConfigCompleteSift.createPaper (sigmaEnlarge 1.5, firstOctave -1) on 80x70
  grid-3-2-4              widthSubregion 3, widthGrid 2, numHistogramBins 4, sigmaToPixels 1.5: the generic describe kernel, dof 16
  ramp-y, ramp-x          rows (columns) constant: 80 x 70, value 2 * y (2 * x), plus the white and the dark square (radius 5 and 2) of
                          TestSiftDetector at (40, 42), (20, 20), (60, 25) and (25, 50): every gradient away from the squares is axis-aligned"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import assoc_ref as ar
import sift_describe_ref as dr
import sift_ref as sr
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S0 = float(np.float32(2.75))
S16 = float(np.float32(1.6))
DEFAULT = (0, 5, 3, S0, 2, 10.0, 0)           # firstOctave, lastOctave, numScales, sigma0, extractor radius, edgeR, maxFeaturesPerScale
REF_CFG = (-1, 5, 3, 1.6, 1, 10.0, 1000)      # TestSiftDetector.createDetector
ORI, ORI_PAPER = (36, 2.0), (36, 1.5)
DESC = (4, 4, 8, 1.0, 0.5, 0.2)
# name -> (W, H, image kind, seed, detector config, orientation config, describe config)
CASES = {
    "304x72": (304, 72, "noise", 1, DEFAULT, ORI, DESC),
    "97x61": (97, 61, "noise", 1, DEFAULT, ORI, DESC),
    "128x65": (128, 65, "noise", 1, DEFAULT, ORI, DESC),
    "80x70-ref": (80, 70, "noise", 1, REF_CFG, ORI, DESC),
    "large-r": (128, 65, "noise", 1, DEFAULT, (36, 5.0), DESC),
    "paper": (80, 70, "noise", 1, (-1, 5, 3, S16, 1, 10.0, 0), ORI_PAPER, DESC),
    "grid-3-2-4": (304, 72, "noise", 1, DEFAULT, ORI, (3, 2, 4, 1.5, 0.5, 0.2)),
    "ramp-y": (80, 70, "ramp-y", 0, REF_CFG, ORI, DESC),
    "ramp-x": (80, 70, "ramp-x", 0, REF_CFG, ORI, DESC),
    "u8": (304, 72, "noise-u8", 1, DEFAULT, ORI, DESC),
    "304x72-s21": (304, 72, "noise", 21, DEFAULT, ORI, DESC),
    "304x72-s3": (304, 72, "noise", 3, DEFAULT, ORI, DESC),
}
AXIS = ("ramp-y", "ramp-x")
ANGLE_TOL = 1e-12
DESC_TOL = 1e-12
MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def _image(W, H, kind, seed):
    if kind.startswith("noise"):
        a = orc.noise_image(W, H, seed).array().copy()
        if kind == "noise-u8":
            a = np.floor(a * np.float32(2.55)).astype(np.uint8)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        a = (2.0 * (yy if kind == "ramp-y" else xx)).astype(np.float32)
        for (cx, cy, radius, value) in ((40, 42, 5, 200.0), (20, 20, 2, 200.0), (60, 25, 5, 0.0), (25, 50, 2, 0.0)):
            a[cy - radius:cy + radius + 1, cx - radius:cx + radius + 1] = value
    a.setflags(write=False)
    return a


def _ref_configs(name):
    W, H, kind, seed, cfg, ori, desc = CASES[name]
    fo, lo, ns, s0, radius, edgeR, limit = cfg
    return sr.ConfigSS(fo, lo, ns, s0), sr.ConfigDet(radius, 0.0, limit, edgeR), dr.Orientation(*ori), dr.Describe(*desc)


def _mirror_config(name):
    from boofcv_amd import sift
    from boofcv_amd.api.detect import ConfigExtract
    W, H, kind, seed, cfg, ori, desc = CASES[name]
    fo, lo, ns, s0, radius, edgeR, limit = cfg
    c = sift.ConfigCompleteSift()
    c.scaleSpace = sift.ConfigSiftScaleSpace(fo, lo, ns)
    c.scaleSpace.sigma0 = s0
    c.detector = sift.ConfigSiftDetector(ConfigExtract(radius, 0.0, 1, True, True, True), limit, edgeR)
    c.orientation, c.describe = sift.ConfigSiftOrientation(*ori), sift.ConfigSiftDescribe(*desc)
    return c


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(features, stats) of sift_describe_ref, computed once per case and shared by the tests that need it"""
    W, H, kind, seed = CASES[name][:4]
    ss, det, ori, desc = _ref_configs(name)
    stats = dr.new_stats()
    res = dr.complete(ss, det, ori, desc, _image(W, H, kind, seed), stats)
    for v in res.values():
        v.setflags(write=False)
    return res, stats


def _check_preconditions(name):
    res, st = _reference(name)
    print("%s: %d detections, %d features, angles per detection %s, largest r %d, bin margin %.3g, pixel margin %.3g, threshold margin %.3g, axis samples %d of %d, "
          "descriptor samples inside %d outside %d in (-1, 0) %d" % (name, st["detections"], st["features"], dict(sorted(st["anglesPerDetection"].items())), st["maxR"],
                                                                       st["binMargin"], st["pixelMargin"], st["thresholdMargin"], st["axisSamples"], st["oriSamples"],
                                                                       st["inside"], st["outside"], st["negativeCoordinate"]))
    assert st["binMargin"] > MARGIN and st["pixelMargin"] > MARGIN and st["thresholdMargin"] > MARGIN, st
    per = st["anglesPerDetection"]
    assert st["features"] >= 20 and per.get(1, 0) >= 1 and sum(v for k, v in per.items() if k >= 2) >= 1, st
    assert st["inside"] >= 1 and st["outside"] >= 1, st
    if name in AXIS:
        assert st["axisSamples"] >= 1000 and st["axisSamples"] >= 0.2 * st["oriSamples"], st   # (the rest are the samples around the squares)
    return res, st


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _groups(x, y, scale, white):
    """run lengths of consecutive records that carry the same ScalePoint: the angles of one detection"""
    n = len(x)
    if n == 0:
        return []
    new = np.ones(n, bool)
    new[1:] = (_bits(x)[1:] != _bits(x)[:-1]) | (_bits(y)[1:] != _bits(y)[:-1]) | (_bits(scale)[1:] != _bits(scale)[:-1]) | (white[1:] != white[:-1])
    starts = np.nonzero(new)[0]
    return np.diff(np.append(starts, n)).tolist()


def _assert_features(got, res, what, n=None):
    """got: (x, y, scale, orientation, white, desc) of one frame cut to the count.  n: only the first n records of the reference"""
    x, y, scale, ori, white, desc = got
    n = len(res["x"]) if n is None else n
    assert len(x) == n, (what, len(x), n)
    assert _same(x, res["x"][:n]) and _same(y, res["y"][:n]), what + ": location"
    assert _same(scale, res["scale"][:n]) and _same(white, res["white"][:n]), what + ": scale / white"
    if n == len(res["x"]):
        assert _groups(x, y, scale, white) == [int(k) for k in res["anglesPerDetection"] if k > 0], what + ": angles per detection"
    ea = float(dr.angle_dist(ori, res["orientation"][:n]).max()) if n else 0.0
    ed = float(np.abs(desc - res["desc"][:n]).max()) if n else 0.0
    print("%s: %d features, max angle error %.3g rad, max descriptor element error %.3g" % (what, n, ea, ed))
    assert desc.shape == res["desc"][:n].shape and np.isfinite(desc).all()
    assert ea <= ANGLE_TOL, (what, ea)
    assert ed <= DESC_TOL, (what, ed)


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _device_run(dev, frames, name, cap=2048):
    ops, torch = dev
    t = frames if torch.is_tensor(frames) else torch.from_numpy(np.array(frames)).cuda()
    out = ops.siftDetectDescribe(t, _mirror_config(name), cap=cap)
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in out]


def _frame(out, b):
    x, y, scale, ori, white, desc, count = out
    n = int(count[b])
    return (x[b, :n], y[b, :n], scale[b, :n], ori[b, :n], white[b, :n], desc[b, :n]), n


@pytest.mark.parametrize("name", ["304x72", "97x61", "128x65", "80x70-ref", "large-r", "paper", "grid-3-2-4", "ramp-y", "ramp-x", "u8"])
def test_features_equal_the_reference(dev, name):
    ops, torch = dev
    W, H, kind, seed = CASES[name][:4]
    res, st = _check_preconditions(name)
    if name == "large-r":
        assert st["maxR"] > 16        # windows of more than four chunks in each direction
    if name == "80x70-ref":
        from boofcv_amd import _lib
        assert max(st["anglesPerDetection"]) > _lib.BHIP_CSIFT_ANGLE_SLOTS
    ops.ctx.profileReset()
    ops.ctx.profile(True)
    try:
        out = _device_run(dev, _image(W, H, kind, seed)[None], name)
        launches = ops.ctx.profileReport()
    finally:
        ops.ctx.profile(False)
    got, n = _frame(out, 0)
    _assert_features(got, res, name)
    generic = name == "grid-3-2-4"
    assert launches.get("k_sift_describe_generic" if generic else "k_sift_describe", {"launches": 0})["launches"] > 0
    assert ("k_sift_describe" if generic else "k_sift_describe_generic") not in launches
    assert launches["k_sift_orient"]["launches"] == launches["k_sift_angle_scan"]["launches"] > 0
    if name == "grid-3-2-4":
        assert got[5].shape[1] == 16


def test_batch_of_three_frames(dev):
    """three different frames in one call: per-frame offsets and counts"""
    names = ["304x72", "304x72-s21", "304x72-s3"]
    refs = [_check_preconditions(n)[0] for n in names]
    assert len({len(r["x"]) for r in refs}) == 3
    out = _device_run(dev, np.stack([_image(*CASES[n][:4]) for n in names]), names[0])
    for b, n in enumerate(names):
        got, cnt = _frame(out, b)
        assert cnt == len(refs[b]["x"])
        _assert_features(got, refs[b], "frame %d" % b)


def test_small_cap_counts_everything_and_writes_only_its_records(dev):
    """cap = 5: the count is the full number, the first 5 records are right, the memory behind them keeps its guard value; the host mirror
    grows and returns everything"""
    ops, torch = dev
    from boofcv_amd import sift
    name = "97x61"
    W, H, kind, seed = CASES[name][:4]
    res, _ = _check_preconditions(name)
    n, cap, extra, dof = len(res["x"]), 5, 16, 128
    assert n > 4 * cap
    cfg = _mirror_config(name)
    c, dc = sift._cfg(cfg.scaleSpace, cfg.detector), sift._desc_cfg(cfg.orientation, cfg.describe)
    src = torch.from_numpy(_image(W, H, kind, seed).copy()).cuda()
    x, y, scale, ori = (torch.full((cap + extra,), -5.0, dtype=torch.float64, device="cuda") for _ in range(4))
    white = torch.full((cap + extra,), 77, dtype=torch.uint8, device="cuda")
    desc = torch.full((cap + extra, dof), -5.0, dtype=torch.float64, device="cuda")
    count = torch.full((3,), -9, dtype=torch.int32, device="cuda")
    p = lambda v: C.c_void_p(v.data_ptr())
    assert ops.L.bhip_csift_dev_f32(ops.ctx._h, C.byref(c), C.byref(dc), p(src), W * H, W, W, H, 1, p(x), p(y), p(scale), p(ori), p(white), p(desc), p(count[1:]), cap) == 0
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [-9, n, -9]
    _assert_features([v.cpu().numpy()[:cap] for v in (x, y, scale, ori, white, desc)], res, "cap 5", cap)
    assert (x[cap:] == -5).all() and (y[cap:] == -5).all() and (scale[cap:] == -5).all() and (ori[cap:] == -5).all() and (white[cap:] == 77).all() and (desc[cap:] == -5).all()
    # cap 0: only the count
    assert ops.L.bhip_csift_dev_f32(ops.ctx._h, C.byref(c), C.byref(dc), p(src), W * H, W, W, H, 1, None, None, None, None, None, None, p(count[1:]), 0) == 0
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [-9, n, -9]
    # the mirror starts from a list of 5 and grows
    dd = sift.FactoryDetectDescribeSift.sift(cfg, sift.GrayF32)
    dd.alg._cap = cap
    dd.detect(sift.GrayF32.wrap(_image(W, H, kind, seed)))
    assert dd.getNumberOfFeatures() == n and dd.alg._cap == n
    _assert_features((dd.alg.x, dd.alg.y, dd.alg.scale, dd.alg.orientation, dd.alg.white, dd.alg.descriptors), res, "mirror regrown")


def test_two_calls_give_the_same_bits(dev):
    name = "80x70-ref"
    a = _device_run(dev, _image(*CASES[name][:4])[None], name)
    b = _device_run(dev, _image(*CASES[name][:4])[None], name)
    n = int(a[6][0])
    assert n == int(b[6][0]) == len(_reference(name)[0]["x"])
    for u, v in zip(a[:6], b[:6]):
        assert _same(u[0, :n], v[0, :n])


def test_host_form_and_mirror_equal_the_device_call(dev):
    """bhip_csift_f32 / _u8 through the mirror's factory: the same bits as the device-batched call, and the methods of DetectDescribe_CompleteSift"""
    from boofcv_amd import sift
    for name in ("128x65", "u8"):
        W, H, kind, seed = CASES[name][:4]
        res, _ = _check_preconditions(name)
        img = _image(W, H, kind, seed)
        got, n = _frame(_device_run(dev, img[None], name), 0)
        t = sift.GrayU8 if img.dtype == np.uint8 else sift.GrayF32
        dd = sift.FactoryDetectDescribeSift.sift(_mirror_config(name), t)
        dd.detect(t.wrap(img))
        alg = dd.alg
        assert dd.getNumberOfFeatures() == n and dd.hasScale() and dd.hasOrientation() and dd.getDescriptionType() is sift.BrightFeature
        for u, v in zip(got, (alg.x, alg.y, alg.scale, alg.orientation, alg.white, alg.descriptors)):
            assert _same(u, v), name
        _assert_features((alg.x, alg.y, alg.scale, alg.orientation, alg.white, alg.descriptors), res, name + " mirror")
        assert alg.getDescriptorLength() == 128 and dd.createDescription().size() == 128
        k = n // 2
        assert dd.getRadius(k) == alg.scale[k] and dd.getOrientation(k) == alg.orientation[k] and dd.getLocation(k).x == alg.x[k]
        f = dd.getDescription(k)
        assert f.white == bool(alg.white[k]) and _same(f.value, alg.descriptors[k])
        assert len(alg.getLocations()) == len(alg.getDescriptions()) == len(alg.getOrientations()) == n


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_sift_describe as t
from boofcv_amd import sift
from boofcv_amd.api.core import Context
Context.default().profile(True)
out = {}
for name in ("304x72", "80x70-ref"):
    W, H, kind, seed = t.CASES[name][:4]
    dd = sift.FactoryDetectDescribeSift.sift(t._mirror_config(name), sift.GrayF32)
    dd.detect(sift.GrayF32.wrap(t._image(W, H, kind, seed)))
    for k in ("x", "y", "scale", "orientation", "white", "descriptors"):
        out[name + "/" + k] = getattr(dd.alg, k)
rep = Context.default().profileReport()
out["generic"] = np.array([rep.get("k_sift_describe_generic", {"launches": 0})["launches"], rep.get("k_sift_describe", {"launches": 0})["launches"]])
np.savez(sys.argv[1], **out)
"""


def test_generic_describe_kernel_gives_the_same_bits(dev, tmp_path):
    """BHIP_SIFT_DESCRIBE_GENERIC=1 in a child process: the default grid through the kernel that takes any grid, bit for bit what the
    specialised kernel gives in this process"""
    path = str(tmp_path / "generic.npz")
    env = dict(os.environ, BHIP_SIFT_DESCRIBE_GENERIC="1")
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    p = subprocess.run([sys.executable, "-c", code, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    got = np.load(path)
    assert got["generic"][0] > 0 and got["generic"][1] == 0
    for name in ("304x72", "80x70-ref"):
        here, n = _frame(_device_run(dev, _image(*CASES[name][:4])[None], name), 0)
        assert n == len(_reference(name)[0]["x"])
        for u, k in zip(here, ("x", "y", "scale", "orientation", "white", "descriptors")):
            assert _same(u, got[name + "/" + k]), (name, k)


def test_descriptors_feed_the_device_l2_association(dev):
    """two frames' descriptors straight from siftDetectDescribe into bhip_assoc_l2_dev: pairs and fit equal assoc_ref.greedy on the same
    descriptors (the layout is the one the association reads)"""
    ops, torch = dev
    names = ["304x72", "304x72-s21"]
    frames = torch.from_numpy(np.stack([_image(*CASES[n][:4]) for n in names])).cuda()
    x, y, scale, ori, white, desc, count = ops.siftDetectDescribe(frames, _mirror_config(names[0]), cap=512)
    torch.cuda.synchronize()
    ns, nd = (int(v) for v in count.cpu().tolist())
    assert ns == len(_reference(names[0])[0]["x"]) and nd == len(_reference(names[1])[0]["x"]) and min(ns, nd) >= 20
    pairs = torch.full((ns,), -7, dtype=torch.int32, device="cuda")
    fit = torch.zeros(ns, dtype=torch.float64, device="cuda")
    p = lambda v: C.c_void_p(v.data_ptr())
    MAXV = ar.MAX_VALUE
    assert ops.L.bhip_assoc_l2_dev(ops.ctx._h, p(desc[0]), ns, p(desc[1]), nd, 128, MAXV, 1, 0, p(pairs), p(fit)) == 0
    torch.cuda.synchronize()
    a, b = desc[0, :ns].cpu().numpy(), desc[1, :nd].cpu().numpy()
    W = np.zeros((ns, nd))
    for k in range(128):               # DescriptorDistance.euclideanSq: the sum in index order
        d = a[:, k, None] - b[None, :, k]
        W += d * d
    rp, rf = ar.greedy(W, MAXV, True)
    assert (rp >= 0).sum() >= 5
    assert np.array_equal(pairs.cpu().numpy(), rp) and _same(fit.cpu().numpy(), rf)


def test_refusals_on_the_device(dev):
    """the describe config's refusals through the device call: nothing is written"""
    ops, torch = dev
    from boofcv_amd import _lib, sift
    W, H = 40, 30
    src = torch.zeros((1, H, W), dtype=torch.float32, device="cuda")
    keep = torch.full((5, 8), -1.0, dtype=torch.float64, device="cuda")
    desc = torch.full((8, 128), -1.0, dtype=torch.float64, device="cuda")
    white = torch.full((8,), 7, dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    p = lambda v: C.c_void_p(v.data_ptr())

    def run(cap=8, **kw):
        c, dc = sift._cfg(None, None), sift._desc_cfg()
        for k, v in kw.items():
            setattr(dc if hasattr(dc, k) else c, k, v)
        return ops.L.bhip_csift_dev_f32(ops.ctx._h, C.byref(c), C.byref(dc), p(src), W * H, W, W, H, 1, p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), p(white), p(desc), p(cnt), cap)
    INV, UNS = _lib.BHIP_ERR_INVALID, _lib.BHIP_ERR_UNSUPPORTED
    for bad in (dict(histogramSize=2), dict(sigmaEnlarge=0.0), dict(widthSubregion=0), dict(widthGrid=0), dict(numHistogramBins=0), dict(sigmaToPixels=0.0),
                dict(weightingSigmaFraction=-1.0), dict(maxDescriptorElementValue=0.0), dict(widthSubregion=3, widthGrid=3), dict(cap=-1), dict(edgeR=0.5), dict(numScales=0)):
        assert run(**bad) == INV, bad
    for bad in (dict(histogramSize=257), dict(widthSubregion=7, widthGrid=8), dict(widthSubregion=2, widthGrid=24, numHistogramBins=4), dict(extractUseStrictRule=0)):
        assert run(**bad) == UNS, bad
    torch.cuda.synchronize()
    assert (keep == -1).all() and (desc == -1).all() and (white == 7).all() and cnt.item() == -9
    assert run() == 0
    torch.cuda.synchronize()
    assert cnt.item() == 0     # a flat image has no features
