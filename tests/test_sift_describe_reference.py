"""CPU: tests/sift_describe_ref.py, the restatement of CompleteSift's orientation and description, against what the reference's own tests pin
(TestOrientationHistogramSift, TestDescribeSiftCommon, TestDescribePointSift, TestCompleteSift, with their tolerances); the two host-built
weight tables of the library against the restatement, bit for bit; the describe config's defaults and refusals through the host-only
exports; and the classes and factory arguments of the Python mirror.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import sift_describe_ref as dr
import sift_ref as sr
from oracle import pyoracle as orc

f32 = np.float32


def _fill(w, h, v):
    return np.full((h, w), f32(v), f32)


# ---------------- TestOrientationHistogramSift ----------------
def test_orientation_process_easy():
    theta0, theta1 = 0.5, -1.2
    dX, dY = _fill(50, 60, f32(math.cos(theta0)) * f32(1.5)), _fill(50, 60, f32(math.sin(theta0)) * f32(1.5))
    dX[0:60, 20:50], dY[0:60, 20:50] = f32(math.cos(theta1)), f32(math.sin(theta1))   # fillRectangle(x0 20, y0 0, width 30, height 60)
    alg = dr.Orientation(36, 1.5)
    angles = alg.process(dX, dY, 20, 25, 4)
    assert len(angles) == 2
    assert abs(alg.peakAngle - theta0) <= 1e-5 and abs(angles[0] - theta0) <= 1e-5
    assert dr.angle_dist(theta1, angles[1]) <= 1e-5


def test_orientation_compute_histogram():
    N = 36
    alg = dr.Orientation(N, 1.5)
    for degrees in range(5, 360, 10):
        theta = math.radians(degrees)
        dX, dY = _fill(50, 60, math.cos(theta)), _fill(50, 60, math.sin(theta))
        for cx, cy in ((20, 15), (0, 0)):
            alg.compute_histogram(dX, dY, cx, cy, 3)
            for i in range(N):
                if i == degrees * N // 360:
                    assert dr.angle_dist(theta, math.atan2(alg.hy[i], alg.hx[i])) <= 1e-5 and alg.mag[i] > 0
                else:
                    assert abs(alg.hx[i]) <= 1e-5 and abs(alg.hy[i]) <= 1e-5 and abs(alg.mag[i]) <= 1e-5


def test_orientation_find_histogram_peaks():
    alg = dr.Orientation(36, 1.5)
    N = alg.N
    expected = [dr.bound(2.0 * i * math.pi / N) for i in range(N)]
    alg.mag = np.ones(N)
    alg.hx, alg.hy = np.cos(expected), np.sin(expected)
    alg.mag[5] = 5.0
    alg.mag[15], alg.mag[16], alg.mag[17] = 4.4, 4.5, 4.4
    alg.mag[20] = alg.mag[21] = 6
    alg.find_histogram_peaks()
    assert len(alg.angles) == 2
    assert abs(alg.peakAngle - expected[5]) <= 1e-8 and abs(alg.angles[0] - expected[5]) <= 1e-8 and abs(alg.angles[1] - expected[16]) <= 1e-8


def test_orientation_compute_and_interpolate_angle():
    t0, t1, t2 = 0.5, 0.7, 0.8
    alg = dr.Orientation(36, 1.5)
    N = alg.N
    i, j = N - 2, N - 1
    for k in range(N):
        for idx, t in ((i, t0), (j, t1), (k, t2)):
            alg.hx[idx], alg.hy[idx] = math.cos(t), math.sin(t)
        alg.mag[i], alg.mag[j], alg.mag[k] = 1.5, 3.1, 1.5
        assert abs(alg.compute_angle(j) - t1) <= 1e-8
        alg.mag[i] = 2.0
        assert alg.compute_angle(j) < t1
        alg.mag[i], alg.mag[k] = 1.5, 2.0
        assert alg.compute_angle(j) > t1
        i, j = j, k
    alg = dr.Orientation(36, 1.5)
    for idx, t in ((2, t0), (3, t1), (4, t2)):
        alg.hx[idx], alg.hy[idx] = math.cos(t), math.sin(t)
    for offset, want in ((-1, t0), (0, t1), (1, t2), (-0.5, 0.6), (0.5, 0.75)):
        assert abs(alg.interpolate_angle(2, 3, 4, offset) - want) <= 1e-6


def test_orientation_compute_weight():
    alg = dr.Orientation(36, 1.5)
    rng = np.random.default_rng(234324)
    d = (rng.random((50, 2)) - 0.5) * 3
    found = alg.compute_weight(d[:, 0], d[:, 1], 2.0)
    assert np.abs(found - np.exp(-0.5 * ((d[:, 0] ** 2 + d[:, 1] ** 2) / 4.0))).max() <= 1e-3
    # InterpolateArray: nothing beyond the table's last interval, the table's own values at its samples
    assert alg.compute_weight(40.0, 0.0, 1.0) == 0 and float(alg.compute_weight(math.sqrt(0.5), 0.0, 1.0)) == pytest.approx(math.exp(-0.25), abs=1e-3)
    assert len(alg.table) == 160 and alg.table[0] == 1.0


# ---------------- TestDescribeSiftCommon ----------------
def test_describe_normalize_descriptor():
    alg = dr.Describe(4, 4, 8, 1.0, 0.5, 0.2)
    d = np.zeros(128)
    d[5], d[20], d[60] = 100, 120, 20
    out = alg.normalize(d, alg.maxValue)
    assert abs(math.sqrt(float((out * out).sum())) - 1) <= 1e-8 and abs(out[5] - out[20]) <= 1e-8
    assert np.array_equal(alg.normalize(np.zeros(128)), np.zeros(128))   # an all-zero descriptor is left alone


def test_describe_trilinear_interpolation():
    alg = dr.Describe(4, 4, 8, 1.0, 0.5, 0.2)
    d = np.zeros(128)
    alg.trilinear(2.0, 1.25, 2.0, 0.5, d)
    assert abs(d.sum() - 2.0) <= 1e-6 and np.count_nonzero(d) > 1
    d = np.zeros(128)
    alg.trilinear(2.0, 3.25, 3.25, 0.5, d)
    assert abs(d.sum() - 2.0 * 0.75 * 0.75 * 1.0) <= 1e-8
    d = np.zeros(128)
    alg.trilinear(2.0, 3.0, 3.0, 2 * math.pi / 8, d)
    assert np.count_nonzero(d > 0) == 1 and abs(d[d > 0][0] - 2.0) <= 1e-8


# ---------------- TestDescribePointSift ----------------
def test_describe_process_on_the_border_and_in_the_centre():
    rng = np.random.default_rng(234)
    dX, dY = (rng.uniform(-100, 100, (200, 200)).astype(f32) for _ in range(2))
    alg = dr.Describe(4, 4, 8, 1.5, 0.5, 0.2)
    for x, y in ((100, 0), (100, 199), (0, 100), (199, 100), (100, 100)):
        d = alg.process(dX, dY, x, y, 2, 0.5)
        assert d.shape == (128,) and np.isfinite(d).all() and abs(float((d * d).sum()) - 1) <= 1e-8


def _inside(d):
    assert np.abs(d[np.arange(128) % 8 != 0]).max() <= 1e-4
    return int((d[0::8] > 0).sum())


def test_describe_raw_descriptor_scale():
    dX, dY = np.zeros((200, 200), f32), np.zeros((200, 200), f32)
    alg = dr.Describe(4, 4, 8, 1.5, 0.5, 0.2)
    r = alg.canonical_radius()
    dX[60:60 + 2 * r, 60:60 + 2 * r] = 5.0
    assert _inside(alg.compute_raw(dX, dY, 60 + r, 60 + r, 1, 0)) == 4 * 4
    assert _inside(alg.compute_raw(dX, dY, 60 + r, 60 + r, 2, 0)) == 3 * 3


def test_describe_raw_descriptor_rotation():
    dX, dY = _fill(60, 55, 5.0), np.zeros((55, 60), f32)
    alg = dr.Describe(4, 4, 8, 1.5, 0.5, 0.2)
    for i in range(8):
        angle = dr.bound(i * math.pi / 4)
        d = alg.compute_raw(dX, dY, 20, 21, 1, angle)
        b = int(float(dr.domain2pi(-angle)) * 8 / (2 * math.pi))
        assert (d[b::8] > 0).all() and np.abs(d[np.arange(128) % 8 != b]).max() <= 1e-4


def test_vectorised_sums_keep_the_loop_order():
    """compute_raw (all samples at once, cumulative sums) against the reference's loops, bit for bit, on a sample grid that leaves the image;
    the histogram sums against a plain loop over the window"""
    rng = np.random.default_rng(5)
    dX, dY = (rng.uniform(-50, 50, (40, 45)).astype(f32) for _ in range(2))
    for alg in (dr.Describe(4, 4, 8, 1.0, 0.5, 0.2), dr.Describe(3, 2, 4, 1.5, 0.5, 0.2)):
        a = alg.compute_raw(dX, dY, 3.3, 20.7, 1.7, 0.9)
        b = alg.compute_raw_loops(dX, dY, 3.3, 20.7, 1.7, 0.9)
        assert np.count_nonzero(a) > alg.dof // 2 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    ori = dr.Orientation(36, 2.0)
    ori.compute_histogram(dX, dY, 4, 30, 2.4)
    mag, hx, hy = np.zeros(36), np.zeros(36), np.zeros(36)
    r = int(math.ceil(2.4 * 2.0))
    for y in range(max(30 - r, 0), min(30 + r + 1, 40)):
        for x in range(max(4 - r, 0), min(4 + r + 1, 45)):
            dx, dy = dX[y, x], dY[y, x]
            m = math.sqrt(float(f32(dx * dx + dy * dy)))
            theta = math.atan2(float(dy), float(dx))
            theta = theta + dr.PI2 if theta < 0 else theta
            w = float(ori.compute_weight(x - 4, y - 30, 2.4))
            h = int(theta / ori.histAngleBin) % 36
            mag[h] += m * w; hx[h] += float(dx) * w; hy[h] += float(dy) * w
    for a, b in ((ori.mag, mag), (ori.hx, hx), (ori.hy, hy)):
        assert np.array_equal(np.asarray(a).view(np.uint64), b.view(np.uint64))


def test_gradient_three_is_the_extended_border_form():
    """every pixel of the gradient, frame included, equals (a - b) * 0.5f on clamped reads: what the kernels evaluate on the fly"""
    img = orc.noise_image(37, 23, 4).array().copy()
    dX, dY = dr.gradient_three(img)
    h, w = img.shape
    xs, ys = np.arange(w), np.arange(h)
    fx = (img[:, np.clip(xs + 1, 0, w - 1)] - img[:, np.clip(xs - 1, 0, w - 1)]) * f32(0.5)
    fy = (img[np.clip(ys + 1, 0, h - 1), :] - img[np.clip(ys - 1, 0, h - 1), :]) * f32(0.5)
    assert np.array_equal(dX.view(np.uint32), fx.view(np.uint32)) and np.array_equal(dY.view(np.uint32), fy.view(np.uint32))
    assert np.count_nonzero(dX[:, 0]) == h and np.count_nonzero(dY[0, :]) == w   # the frame is not zero


# ---------------- TestCompleteSift ----------------
def test_complete_sift_basic():
    """TestCompleteSift.basic on a smaller random image (80 x 70 instead of 300 x 290; same configs)"""
    img = orc.noise_image(80, 70, 234, 0.0, 200.0).array().copy()
    ss, det = sr.ConfigSS(-1, 4, 3, 1.6), sr.ConfigDet(1, 0.0, 300, 10.0)
    desc = dr.Describe(4, 4, 8, 1.5, 0.5, 0.2)
    st = dr.new_stats()
    res = dr.complete(ss, det, dr.Orientation(36, 1.5), desc, img, st)
    assert desc.dof == 128 and len(res["orientation"]) > 10
    assert len(res["x"]) == len(res["orientation"]) == len(res["desc"]) == int(res["anglesPerDetection"].sum()) == st["features"]
    assert (np.abs(res["orientation"]) <= math.pi).all()


# ---------------- the library's host-only exports ----------------
@pytest.fixture(scope="module")
def lib():
    from boofcv_amd import _lib
    return _lib


def _cfg(lib, **kw):
    c = lib.CompleteSiftCfg()
    assert lib.load().bhip_csift_cfg_default(C.byref(c)) == 0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_weight_tables_equal_the_restatement_bit_for_bit(lib):
    L = lib.load()
    for kw in (dict(), dict(widthSubregion=3, widthGrid=2, numHistogramBins=4, sigmaToPixels=1.5), dict(widthSubregion=2, widthGrid=5, weightingSigmaFraction=0.3)):
        c = _cfg(lib, **kw)
        sw = c.widthSubregion * c.widthGrid
        exp_table, weight = np.full(lib.BHIP_CSIFT_EXP_TABLE + 1, -1.0), np.full(sw * sw + 1, -1.0, f32)
        assert L.bhip_csift_weights(C.byref(c), exp_table.ctypes.data_as(lib._dp), weight.ctypes.data_as(lib._fp)) == 0
        ref = dr.Describe(c.widthSubregion, c.widthGrid, c.numHistogramBins, c.sigmaToPixels, c.weightingSigmaFraction, c.maxDescriptorElementValue)
        assert exp_table[-1] == -1 and weight[-1] == -1
        assert np.array_equal(exp_table[:-1].view(np.uint64), dr.Orientation().table.view(np.uint64))
        assert np.array_equal(weight[:-1].view(np.uint32), ref.gaussianWeight.view(np.uint32)) and weight[:-1].max() == 1.0
        assert L.bhip_csift_dof(C.byref(c)) == ref.dof
    assert L.bhip_csift_weights(C.byref(_cfg(lib)), None, None) == 0


def test_describe_config_defaults_and_refusals(lib):
    L = lib.load()
    d = _cfg(lib)
    assert (d.histogramSize, d.sigmaEnlarge) == (36, 2.0)
    assert (d.widthSubregion, d.widthGrid, d.numHistogramBins, d.sigmaToPixels, d.weightingSigmaFraction, d.maxDescriptorElementValue) == (4, 4, 8, 1.0, 0.5, 0.2)
    assert L.bhip_csift_dof(C.byref(d)) == 128 and L.bhip_csift_cfg_default(None) == lib.BHIP_ERR_INVALID and L.bhip_csift_dof(None) == lib.BHIP_ERR_INVALID
    INV, UNS = lib.BHIP_ERR_INVALID, lib.BHIP_ERR_UNSUPPORTED
    for bad in (dict(histogramSize=2), dict(histogramSize=-1), dict(sigmaEnlarge=0.0), dict(sigmaEnlarge=float("nan")), dict(widthSubregion=0), dict(widthGrid=-2),
                dict(numHistogramBins=0), dict(sigmaToPixels=0.0), dict(weightingSigmaFraction=0.0), dict(maxDescriptorElementValue=-0.1),
                dict(widthSubregion=3, widthGrid=3), dict(widthSubregion=1, widthGrid=1)):
        assert L.bhip_csift_dof(C.byref(_cfg(lib, **bad))) == INV, bad
        assert L.bhip_csift_weights(C.byref(_cfg(lib, **bad)), None, None) == INV, bad
    for bad in (dict(histogramSize=lib.BHIP_CSIFT_MAX_HISTOGRAM + 1), dict(widthSubregion=5, widthGrid=10), dict(widthSubregion=2, widthGrid=24, numHistogramBins=4)):
        assert L.bhip_csift_dof(C.byref(_cfg(lib, **bad))) == UNS, bad
    assert L.bhip_csift_dof(C.byref(_cfg(lib, histogramSize=3, widthSubregion=2, widthGrid=24, numHistogramBins=3))) == 24 * 24 * 3
    assert (lib.BHIP_CSIFT_EXP_TABLE, lib.BHIP_CSIFT_MAX_HISTOGRAM, lib.BHIP_CSIFT_MAX_SAMPLE_WIDTH, lib.BHIP_CSIFT_MAX_DOF) == (160, 256, 48, 2048)


def test_describe_config_layout_matches_the_c_compiler(lib, tmp_path):
    """bhip_csift_cfg is the header's one forward-declared struct (Header.forward): sizeof / offsetof from gcc against the ctypes Structure; every
    bhip_csift_* export is bound and has a JNI entry point"""
    import os
    import subprocess
    from boofcv_amd import _header
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    H = _header.load()
    assert list(H.forward) == ["bhip_csift_cfg"] and lib.STRUCTS["bhip_csift_cfg"] is lib.CompleteSiftCfg
    fields = [f for _, f in H.forward["bhip_csift_cfg"]]
    assert fields == ["histogramSize", "sigmaEnlarge", "widthSubregion", "widthGrid", "numHistogramBins", "sigmaToPixels", "weightingSigmaFraction", "maxDescriptorElementValue"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "boofhip.h"', "int main(void) {", '\tprintf("sizeof %zu\\n", sizeof(bhip_csift_cfg));']
    lines += ['\tprintf("%s %%zu\\n", offsetof(bhip_csift_cfg, %s));' % (f, f) for f in fields] + ["\treturn 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    seen = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(lib.CompleteSiftCfg) == int(seen.pop("sizeof"))
    for f in fields:
        assert getattr(lib.CompleteSiftCfg, f).offset == int(seen.pop(f)), f
    names = [n for _, n, _ in H.functions if n.startswith("bhip_csift_")]
    assert sorted(names) == sorted(["bhip_csift_cfg_default", "bhip_csift_dof", "bhip_csift_weights"] + ["bhip_csift%s_%s" % (dev, t) for dev in ("", "_dev") for t in ("f32", "u8")])
    with open(os.path.join(root, "integration", "jni", "boofhip_jni.c")) as fh:
        shim = fh.read()
    assert all(n + "(" in shim for n in names)


# ---------------- the Python mirror (no context is created) ----------------
def test_mirror_classes_and_factory_arguments():
    from boofcv_amd import sift
    from boofcv_amd.api.image import GrayF32, GrayS16, GrayU8, InterleavedType, PlanarType
    o, d = sift.ConfigSiftOrientation(), sift.ConfigSiftDescribe()
    assert (o.histogramSize, o.sigmaEnlarge) == (36, 2.0)
    p = sift.ConfigSiftOrientation.createPaper()
    assert (p.histogramSize, p.sigmaEnlarge) == (36, 1.5)
    assert (d.widthSubregion, d.widthGrid, d.numHistogramBins, d.sigmaToPixels, d.weightingSigmaFraction, d.maxDescriptorElementValue) == (4, 4, 8, 1.0, 0.5, 0.2)
    c = sift.ConfigCompleteSift()
    assert (c.scaleSpace.firstOctave, c.scaleSpace.lastOctave, c.detector.maxFeaturesPerScale) == (0, 5, 0)
    c = sift.ConfigCompleteSift(-1, 4, 300)
    assert (c.scaleSpace.firstOctave, c.scaleSpace.lastOctave, c.detector.maxFeaturesPerScale) == (-1, 4, 300)
    with pytest.raises(TypeError):
        sift.ConfigCompleteSift(1, 2)
    c = sift.ConfigCompleteSift.createPaper()
    assert (c.scaleSpace.firstOctave, c.scaleSpace.lastOctave, c.scaleSpace.numScales, c.scaleSpace.sigma0) == (-1, 5, 3, float(f32(1.6)))
    assert (c.detector.extract.radius, c.detector.extract.ignoreBorder, c.detector.maxFeaturesPerScale, c.detector.edgeR) == (1, 1, 0, 10)
    assert c.orientation.sigmaEnlarge == 1.5 and c.describe.sigmaToPixels == 1.0
    c.checkValidity()
    dc = sift._desc_cfg(sift.ConfigSiftOrientation(18, 3.0), sift.ConfigSiftDescribe(3, 2, 4, 1.5, 0.25, 0.3))
    assert (dc.histogramSize, dc.sigmaEnlarge, dc.widthSubregion, dc.widthGrid, dc.numHistogramBins, dc.sigmaToPixels, dc.weightingSigmaFraction,
            dc.maxDescriptorElementValue) == (18, 3.0, 3, 2, 4, 1.5, 0.25, 0.3)
    assert sift.DescribePointSift(4, 4, 8, 1.5, 0.5, 0.2).getDescriptorLength() == 128 and sift.DescribePointSift(4, 4, 8, 1.5, 0.5, 0.2).getCanonicalRadius() == 8
    for t in (GrayS16, PlanarType(3, GrayF32), InterleavedType(3)):
        with pytest.raises(RuntimeError):
            sift.FactoryDetectDescribeSift.sift(None, t)
    for name in ("CompleteSift", "DetectDescribeCompleteSift", "FactoryDetectDescribeSift", "OrientationHistogramSift"):
        assert name in sift.__all__
    assert issubclass(sift.CompleteSift, sift.SiftDetector)
    for m in ("process", "getLocations", "getDescriptions", "getOrientations", "getDescriptorLength"):
        assert callable(getattr(sift.CompleteSift, m))
    for m in ("createDescription", "getDescription", "getDescriptionType", "detect", "getNumberOfFeatures", "getLocation", "getRadius", "getOrientation", "hasScale",
              "hasOrientation"):
        assert callable(getattr(sift.DetectDescribeCompleteSift, m))
    assert sift.DetectDescribeCompleteSift(None, GrayU8).hasOrientation() and sift.DetectDescribeCompleteSift(None, GrayU8).getInputType() is GrayU8
    # the detector's mirror is as it was
    assert not sift.InterestPointDetectorSift(None, GrayF32).hasOrientation()
