"""CPU: tests/sift_ref.py against the reference's own known answers (TestSiftScaleSpace, TestSiftDetector) and against independent forms of
its pieces.  tests/test_gpu_sift.py compares the GPU with sift_ref bit for bit; this file is what ties sift_ref to the reference."""
import math

import numpy as np
import pytest

import fast_ref
import sift_ref as sr
from oracle import pyoracle as orc

f32 = np.float32


def _detector_cfg():
    """TestSiftDetector.createDetector: SiftScaleSpace(-1,5,3,1.6), ConfigExtract(1,0,1,true,true,true), limit 1000, edgeR 10"""
    return sr.ConfigSS(-1, 5, 3, 1.6), sr.ConfigDet(1, 0.0, 1000, 10.0)


@pytest.mark.parametrize("radius", [2, 5])
@pytest.mark.parametrize("white", [True, False])
def test_process_squares(radius, white):   # TestSiftDetector.process :41-74
    c_x, c_y = 40, 42
    img = np.zeros((70, 80), f32) if white else np.full((70, 80), 200, f32)
    img[c_y - radius:c_y + radius + 1, c_x - radius:c_x + radius + 1] = 200 if white else 0
    ss, det = _detector_cfg()
    xy, scale, wh, where = sr.detect(ss, det, img)
    assert len(scale) > 0
    found = False
    for i in range(len(scale)):
        if math.hypot(xy[i, 0] - c_x, xy[i, 1] - c_y) <= 0.2:
            assert abs(radius * 1.25 - scale[i]) <= 0.5
            assert bool(wh[i]) == white
            found = True
    assert found


def test_is_scale_space_extremum():   # :76-94
    for sign in (-1.0, 1.0):
        upper, lower = np.zeros((40, 30), f32), np.zeros((40, 30), f32)
        assert sr.is_scale_space_extremum(lower, upper, 15, 16, sign * 100, sign)
        upper[16, 15] = sign * 100
        assert not sr.is_scale_space_extremum(lower, upper, 15, 16, sign * 100, sign)
        upper[16, 15] = 0
        lower[16, 15] = sign * 100
        assert not sr.is_scale_space_extremum(lower, upper, 15, 16, sign * 100, sign)
    z = np.zeros((40, 30), f32)
    for x, y in ((1, 16), (15, 1), (29, 16), (15, 39), (28, 16)):   # the strict frame: c_x <= 1 || ... >= width - 1; 28 = width - 2 passes
        assert sr.is_scale_space_extremum(z, z, x, y, 100, 1.0) == ((x, y) == (28, 16))


def test_process_feature_candidate_no_change():   # :99-121
    for sign in (-1.0, 1.0):
        upper, current, lower = (np.zeros((40, 30), f32) for _ in range(3))
        current[16, 15] = sign * 100
        assert not sr.is_edge(current, 15, 16, 10.0)
        px, py, scale, white = sr.feature_candidate(lower, current, upper, 15, 16, sign * 100, sign > 0, 2.0, (4.0, 5.0, 6.0))
        assert abs(px - 30) < 1e-8 and abs(py - 32) < 1e-8 and abs(scale - 5) < 1e-8 and white == (sign < 0)


def test_process_feature_candidate_shift():   # :127-173
    x, y = 15, 16
    for sign in (-1.0, 1.0):
        upper, current, lower = (np.zeros((40, 30), f32) for _ in range(3))
        current[y - 1, x] = sign * 90; current[y, x] = sign * 100; current[y + 1, x] = sign * 80
        current[y, x - 1] = sign * 90; current[y, x + 1] = sign * 80
        upper[y, x] = sign * 80; lower[y, x] = sign * 90
        px, py, scale, _ = sr.feature_candidate(lower, current, upper, x, y, sign * 100, sign > 0, 2.0, (4.0, 5.0, 6.0))
        assert abs(x * 2 - px) < 2 and abs(y * 2 - py) < 2 and abs(5 - scale) < 2
        assert x * 2 > px and y * 2 > py and 5 > scale
        upper[y, x] = sign * 90; lower[y, x] = sign * 80
        _, _, scale, _ = sr.feature_candidate(lower, current, upper, x, y, sign * 100, sign > 0, 2.0, (4.0, 5.0, 6.0))
        assert abs(5 - scale) < 2 and 5 < scale


def test_is_edge():   # :175-193
    img = np.zeros((120, 100), f32)
    img[:, :50] = 100
    assert sr.is_edge(img, 50, 50, 10.0)
    img[:] = 0
    img[50, 50] = 100
    assert not sr.is_edge(img, 50, 50, 10.0)


def test_sparse_derivative_kernels():
    """createSparseDerivatives: [-1,0,1] convolved with itself, and the outer product, with the signed zeros KernelMath leaves"""
    assert [float(v) for v in sr.KERNEL_DD] == [1, 0, -2, 0, 1] and not any(np.signbit(v) for v in sr.KERNEL_DD[1::2])
    assert [[float(v) for v in row] for row in sr.KERNEL_XY] == [[1, 0, -1], [0, 0, 0], [-1, 0, 1]]
    assert [[bool(np.signbit(v)) for v in row] for row in sr.KERNEL_XY] == [[False, True, True], [True, False, False], [True, False, False]]
    # against plain second differences on a smooth patch, border clamped
    rng = np.random.RandomState(3)
    img = rng.rand(9, 11).astype(f32)
    xx, xy, yy = sr.sparse_derivs(img, 5, 4)
    assert abs(float(xx) - float(img[4, 7] - 2 * img[4, 5] + img[4, 3])) < 1e-5
    assert abs(float(yy) - float(img[6, 5] - 2 * img[4, 5] + img[2, 5])) < 1e-5
    assert abs(float(xy) - float(img[3, 4] - img[3, 6] - img[5, 4] + img[5, 6])) < 1e-5
    xx, _, _ = sr.sparse_derivs(img, 9, 4)   # x + 2 = 11 is clamped to 10
    assert abs(float(xx) - float(img[4, 10] - 2 * img[4, 9] + img[4, 7])) < 1e-5


def test_compute_sigma_scale():   # TestSiftScaleSpace.computeSigmaScale :97-111
    ss = sr.ConfigSS(-1, 4, 3, 1.6)
    k = math.pow(2.0, 1.0 / 3.0)
    for i in range(5):
        assert abs(0.8 * math.pow(k, i) - sr.sigma_scale(ss, -1, i)) < 1e-8
        assert abs(1.6 * math.pow(k, i) - sr.sigma_scale(ss, 0, i)) < 1e-8


def test_image_too_small_for_octaves():   # :152-163: two more octaves after the first, then false
    assert [(w, h) for _, w, h in sr.layout(sr.ConfigSS(0, 5, 3, 1.6), 20, 20)] == [(20, 20), (10, 10), (5, 5)]
    assert len(sr.scale_space(sr.ConfigSS(0, 5, 3, 1.6), np.zeros((20, 20), f32))) == 3


def _compare(expected, found, octave):
    """TestSiftScaleSpace.compareImage :121-147"""
    if found.shape[1] > expected.shape[1]:
        s = int(math.pow(2, -octave))
        return float(np.abs(expected - found[::s, ::s][:expected.shape[0], :expected.shape[1]]).mean())
    s = int(math.pow(2, octave))
    h, w = found.shape
    return float(np.abs(expected[::s, ::s][:h, :w] - found).mean())


@pytest.mark.parametrize("firstOctave", [-1, 0, 1])
def test_octave_blur(firstOctave):   # checkOctaveBlur :40-68 on a smaller frame
    img = orc.noise_image(120, 136, 234).array().copy()
    sigma0 = float(f32(1.6))
    space = sr.scale_space(sr.ConfigSS(firstOctave, 5, 2, sigma0), img)
    assert [o for o, _, _ in space] == list(range(firstOctave, firstOctave + len(space)))
    for o, octv, _ in space:
        sigma = float(f32(sigma0 * math.pow(2, o)))
        expected = orc.gaussian_blur(orc.Gray.from_array(img), sigma, -1).array()
        assert _compare(expected, octv[0], o) < 2, (firstOctave, o)


def test_scale_blur():   # checkScaleBlur :73-95
    img = orc.noise_image(120, 136, 234).array().copy()
    ss = sr.ConfigSS(0, 3, 2, float(f32(1.6)))
    o, octv, dog = sr.scale_space(ss, img)[0]
    assert len(octv) == 5 and len(dog) == 4
    for i in range(5):
        expected = orc.gaussian_blur(orc.Gray.from_array(img), sr.sigma_scale(ss, 0, i), -1).array()
        assert _compare(expected, octv[i], 0) < 2
        if i:
            assert np.array_equal(dog[i - 1], octv[i] - octv[i - 1])


def test_layouts_of_the_gpu_test_shapes():
    """the octave count and sizes the GPU test's shapes were chosen for; layout() agrees with what scale_space() computes"""
    ref = sr.ConfigSS(-1, 5, 3, 1.6)
    dflt = sr.ConfigSS()
    assert dflt.sigma0 == float(f32(2.75)) and (dflt.firstOctave, dflt.lastOctave, dflt.numScales) == (0, 5, 3)
    want = {
        (80, 70, ref): [(160, 140), (80, 70), (40, 35), (20, 17), (10, 8), (5, 4)],
        (97, 61, dflt): [(97, 61), (48, 30), (24, 15), (12, 7), (6, 3)],
        (300, 70, dflt): [(300, 70), (150, 35), (75, 17), (37, 8), (18, 4)],
        (304, 72, dflt): [(304, 72), (152, 36), (76, 18), (38, 9), (19, 4)],
        (128, 64, dflt): [(128, 64), (64, 32), (32, 16), (16, 8), (8, 4)],
        (128, 65, dflt): [(128, 65), (64, 32), (32, 16), (16, 8), (8, 4)],
        (304, 200, sr.ConfigSS(1, 5, 3, 1.6)): [(152, 100), (76, 50), (38, 25), (19, 12), (9, 6)],
    }
    for (w, h, ss), dims in want.items():
        assert [(a, b) for _, a, b in sr.layout(ss, w, h)] == dims
        space = sr.scale_space(ss, orc.noise_image(w, h, 1).array())
        assert [(o[1][0].shape[1], o[1][0].shape[0]) for o in space] == dims
        assert all(len(o[1]) == ss.numScales + 3 and len(o[2]) == ss.numScales + 2 for o in space)
    assert [len(k) for k in sr.kernels(dflt)[1]] == [9, 9, 13, 15, 19] and len(sr.kernels(dflt)[0]) == 15


def test_scale_image_up_against_the_scalar_interpolator():
    """the vectorised scaleImageUp against ImplBilinearPixel_F32.get written out per pixel (get_fast inside, get_border with clamped reads)"""
    img = orc.noise_image(7, 5, 9).array().copy()
    h, w = img.shape
    for scale in (2, 4):
        up = sr.scale_image_up(img, scale)
        assert up.shape == (h * scale, w * scale) and up.dtype == f32
        fdiv = f32(1) / f32(scale)
        for y in range(h * scale):
            for x in range(w * scale):
                sx, sy = f32(x) * fdiv, f32(y) * fdiv
                if sx < 0 or sy < 0 or sx > w - 2 or sy > h - 2:
                    xf, yf = f32(math.floor(sx)), f32(math.floor(sy))
                    xt, yt = int(xf), int(yf)
                    g = lambda a, b: img[min(max(b, 0), h - 1), min(max(a, 0), w - 1)]
                else:
                    xt, yt = int(sx), int(sy)
                    xf, yf = f32(xt), f32(yt)
                    g = lambda a, b: img[b, a]
                ax, ay = f32(sx - xf), f32(sy - yf)
                one = f32(1)
                v = f32(f32((one - ax) * (one - ay)) * g(xt, yt))
                v = f32(v + f32(f32(ax * (one - ay)) * g(xt + 1, yt)))
                v = f32(v + f32(f32(ax * ay) * g(xt + 1, yt + 1)))
                v = f32(v + f32(f32((one - ax) * ay) * g(xt, yt + 1)))
                assert v.tobytes() == up[y, x].tobytes(), (scale, x, y)


def test_nonmax_limiter_against_the_block_algorithm_and_the_cut():
    """the oracle's strict maxima of the image and of its negation are NonMaxBlockSearchStrict.MinMax with thresholds (-t, t) and border 1; the
    cut keeps the k largest |value|"""
    ss = sr.ConfigSS()
    dog = sr.scale_space(ss, orc.noise_image(97, 61, 1).array())[0][2][1]
    for radius in (1, 2, 3):
        found, full = sr.nonmax_limiter(dog, sr.ConfigDet(radius))
        mins, maxs = fast_ref.nonmax_block(dog, radius, 0.0, 0.0, 1, True, True)
        assert found == full and [(x, y) for _, m, x, y in found if not m] == [tuple(p) for p in mins.tolist()]
        assert [(x, y) for _, m, x, y in found if m] == [tuple(p) for p in maxs.tolist()]
        assert all(v == (dog[y, x] if m else -dog[y, x]) for v, m, x, y in found) and len(mins) > 5 and len(maxs) > 5
    found, full = sr.nonmax_limiter(dog, sr.ConfigDet(2, 0.0, 10))
    assert len(full) > 10 and len(found) == 10
    assert sorted(e[0] for e in found) == sorted(e[0] for e in full)[-10:]


# ---------------- the surface, without a GPU ----------------
def test_sift_cfg_layout_matches_the_c_compiler_and_exports_are_bound(tmp_path):
    """bhip_sift_cfg is declared as `struct name { }; typedef struct name name;` (Header.declared): sizeof / offsetof from gcc against the ctypes
    Structure; every bhip_sift_* export of the header is bound and has a JNI entry point"""
    import ctypes as C
    import os
    import subprocess
    from boofcv_amd import _header, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    H = _header.load()
    assert list(H.declared) == ["bhip_sift_cfg"] and _lib.STRUCTS["bhip_sift_cfg"] is _lib.SiftCfg
    fields = [f for _, f in H.declared["bhip_sift_cfg"]]
    assert fields == ["firstOctave", "lastOctave", "numScales", "sigma0", "extractRadius", "extractThreshold", "extractIgnoreBorder", "extractUseStrictRule",
                      "extractDetectMin", "extractDetectMax", "maxFeaturesPerScale", "edgeR"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "boofhip.h"', "int main(void) {", '\tprintf("sizeof %zu\\n", sizeof(bhip_sift_cfg));']
    lines += ['\tprintf("%s %%zu\\n", offsetof(bhip_sift_cfg, %s));' % (f, f) for f in fields]
    lines += ['\tprintf("tile %d\\n", BHIP_SIFT_LEVEL_TILE_WIDTH * 1000 + BHIP_SIFT_LEVEL_TILE_HEIGHT);', "\treturn 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    seen = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(_lib.SiftCfg) == int(seen.pop("sizeof")) == 64
    assert int(seen.pop("tile")) == _lib.BHIP_SIFT_LEVEL_TILE_WIDTH * 1000 + _lib.BHIP_SIFT_LEVEL_TILE_HEIGHT and _lib.BHIP_SIFT_LEVEL_MAX_TAPS == 27
    for f in fields:
        assert getattr(_lib.SiftCfg, f).offset == int(seen.pop(f)), f
    names = [n for _, n, _ in H.functions if n.startswith("bhip_sift_")]
    assert sorted(names) == sorted(["bhip_sift_cfg_default", "bhip_sift_layout"] + ["bhip_sift_%s%s_%s" % (op, dev, t) for op in ("scale_space", "detect")
                                                                                     for dev in ("", "_dev") for t in ("f32", "u8")])
    with open(os.path.join(root, "integration", "jni", "boofhip_jni.c")) as fh:
        shim = fh.read()
    assert all(n + "(" in shim for n in names)
