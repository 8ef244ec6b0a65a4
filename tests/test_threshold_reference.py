"""tests/threshold_ref.py against the reference's own known answers (IT:alg/filter/binary/TestGThresholdImageOps.java, TestThresholdBlock.java,
TestThresholdBlockOtsu.java, impl/TestThresholdBlockMean_*.java, impl/TestThresholdBlockMinMax_*.java, TestThresholdImageOps.java, re-expressed:
their literals as data, none of their text), the conditions that make the GPU cases discriminate, and the new surface without a GPU: the header's
struct and constants, the config defaults, the mirror's refusals and its view checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import threshold_ref as R
from boofcv_amd import _header, _lib, api, binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = binary.ThresholdType


# ---------------- Otsu ----------------
def _variance(hist, start, stop, allPixels):
    idx = np.arange(start, stop + 1)
    h = hist[start:stop + 1].astype(np.float64)
    total = h.sum()
    if total == 0:
        return None
    mean = (idx * h).sum() / total
    return ((h * (idx - mean) ** 2).sum() / total, total / allPixels)


def _brute_force_otsu(hist, total):
    """minimise the weighted within-class variance, threshold inclusive (TestGThresholdImageOps.bruteForceOtsu)"""
    best, bestScore = -1, np.inf
    for j in range(len(hist) - 1):
        s0, s1 = _variance(hist, 0, j, total), _variance(hist, j + 1, len(hist) - 1, total)
        if s0 is None or s1 is None:
            continue
        score = s0[1] * s0[0] + s1[1] * s1[0]
        if score < bestScore:
            best, bestScore = j, score
    return best


@pytest.mark.parametrize("zeros", [False, True])
def test_compute_otsu_matches_brute_force(zeros):
    rng = np.random.default_rng(234)
    for _ in range(10):
        hist = rng.integers(0, 400, 256)
        if zeros:   # computeOtsu_zeros: empty bins at both ends
            hist[:15] = 0
            hist[240:] = 0
        total = int(hist.sum())
        found = R.compute_otsu(hist, 256, total)
        assert found == _brute_force_otsu(hist, total)
        assert binary.GThresholdImageOps.computeOtsu(hist, 256, total) == found
        o = R.ComputeOtsu(False, 0.0, True, 1.0)
        assert o.compute(hist, 256, total) == found   # ComputeOtsu.computeOtsu is the same loop; (int)(1.0*found + 0.5) == found


def test_otsu2_pathological_histogram():
    """computeOtsu2_pathological: two spikes, the threshold half way between them"""
    hist = np.zeros(256, np.int64)
    hist[10], hist[120] = 200, 500
    assert R.ComputeOtsu(True, 0.0, True, 1.0).compute(hist, 256, 700) == 65
    assert R.ComputeOtsu(True, 0.0, True, 0.5).compute(hist, 256, 700) == 33   # (int)(0.5*65 + 0.5)
    assert R.compute_otsu(hist, 256, 700) == 10


def test_otsu_tuning_penalises_low_texture():
    hist = np.zeros(256, np.int64)
    hist[100], hist[103] = 50, 50
    plain = R.ComputeOtsu(True, 0.0, True, 1.0).compute(hist, 256, 100)
    tuned = R.ComputeOtsu(True, 15.0, True, 1.0).compute(hist, 256, 100)
    up = R.ComputeOtsu(True, 15.0, False, 1.0).compute(hist, 256, 100)
    assert plain == 102 and tuned < plain < up
    const = np.zeros(256, np.int64)
    const[0] = 77   # wF == 0 on the first bin: threshold 0, variance 0.001
    assert R.ComputeOtsu(True, 0.0, True, 1.0).compute(const, 256, 77) == 0
    assert R.ComputeOtsu(False, 0.0, True, 1.0).compute(const, 256, 77) == 0


# ---------------- ConfigLength and the block geometry ----------------
def test_config_length():
    assert R.compute_i(11, -1, 100) == 11 and R.compute_i(10.5, -1, 7) == 11 and R.compute_i(10.49, -1, 7) == 10
    assert R.compute_i(5, 0.2, 37) == 7 and R.compute_i(20, 0.2, 37) == 20 and R.compute_i(-1, -1, 37) == -1
    for args in ((11, -1, 100), (5, 0.2, 37), (20, 0.2, 37), (-1, -1, 37), (0.4, -1, 3)):
        assert binary.ConfigLength(args[0], args[1]).computeI(args[2]) == R.compute_i(*args)
    assert binary.ConfigLength.relative(0.2, 5).isRelative() and binary.ConfigLength.fixed(3).isFixed()


def test_select_block_size():
    assert R.select_block_size(300, 330, 30) == (30, 30)
    assert R.select_block_size(329, 301, 30) == (32, 30)
    assert R.select_block_size(301, 329, 30) == (30, 32)
    assert R.select_block_size(10, 12, 20) == (10, 12)   # widthLargerThanImage
    with pytest.raises(ZeroDivisionError):
        R.select_block_size(10, 12, 0)
    bw, bh = C.c_int(), C.c_int()
    L = _lib.load()
    for w, h, req in ((300, 330, 30), (329, 301, 30), (301, 329, 30), (10, 12, 20), (67, 37, 8), (259, 17, 10), (5, 5, 8)):
        assert L.bhip_threshold_block_size(w, h, req, C.byref(bw), C.byref(bh)) == _lib.BHIP_OK
        assert (bw.value, bh.value) == R.select_block_size(w, h, req)
    assert L.bhip_threshold_block_size(10, 12, 0, C.byref(bw), C.byref(bh)) == _lib.BHIP_ERR_INVALID


@pytest.mark.parametrize("w, h, req", [(67, 37, 8), (259, 17, 10), (5, 5, 8), (32, 32, 16), (100, 120, 6), (101, 121, 14)])
def test_blocks_cover_every_pixel_once(w, h, req):
    bw, bh, nbx, nby, rect = R.block_geometry(w, h, req)
    count = np.zeros((h, w), int)
    for by in range(nby):
        for bx in range(nbx):
            x0, y0, x1, y1 = rect(bx, by)
            count[y0:y1, x0:x1] += 1
    assert (count == 1).all()
    if (w, h, req) == (67, 37, 8):   # last block 11 wide and 10 high
        assert (bw, bh, nbx, nby) == (8, 9, 8, 4) and rect(7, 3) == (56, 27, 67, 37)


# ---------------- block processors ----------------
KINDS = [(R.BLOCK_MIN_MAX, np.uint8), (R.BLOCK_MIN_MAX, np.float32), (R.BLOCK_MEAN, np.uint8), (R.BLOCK_MEAN, np.float32), (R.BLOCK_OTSU, np.uint8)]


def _uniform(dtype, w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 255, (h, w)).astype(dtype)


@pytest.mark.parametrize("kind, dtype", KINDS)
def test_block_threshold_sanity_toggle_and_small_image(kind, dtype):
    """GenericThresholdCommon: about half the pixels either way, up is the inverse of down (texture test off), a block wider than the image"""
    img = _uniform(dtype, 100, 120, 234)
    spread = 1.0 if kind == R.BLOCK_MIN_MAX else 10.0
    down = R.threshold_block(img, kind, 6, 1.0, True, minimumSpread=spread)
    up = R.threshold_block(img, kind, 6, 1.0, False, minimumSpread=spread)
    assert down.sum() > down.size / 4 and up.sum() > up.size / 4
    if kind != R.BLOCK_MIN_MAX:   # the min/max form marks textureless blocks 1 both ways
        assert ((down == 0) == (up != 0)).all()
    small = _uniform(dtype, 10, 12, 5)
    assert R.threshold_block(small, kind, 20, 1.0, True, minimumSpread=spread).sum() > small.size / 4


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_min_max_threshold_square(dtype):
    """GenericThresholdBlockMinMaxChecks.thresholdSquare"""
    img = np.full((120, 100), 200, dtype)
    img[45:77, 40:70] = 20
    out = R.threshold_block(img, R.BLOCK_MIN_MAX, 6, 1.0, True, minimumSpread=10.0)
    assert out[45:77, 40:70].sum() == 30 * 32
    assert not out[44, 39:72].any() and not out[78, 39:72].any() and not out[45:77, 39].any() and not out[45:77, 71].any()


def test_min_max_nan_first_pixel_stays():
    img = R.image_f32(16, 8, 3)
    img[0, 0] = np.nan     # first pixel of block (0, 0): min and max stay NaN
    img[5, 11] = np.nan    # elsewhere in block (1, 0): skipped
    stats = R.block_stats(img, R.BLOCK_MIN_MAX, 8)
    assert np.isnan(stats[0, 0]).all() and not np.isnan(stats[0, 1]).any()
    blk = img[:, 8:]
    assert stats[0, 1, 0] == np.nanmin(blk) and stats[0, 1, 1] == np.nanmax(blk)


def test_block_mean_u8_byte_wrap():
    img = np.full((16, 16), 250, np.uint8)
    stats = R.block_stats(img, R.BLOCK_MEAN, 8, scale=1.3)
    assert (stats == (325 & 0xFF)).all()   # (byte)325 read back & 0xFF


# ---------------- local thresholds ----------------
@pytest.mark.parametrize("w, h, radius", [(20, 13, 1), (20, 13, 3), (20, 13, 6), (5, 5, 5), (13, 20, 8), (20, 9, 7), (7, 31, 5)])
def test_mean_u8_equals_the_dispatch_loop_by_loop(w, h, radius):
    img = R.image_u8(w, h, w + radius)
    assert (R.mean_u8(img, radius) == R.mean_u8_literal(img, radius)).all()


def test_local_mean_is_blur_then_compare():
    """TestThresholdImageOps.localMean: the threshold is the mean blur scaled"""
    img = R.image_u8(30, 21, 9)
    blur = R.mean_u8(img, 3).astype(np.float32)
    for down in (True, False):
        got = R.local_mean(img, 7, -1, 0.95, down)
        exp = (img <= blur * np.float32(0.95)) if down else (img * np.float32(0.95) > blur)
        assert (got == exp).all()
    f = R.image_f32(30, 21, 9)
    bf = R.mean_f32(f, 3)
    assert (R.local_mean(f, 7, -1, 1.0, True) == (f <= bf)).all()
    # a constant image blurs to itself, border and interior alike (GrayF32: up to the rounding of total / weight with the 1/5 taps)
    c = np.full((9, 14), 7.25, np.float32)
    assert np.allclose(R.mean_f32(c, 2), c, rtol=1e-6, atol=0) and (R.mean_f32(c, 2)[2:-2, 2:-2] == c[2:-2, 2:-2]).all()
    assert (R.mean_u8(np.full((9, 14), 200, np.uint8), 3) == 200).all()


# ---------------- the conditions that let the GPU cases discriminate ----------------
def test_gpu_block_mean_f32_input_is_order_sensitive():
    d = R.BLOCK_MEAN_F32_INPUT
    img = R.image_f32(d["width"], d["height"], d["seed"])
    raster = R.block_stats(img, R.BLOCK_MEAN, d["requested"], 0.95)
    pairwise = R.block_stats(img, R.BLOCK_MEAN, d["requested"], 0.95, pairwise=True)
    assert (raster.view(np.int32) != pairwise.view(np.int32)).any()


def test_gpu_local_mean_u8_input_tells_two_roundings_from_one():
    d = R.LOCAL_MEAN_U8_INPUT
    img = R.image_u8(d["width"], d["height"], d["seed"])
    radius = d["length"] // 2
    single = R.box_mean_u8_single_division(img, radius)
    assert (R.local_mean(img, d["length"], -1, 0.95, True) != R.local_mean(img, d["length"], -1, 0.95, True, blur=single)).any()


# ---------------- the surface, without a GPU ----------------
def test_threshold_struct_layout_and_constants_match_the_c_compiler(tmp_path):
    """bhip_threshold_cfg is the header's one tagged struct (Header.tagged): sizeof / offsetof from gcc against the ctypes Structure"""
    H = _header.load()
    assert list(H.tagged) == ["bhip_threshold_cfg"] and _lib.STRUCTS["bhip_threshold_cfg"] is _lib.ThresholdCfg
    fields = [f for _, f in H.tagged["bhip_threshold_cfg"]]
    assert fields == ["type", "fixedThreshold", "scale", "down", "widthLength", "widthFraction", "minPixelValue", "maxPixelValue", "thresholdFromLocalBlocks",
                      "minimumSpread", "useOtsu2", "tuning"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "boofhip.h"', "int main(void) {", '\tprintf("sizeof %zu\\n", sizeof(bhip_threshold_cfg));']
    lines += ['\tprintf("%s %%zu\\n", offsetof(bhip_threshold_cfg, %s));' % (f, f) for f in fields]
    lines += ['\tprintf("const_%s %%d\\n", BHIP_THRESHOLD_%s);' % (t.name, t.name) for t in T]
    lines += ["\treturn 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    seen = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert C.sizeof(_lib.ThresholdCfg) == int(seen.pop("sizeof"))
    for f in fields:
        assert getattr(_lib.ThresholdCfg, f).offset == int(seen.pop(f)), f
    assert {k[6:]: int(v) for k, v in seen.items()} == {t.name: int(t) for t in T}
    assert [t.name for t in T] == ["FIXED", "GLOBAL_ENTROPY", "GLOBAL_OTSU", "GLOBAL_LI", "GLOBAL_HUANG", "LOCAL_GAUSSIAN", "LOCAL_MEAN", "LOCAL_OTSU", "BLOCK_MIN_MAX",
                                   "BLOCK_MEAN", "BLOCK_OTSU", "LOCAL_SAVOLA", "LOCAL_NICK"]   # ThresholdType's order


def test_new_exports_are_declared_and_bound():
    L = _lib.load()
    for name in ("bhip_threshold_cfg_default", "bhip_threshold_block_size", "bhip_threshold_dev_u8", "bhip_threshold_dev_f32", "bhip_threshold_u8", "bhip_threshold_f32",
                 "bhip_mean_u8", "bhip_gaussian_u8", "bhip_mean_dev_u8", "bhip_gaussian_dev_u8"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    assert _lib.SIGNATURES["bhip_threshold_dev_f32"] == (i, [vp, C.POINTER(_lib.ThresholdCfg), vp, ll, i, i, i, i, vp, ll, i])


def _fields(c):
    return (c.type, c.fixedThreshold, c.scale, c.down, c.widthLength, c.widthFraction, c.minPixelValue, c.maxPixelValue, c.thresholdFromLocalBlocks, c.minimumSpread,
            c.useOtsu2, c.tuning)


def test_config_defaults_match_the_mirror():
    L = _lib.load()
    for t in T:
        c = _lib.ThresholdCfg()
        assert L.bhip_threshold_cfg_default(int(t), c) == _lib.BHIP_OK
        mirror = binary.ConfigThreshold.fixed(0) if t == T.FIXED else binary.ConfigThreshold.global_(t) if t.isGlobal() else binary.ConfigThreshold.local(t, 11)
        assert _fields(c) == _fields(mirror._c()), t.name
    c = _lib.ThresholdCfg()
    L.bhip_threshold_cfg_default(int(T.BLOCK_MIN_MAX), c)
    assert (c.scale, c.minimumSpread, c.widthLength, c.widthFraction, c.down, c.thresholdFromLocalBlocks) == (0.95, 10.0, 11.0, -1.0, 1, 1)
    L.bhip_threshold_cfg_default(int(T.GLOBAL_OTSU), c)
    assert (c.scale, c.minPixelValue, c.maxPixelValue, c.useOtsu2, c.tuning) == (1.0, 0, 255, 1, 0.0)
    assert L.bhip_threshold_cfg_default(13, c) == _lib.BHIP_ERR_INVALID and L.bhip_threshold_cfg_default(-1, c) == _lib.BHIP_ERR_INVALID
    assert binary.ConfigThresholdBlockMinMax().scale == 0.85 and binary.ConfigThresholdLocalOtsu().type == T.BLOCK_OTSU
    with pytest.raises(api.IllegalArgumentException):
        binary.ConfigThreshold.global_(T.LOCAL_MEAN)
    with pytest.raises(api.IllegalArgumentException):
        binary.ConfigThreshold.local(T.GLOBAL_OTSU, 11)


def test_mirror_refuses_what_the_gpu_does_not_implement():
    F = binary.FactoryThresholdBinary
    for t in (T.GLOBAL_ENTROPY, T.GLOBAL_LI, T.GLOBAL_HUANG):
        for imageType in (api.GrayU8, api.GrayF32):
            with pytest.raises(api.IllegalArgumentException):
                F.threshold(binary.ConfigThreshold.global_(t), imageType)
    for t in (T.LOCAL_SAVOLA, T.LOCAL_NICK, T.LOCAL_OTSU):
        for imageType in (api.GrayU8, api.GrayF32):
            with pytest.raises(api.IllegalArgumentException):
                F.threshold(binary.ConfigThreshold.local(t, 11), imageType)
    for t in (T.GLOBAL_OTSU, T.BLOCK_OTSU):
        cfg = binary.ConfigThreshold.global_(t) if t.isGlobal() else binary.ConfigThreshold.local(t, 11)
        with pytest.raises(api.IllegalArgumentException):
            F.threshold(cfg, api.GrayF32)
        assert F.threshold(cfg, api.GrayU8).getInputType() is api.GrayU8
    with pytest.raises(api.IllegalArgumentException):
        F.threshold(binary.ConfigThreshold.fixed(3), api.GrayS16)
    with pytest.raises(api.IllegalArgumentException):
        F.globalOtsu(0, 200, 1.0, True, api.GrayU8)
    for refused in (lambda: F.localSauvola(11, True, 0.3, api.GrayU8), lambda: F.localNick(11, True, -0.2, api.GrayU8),
                    lambda: F.localOtsu(11, 1.0, True, True, 0.0, api.GrayU8), lambda: F.globalEntropy(0, 255, 1.0, True, api.GrayU8),
                    lambda: F.globalLi(0, 255, 1.0, True, api.GrayU8), lambda: F.globalHuang(0, 255, 1.0, True, api.GrayU8)):
        with pytest.raises(api.IllegalArgumentException):
            refused()
    assert boofcv_amd_has_the_names()


def boofcv_amd_has_the_names():
    import boofcv_amd
    return all(getattr(boofcv_amd, n) is getattr(binary, n) for n in binary.__all__) and not any(hasattr(api, n) for n in binary.__all__)


VIEWS_CHILD = """
import types
import numpy as np
from boofcv_amd import _lib, api, binary

calls = []

class Fake:
    def __getattr__(self, name):
        def fn(*args):
            calls.append(name)
            return _lib.BHIP_OK
        return fn

_lib.load = lambda: Fake()
ctx = types.SimpleNamespace(_h=1, _children=set())
W, H = 16, 12
F32, U8 = api.GrayF32, api.GrayU8
T = binary.ThresholdType
local = binary.ConfigThreshold.local

ENTRIES = [
    ("InputToBinary.process LOCAL_MEAN u8", lambda a, o: binary.FactoryThresholdBinary.threshold(local(T.LOCAL_MEAN, 5), U8, ctx).process(a, o), (U8, U8), ["bhip_threshold_u8"]),
    ("InputToBinary.process BLOCK_MEAN f32", lambda a, o: binary.FactoryThresholdBinary.threshold(local(T.BLOCK_MEAN, 5), F32, ctx).process(a, o), (F32, U8), ["bhip_threshold_f32"]),
    ("GThresholdImageOps.threshold", lambda a, o: binary.GThresholdImageOps.threshold(a, o, 100, True, ctx=ctx), (U8, U8), ["bhip_threshold_u8"]),
    ("BlurImageOps.mean u8", lambda a, o: api.BlurImageOps.mean(a, o, 2, ctx=ctx), (U8, U8), ["bhip_mean_u8"]),
    ("BlurImageOps.gaussian u8", lambda a, o: api.BlurImageOps.gaussian(a, o, -1, 2, ctx=ctx), (U8, U8), ["bhip_gaussian_u8"]),
]

def grow(im): im.height += 1
def narrow(im): im.stride = im.width - 1
def past(im): im.startIndex = im.data.size

for what, call, types_, expected in ENTRIES:
    for i in range(len(types_)):
        for damage in (grow, narrow, past):
            if "BLOCK" in what and i == 1 and damage is grow:
                continue   # ThresholdBlock.process reshapes its output to the input's size first
            images = [t(W, H) for t in types_]
            damage(images[i])
            del calls[:]
            try:
                call(*images)
            except api.IllegalArgumentException:
                pass
            else:
                raise AssertionError("%s: image %d after %s reached C: %s" % (what, i, damage.__name__, calls))
            assert not calls, "%s: image %d after %s: %s was called before the view was refused" % (what, i, damage.__name__, calls)
    del calls[:]
    call(*[t(W, H) for t in types_])
    assert calls == expected, (what, calls)
print("ok", len(ENTRIES))
"""


def test_views_are_checked_before_any_c_call():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", VIEWS_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok 5" in r.stdout
