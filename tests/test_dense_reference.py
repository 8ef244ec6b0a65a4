"""CPU: tests/dense_ref.py against the reference's own known answers (TestDescribeDenseHogFastAlg, TestDescribeDenseHogAlg, TestDescribeDenseSiftAlg,
TestDescribeImageDenseHoG, TestDescribeImageDenseSift), its scatter and gather forms against each other bit for bit, the mirror classes of
boofcv_amd/dense.py without a context, and the host-only exports of the C ABI (bhip_dense_*_layout, bhip_dense_hog_weights)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import dense_ref as dr
import sift_describe_ref as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _noise(W, H, seed, u8=False):
    a = (np.random.default_rng(seed).random((H, W)) * 200.0).astype(f32)
    return np.floor(a).astype(np.uint8) if u8 else a


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ---------------- TestDescribeDenseHogFastAlg ----------------
def test_fast_hog_grow_cell_array():
    hog = dr.Hog(10, 8, 2, 2, 1)
    for (w, h), (cols, rows) in (((64, 32), (8, 4)), ((32, 16), (4, 2)), ((64, 40), (8, 5)), ((61, 45), (7, 5))):
        cells = hog.cell_histograms(np.zeros((h, w), f32), np.zeros((h, w), f32))
        assert cells.shape == (rows, cols, 10)


def test_fast_hog_compute_descriptor():
    """two-value histograms in four cells of a 60 x 80 frame: dof 40, location (16, 0), the descriptor within 1e-8"""
    hog = dr.Hog(10, 8, 2, 2, 1)
    cellCols, cellRows = 60 // 8, 80 // 8
    cells = np.zeros((cellRows, cellCols, 10), f32)
    expected = np.zeros(40)
    for (row, col, a, b, index0) in ((0, 2, 2, 3, 0), (0, 3, 2, 3, 10), (1, 2, 5, 0, 20), (1, 3, 7, 8, 30)):
        cells[row, col, a], cells[row, col, b] = f32(2.4), f32(1.2)
        expected[index0 + a], expected[index0 + b] = float(f32(2.4)), float(f32(1.2))
    expected = sd.Describe.normalize_l2(np.where((e := sd.Describe.normalize_l2(expected)) > 0.2, 0.2, e))
    found = hog.block_descriptor(cells, 0, 2)
    assert found.shape == (40,) and math.sqrt(float(((expected - found) ** 2).sum())) < 1e-8
    perRow, perCol, locs = hog.layout(60, 80)
    assert (perRow, perCol) == (6, 9) and locs[2] == (16, 0)


def test_fast_hog_compute_cells():
    """a constant gradient (cos, sin) of every 7th degree and the axes: N * weight in the bin of the angle and the rest in the next one"""
    hog = dr.Hog(10, 8, 3, 3, 1)
    N = 64
    for degree in sorted(set(range(0, 360, 7)) | {0, 90, 180, 270, 45, 135}):
        theta = degree * math.pi / 180.0
        dx, dy = np.full((16, 16), f32(math.cos(theta))), np.full((16, 16), f32(math.sin(theta)))
        floatBin = (degree + 90.0) * 10.0 / 180
        targetBin = int(floatBin)
        expected = float(f32(1.0 - (floatBin - targetBin)))
        cells = hog.cell_histograms(*hog.pixel_features(dx, dy))
        targetBin %= 10
        assert cells.shape == (2, 2, 10)
        for c in cells.reshape(-1, 10):
            for j in range(10):
                want = N * expected if j == targetBin else N * (1.0 - expected) if j == (targetBin + 1) % 10 else 0.0
                if targetBin == (targetBin + 1) % 10:
                    want = N
                assert abs(float(c[j]) - want) < 2e-3, (degree, j, float(c[j]), want)


def test_fast_hog_descriptors_in_region():
    """120 x 110, (10, 8, 2, 2, 1), the region (5, 9) - (67, 89): as many descriptors as the brute-force count of the reference's test"""
    hog = dr.Hog(10, 8, 2, 2, 1)
    w, h, x0, y0, x1, y1, c = 120, 110, 5, 9, 67, 89, 8
    perRow, perCol, locs = hog.layout(w, h)
    cellCols = w // c
    expected = []
    for y in range(0, h - 2 * c, c):
        i = (y // c) * cellCols
        for x in range(0, w - 2 * c, c):
            if x >= x0 and x + 2 * c < x1 and y >= y0 and y + 2 * c < y1:
                expected.append(i)
            i += 1
    found = hog.descriptors_in_region(len(locs), cellCols, x0, y0, x1, y1)
    assert len(found) == len(expected) > 0 and sorted(found) == sorted(expected)


# ---------------- TestDescribeDenseHogAlg ----------------
def test_std_hog_weight_block_pixels():
    pixelsPerCell = 3
    for widthCells in (3, 4):
        hog = dr.Hog(10, pixelsPerCell, widthCells, widthCells + 1, 1, False)
        wx, wy = widthCells * pixelsPerCell, (widthCells + 1) * pixelsPerCell
        rx, ry = wx // 2 + wx % 2, wy // 2 + wy % 2
        totalOne, mx = 0, 0.0
        for i in range(ry):
            for j in range(rx):
                v0, v1 = hog.weights[i * wx + j], hog.weights[i * wx + (wx - j - 1)]
                v2, v3 = hog.weights[(wy - i - 1) * wx + (wx - j - 1)], hog.weights[(wy - i - 1) * wx + j]
                assert abs(v0 - v1) < 1e-8 and abs(v1 - v2) < 1e-8 and abs(v2 - v3) < 1e-8
                mx = max(mx, v0)
                totalOne += v0 == 1.0
        assert hog.weights[0] < hog.weights[1] and hog.weights[0] < hog.weights[widthCells]
        assert abs(mx - 1.0) < 1e-8
        if wx % 2 == 1:
            assert totalOne == 1


def test_std_hog_compute_cell_histogram_and_add():
    hog = dr.Hog(10, 4, 3, 4, 1, False)
    findex, magnitude = np.zeros((80, 60), f32), np.ones((80, 60))
    hist = [0.0] * (10 * 3 * 4)
    cellX, cellY = 1, 2
    hog.compute_cell_histogram(findex, magnitude, hist, 20, 25, cellX, cellY)
    modified = lambda x, y: any(v != 0 for v in hist[(y * 3 + x) * 10:(y * 3 + x) * 10 + 10])
    assert all(modified(cellX + j, cellY + i) for i in (-1, 0, 1) for j in (-1, 0, 1)) and not modified(0, 0)
    # addToHistogram
    hist = [0.0] * (10 * 3 * 4)
    for (x, y) in ((-1, 2), (10, 2), (1, -2), (1, 20)):
        hog.add_to_histogram(hist, x, y, 3, 1.0)
        assert not any(hist)
    hog.add_to_histogram(hist, 1, 2, 3, 1.0)
    assert [i for i, v in enumerate(hist) if v != 0] == [(2 * 3 + 1) * 10 + 3]


# ---------------- TestDescribeDenseSiftAlg ----------------
def _random_gradient(W, H, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((H, W)) * 200).astype(f32), (rng.random((H, W)) * 200).astype(f32)


def test_dense_sift_locations_span_the_image_and_descriptors_sit_there():
    alg = dr.DenseSift(4, 4, 8, 0.5, 0.2, 10, 10)
    numX, numY, locs = alg.layout(100, 102)
    r = 8
    cols, rows = (100 - 2 * r) // 10, (102 - 2 * r) // 10
    assert (numX, numY) == (cols, rows) and len(locs) == cols * rows
    w, h = 100 - 2 * r, 102 - 2 * r
    assert locs == [(col * w // (cols - 1) + r, row * h // (rows - 1) + r) for row in range(rows) for col in range(cols)]
    assert locs[0] == (r, r) and locs[-1] == (100 - r, 102 - r)


def test_dense_sift_precompute_angles():
    dx, dy = _random_gradient(50, 40, 234)
    dx[3, 4], dy[3, 4] = 0, 5          # the zero-argument cases of Math.atan2
    dx[3, 5], dy[3, 5] = 0, -5
    dx[3, 6], dy[3, 6] = -5, 0
    dx[3, 7], dy[3, 7] = 0, 0
    alg = dr.DenseSift(4, 4, 8, 0.5, 0.2, 10, 10)
    angle, magnitude = alg.precompute_angles(dx, dy)
    for y in range(40):
        for x in range(50):
            a = math.atan2(float(dy[y, x]), float(dx[y, x]))
            assert abs((a + 2 * math.pi if a < 0 else a) - angle[y, x]) < 1e-8
            assert abs(float(f32(math.sqrt(float(dx[y, x] * dx[y, x] + dy[y, x] * dy[y, x])))) - magnitude[y, x]) < 1e-4
    assert angle[3, 4] == math.pi / 2 and angle[3, 5] == 1.5 * math.pi and angle[3, 6] == math.pi and angle[3, 7] == 0
    assert magnitude.dtype == f32 and angle.dtype == np.float64


def test_dense_sift_compute_descriptor_against_the_point_descriptor():
    """DescribeDenseSiftAlg.computeDescriptor equals DescribePointSift.process(x, y, sigma 1, orientation 0) within 1e-8"""
    dx, dy = _random_gradient(100, 102, 235)
    alg = dr.DenseSift(4, 4, 8, 0.5, 0.2, 10, 10)
    point = sd.Describe(4, 4, 8, 1.0, 0.5, 0.2)
    angle, magnitude = alg.precompute_angles(dx, dy)
    for (x, y) in ((30, 35), (45, 10), (60, 12), (50, 50)):
        found = dr.normalize_descriptor(alg.descriptor_raw(angle, magnitude, x, y), 0.2)
        expected = point.process(dx, dy, x, y, 1.0, 0.0)
        assert np.abs(found - expected).max() < 1e-8


# ---------------- TestDescribeImageDenseHoG / TestDescribeImageDenseSift ----------------
@pytest.mark.parametrize("fast", [True, False])
def test_hog_locations_lie_on_the_grid(fast):
    hog = dr.Hog(fastVariant=fast)
    perRow, perCol, locs = hog.layout(120, 90)
    assert len(locs) == perRow * perCol == 13 * 9
    for (x, y) in locs:   # top-left pixels; DescribeImageDenseHoG adds half the region
        assert x % 8 == 0 and y % 8 == 0 and 0 <= x <= 120 - 24 and 0 <= y <= 90 - 24


def test_dense_sift_border_and_count():
    alg = dr.DenseSift(periodX=8, periodY=9)
    numX, numY, locs = alg.layout(120, 90)
    assert len(locs) == ((120 - 16) // 8) * ((90 - 16) // 9)
    assert all(8 <= x <= 120 - 8 and 8 <= y <= 90 - 8 for x, y in locs)


# ---------------- scatter against gather, bit for bit ----------------
@pytest.mark.parametrize("cfg", [(9, 8, 3, 3, 1), (10, 8, 2, 2, 1), (9, 5, 3, 2, 2), (1, 1, 3, 3, 1), (2, 3, 2, 2, 1)])
def test_fast_hog_cells_scatter_equals_gather(cfg):
    hog = dr.Hog(*cfg)
    img = _noise(29 if cfg[1] == 1 else 45, 12 if cfg[1] == 1 else 37, 3)
    findex, sumsq = hog.pixel_features(*dr.gradient_f32(img))
    assert _same(hog.cell_histograms(findex, sumsq), hog.cell_histograms_gather(findex, sumsq))


@pytest.mark.parametrize("cfg", [(9, 8, 3, 3, 1), (9, 5, 3, 2, 2), (1, 4, 2, 3, 1), (9, 5, 3, 3, 1), (4, 2, 1, 1, 1)])
def test_std_hog_scatter_equals_gather(cfg):
    hog = dr.Hog(*cfg, fastVariant=False)
    img = _noise(40, 33, 4)
    findex, sumsq = hog.pixel_features(*dr.gradient_f32(img))
    perRow, perCol, locs = hog.layout(40, 33)
    assert locs
    for (x, y) in (locs[0], locs[-1]):
        a, b = hog.std_descriptor_raw(findex, sumsq, x, y), hog.std_descriptor_raw_gather(findex, sumsq, x, y)
        assert _same(a, b) and a.any()


@pytest.mark.parametrize("cfg,u8", [((4, 4, 8), False), ((3, 2, 4), False), ((4, 4, 8), True), ((2, 3, 5), False)])
def test_dense_sift_scatter_equals_gather(cfg, u8):
    alg = dr.DenseSift(*cfg)
    img = _noise(40, 33, 5, u8)
    dx, dy = dr.gradient_s16(img) if u8 else dr.gradient_f32(img)
    angle, magnitude = alg.precompute_angles(dx, dy)
    numX, numY, locs = alg.layout(40, 33)
    for (x, y) in (locs[0], locs[-1]):
        loops = alg.descriptor_raw_loops(angle, magnitude, x, y)
        assert _same(loops, alg.descriptor_raw(angle, magnitude, x, y)) and _same(loops, alg.descriptor_raw_gather(angle, magnitude, x, y)) and loops.any()


def test_s16_gradient_has_no_divisor():
    img = np.array([[0, 10, 30], [5, 5, 5], [200, 0, 255]], np.uint8)
    dx, dy = dr.gradient_s16(img)
    assert dx.tolist() == [[10, 30, 20], [0, 0, 0], [-200, 55, 255]] and dy.tolist() == [[5, -5, -25], [200, -10, 225], [195, -5, 250]]


# ---------------- the mirror, without a context ----------------
def test_mirror_configs_factory_and_refusals():
    from boofcv_amd import dense
    from boofcv_amd.api.core import IllegalArgumentException
    from boofcv_amd.api.image import GrayF32, GrayS16, GrayU8, InterleavedType, PlanarType, TupleDesc_F64
    c = dense.ConfigDenseHoG()
    assert (c.orientationBins, c.pixelsPerCell, c.cellsPerBlockX, c.cellsPerBlockY, c.stepBlock, c.fastVariant) == (9, 8, 3, 3, 1, True)
    s = dense.ConfigDenseSift()
    assert (s.sampling.periodX, s.sampling.periodY) == (6.0, 6.0)
    assert (s.sift.widthSubregion, s.sift.widthGrid, s.sift.numHistogramBins, s.sift.weightingSigmaFraction, s.sift.maxDescriptorElementValue) == (4, 4, 8, 0.5, 0.2)
    assert (dense.DenseSampling().periodX, dense.DenseSampling(5.5, 7.25).periodY) == (0.0, 7.25)
    F = dense.FactoryDescribeImageDense
    for T in (GrayF32, GrayU8):
        hog, sift = F.hog(None, T), F.sift(None, T)
        assert isinstance(hog, dense.DescribeImageDenseHoG) and isinstance(sift, dense.DescribeImageDenseSift) and isinstance(hog, dense.DescribeImageDense)
        assert hog.getImageType() is T and sift.getImageType() is T and hog.getDescriptionType() is TupleDesc_F64
        assert hog.createDescription().size() == 81 and sift.createDescription().size() == 128
        assert hog.getLocations() == [] and sift.getDescriptions() == []
        assert (hog.getRegionWidthPixelX(), hog.getRegionWidthPixelY()) == (24, 24)
    assert F.hog(dense.ConfigDenseHoG(10, 8, 3, 2, 1, False)).createDescription().size() == 60
    with pytest.raises(IllegalArgumentException):
        F.hog(dense.ConfigDenseHoG(fastVariant=False)).getCellRows()
    for bad in (dense.ConfigDenseHoG(stepBlock=0), dense.ConfigDenseHoG(pixelsPerCell=0), dense.ConfigDenseHoG(orientationBins=0), dense.ConfigDenseHoG(cellsPerBlockX=-1)):
        with pytest.raises(IllegalArgumentException):
            F.hog(bad)
    for big in (dense.ConfigDenseHoG(orientationBins=65), dense.ConfigDenseHoG(pixelsPerCell=33), dense.ConfigDenseHoG(9, 8, 16, 16, 1)):
        with pytest.raises(RuntimeError):
            F.hog(big)
    odd = dense.ConfigDenseSift()
    odd.sift.widthSubregion, odd.sift.widthGrid = 3, 3
    none = dense.ConfigDenseSift()
    none.sampling = None
    for bad in (odd, none):
        with pytest.raises(IllegalArgumentException):
            F.sift(bad)
    wide = dense.ConfigDenseSift()
    wide.sift.widthSubregion, wide.sift.widthGrid = 5, 10
    with pytest.raises(RuntimeError):
        F.sift(wide)
    for refuse in (lambda: F.surfFast(None, GrayF32), lambda: F.surfStable(None, GrayF32), lambda: F.hog(None, PlanarType(3)), lambda: F.hog(None, InterleavedType(3)),
                   lambda: F.sift(None, PlanarType(2)), lambda: F.hog(None, GrayS16), lambda: F.sift(None, GrayS16)):
        with pytest.raises(IllegalArgumentException):
            refuse()
    with pytest.raises(IllegalArgumentException, match="orientation"):
        F.surfFast()
    with pytest.raises(IllegalArgumentException):   # the wrong image type, before any context exists
        F.hog(None, GrayF32).process(GrayU8(8, 8))


# ---------------- the C ABI ----------------
EXPORTS = sorted(["bhip_dense_hog_layout", "bhip_dense_sift_layout", "bhip_dense_hog_weights"]
                 + ["bhip_dense_%s%s_%s" % (a, dev, t) for a in ("hog", "sift") for dev in ("", "_dev") for t in ("f32", "u8")])


def test_exports_are_bound_and_have_jni_entry_points():
    from boofcv_amd import _header, _lib
    H = _header.load()
    assert sorted(n for _, n, _ in H.functions if n.startswith("bhip_dense_")) == EXPORTS
    assert all(n in _lib.SIGNATURES for n in EXPORTS)
    L = _lib.load()
    assert all(hasattr(L, n) for n in EXPORTS)
    with open(os.path.join(ROOT, "integration", "jni", "boofhip_jni.c")) as f:
        jni = f.read()
    assert all("(jint)%s(" % n in jni for n in EXPORTS)
    assert not any("dense" in c for c in list(H.structs) + list(H.tagged) + list(H.declared) + list(H.forward))   # plain scalar arguments, no struct
    assert (_lib.BHIP_DENSE_MAX_DOF, _lib.BHIP_DENSE_MAX_BINS, _lib.BHIP_DENSE_MAX_CELL, _lib.BHIP_DENSE_MAX_SAMPLE_WIDTH) == (2048, 64, 32, 48)


def _hog_layout(L, lib, args, W, H, cap=4096):
    pr, pc, dof = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    xy = np.full((cap + 1, 2), -7, np.int32)
    n = L.bhip_dense_hog_layout(*args, W, H, C.byref(pr), C.byref(pc), C.byref(dof), xy.ctypes.data_as(lib._i32p), cap)
    return n, pr.value, pc.value, dof.value, xy


def _sift_layout(L, lib, args, W, H, cap=4096):
    pr, pc, dof = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    xy = np.full((cap + 1, 2), -7, np.int32)
    n = L.bhip_dense_sift_layout(*args, W, H, C.byref(pr), C.byref(pc), C.byref(dof), xy.ctypes.data_as(lib._i32p), cap)
    return n, pr.value, pc.value, dof.value, xy


def test_layout_exports_equal_the_reference_on_the_gpu_cases():
    from boofcv_amd import _lib as lib
    import test_gpu_dense as g
    L = lib.load()
    seen = 0
    for name, (alg, W, H, kind, seed, cfg) in g.CASES.items():
        if alg == "sift":
            ref = dr.DenseSift(*cfg)
            n, pr, pc, dof, xy = _sift_layout(L, lib, (cfg[0], cfg[1], cfg[2], cfg[5], cfg[6]), W, H)
        else:
            ref = dr.Hog(*cfg, fastVariant=(alg == "fast"))
            n, pr, pc, dof, xy = _hog_layout(L, lib, ref.args(), W, H)
        perRow, perCol, locs = ref.layout(W, H)
        assert (n, pr, pc, dof) == (len(locs), perRow, perCol, ref.dof), name
        assert np.array_equal(xy[:n], np.array(locs, np.int32).reshape(-1, 2)) and (xy[n:] == -7).all(), name
        seen += n > 0
    assert seen >= 30
    # larger frames, both variants, a cap below the count
    for (W, H) in ((1920, 1080), (120, 90), (23, 24), (24, 24), (8, 300)):
        for fast in (1, 0):
            ref = dr.Hog(fastVariant=bool(fast))
            perRow, perCol, locs = ref.layout(W, H)
            n, pr, pc, dof, xy = _hog_layout(L, lib, ref.args(), W, H, cap=7)
            assert (n, pr, pc, dof) == (len(locs), perRow, perCol, 81)
            assert np.array_equal(xy[:min(n, 7)], np.array(locs[:7], np.int32).reshape(-1, 2)) and (xy[min(n, 7):] == -7).all()
    ref = dr.DenseSift()
    assert L.bhip_dense_sift_layout(4, 4, 8, 6.0, 6.0, 1920, 1080, None, None, None, None, 0) == 317 * 177 == len(ref.layout(1920, 1080)[2])
    for (W, H, px, py) in ((120, 90, 8.0, 9.0), (100, 102, 10.0, 10.0), (16, 40, 6.0, 6.0), (15, 40, 6.0, 6.0), (40, 21, 6.0, 6.0), (53, 47, 5.5, 7.25), (28, 29, 6.0, 6.0)):
        numX, numY, locs = dr.DenseSift(periodX=px, periodY=py).layout(W, H)
        n, pr, pc, dof, xy = _sift_layout(L, lib, (4, 4, 8, px, py), W, H)
        assert (n, pr, pc, dof) == (len(locs), numX, numY, 128), (W, H)
        assert np.array_equal(xy[:n], np.array(locs, np.int32).reshape(-1, 2))


def test_layout_exports_refuse_what_the_reference_throws_on():
    from boofcv_amd import _lib as lib
    L = lib.load()
    INV, UNS = lib.BHIP_ERR_INVALID, lib.BHIP_ERR_UNSUPPORTED
    hog = lambda *a: L.bhip_dense_hog_layout(*a, None, None, None, None, 0)
    sift = lambda *a: L.bhip_dense_sift_layout(*a, None, None, None, None, 0)
    for bad in ((9, 8, 3, 3, 0, 1, 64, 48), (9, 8, 3, 3, -1, 0, 64, 48), (0, 8, 3, 3, 1, 1, 64, 48), (9, 0, 3, 3, 1, 1, 64, 48), (9, 8, 0, 3, 1, 0, 64, 48),
                (9, 8, 3, 3, 1, 1, 0, 48), (9, 8, 3, 3, 1, 1, 64, -1)):
        assert hog(*bad) == INV, bad
    for big in ((65, 8, 3, 3, 1, 1, 64, 48), (9, 33, 3, 3, 1, 0, 64, 48), (9, 8, 16, 16, 1, 1, 64, 48), (9, 8, 3, 3, 1, 1, 64, 65536)):
        assert hog(*big) == UNS, big
    assert hog(64, 32, 4, 8, 1, 0, 64, 48) == 0 and hog(1, 1, 1, 1, 1, 1, 5, 4) == 20
    # numX == 1 with rows, numY == 1: ArithmeticException; numX == 1 without rows: an empty list
    for (W, H) in ((24, 40), (40, 24), (24, 24), (16, 24)):
        assert sift(4, 4, 8, 6.0, 6.0, W, H) == INV, (W, H)
        with pytest.raises(ZeroDivisionError):
            dr.DenseSift().layout(W, H)
    assert sift(4, 4, 8, 6.0, 6.0, 24, 16) == 0 and dr.DenseSift().layout(24, 16)[2] == []
    # a frame narrower than the window with a tiny period: (int) of a quotient below -2^31 saturates in Java, the loops are empty
    assert sift(4, 4, 8, 1e-9, 6.0, 10, 40) == 0 and sift(4, 4, 8, 6.0, 1e-12, 40, 3) == 0 and sift(4, 4, 8, 1e-9, 1e-9, 3, 3) == 0
    for bad in ((0, 4, 8, 6.0, 6.0, 40, 33), (4, 4, 0, 6.0, 6.0, 40, 33), (3, 3, 8, 6.0, 6.0, 40, 33), (4, 4, 8, 0.0, 6.0, 40, 33), (4, 4, 8, 6.0, -1.0, 40, 33),
                (4, 4, 8, float("nan"), 6.0, 40, 33), (4, 4, 8, 6.0, 6.0, 0, 33)):
        assert sift(*bad) == INV, bad
    for big in ((5, 10, 8, 6.0, 6.0, 400, 330), (4, 4, 65, 6.0, 6.0, 40, 33), (2, 24, 4, 6.0, 6.0, 400, 330), (4, 4, 8, 1e-9, 6.0, 400, 330)):
        assert sift(*big) == UNS, big


def test_hog_weights_export_equals_the_reference():
    from boofcv_amd import _lib as lib
    L = lib.load()
    for (ppc, cbx, cby) in ((8, 3, 3), (3, 3, 4), (3, 4, 5), (5, 3, 2), (4, 1, 2)):
        ref = dr.Hog(9, ppc, cbx, cby, 1, False).weights
        got = np.full(len(ref) + 1, -1.0)
        assert L.bhip_dense_hog_weights(ppc, cbx, cby, got.ctypes.data_as(lib._dp)) == len(ref) == ppc * ppc * cbx * cby
        assert _same(got[:-1], ref) and got[-1] == -1.0 and ref.max() == 1.0
    assert L.bhip_dense_hog_weights(8, 3, 3, None) == 576
    assert np.isnan(dr.Hog(9, 1, 1, 1, 1, False).weights).all()   # a side of one pixel: sigma 0
    got = np.zeros(1)
    assert L.bhip_dense_hog_weights(1, 1, 1, got.ctypes.data_as(lib._dp)) == 1 and np.isnan(got[0])
    assert L.bhip_dense_hog_weights(0, 3, 3, None) == lib.BHIP_ERR_INVALID and L.bhip_dense_hog_weights(33, 3, 3, None) == lib.BHIP_ERR_UNSUPPORTED
