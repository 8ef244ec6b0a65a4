"""CPU checks of tests/binaryops_ref.py (the oracle of the GPU binary-image tests) against the reference's own answers, and of the Python mirror's
argument checks.  The literals are the fixtures of the reference's TestBinaryImageOps and TestLinearContourLabelChang2004."""
import numpy as np
import pytest

import binaryops_ref as ref

# TestBinaryImageOps.TEST -> EXPECTED8 (13 x 8)
TEST = np.array([0,0,0,1,1,1,0,0,0,0,0,0,0,
                 0,0,1,1,0,1,1,0,0,0,0,0,0,
                 0,0,1,1,1,1,0,0,0,0,1,1,0,
                 0,0,0,1,1,0,0,0,1,1,1,1,1,
                 0,0,0,0,0,1,0,0,1,1,1,1,0,
                 0,0,0,0,0,1,0,0,0,1,1,0,0,
                 0,0,0,0,0,0,0,0,0,0,0,0,0,
                 0,0,0,0,0,0,0,0,0,0,0,0,0], np.uint8).reshape(8, 13)
EXPECTED8 = np.array([0,0,0,1,1,1,0,0,0,0,0,0,0,
                      0,0,1,1,0,1,1,0,0,0,0,0,0,
                      0,0,1,1,1,1,0,0,0,0,2,2,0,
                      0,0,0,1,1,0,0,0,2,2,2,2,2,
                      0,0,0,0,0,1,0,0,2,2,2,2,0,
                      0,0,0,0,0,1,0,0,0,2,2,0,0,
                      0,0,0,0,0,0,0,0,0,0,0,0,0,
                      0,0,0,0,0,0,0,0,0,0,0,0,0], np.int32).reshape(8, 13)

# TestLinearContourLabelChang2004.TEST1 .. TEST4
CHANG1 = np.array([[0,0,0,0,0,0,0,1,0,0,0,1,1],
                   [0,0,0,0,0,0,0,1,0,0,0,1,1],
                   [0,0,0,0,0,0,0,1,0,0,1,1,0],
                   [0,0,0,0,0,0,0,0,1,1,1,1,0],
                   [0,0,1,0,0,0,0,0,1,1,1,0,0],
                   [0,0,1,0,0,0,1,1,1,1,1,0,0],
                   [1,1,1,1,1,1,1,1,1,1,0,0,0],
                   [0,0,0,1,1,1,1,1,0,0,0,0,0]], np.uint8)
CHANG2 = np.array([[0,0,1,0,0,0,0,1,0,0,0,0,0],
                   [0,1,0,1,0,0,1,0,0,1,0,0,0],
                   [0,0,1,0,0,1,0,1,0,1,1,1,0],
                   [0,0,0,0,1,0,0,0,1,1,1,1,0],
                   [0,0,1,0,1,0,0,0,1,0,0,0,0],
                   [0,0,0,0,1,0,1,1,1,0,1,1,0],
                   [1,1,1,0,0,1,0,0,1,0,0,1,0],
                   [0,0,0,1,1,1,1,1,0,0,0,0,0]], np.uint8)
CHANG3 = np.array([[0,0,0,0,0],
                   [0,1,1,1,0],
                   [0,1,1,1,0],
                   [0,1,0,1,0],
                   [0,1,1,1,0],
                   [0,0,0,0,0]], np.uint8)
CHANG4 = np.array([[0,0,0,0,0,0,0],
                   [0,0,1,1,1,1,1],
                   [0,1,0,1,1,1,1],
                   [0,1,1,1,0,1,1],
                   [0,1,1,1,1,1,1],
                   [0,1,1,1,1,1,1],
                   [0,1,1,1,1,1,1],
                   [0,0,0,0,0,0,0]], np.uint8)


def test_labelled_image_of_the_reference_fixture():
    labeled, n = ref.contourLabels(TEST, ref.EIGHT)
    assert n == 2 and np.array_equal(labeled, EXPECTED8)


@pytest.mark.parametrize("image,four,eight", [(CHANG1, 2, 1), (CHANG2, 14, 4), (CHANG3, 1, 1), (CHANG4, 1, 1)])
def test_contour_counts_of_the_reference_tests(image, four, eight):
    assert ref.contourLabels(image, ref.FOUR)[1] == four
    assert ref.contourLabels(image, ref.EIGHT)[1] == eight


def test_logic_literals_of_the_reference_tests():
    """TestBinaryImageOps:78-125"""
    a, b = np.zeros((6, 5), np.uint8), np.zeros((6, 5), np.uint8)
    a[0, 0] = 1; a[1, 1] = 1; b[0, 0] = 0; b[1, 1] = 1
    out = ref.logicAnd(a, b)
    assert (out[0, 0], out[1, 1], out[1, 0]) == (0, 1, 0)
    out = ref.logicOr(a, b)
    assert (out[0, 0], out[1, 1], out[1, 0]) == (1, 1, 0)
    out = ref.logicXor(a, b)
    assert (out[0, 0], out[1, 1], out[1, 0]) == (1, 0, 0)
    assert np.array_equal(ref.invert(a), 1 - a)


def test_chang_restatement_equals_raster_first_flood_fill():
    """The equivalence the GPU labelling rests on: the reference's labelled image is connected components numbered in the raster order of their
    first pixel, and its contour count is the number of components."""
    rng = np.random.RandomState(2004)
    for case in range(200):
        h, w = rng.randint(1, 41), rng.randint(1, 41)
        density = rng.uniform(0.2, 0.95)
        img = (rng.rand(h, w) < density).astype(np.uint8)
        if case % 5 == 0:
            img = ref.dilate8(img, 1)
        for rule in (ref.FOUR, ref.EIGHT):
            got, n = ref.contourLabels(img, rule)
            want, m = ref.floodLabels(img, rule)
            assert n == m and np.array_equal(got, want), (case, h, w, rule)
    for img in (np.ones((7, 9), np.uint8), np.zeros((7, 9), np.uint8), (np.indices((9, 11)).sum(0) % 2).astype(np.uint8)):
        for rule in (ref.FOUR, ref.EIGHT):
            got, n = ref.contourLabels(img, rule)
            want, m = ref.floodLabels(img, rule)
            assert n == m and np.array_equal(got, want)


@pytest.mark.parametrize("name", sorted(ref.MORPH))
def test_num_times_three_is_three_single_applications(name):
    rng = np.random.RandomState(7)
    op = ref.MORPH[name]
    for shape in ((8, 13), (1, 7), (2, 2), (11, 3)):
        img = (rng.rand(*shape) < (0.8 if "erode" in name else 0.2)).astype(np.uint8)
        assert np.array_equal(op(img, 3), op(op(op(img, 1), 1), 1))


def test_outside_values_of_the_border_forms():
    ones = np.ones((5, 6), np.uint8)
    assert ref.erode8(ones, 2).all()                      # outside is 1 (ImplBinaryBorderOps.java:105)
    e4 = ref.erode4(ones, 1)
    assert e4[0, 0] == 0 and e4[0, 2] == 1 and e4[2, 0] == 1   # outside is 0 along the frame, the outward cell is not read
    assert not ref.erode4(np.ones((4, 1), np.uint8), 1).any()
    assert ref.edge8(ones, False).sum() == 0 and ref.edge8(ones, True).sum() == 18
    noise = ref.removePointNoise(np.array([[0, 1, 1], [1, 1, 1], [1, 1, 1]], np.uint8))
    assert noise[0, 0] == 0 and noise[1, 1] == 1            # no "> 6 -> 1" on the frame


# ---- the Python mirror (these need the built library, not a GPU) ----
def test_mirror_module_imports_and_refuses_before_c():
    from boofcv_amd import api, binaryops
    ops = binaryops.BinaryImageOps
    img = api.GrayU8(5, 4)
    with pytest.raises(api.IllegalArgumentException):
        ops.erode4(img, 0, None)
    with pytest.raises(api.IllegalArgumentException):
        ops.erode8(img, 1, api.GrayU8(4, 4))
    with pytest.raises(api.IllegalArgumentException):
        ops.logicAnd(img, api.GrayU8(5, 5), None)
    with pytest.raises(api.IllegalArgumentException):
        ops.contourLabels(img, binaryops.ConnectRule.EIGHT, api.GrayS32(5, 5))
    with pytest.raises(api.IllegalArgumentException):
        ops.thin(img, -1, None)
    assert [int(r) for r in binaryops.ConnectRule] == [4, 8]


def test_library_exports_the_binary_symbols():
    from boofcv_amd import _lib
    L = _lib.load()
    for name in ("bhip_binary_logic_dev_u8", "bhip_binary_logic_u8", "bhip_binary_invert_dev_u8", "bhip_binary_invert_u8", "bhip_binary_morph_dev_u8",
                 "bhip_binary_morph_u8", "bhip_binary_edge_dev_u8", "bhip_binary_edge_u8", "bhip_binary_remove_point_noise_dev_u8",
                 "bhip_binary_remove_point_noise_u8", "bhip_label_blobs_dev_u8_s32", "bhip_label_blobs_u8_s32", "bhip_relabel_dev_s32", "bhip_relabel_s32",
                 "bhip_label_to_binary_dev_s32_u8", "bhip_label_to_binary_s32_u8"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert (_lib.BHIP_MORPH_ERODE4, _lib.BHIP_MORPH_DILATE4, _lib.BHIP_MORPH_ERODE8, _lib.BHIP_MORPH_DILATE8) == (0, 1, 2, 3)
