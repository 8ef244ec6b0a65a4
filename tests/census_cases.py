"""The census block-matching cases that tests/test_gpu_disparity_census.py runs on the GPU and tests/test_census_reference.py checks for
non-vacuity on the CPU: scenes, reference outputs (computed once per process, read-only) and the pixel classes each case claims to exercise.

The geometry is test_gpu_disparity.py's table (SAD); the kernel's tile is 64 block columns wide, 16 output rows high for BLOCK_3_3 and
22 - 2*regionRadiusY rows for the 4-byte census words (boofcv_amd/csrc/disparity.hip)."""
import functools

import census_ref as cr
import disparity_ref as dr

BM_VARIANTS = ("BLOCK_3_3", "BLOCK_5_5", "BLOCK_7_7", "CIRCLE_9")   # one per word size (GrayU8, GrayS32, GrayS64), and the circle

# maxPerPixelError, in differing bits per pixel of the region: about half of what two unrelated words differ by (4 of 8 bits, 12 of 24, and for
# the GrayS64 words 15.5 of bits 0..30 plus 33/2 for sample 31), so that wrong matches are rejected and right ones kept
MPE = {"BLOCK_3_3": 2.0, "BLOCK_5_5": 6.0, "BLOCK_7_7": 14.0, "CIRCLE_9": 14.0}

V, E, R, T, I = dr.VALID_INT, dr.REJECT_ERROR, dr.REJECT_RTOL, dr.REJECT_TEXTURE, dr.VALID_INTERP

# name, W, H, minD, range, rx, ry, maxPerPixelError as a multiple of MPE[variant] (0: the test is off), validateRtoL, texture, outputs, the classes
# the case claims to exercise in its first output (tests/test_census_reference.py: at least 10 reference pixels of each, for every variant).
# The 259-wide case has the steepest disparity ramp under the largest region of the three error cases, hence its 1.5.
BM_CASES = [
    ("default", 50, 60, 0, 40, 3, 3, 0, 1, .15, ("f32",), (V, T, I)),
    ("min2_u8", 67, 21, 2, 30, 2, 1, 1.0, 1, .15, ("u8",), (V, E, R, T)),
    ("five_column_tiles", 259, 17, 5, 120, 4, 3, 1.5, 0, .1, ("f32",), (V, E, R, T, I)),
    ("lm3_wrap", 48, 11, 0, 3, 2, 2, 0, -1, .15, ("f32", "u8"), (V, T)),
    ("radius0", 44, 9, 1, 20, 0, 0, 0, 1, .15, ("f32", "u8"), (V, R, T, I)),
    ("maxD_limit", 30, 9, 0, 24, 3, 1, 0, 1, .15, ("f32", "u8"), (V, R, T, I)),
    ("radius7", 96, 20, 0, 82, 7, 7, 0, 1, .15, ("f32", "u8"), (V, T, I)),
    ("row_bands", 200, 40, 0, 50, 2, 2, 1.0, 1, .15, ("f32",), (V, E, R, T, I)),
]


def params(case, variant):
    """-> (minD, range, rx, ry, maxPerPixelError, validateRtoL, texture)"""
    _, W, H, minD, rng, rx, ry, mpe, rtol, tex, _, _ = case
    return (minD, rng, rx, ry, MPE[variant] * mpe, rtol, tex)


def each_check_params(variant, off):
    """-> (maxPerPixelError, validateRtoL, texture) of the row_bands case with one check (`off`), or with "all", disabled"""
    mpe, rtol, tex = MPE[variant], 1, .15
    if off in ("maxPerPixelError", "all"):
        mpe = 0
    if off in ("validateRtoL", "all"):
        rtol = -1
    if off in ("texture", "all"):
        tex = 0.0
    return mpe, rtol, tex


@functools.lru_cache(maxsize=None)
def scene(W, H, minD, rng, seed=1):
    left, right = dr.stereo_scene(W, H, minD, rng, seed)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def want(variant, W, H, minD, rng, rx, ry, mpe, rtol, tex, subpixel, seed=1):
    """-> (disparity, class map) of census_ref.block_match, read-only"""
    left, right = scene(W, H, minD, rng, seed)
    disp, cls = cr.block_match(left, right, variant, minD, rng, rx, ry, mpe, rtol, tex, subpixel)
    disp.setflags(write=False)
    cls.setflags(write=False)
    return disp, cls
