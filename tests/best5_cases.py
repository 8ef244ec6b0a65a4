"""The five-region block-matching cases that tests/test_gpu_best5.py and tests/test_gpu_best5_census.py run on the GPU and
tests/test_best5_reference.py checks for non-vacuity on the CPU: scenes and reference outputs, computed once per process and read-only.

The kernel's tile (boofcv_amd/csrc/disparity.hip): DISP5_TW = 32 selector columns; DISP5_TH = 16 output rows for 1-byte elements (SAD, census
3x3), DISP5_ROWS_W32 - 4*regionRadiusY = 32 - 4*ry rows for the 4-byte census words.  A range above 128 runs the wide-slab instantiation."""
import functools

import numpy as np

import best5_ref as b5
import census_cases as cc
import disparity_ref as dr

TILE_W, TILE_H, ROWS_W32 = 32, 16, 32
RANGE_SPLIT = 128     # range <= 128: the narrow slab; above: the wide one

# W, H, minD, range, rx, ry, maxPerPixelError, validateRtoL, texture, outputs ("f32", "u8"), binarise the pair
SAD_CASES = [
    (50, 60, 0, 20, 3, 3, 0, 1, .15, ("f32", "u8"), False),
    (67, 25, 2, 30, 2, 1, 25, 1, .15, ("f32", "u8"), False),
    (131, 23, 0, 100, 3, 2, 30, 1, .15, ("f32", "u8"), False),
    (150, 33, 5, 120, 4, 3, 30, 0, .1, ("f32", "u8"), False),
    (96, 36, 0, 60, 7, 7, 0, 1, .15, ("f32", "u8"), False),      # the largest region
    (96, 36, 0, 60, 7, 7, 0, 1, .15, ("f32", "u8"), True),       # its scores pass 65535
    (200, 44, 0, 50, 2, 2, 20, 1, .15, ("f32", "u8"), False),    # several column tiles and row bands
    (44, 9, 1, 20, 0, 0, 0, 1, .15, ("f32", "u8"), False),       # radius 0
    (40, 9, 0, 2, 1, 1, 0, 1, .15, ("f32", "u8"), False),        # texture never applies (lm < 3)
    (300, 13, 0, 253, 2, 1, 0, 1, .15, ("f32", "u8"), False),    # the GrayU8 ceiling; the wide slab
    (20, 20, 5, 7, 4, 1, 0, 1, .15, ("f32", "u8"), False),       # legal, no selector column: W - (4*rx+1) = 3 < minD
    (40, 9, 0, 10, 1, 3, 0, 1, .15, ("f32", "u8"), False),       # legal, rh <= H < 4*ry + 1: no output row
    # W and H one short of, at and one past the tile: selector columns W - 4*rx - minD = TILE_W - 1, TILE_W, TILE_W + 1 with rx = 1, minD = 0,
    # output rows H - 4*ry = TILE_H - 1, TILE_H, TILE_H + 1 with ry = 1; the range straddles RANGE_SPLIT on the last two
    (TILE_W + 3, TILE_H + 3, 0, 12, 1, 1, 0, 1, .15, ("f32",), False),
    (TILE_W + 4, TILE_H + 4, 0, 12, 1, 1, 0, 1, .15, ("f32",), False),
    (TILE_W + 5, TILE_H + 5, 0, 12, 1, 1, 0, 1, .15, ("f32",), False),
    (140, 9, 0, RANGE_SPLIT, 1, 1, 0, 1, .15, ("f32",), False),
    (140, 9, 0, RANGE_SPLIT + 1, 1, 1, 0, 1, .15, ("f32",), False),
]


def case_id(c):
    return "%dx%d_min%d_range%d_r%dx%d%s" % (c[:6] + ("_bin" if c[10] else "",))


def binarise(img):
    return np.where(img >= 128, 255, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(W, H, minD, rng, seed=1, binary=False):
    left, right = dr.stereo_scene(W, H, minD, rng, seed)
    if binary:
        left, right = binarise(left), binarise(right)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def want(W, H, minD, rng, rx, ry, mpe, rtol, tex, subpixel, seed=1, binary=False, variant=None):
    """-> (disparity, class map) of best5_ref.block_match_best5, read-only"""
    left, right = scene(W, H, minD, rng, seed, binary)
    disp, cls = b5.block_match_best5(left, right, minD, rng, rx, ry, mpe, rtol, tex, subpixel, variant)
    disp.setflags(write=False)
    cls.setflags(write=False)
    return disp, cls


# census: name, W, H, minD, range, rx, ry, maxPerPixelError as a multiple of census_cases.MPE[variant], validateRtoL, texture
CENSUS_VARIANTS = cc.BM_VARIANTS
CENSUS_CASES = [
    ("range100", 131, 23, 0, 100, 3, 2, 1.0, 1, .15),
    ("radius7", 96, 36, 0, 60, 7, 7, 0, 1, .15),               # the 4-byte geometry at its smallest band: 32 - 28 = 4 output rows, two bands
    ("multi_tile", 110, 40, 2, 30, 2, 1, 1.0, 1, .15),         # four column tiles; 36 output rows: three bands of 16, two of 28
]


def census_params(case, variant):
    _, W, H, minD, rng, rx, ry, mpe, rtol, tex = case
    return (minD, rng, rx, ry, cc.MPE[variant] * mpe, rtol, tex)
