"""The inputs of the Hough tests, shared by tests/test_hough_reference.py (CPU: the order sensitivity of these very inputs) and
tests/test_gpu_hough.py.  numpy only; every array is cached and read-only.

Sizes (width, height): 61x47 (odd both ways), 64x32 (one wave wide, one tile high), 2x3 and 3x2 (no inner pixel), 130x70 (wider than a
64-lane row and taller than a 32-row tile, so tile edges are crossed).  Every case is a batch of 3 images with different content."""
import functools

import numpy as np

SIZES = ((61, 47), (64, 32), (2, 3), (3, 2), (130, 70))
LARGE = ((61, 47), (64, 32), (130, 70))
GRADIENT_CASES = ("noise100", "noise10", "column47", "extremes", "s16")
DENSITIES = (0.05, 0.5, 1.0)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def binary_frames(w, h):
    """uint8 [3,h,w]: 5 %, 50 % and 100 % foreground; non-zero pixels are not all 1 (the vote tests != 0)"""
    rng = np.random.RandomState(7000 + 100 * w + h)
    f = np.stack([((rng.rand(h, w) < d) * rng.randint(1, 256, (h, w))).astype(np.uint8) for d in DENSITIES])
    return _ro(f)


@functools.lru_cache(maxsize=None)
def gray_frames(w, h, dtype="u8"):
    """[3,h,w] noise images for the gradient and edge stages: uint8, or float32 with a fractional part"""
    rng = np.random.RandomState(8000 + 100 * w + h)
    if dtype == "u8":
        return _ro(rng.randint(0, 256, (3, h, w)).astype(np.uint8))
    return _ro((rng.rand(3, h, w) * 255.0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def gradient_case(name, w, h):
    """-> (derivX [3,h,w], derivY, binary uint8 [3,h,w]); float32 derivatives but for "s16" (int16)
      noise100   noise gradients, every pixel an edge pixel
      noise10    the same gradients on a 10 % binary image
      column47   one column of edge pixels over the whole height with derivX near 20 and a small noisy derivY: the feet of its normals
                 fall on a few cells, which get many ordered contributions (47 at 61x47)
      extremes   gradients of 1e-30 (the squares underflow: division by zero, saturation at Integer.MAX_VALUE, x0+1 wraps), zero
                 gradients (0/0: NaN -> cell (0,0) with NaN weights) and a few ordinary ones
      s16        int16 noise gradients, every pixel an edge pixel"""
    rng = np.random.RandomState(9000 + 100 * w + h + 17 * GRADIENT_CASES.index(name))
    if name == "s16":
        dx = rng.randint(-300, 301, (3, h, w)).astype(np.int16)
        dy = rng.randint(-300, 301, (3, h, w)).astype(np.int16)
        return _ro(dx, dy, np.ones((3, h, w), np.uint8))
    dx = ((rng.rand(3, h, w) - 0.5) * 80.0).astype(np.float32)
    dy = ((rng.rand(3, h, w) - 0.5) * 80.0).astype(np.float32)
    if name == "noise100":
        binary = np.ones((3, h, w), np.uint8)
    elif name == "noise10":
        binary = (rng.rand(3, h, w) < 0.1).astype(np.uint8) * 255
    elif name == "column47":
        binary = np.zeros((3, h, w), np.uint8)
        for b in range(3):
            x = min(w - 1, 1 + 2 * b + w // 12)
            binary[b, :, x] = 1
            dx[b, :, x] = np.float32(20.0) + ((rng.rand(h) - 0.5) * 0.5).astype(np.float32)
            dy[b, :, x] = ((rng.rand(h) - 0.5) * 0.5).astype(np.float32)
    elif name == "extremes":
        binary = np.ones((3, h, w), np.uint8)
        kind = rng.randint(0, 4, (3, h, w))
        sign = np.where(rng.rand(3, h, w) < 0.5, -1.0, 1.0).astype(np.float32)
        dx = np.where(kind == 0, np.float32(1e-30) * sign, np.where(kind == 1, np.float32(0), dx)).astype(np.float32)
        dy = np.where(kind == 0, np.float32(1e-30), np.where(kind == 1, np.float32(0), dy)).astype(np.float32)
    else:
        raise ValueError(name)
    return _ro(dx, dy, binary)


@functools.lru_cache(maxsize=None)
def scene(kind, w=120, h=90):
    """A synthetic scene of three lines plus noise.  "dark": uint8, dark one-pixel lines on a bright noisy ground (the binary detector's
    GLOBAL_OTSU marks the dark pixels); "bars": three bright bars on a dark noisy ground, uint8 or float32 (the gradient detector finds
    their edges)."""
    rng = np.random.RandomState(4242)
    ys, xs = np.mgrid[0:h, 0:w]
    lines = ((0.0, 1.0, -30.0), (1.0, 0.0, -45.0), (0.6, 0.8, -70.0))   # a*x + b*y + c = 0 with a^2 + b^2 = 1
    if kind == "dark":
        img = 190.0 + rng.rand(h, w) * 40.0
        for a, b, c in lines:
            img[np.abs(a * xs + b * ys + c) < 0.6] = 20.0
        img[rng.rand(h, w) < 0.01] = 10.0
        return _ro(img.astype(np.uint8))
    img = 30.0 + rng.rand(h, w) * 6.0
    for a, b, c in lines:
        img[np.abs(a * xs + b * ys + c) < 3.0] = 200.0
    return _ro(img.astype(np.uint8) if kind == "bars_u8" else (img + 0.25).astype(np.float32))
