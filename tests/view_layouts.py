"""Output views with guard bands, for the tests of the device image ops (tests/test_gpu_device_views.py; self-test: tests/test_view_layouts.py).

A launcher of include/boofhip.h takes an image as (pointer, imageStride, rowStride): a [B,H,W] window into a larger buffer.  make_view() builds
such a window inside a 1-D parent filled with a bit pattern no result can have, so a store outside the window -- past a row's end, before its
start, into the rows between two images, above the first or below the last -- is found by comparing the parent's bits before and after.
Everything takes a `device`, so the same code runs on torch CPU tensors.

Layouts (strides in elements; `lead` = elements in front of row 0 of image 0, a multiple of 16 so that it is 16-byte aligned for every dtype):

  dense     pitch W, images H*W apart: the control case (guards in front of the first and behind the last image only)
  pad4      pitch roundup4(W)+8, x0 = 0, images pitch*(H+2) apart (2 guard rows between them): base, pitch and image stride allow 16-byte
            vector accesses on float32
  pad4_x4   pad4 with x0 = 4: still so, with guard pixels on the left as well
  pad4_x1   pad4 with x0 = 1: pitch and image stride are multiples of 4 but the base is one element past a 16-byte boundary (int16: rows
            start 2-byte but not 4-byte aligned)
  odd       pitch W+3, x0 = 2, images pitch*(H+2)+1 apart: nothing is aligned
"""
import numpy as np
import torch

LAYOUTS = ("dense", "pad4", "pad4_x4", "pad4_x1", "odd")
GUARD_ROWS = 2      # full rows of the parent above the first and below the last image
GUARD_ELEMS = 64    # elements at either end of the parent, at least

# one fixed quiet-NaN payload / patterns that are no value of an image op (int16: 0xAA55 as a signed short)
SENTINEL = {torch.float32: 0x7FC5A5A5, torch.uint8: 0xA5, torch.int16: 0xAA55 - 0x10000, torch.int32: 0x5A5AA5A5}


def geometry(layout, B, H, W):
    """-> (offset of pixel (0,0) of image 0, image stride, pitch, elements of the parent)"""
    r4 = (W + 3) // 4 * 4
    if layout == "dense":
        pitch, x0, image = W, 0, H * W
    elif layout in ("pad4", "pad4_x4", "pad4_x1"):
        pitch, x0 = r4 + 8, {"pad4": 0, "pad4_x4": 4, "pad4_x1": 1}[layout]
        image = pitch * (H + GUARD_ROWS)
    elif layout == "odd":
        pitch, x0 = W + 3, 2
        image = pitch * (H + GUARD_ROWS) + 1
    else:
        raise ValueError("unknown layout " + layout)
    guard = max(GUARD_ELEMS, GUARD_ROWS * pitch)
    lead = (guard + 15) // 16 * 16
    offset = lead + x0
    total = offset + (B - 1) * image + H * pitch + guard
    return offset, image, pitch, total


def bits(t):
    """the elements as integers: float32 -> int32 bit patterns, integer types as they are (a contiguous tensor of t's shape)"""
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def sentinel_buffer(n, dtype, device):
    if dtype == torch.float32:
        return torch.full((n,), SENTINEL[dtype], dtype=torch.int32, device=device).view(torch.float32)
    return torch.full((n,), SENTINEL[dtype], dtype=dtype, device=device)


def make_view(layout, B, H, W, dtype, device, shift=0):
    """-> (parent, view): a 1-D sentinel-filled parent and the [B,H,W] torch.as_strided window of `layout` into it.  shift moves the window
    by that many elements (a derivY whose base is not aligned like its derivX; |shift| <= 16 stays inside the guards)."""
    offset, image, pitch, total = geometry(layout, B, H, W)
    assert abs(shift) <= 16
    parent = sentinel_buffer(total + 16, dtype, device)
    view = torch.as_strided(parent, (B, H, W), (image, pitch, 1), offset + shift)
    return parent, view


def snapshot(parent):
    """the parent's bits, to be handed to assert_only_view_written after the op"""
    return bits(parent).clone()


def inside_mask(parent, view):
    """bool [parent.numel()]: True on the elements of the view"""
    m = torch.zeros(parent.numel(), dtype=torch.bool, device=parent.device)
    torch.as_strided(m, tuple(view.shape), tuple(view.stride()), view.storage_offset() - parent.storage_offset()).fill_(True)
    return m


def assert_only_view_written(parent, view, before_bits, what=""):
    """every element of `parent` outside `view` is bit-identical to before_bits"""
    now = bits(parent)
    assert now.shape == before_bits.shape and now.dtype == before_bits.dtype
    changed = (now != before_bits) & ~inside_mask(parent, view)
    if bool(changed.any()):
        idx = torch.nonzero(changed).flatten()[:8].cpu().numpy()
        off = view.storage_offset() - parent.storage_offset()
        image, pitch = view.stride(0), view.stride(1)
        where = []
        for i in idx:   # (image, row, column) relative to the view; a column outside [0, W) or a row outside [0, H) names the guard
            r = int(i) - off
            b = min(max(r // image, 0), view.shape[0] - 1)
            r -= b * image
            where.append((b, r // pitch, r % pitch))
        raise AssertionError("%s: %d elements outside the view were written; first (image, row, column): %s" % (what, int(changed.sum()), where))


def assert_kept(view, mask, what=""):
    """the masked elements of the view ([H,W] or [B,H,W] bool) still hold the sentinel: the frame a no-border op must not write"""
    m = torch.as_tensor(np.asarray(mask, bool), device=view.device)
    m = m.expand(view.shape)
    got = bits(view)[m]
    bad = got != SENTINEL[view.dtype]
    assert not bool(bad.any()), "%s: %d frame elements of the view were written" % (what, int(bad.sum()))
