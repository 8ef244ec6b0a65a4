#!/usr/bin/env python3
"""Side measurement of the image remap (ImageDistort, bilinear + EXTENDED) on 64 device-resident 1920x1080 frames, GrayU8 and GrayF32
(bench.py is not involved).

Cases, per pixel type: the map form with one map shared by the batch (a rotation by 2 degrees about the centre with a 2 % zoom), the map
form with one map per image (the angle grows with the image), the homography model form (coordinates computed in the kernel, no map in
memory) and the rotation by 90 degrees (sx = y, sy = dw-1-x into a 1080x1920 destination: an exact permutation and the worst gather pattern).
Per case: ms per call (device events around REPS calls after WARM warm-up calls), the ctx profiler's ms per kernel, the byte floor -- map
bytes as they have to be read once (8 B per destination pixel, times the batch only for per-image maps) + one source element per pixel + the
output -- and the share of the 6.29 TB/s measured copy rate that the floor reaches over the kernel time.
bhip_sobel_dev_u8_s16 (k_sobel_u8) is timed on the same GrayU8 frames in the same run as the streaming yardstick.
A 256 x 64 block of the first destination of every case is checked against tests/distort_ref.py before anything is timed.  One JSON line per
case, printed and written to profiles/bench_distort.jsonl.  --counters CASE: one call of that case (0..3, GrayU8) only and nothing written
(for a counter run)."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd import _lib  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import distort_ref  # noqa: E402

COPY_RATE = 6.29e12   # bytes/s
B, W, H = 64, 1920, 1080
REPS, WARM = 5, 2
OUT = os.path.join(ROOT, "profiles", "bench_distort.jsonl")
HOMOGRAPHY = (1.01, 0.02, -12.0, -0.015, 0.99, 9.0, 4e-6, -6e-6, 1.0)
BILINEAR, EXTENDED = _lib.BHIP_INTERP_BILINEAR, _lib.BHIP_BORDER_EXTENDED


def rotation_maps(degrees):
    """[len(degrees), H, W, 2] float32 on the device"""
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    out = torch.empty((len(degrees), H, W, 2), dtype=torch.float32, device="cuda")
    for i, d in enumerate(degrees):
        c, s = 0.98 * math.cos(math.radians(d)), 0.98 * math.sin(math.radians(d))
        out[i, ..., 0] = c * (xs - cx) - s * (ys - cy) + cx
        out[i, ..., 1] = s * (xs - cx) + c * (ys - cy) + cy
    return out


def check_block(ops, frames, out, dmap_np_block, x0, y0):
    """out[0, y0:y0+64, x0:x0+256] against the reference on frame 0 with that block of the map"""
    src = frames[0].cpu().numpy()
    want, _, _ = distort_ref.distort(src, dmap_np_block, distort_ref.BILINEAR, distort_ref.EXTENDED, True, np.zeros(dmap_np_block.shape[:2], src.dtype))
    got = out[0, y0:y0 + 64, x0:x0 + 256].cpu().numpy()
    bits = (lambda a: a.view(np.uint32)) if src.dtype == np.float32 else (lambda a: a)
    if not np.array_equal(bits(np.ascontiguousarray(got)), bits(want)):
        raise SystemExit("the remap differs from tests/distort_ref.py")


def timed(ops, fn):
    for _ in range(WARM):
        fn()
    ops.ctx.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    stop.record()
    stop.synchronize()
    call_ms = start.elapsed_time(stop) / REPS
    ops.ctx.profile(True)
    ops.ctx.profileReset()
    for _ in range(REPS):
        fn()
    ops.ctx.synchronize()
    prof = ops.ctx.profileReport()
    ops.ctx.profile(False)
    return call_ms, {tag: round(v["ms"] / REPS, 4) for tag, v in prof.items()}


def main():
    counters = int(sys.argv[sys.argv.index("--counters") + 1]) if "--counters" in sys.argv else None
    ops = DeviceImageOps(device=0)
    gen = torch.Generator(device="cuda").manual_seed(23)
    u8 = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    f32 = (torch.rand((B, H, W), dtype=torch.float32, device="cuda", generator=gen) * 500 - 100)
    each = rotation_maps([2.0 + 0.05 * b for b in range(B)])
    shared = each[0].contiguous()
    ys, xs = torch.meshgrid(torch.arange(W, device="cuda", dtype=torch.float32), torch.arange(H, device="cuda", dtype=torch.float32), indexing="ij")
    rot90 = torch.stack([ys, (H - 1) - xs], -1).contiguous()      # destination H wide, W high: sx = y, sy = dw-1-x
    hmap = ops.distortBuildMap(_lib.BHIP_DISTORT_HOMOGRAPHY, HOMOGRAPHY, W, H)
    torch.cuda.synchronize()
    ops.ctx.synchronize()
    # (name, kwargs of ops.distort, destination (dh, dw), map bytes the floor counts, the map the check reads)
    cases = [("map, shared by the batch", dict(map=shared), (H, W), 8 * W * H, shared),
             ("map, one per image", dict(map=each), (H, W), 8 * W * H * B, each[0]),
             ("homography model", dict(model=_lib.BHIP_DISTORT_HOMOGRAPHY, coeff=HOMOGRAPHY), (H, W), 0, hmap),
             ("rotation by 90 degrees (map, shared)", dict(map=rot90), (W, H), 8 * W * H, rot90)]
    if counters is not None:
        name, kw, (dh, dw), _, _ = cases[counters]
        out = torch.empty((B, dh, dw), dtype=torch.uint8, device="cuda")
        ops.distort(u8, interp=BILINEAR, border=EXTENDED, out=out, **kw)
        ops.ctx.synchronize()
        print("one call of '%s' (GrayU8) done" % name, tuple(out.shape))
        return
    lines = []
    dx, dy = ops.sobel(u8, 0)
    sobel_ms, sobel_kernels = timed(ops, lambda: ops.sobel(u8, 0, dx, dy))
    lines.append({"op": "sobel u8 -> s16 (yardstick)", "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(sobel_ms, 4), "kernels_ms": sobel_kernels})
    for tname, frames in (("u8", u8), ("f32", f32)):
        size = frames.element_size()
        for name, kw, (dh, dw), map_bytes, cmap in cases:
            out = torch.empty((B, dh, dw), dtype=frames.dtype, device="cuda")
            ops.distort(frames, interp=BILINEAR, border=EXTENDED, out=out, **kw)
            ops.ctx.synchronize()
            x0, y0 = dw // 2 - 128, 8                   # a block that crosses the source's border in the rotated cases
            check_block(ops, frames, out, np.ascontiguousarray(cmap[y0:y0 + 64, x0:x0 + 256].cpu().numpy()), x0, y0)
            call_ms, kernels = timed(ops, lambda: ops.distort(frames, interp=BILINEAR, border=EXTENDED, out=out, **kw))
            kernel_ms = sum(kernels.values())
            floor_bytes = map_bytes + 2 * size * B * W * H
            lines.append({"op": "distort %s bilinear EXTENDED: %s" % (tname, name), "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(call_ms, 4),
                          "kernels_ms": kernels, "ms_per_frame": round(call_ms / B, 5), "byte_floor_bytes": floor_bytes,
                          "byte_floor_share_of_copy_rate": round(floor_bytes / (kernel_ms * 1e-3) / COPY_RATE, 4),
                          "ratio_to_sobel_u8": round(call_ms / sobel_ms, 2), "sobel_u8_ms": round(sobel_ms, 4), "checked_block": [x0, y0, x0 + 256, y0 + 64]})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
