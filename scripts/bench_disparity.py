#!/usr/bin/env python3
"""Side measurement of SAD block matching (FactoryStereoDisparity.blockMatch on GrayU8 pairs) on 64 device-resident 1920x1080 pairs
(bench.py is not involved).

Pairs: the left frames are Gaussian-blurred noise, the right frames the left ones shifted by a disparity that grows down the frame in
bands of 40 rows (8 .. 60 pixels), plus noise in [-3, 3].  Cases: the default ConfigDisparityBM (range 100, 7x7 region, sub-pixel GrayF32
output, right-to-left and texture checks), range 32, and range 253 with GrayU8 output.  Per case: ms per call (device events around REPS calls,
and the ctx profiler's ms per kernel), block comparisons per second (width * height * range * pairs over the call time) and the share of the
6.29 TB/s measured copy rate that the byte floor -- 2 B read + 1 or 4 B written per pixel -- reaches over the call time.
bhip_sobel_dev_u8_s16 (k_sobel_u8) is timed on the left frames in the same run as the streaming yardstick.
A 256 x 64 crop of one pair is checked against tests/disparity_ref.py before anything is timed.  One JSON line per case, printed and
written to profiles/bench_disparity.jsonl.  --counters: one call of the default case only and nothing written (for a counter run)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd import api  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import disparity_ref  # noqa: E402

COPY_RATE = 6.29e12   # bytes/s
B, W, H = 64, 1920, 1080
REPS, WARM = 5, 2
OUT = os.path.join(ROOT, "profiles", "bench_disparity.jsonl")


def make_pairs(ops):
    gen = torch.Generator(device="cuda").manual_seed(17)
    noise = torch.randint(0, 256, (B, H, W + 64), dtype=torch.uint8, device="cuda", generator=gen)
    scene = ops.gaussian(noise.float(), -1, 2)
    torch.cuda.synchronize()
    ops.ctx.synchronize()
    left = scene[:, :, :W].round().clamp(0, 255).to(torch.uint8).contiguous()
    right = torch.empty_like(left)
    for y0 in range(0, H, 40):
        d = 8 + 2 * (y0 // 40)      # right pixel x shows the left pixel x + d
        right[:, y0:y0 + 40] = scene[:, y0:y0 + 40, d:d + W].round().clamp(0, 255).to(torch.uint8)
    jitter = torch.randint(-3, 4, (B, H, W), dtype=torch.int16, device="cuda", generator=gen)
    right = (right.to(torch.int16) + jitter).clamp(0, 255).to(torch.uint8).contiguous()
    torch.cuda.synchronize()
    return left, right


def check_against_reference(ops, left, right, cfg, subpixel):
    l, r = left[:1, 500:564, 700:956].contiguous(), right[:1, 500:564, 700:956].contiguous()
    small = api.ConfigDisparityBM(**dict(cfg.__dict__, rangeDisparity=min(cfg.rangeDisparity, 200)))
    got = ops.disparityBM(l, r, small, subpixel=subpixel)
    ops.ctx.synchronize()
    want, cls = disparity_ref.block_match(l[0].cpu().numpy(), r[0].cpu().numpy(), small.minDisparity, small.rangeDisparity, small.regionRadiusX,
                                          small.regionRadiusY, small.maxPerPixelError, small.validateRtoL, small.texture, subpixel)
    g = got[0].cpu().numpy()
    if not np.array_equal(g.view(np.uint32) if subpixel else g, want.view(np.uint32) if subpixel else want):
        raise SystemExit("block matching differs from tests/disparity_ref.py")
    return dict(zip(disparity_ref.CLASS_NAMES, disparity_ref.class_counts(cls)))


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
    counters = "--counters" in sys.argv
    ops = DeviceImageOps(device=0)
    left, right = make_pairs(ops)
    cases = [("default: range 100, 7x7, sub-pixel F32", api.ConfigDisparityBM(), True),
             ("range 32, 7x7, sub-pixel F32", api.ConfigDisparityBM(rangeDisparity=32), True),
             ("range 253, 7x7, U8", api.ConfigDisparityBM(rangeDisparity=253, subpixel=False), False)]
    if counters:
        out = ops.disparityBM(left, right, cases[0][1], subpixel=True)
        ops.ctx.synchronize()
        print("one call of the default case done", tuple(out.shape))
        return
    lines = []
    dx, dy = ops.sobel(left, 0)
    sobel_ms, sobel_kernels = timed(ops, lambda: ops.sobel(left, 0, dx, dy))
    lines.append({"op": "sobel u8 -> s16 (yardstick)", "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(sobel_ms, 4), "kernels_ms": sobel_kernels})
    for name, cfg, subpixel in cases:
        classes = check_against_reference(ops, left, right, cfg, subpixel)
        out = torch.empty((B, H, W), dtype=torch.float32 if subpixel else torch.uint8, device="cuda")
        call_ms, kernels = timed(ops, lambda: ops.disparityBM(left, right, cfg, subpixel=subpixel, out=out))
        floor_bytes = (2 + (4 if subpixel else 1)) * B * W * H
        lines.append({"op": "blockMatch SAD u8: " + name, "pairs": "%d x %dx%d" % (B, W, H), "call_ms": round(call_ms, 3), "ms_per_pair": round(call_ms / B, 4),
                      "kernels_ms": kernels, "block_comparisons_per_s": float("%.4g" % (B * W * H * cfg.rangeDisparity / (call_ms * 1e-3))),
                      "byte_floor_bytes": floor_bytes, "byte_floor_share_of_copy_rate": round(floor_bytes / (call_ms * 1e-3) / COPY_RATE, 5),
                      "ratio_to_sobel_u8": round(call_ms / sobel_ms, 1), "sobel_u8_ms": round(sobel_ms, 4), "checked_crop_classes": classes})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
