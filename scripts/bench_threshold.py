#!/usr/bin/env python3
"""Side measurement of the thresholding family (FactoryThresholdBinary.threshold) on 64 device-resident 1920x1080 frames, GrayU8 and GrayF32
(bench.py is not involved).

One case per (ThresholdType, image type) the library implements, with the reference's default configuration of that type (width 11: radius 5 for
the local forms, blocks of about 11 x 11) and additionally the local GrayU8 forms at width 35 (radius 17, the two-pass path beyond the fused
kernel).  Per case: ms per call (device events around REPS calls after WARM warm-up calls), the ctx profiler's ms per kernel, the bytes the kernels
actually move -- `traffic_bytes`, spelled out per case in traffic() below: one read of the input and one write of the 0/1 byte where the form
allows it (2 B/px GrayU8, 5 B/px GrayF32), plus every further pass over the image, the tile halo of the fused kernel and the block statistics;
never the reference's pass count -- the GB/s that is over the kernel time, and its share of the copy ceiling.  The ceiling is measured in the same
run: a device-to-device copy of the GrayF32 batch (read + write bytes over the event time).
A 640 x 360 crop of the first frame goes through the same entry point and is compared with tests/threshold_ref.py before a case is timed.
One JSON line per case, printed and written to profiles/bench_threshold.jsonl."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd import api, binary  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import threshold_ref  # noqa: E402

B, W, H = 64, 1920, 1080
REPS, WARM = 5, 2
OUT = os.path.join(ROOT, "profiles", "bench_threshold.jsonl")
T = binary.ThresholdType
P = B * W * H


def traffic(t, size, width, kernels):
    """bytes the kernels of one call move (size: bytes per input pixel; kernels: the profiler's tags of the call)"""
    radius = width // 2
    if t == T.FIXED:
        return (size + 1) * P
    if t == T.GLOBAL_OTSU:                       # histogram pass + apply pass
        return (2 * size + 1) * P
    if t in (T.LOCAL_MEAN, T.LOCAL_GAUSSIAN):
        if size == 1 and radius <= 16:           # fused: the 64 x 32 tile with its halo is read once, the byte written once
            return int(P * (64 + 2 * radius) * (32 + 2 * radius) / (64.0 * 32.0)) + P
        if size == 1:                            # two blur passes (read + write each) and the compare (two reads, one write)
            return (2 + 2 + 3) * P
        if "k_blur_fused" in kernels:            # GrayF32 Gaussian in one fused pass: one read and one write of the image (halo from cache), then the compare
            return (8 + 9) * P
        return (8 + 8 + 9) * P                   # GrayF32: two blur passes (read + write each) and the compare (two reads, one write)
    blocks = B * (W // width) * (H // width)     # about; the exact grid is within a block of it
    stats = {T.BLOCK_MIN_MAX: 8, T.BLOCK_MEAN: 4, T.BLOCK_OTSU: 1024}[t]
    # statistics pass + statistics written and read once + records + apply pass.  Stage 2 reads every block's statistics nine times (the 3 x 3
    # neighbourhoods overlap); eight of the nine are cache hits and are not counted as traffic -- for Otsu they are 8 KiB per block of L2 reads.
    return size * P + blocks * stats * 2 + 8 * blocks + (size + 1) * P


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


def config(t, width):
    if t == T.FIXED:
        return binary.ConfigThreshold.fixed(120)
    return binary.ConfigThreshold.global_(t) if t.isGlobal() else binary.ConfigThreshold.local(t, width)


def check(ops, frames, cfg):
    """a 640 x 360 crop of frame 0 through the same entry point against tests/threshold_ref.py"""
    crop = frames[:1, :360, :640]
    got = ops.threshold(crop, cfg).cpu().numpy()[0]
    img = np.ascontiguousarray(crop[0].cpu().numpy())
    kernel = None
    if cfg.type == T.LOCAL_GAUSSIAN and img.dtype == np.float32:
        kernel = api.FactoryKernelGaussian.gaussian1D_F32(-1, threshold_ref.local_radius(img, cfg.width.length, cfg.width.fraction)).data
    if not np.array_equal(got, threshold_ref.threshold_config(img, cfg, kernel)):
        raise SystemExit("%s differs from tests/threshold_ref.py" % cfg.type.name)


def main():
    ops = DeviceImageOps(device=0)
    gen = torch.Generator(device="cuda").manual_seed(29)
    u8 = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    f32 = torch.rand((B, H, W), dtype=torch.float32, device="cuda", generator=gen) * 255
    out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    copy = torch.empty_like(f32)
    torch.cuda.synchronize()
    # the copy ceiling of this run: read + write of the GrayF32 batch
    for _ in range(WARM):
        copy.copy_(f32)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(REPS):
        copy.copy_(f32)
    stop.record()
    stop.synchronize()
    copy_ms = start.elapsed_time(stop) / REPS
    copy_rate = 8.0 * P / (copy_ms * 1e-3)
    lines = [{"op": "device copy f32 (the ceiling)", "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(copy_ms, 4), "GBps": round(copy_rate / 1e9, 1)}]
    cases = [(t, torch.uint8, 11) for t in (T.FIXED, T.GLOBAL_OTSU, T.LOCAL_MEAN, T.LOCAL_GAUSSIAN, T.BLOCK_MIN_MAX, T.BLOCK_MEAN, T.BLOCK_OTSU)]
    cases += [(T.LOCAL_MEAN, torch.uint8, 35), (T.LOCAL_GAUSSIAN, torch.uint8, 35)]
    cases += [(t, torch.float32, 11) for t in (T.FIXED, T.LOCAL_MEAN, T.LOCAL_GAUSSIAN, T.BLOCK_MIN_MAX, T.BLOCK_MEAN)]
    for t, dtype, width in cases:
        frames = u8 if dtype == torch.uint8 else f32
        size = frames.element_size()
        cfg = config(t, width)
        check(ops, frames, cfg)
        call_ms, kernels = timed(ops, lambda: ops.threshold(frames, cfg, out=out))
        kernel_ms = sum(kernels.values())
        moved = traffic(t, size, width, kernels)
        rate = moved / (kernel_ms * 1e-3)
        lines.append({"op": "threshold %s %s width %d" % (t.name, "u8" if size == 1 else "f32", width), "frames": "%d x %dx%d" % (B, W, H),
                      "call_ms": round(call_ms, 4), "kernels_ms": kernels, "ms_per_frame": round(call_ms / B, 5), "traffic_bytes": moved,
                      "bytes_per_pixel": round(moved / P, 3), "GBps": round(rate / 1e9, 1), "share_of_copy_rate": round(rate / copy_rate, 4),
                      "ideal_bytes_per_pixel": size + 1, "ideal_ms_at_copy_rate": round((size + 1) * P / copy_rate * 1e3, 4)})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
