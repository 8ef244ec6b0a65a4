#!/usr/bin/env python3
"""Side measurement of the corner front end on 64 device-resident 1920x1080 frames (bench.py is not involved).

For each kernel: ctx-profiler ms per batch, modelled bytes (the ProfScope figure) and the share of the 6.29 TB/s measured copy rate
 that bytes / ms reaches.  Then the full GrayU8 chain (Sobel U8 -> box S16 Shi-Tomasi r=2 -> nonmax_block_dev) next to the
GrayF32 chain (Sobel F32 -> k_corner_rows / k_corner_cols -> nonmax_block_dev) on the same frames, timed with HIP events.
Prints one JSON line per measurement."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boofcv_amd.device import DeviceImageOps  # noqa: E402

COPY_RATE = 6.29e12   # bytes/s
B, W, H = 64, 1920, 1080
REPS, WARM = 10, 3


def profiled(ops, name, fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ops.ctx.profile(True)
    ops.ctx.profileReset()
    for _ in range(REPS):
        fn()
    ops.ctx.synchronize()
    prof = ops.ctx.profileReport()
    ops.ctx.profile(False)
    kernels = {}
    for tag, v in prof.items():
        ms = v["ms"] / REPS
        by = v["bytes"] / REPS
        kernels[tag] = {"ms": round(ms, 4), "bytes": int(by), "share_of_copy_rate": round(by / (ms * 1e-3) / COPY_RATE, 3) if ms > 0 else None}
    print(json.dumps({"op": name, "frames": "%d x %dx%d" % (B, W, H), "kernels": kernels}), flush=True)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPS):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / REPS


def main():
    ops = DeviceImageOps(device=0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    u8 = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    f32 = u8.float()
    dx16, dy16 = ops.sobel(u8, 0)
    dxf, dyf = ops.sobel(f32, 0)
    inten = torch.empty((B, H, W), dtype=torch.float32, device="cuda")

    profiled(ops, "sobel u8 -> s16", lambda: ops.sobel(u8, 0, dx16, dy16))
    profiled(ops, "box s16 shi-tomasi r=2", lambda: ops.cornerIntensity(0, 2, 0.0, dx16, dy16, inten))
    profiled(ops, "weighted s16 shi-tomasi r=2", lambda: ops.cornerIntensity(0, 2, 0.0, dx16, dy16, inten, weighted=True))
    profiled(ops, "weighted f32 shi-tomasi r=2", lambda: ops.cornerIntensity(0, 2, 0.0, dxf, dyf, inten, weighted=True))

    def chain_u8():
        ops.sobel(u8, 0, dx16, dy16)
        ops.cornerIntensity(0, 2, 0.0, dx16, dy16, inten)
        return ops.nonmax(inten, 2, 1.0, 2, cap=4096)

    def chain_f32():
        ops.sobel(f32, 0, dxf, dyf)
        ops.cornerIntensity(0, 2, 0.0, dxf, dyf, inten)
        return ops.nonmax(inten, 2, 1.0, 2, cap=4096)

    profiled(ops, "chain u8: sobel u8 -> box s16 r=2 -> nonmax", chain_u8)
    profiled(ops, "chain f32: sobel f32 -> k_corner_rows/cols r=2 -> nonmax", chain_f32)
    mu, mf = timed(chain_u8), timed(chain_f32)
    print(json.dumps({"op": "chain wall time (HIP events, per batch)", "u8_ms": round(mu, 4), "f32_ms": round(mf, 4), "speedup": round(mf / mu, 2)}))


if __name__ == "__main__":
    main()
