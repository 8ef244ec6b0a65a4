#!/usr/bin/env python3
"""Side measurement of the stationary background models on 64 device-resident 1920x1080 streams (bench.py is not involved).

Cases: Basic, Gaussian and GMM (the default configs; thresholds 10 / 12), GrayU8 and 3-band Planar<GrayU8> frames, T = 1 and T = 8 frames
per update() call, masks written.  Every model is first fed 3 frames so that it is initialised and the mixtures hold more than one Gaussian.
Per case: ms per call (device events around REPS calls after WARM warm-up calls) and per frame step (one frame of all 64 streams), the bytes of
one call by the kernel's own accounting (model read once and written once, every frame read, every mask written: bhip_bg_bytes, reported by
the ctx profiler), the bytes per frame step and their share of the 6.3 TB/s float4-copy rate over the kernel time.  A 64 x 16 block of stream
0's masks is checked against tests/background_ref.py first (pixels are independent, so the block is a model of its own).  One JSON line per
case, printed and written to profiles/bench_background.jsonl."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd import api  # noqa: E402
from boofcv_amd.device import DeviceBackgroundModel  # noqa: E402
import background_ref as bref  # noqa: E402

COPY_RATE = 6.3e12   # bytes/s
S, W, H = 64, 1920, 1080
REPS, WARM = 3, 1
OUT = os.path.join(ROOT, "profiles", "bench_background.jsonl")


def frames_like(gen, T, bands):
    """[S, T, (bands,) H, W] uint8: three levels with +-8 of noise, the level of a pixel changing from frame to frame now and then"""
    shape = (S, T, H, W) if bands == 0 else (S, T, bands, H, W)
    lshape = (S, T, H, W) if bands == 0 else (S, T, 1, H, W)
    level = torch.randint(0, 8, lshape, device="cuda", generator=gen, dtype=torch.int16)
    level = torch.clamp(level - 5, min=0) * 80 + 40                    # mostly level 0
    noise = torch.randint(-8, 9, shape, device="cuda", generator=gen, dtype=torch.int16)
    return (level + noise).clamp(0, 255).to(torch.uint8)


def configs():
    return [("basic", api.ConfigBackgroundBasic(10.0)), ("gaussian", api.ConfigBackgroundGaussian(12.0)), ("gmm", api.ConfigBackgroundGmm())]


def reference(alg, cfg, bands):
    if alg == "basic":
        return bref.stationaryBasic(cfg.learnRate, cfg.threshold, bands)
    if alg == "gaussian":
        return bref.stationaryGaussian(cfg.learnRate, cfg.threshold, bands)
    return bref.stationaryGmm(bands)


def check_block(alg, cfg, bands, history, masks):
    """masks [S,T,H,W] of the last call against the reference fed the same block of every frame so far"""
    x0, y0 = W // 2 - 32, 8
    ref = reference(alg, cfg, bands)
    blocks = [f[0, :, ..., y0:y0 + 16, x0:x0 + 64].cpu().numpy() for f in history]
    for b in blocks[:-1]:
        for t in range(b.shape[0]):
            ref.updateBackground(b[t])
    want = np.stack([ref.updateBackground(blocks[-1][t], True) for t in range(blocks[-1].shape[0])])
    got = masks[0, :, y0:y0 + 16, x0:x0 + 64].cpu().numpy()
    if not np.array_equal(got, want):
        raise SystemExit("%s: the masks differ from tests/background_ref.py" % alg)


def main():
    ctx = api.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(31)
    lines = []
    for bands in (0, 3):
        warm = frames_like(gen, 3, bands)
        for T in (1, 8):
            fr = frames_like(gen, T, bands)
            masks = torch.empty((S, T, H, W), dtype=torch.uint8, device="cuda")
            for alg, cfg in configs():
                bg = DeviceBackgroundModel(alg, cfg, torch.uint8, bands, ctx=ctx)
                bg.update(warm)
                bg.update(fr, masks)
                ctx.synchronize()
                check_block(alg, cfg, bands, [warm, fr], masks)
                for _ in range(WARM):
                    bg.update(fr, masks)
                ctx.synchronize()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(REPS):
                    bg.update(fr, masks)
                stop.record()
                stop.synchronize()
                call_ms = start.elapsed_time(stop) / REPS
                ctx.profile(True)
                ctx.profileReset()
                for _ in range(REPS):
                    bg.update(fr, masks)
                ctx.synchronize()
                prof = ctx.profileReport()
                ctx.profile(False)
                kernel_ms = sum(v["ms"] for v in prof.values()) / REPS
                call_bytes = sum(v["bytes"] for v in prof.values()) / REPS
                lines.append({"op": "background %s update+mask" % alg, "frames": "%d streams x %dx%d, %s" % (S, W, H, "GrayU8" if bands == 0 else "Planar<GrayU8> x %d" % bands),
                              "T": T, "call_ms": round(call_ms, 4), "kernel_ms": round(kernel_ms, 4), "ms_per_frame_step": round(call_ms / T, 4),
                              "ms_per_frame": round(call_ms / T / S, 6), "bytes_per_call": call_bytes, "bytes_per_frame_step": call_bytes / T,
                              "share_of_copy_rate": round(call_bytes / (kernel_ms * 1e-3) / COPY_RATE, 4), "checked_block": [W // 2 - 32, 8, W // 2 + 32, 24]})
                print(json.dumps(lines[-1]), flush=True)
                bg.close()
            del fr, masks
        del warm
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
