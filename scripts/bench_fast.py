#!/usr/bin/env python3
"""Side measurement of the FAST corner detector on 64 device-resident 1920x1080 GrayU8 frames (bench.py is not involved).

Two frame sets: uniform noise (about 20 % of the pixels are FAST-9 corners at tol 20, so the default maxFeaturesFraction 0.1 stops the
detector early) and Gaussian-blurred noise (few corners).  Per set: FAST-9 at tol 20 with the intensity image, and FAST-9 followed by
the strict MinMax block NMS at radius 2 -- ctx-profiler ms per kernel and batch, modelled bytes (the ProfScope figure) and the share of
the 6.29 TB/s measured copy rate that bytes / ms reaches.  bhip_sobel_dev_u8_s16 (k_sobel_u8 moves the same 1 B in / 4 B out
per pixel) is timed in the same run as the yardstick; the ratio fast_intensity_ms / sobel_u8_ms is part of every FAST line.
One frame of each set is checked against tests/fast_ref.py before anything is timed.  One JSON line per case, printed and written to
profiles/bench_fast.jsonl."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import fast_ref  # noqa: E402

COPY_RATE = 6.29e12   # bytes/s
B, W, H = 64, 1920, 1080
REPS, WARM = 10, 3
TOL, N, FRACTION, NMS_RADIUS = 20, 9, 0.1, 2
OUT = os.path.join(ROOT, "profiles", "bench_fast.jsonl")


def profiled(ops, fn):
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
        ms, by = v["ms"] / REPS, v["bytes"] / REPS
        kernels[tag] = {"ms": round(ms, 4), "bytes": int(by), "share_of_copy_rate": round(by / (ms * 1e-3) / COPY_RATE, 3) if ms > 0 and by > 0 else None}
    return kernels


def check_against_reference(ops, frames, name):
    inten, xyLow, nLow, xyHigh, nHigh = ops.fast(frames[:1], TOL, N, FRACTION)
    ops.ctx.synchronize()
    want = fast_ref.fast(frames[0].cpu().numpy(), TOL, N, FRACTION)
    nl, nh = int(nLow[0]), int(nHigh[0])
    ok = (np.array_equal(inten[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32)) and np.array_equal(xyLow[0, :nl].cpu().numpy(), want[1]) and
          np.array_equal(xyHigh[0, :nh].cpu().numpy(), want[2]))
    if not ok:
        raise SystemExit("FAST on the %s set differs from tests/fast_ref.py" % name)
    return nl, nh, want[3]


def main():
    ops = DeviceImageOps(device=0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    noise = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    blurred = ops.gaussian(noise.float(), -1, 4)
    torch.cuda.synchronize()
    ops.ctx.synchronize()
    blurred = blurred.round().clamp(0, 255).to(torch.uint8)
    dx, dy = ops.sobel(noise, 0)
    inten = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    lines = []

    sobel = profiled(ops, lambda: ops.sobel(noise, 0, dx, dy))
    sobel_ms = sobel["k_sobel_u8"]["ms"]
    lines.append({"op": "sobel u8 -> s16 (yardstick)", "frames": "%d x %dx%d" % (B, W, H), "kernels": sobel})

    for name, frames in (("uniform noise", noise), ("blurred noise", blurred)):
        nl, nh, stop = check_against_reference(ops, frames, name)
        cap = int(FRACTION * W * H) + W
        fast = profiled(ops, lambda: ops.fast(frames, TOL, N, FRACTION, inten, cap))

        def chain():
            ops.fast(frames, TOL, N, FRACTION, inten, cap)
            return ops.nonmaxMinMax(inten, NMS_RADIUS, -1.0, 1.0, 3)

        both = profiled(ops, chain)
        fast_ms = fast["k_fast_u8"]["ms"]
        common = {"frames": "%d x %dx%d %s" % (B, W, H, name), "frame0": {"low": nl, "high": nh, "stop_row": stop}, "sobel_u8_ms": sobel_ms}
        lines.append(dict(common, op="FAST-%d tol %d with intensity" % (N, TOL), kernels=fast, fast_intensity_ms=fast_ms,
                          ratio_fast_to_sobel=round(fast_ms / sobel_ms, 2), total_ms=round(sum(k["ms"] for k in fast.values()), 4)))
        lines.append(dict(common, op="FAST-%d tol %d + MinMax NMS r=%d" % (N, TOL, NMS_RADIUS), kernels=both,
                          total_ms=round(sum(k["ms"] for k in both.values()), 4)))

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
