#!/usr/bin/env python3
"""Side measurement of the image-enhancement family (EnhanceImageOps: the global chain histogram -> equalize table -> applyTransform,
equalizeLocal, sharpen4 / sharpen8) on 16 device-resident 1920x1080 frames (bench.py is not involved).

equalizeLocal is swept over the radii 1, 2, 4, 8, 12, 16, 24, 32, 50, 64, 80, 96, 108 with both forced paths (the direct count out of an LDS tile, the
sliding histogram) and with AUTO, which is how the crossover constant in cabi_enhance.hip (BHIP_EQLOCAL_SLIDING_MIN_RADIUS) was chosen and is
checked: per radius one more line says which forced path was faster, how AUTO compares with it and whether that is within the run-to-run
spread this script records.  Per case: TRIALS trials of REPS calls after WARM warm-up calls, device events around each trial; `call_ms` is the
median trial, `spread` = (slowest - fastest trial) / median.  Beside it the ctx profiler's ms per kernel, the bytes one read of the input and
one write of the output would move (`ideal_bytes`), the time a plain device copy needs for that many bytes AT THE COPY RATE MEASURED IN THIS
RUN, and `times_copy` = call_ms over that.  There is no pass / fail time: nobody had measured these kernels before this script.
A 640 x 360 crop of frame 0 goes through the same entry point and is compared with tests/enhance_ref.py before a case is timed (equalizeLocal:
a 96 x 64 crop, the reference being a Python loop).
One JSON line per case, printed and written to profiles/bench_enhance.jsonl (or to the path given as the first argument)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import enhance_ref as R  # noqa: E402

B, W, H = 16, 1920, 1080
REPS, WARM, TRIALS = 3, 1, 3
RADII = (1, 2, 4, 8, 12, 16, 24, 32, 50, 64, 80, 96, 108)   # 108: the largest radius whose direct tile fits LDS on a large image
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bench_enhance.jsonl")
P = B * W * H


def timed(ops, fn):
    for _ in range(WARM):
        fn()
    ops.ctx.synchronize()
    trials = []
    for _ in range(TRIALS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(REPS):
            fn()
        stop.record()
        stop.synchronize()
        trials.append(start.elapsed_time(stop) / REPS)
    trials.sort()
    ops.ctx.profile(True)
    ops.ctx.profileReset()
    fn()
    ops.ctx.synchronize()
    prof = ops.ctx.profileReport()
    ops.ctx.profile(False)
    med = trials[len(trials) // 2]
    return med, (trials[-1] - trials[0]) / med, {tag: round(v["ms"], 4) for tag, v in prof.items()}


def copy_rate(src):
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(10):
        dst.copy_(src)
    stop.record()
    stop.synchronize()
    ms = start.elapsed_time(stop) / 10
    return ms, 2.0 * src.numel() * src.element_size() / (ms * 1e-3)


def same(got, want, what):
    got = got.cpu().numpy()[0]
    bits = np.uint32 if got.dtype == np.float32 else got.dtype
    if not np.array_equal(got.view(bits), np.asarray(want).view(bits)):
        raise SystemExit("%s differs from tests/enhance_ref.py" % what)


def main():
    ops = DeviceImageOps(device=0)
    gen = torch.Generator(device="cuda").manual_seed(31)
    noise = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    frames = ops.gaussianU8(noise, 2)          # dim, correlated frames: what equalisation is run on
    frames = (frames // 2 + 20).contiguous()
    fframes = frames.float() + torch.rand((B, H, W), device="cuda", generator=gen)
    del noise
    out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    fout = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    u8_ms, u8_rate = copy_rate(frames)
    f32_ms, f32_rate = copy_rate(fframes)
    lines = [{"op": "device copy u8 (the yardstick)", "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(u8_ms, 4), "GBps": round(u8_rate / 1e9, 1)},
             {"op": "device copy f32", "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(f32_ms, 4), "GBps": round(f32_rate / 1e9, 1)}]
    for ln in lines:
        print(json.dumps(ln), flush=True)

    def case(name, fn, ideal_bytes, rate, extra=None):
        call_ms, spread, kernels = timed(ops, fn)
        copy_ms = ideal_bytes / rate * 1e3
        ln = {"op": name, "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(call_ms, 4), "spread": round(spread, 4), "ms_per_frame": round(call_ms / B, 5),
              "kernels_ms": kernels, "ideal_bytes": ideal_bytes, "copy_ms_same_bytes": round(copy_ms, 4), "times_copy": round(call_ms / copy_ms, 2)}
        ln.update(extra or {})
        lines.append(ln)
        print(json.dumps(ln), flush=True)
        return ln

    # ---- the global chain ----
    crop = frames[:1, :360, :640]
    c0 = np.ascontiguousarray(crop.cpu().numpy()[0])
    hist = ops.histogram(crop)
    table = ops.equalizeTable(hist)
    if not np.array_equal(hist.cpu().numpy()[0], R.histogram(c0, 0, 256)) or not np.array_equal(table.cpu().numpy()[0], R.equalize(R.histogram(c0, 0, 256))):
        raise SystemExit("histogram / table differ from tests/enhance_ref.py")
    same(ops.applyTransform(crop, table), R.applyTransform(c0, table.cpu().numpy()[0]), "applyTransform")
    hist = torch.empty((B, 256), dtype=torch.int32, device="cuda")
    table = torch.empty((B, 256), dtype=torch.int32, device="cuda")
    case("histogram", lambda: ops.histogram(frames, 0, 256, out=hist), P, u8_rate)
    case("equalizeTable", lambda: ops.equalizeTable(hist, out=table), 2 * 4 * 256 * B, u8_rate)
    case("applyTransform", lambda: ops.applyTransform(frames, table, out=out), 2 * P, u8_rate)

    def chain():
        ops.histogram(frames, 0, 256, out=hist)
        ops.equalizeTable(hist, out=table)
        ops.applyTransform(frames, table, out=out)

    case("global chain (histogram, table, applyTransform)", chain, 3 * P, u8_rate)

    # ---- sharpen ----
    f0 = np.ascontiguousarray(fframes[0, :360, :640].cpu().numpy())
    for rule in (4, 8):
        if not np.array_equal(_sharpen_np(c0[:64, :96], rule), R.sharpen_rule(c0[:64, :96], rule)):
            raise SystemExit("the vectorised sharpen%d differs from tests/enhance_ref.py" % rule)
        same(ops.sharpen(crop, rule), _sharpen_np(c0, rule), "sharpen%d u8" % rule)
        case("sharpen%d u8" % rule, lambda: ops.sharpen(frames, rule, out=out), 2 * P, u8_rate)
        same(ops.sharpen(fframes[:1, :64, :96], rule), R.sharpen_rule(f0[:64, :96], rule), "sharpen%d f32" % rule)
        case("sharpen%d f32" % rule, lambda: ops.sharpen(fframes, rule, out=fout), 8 * P, f32_rate)

    # ---- equalizeLocal: both forced paths and AUTO per radius ----
    small = frames[:1, :64, :96]
    s0 = np.ascontiguousarray(small.cpu().numpy()[0])
    for r in RADII:
        want = R.rank_local(s0, r, 256)
        got = {}
        for path in ("direct", "sliding", "auto"):
            same(ops.equalizeLocal(small, r, 256, path=path), want, "equalizeLocal r=%d %s" % (r, path))
            got[path] = case("equalizeLocal_r%d_%s" % (r, path), lambda: ops.equalizeLocal(frames, r, 256, out=out, path=path), 2 * P, u8_rate,
                             {"radius": r, "path": path, "window_pixels": (2 * r + 1) ** 2})
        best = min(("direct", "sliding"), key=lambda p: got[p]["call_ms"])
        spread = max(got[p]["spread"] for p in got)
        ratio = got["auto"]["call_ms"] / got[best]["call_ms"]
        ln = {"op": "equalizeLocal_r%d_summary" % r, "radius": r, "faster_forced_path": best, "direct_ms": got["direct"]["call_ms"],
              "sliding_ms": got["sliding"]["call_ms"], "auto_ms": got["auto"]["call_ms"], "auto_over_best": round(ratio, 4), "spread": round(spread, 4),
              "auto_within_spread": bool(ratio <= 1.0 + spread)}
        lines.append(ln)
        print(json.dumps(ln), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


def _sharpen_np(img, rule):
    """sharpen4 / sharpen8 on a GrayU8 image, vectorised (safeGet = edge padding; the owner table of tests/enhance_ref.py for rule 4)"""
    a = np.pad(img.astype(np.int32), 1, mode="edge")
    c = a[1:-1, 1:-1]
    l, r, u, d = a[1:-1, :-2], a[1:-1, 2:], a[:-2, 1:-1], a[2:, 1:-1]
    if rule == 8:
        o = 9 * c - (a[:-2, :-2] + u + a[:-2, 2:] + l + r + a[2:, :-2] + d + a[2:, 2:])
    else:
        h, w = img.shape
        o = 5 * c - (l + r + u + d)
        o[0, :] = (4 * c - (l + r + d))[0, :]
        o[-1, :] = (4 * c - (l + r + u))[-1, :]
        o[1:h - 1, 0] = (4 * c - (r + u + d))[1:h - 1, 0]
        o[1:h - 1, -1] = (4 * c - (l + u + d))[1:h - 1, -1]
    return np.clip(o, 0, 255).astype(np.uint8)


if __name__ == "__main__":
    main()
