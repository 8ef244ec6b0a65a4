#!/usr/bin/env python3
"""Side measurement of the binary-image family (BinaryImageOps: logic, erode / dilate / edge / removePointNoise, blob labelling, label
utilities) on 64 device-resident 1920x1080 0/1 frames (bench.py is not involved).

The frames are made on the device with the library's own front end: uniform noise, BlurImageOps.gaussian on GrayU8 (radius 4), then a fixed
threshold (down: pixel <= threshold is foreground) -- at the blur's mean for the dense image (about half foreground, blobs of a few pixels
across that touch each other) and 12 grey levels below it for the sparse one.  Per case: ms per call (device events around REPS calls after WARM warm-up calls), the ctx profiler's ms per
kernel, the bytes one read of the inputs and one write of the output would move (`ideal_bytes`), the time a plain device copy needs for that
many bytes AT THE COPY RATE MEASURED IN THIS RUN (a device-to-device copy of the uint8 batch, and of an int32 batch for the label images), and
`times_copy` = call_ms over that.  There is no pass / fail threshold: nobody had measured these kernels before this script.
erode8 / dilate8 run at numTimes 1, 2 and K + 1 = 5 (K = 4 iterations fit one launch); labelBlobs runs for both rules on both images.
A 640 x 360 crop of frame 0 goes through the same entry point and is compared with tests/binaryops_ref.py before a case is timed.
One JSON line per case, printed and written to profiles/bench_binary.jsonl."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd import binary  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import binaryops_ref as R  # noqa: E402

B, W, H = 64, 1920, 1080
REPS, WARM = 5, 2
K = 4
OUT = os.path.join(ROOT, "profiles", "bench_binary.jsonl")
P = B * W * H


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


def copy_rate(src):
    dst = torch.empty_like(src)
    for _ in range(WARM):
        dst.copy_(src)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(REPS):
        dst.copy_(src)
    stop.record()
    stop.synchronize()
    ms = start.elapsed_time(stop) / REPS
    return ms, 2.0 * src.numel() * src.element_size() / (ms * 1e-3)


def crop(t):
    return t[:1, :360, :640]


def same(got, want, what):
    if not np.array_equal(got.cpu().numpy()[0], want):
        raise SystemExit("%s differs from tests/binaryops_ref.py" % what)


def main():
    ops = DeviceImageOps(device=0)
    gen = torch.Generator(device="cuda").manual_seed(31)
    noise = torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    blur = ops.gaussianU8(noise, 4)
    mean = float(blur[0].float().mean())
    dense = ops.threshold(blur, binary.ConfigThreshold.fixed(int(mean)))
    sparse = ops.threshold(blur, binary.ConfigThreshold.fixed(int(mean) - 12))
    del noise, blur
    out = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    labels = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    count = torch.empty((B,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    u8_ms, u8_rate = copy_rate(dense)
    s32_ms, s32_rate = copy_rate(labels)
    lines = [{"op": "device copy u8 (the yardstick)", "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(u8_ms, 4), "GBps": round(u8_rate / 1e9, 1)},
             {"op": "device copy s32", "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(s32_ms, 4), "GBps": round(s32_rate / 1e9, 1)},
             {"op": "frames", "foreground_dense": round(float(dense.float().mean()), 4), "foreground_sparse": round(float(sparse.float().mean()), 4)}]

    for ln in lines:
        print(json.dumps(ln), flush=True)

    def case(name, fn, ideal_bytes, rate, extra=None):
        call_ms, kernels = timed(ops, fn)
        copy_ms = ideal_bytes / rate * 1e3
        ln = {"op": name, "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(call_ms, 4), "ms_per_frame": round(call_ms / B, 5), "kernels_ms": kernels,
              "ideal_bytes": ideal_bytes, "copy_ms_same_bytes": round(copy_ms, 4), "times_copy": round(call_ms / copy_ms, 2)}
        ln.update(extra or {})
        lines.append(ln)
        print(json.dumps(ln), flush=True)

    d0, s0 = np.ascontiguousarray(crop(dense).cpu().numpy()[0]), np.ascontiguousarray(crop(sparse).cpu().numpy()[0])
    same(ops.binaryLogic("and", crop(dense), crop(sparse)), R.logicAnd(d0, s0), "logicAnd")
    for op in ("and", "or", "xor"):
        case("logic %s" % op, lambda: ops.binaryLogic(op, dense, sparse, out=out), 3 * P, u8_rate)
    same(ops.binaryInvert(crop(dense)), R.invert(d0), "invert")
    case("invert", lambda: ops.binaryInvert(dense, out=out), 2 * P, u8_rate)
    for name, fn, rule in (("erode4", ops.erode, 4), ("dilate4", ops.dilate, 4), ("erode8", ops.erode, 8), ("dilate8", ops.dilate, 8)):
        for n in ((1,) if rule == 4 else (1, 2, K + 1)):
            same(fn(crop(dense), rule, n), R.MORPH[name](d0, n), "%s x%d" % (name, n))
            case("%s numTimes %d" % (name, n), lambda: fn(dense, rule, n, out=out), 2 * P, u8_rate, {"launches": (n + K - 1) // K})
    for rule in (4, 8):
        same(ops.edge(crop(dense), rule, False), (R.edge4 if rule == 4 else R.edge8)(d0, False), "edge%d" % rule)
        case("edge%d outside 1" % rule, lambda: ops.edge(dense, rule, False, out=out), 2 * P, u8_rate)
    same(ops.removePointNoise(crop(dense)), R.removePointNoise(d0), "removePointNoise")
    case("removePointNoise", lambda: ops.removePointNoise(dense, out=out), 2 * P, u8_rate)
    for which, frames, f0 in (("dense", dense, d0), ("sparse", sparse, s0)):
        for rule in (4, 8):
            got, n = ops.labelBlobs(crop(frames), rule)
            want, m = R.contourLabels(f0, rule)
            same(got, want, "labelBlobs %s rule %d" % (which, rule))
            if int(n[0]) != m:
                raise SystemExit("labelBlobs count differs")
            ops.labelBlobs(frames, rule, out=labels, numBlobs=count)
            blobs = float(count.float().mean())
            case("labelBlobs rule %d %s" % (rule, which), lambda: ops.labelBlobs(frames, rule, out=labels, numBlobs=count), 5 * P, s32_rate,
                 {"blobs_per_frame": round(blobs, 1)})
    ops.labelBlobs(dense, 8, out=labels, numBlobs=count)
    table = torch.arange(int(count.max()) + 1, dtype=torch.int32, device="cuda").flip(0).contiguous()
    case("relabel", lambda: ops.relabel(labels, table), 8 * P, s32_rate)
    case("labelToBinary", lambda: ops.labelToBinary(labels, out=out), 5 * P, s32_rate)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
