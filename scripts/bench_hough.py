#!/usr/bin/env python3
"""Side measurement of the Hough line detectors (FactoryDetectLine.houghLinePolar on a binary image, houghLineFoot on the gradient) on 64
device-resident 1920x1080 frames (bench.py is not involved).

The scene is made on the device: a noisy ground with 12 line segments per frame of random position, direction and length -- dark one-pixel
segments on a bright ground for the binary detector (GLOBAL_OTSU marks the dark pixels), 5-pixel bright bars on a dark ground for the
gradient detector (GrayU8 and GrayF32).  Per stage and per whole detector (its device stages chained; transformToLine and the merge are
host list logic on a few dozen peaks and are not timed): ms per call (device events around REPS calls after WARM warm-up calls), the ctx
profiler's ms per kernel, the bytes one read of the inputs and one write of the outputs would move (`ideal_bytes`), the time a plain device
copy needs for that many bytes AT THE COPY RATE MEASURED IN THIS RUN, and `times_copy` = call_ms over that.  The edge-pixel share of each
vote's input is recorded with it.  There is no pass / fail threshold: nobody had measured these kernels before this script.
A 320 x 180 crop of frame 0 goes through each vote and is compared with tests/hough_ref.py before anything is timed.
One JSON line per case, printed and written to profiles/bench_hough.jsonl."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd import binary, device  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import hough_ref as R  # noqa: E402

B, W, H = 64, 1920, 1080
REPS, WARM = 5, 2
SEGMENTS = 12
GRADIENT_CAP = 1 << 18   # edge pixels per frame that may vote (12.6 % of a frame); the run checks that no frame has more
OUT = os.path.join(ROOT, "profiles", "bench_hough.jsonl")
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


def scene(half_width, line_value, ground, noise):
    """uint8 [B,H,W]: ground + uniform noise, with SEGMENTS segments per frame at line_value"""
    gen = torch.Generator(device="cuda").manual_seed(77)
    img = (ground + torch.rand((B, H, W), device="cuda", generator=gen) * noise)
    ys = torch.arange(H, device="cuda", dtype=torch.float32).view(1, H, 1)
    xs = torch.arange(W, device="cuda", dtype=torch.float32).view(1, 1, W)
    rng = np.random.RandomState(78)
    for _ in range(SEGMENTS):
        cx = torch.tensor(rng.rand(B) * W, device="cuda", dtype=torch.float32).view(B, 1, 1)
        cy = torch.tensor(rng.rand(B) * H, device="cuda", dtype=torch.float32).view(B, 1, 1)
        ang = rng.rand(B) * math.pi
        dx = torch.tensor(np.cos(ang), device="cuda", dtype=torch.float32).view(B, 1, 1)
        dy = torch.tensor(np.sin(ang), device="cuda", dtype=torch.float32).view(B, 1, 1)
        half = torch.tensor(150 + rng.rand(B) * 500, device="cuda", dtype=torch.float32).view(B, 1, 1)
        along = (xs - cx) * dx + (ys - cy) * dy
        across = (ys - cy) * dx - (xs - cx) * dy
        img = torch.where((across.abs() < half_width) & (along.abs() < half), torch.full_like(img, float(line_value)), img)
    return img.to(torch.uint8)


def main():
    ops = DeviceImageOps(device=0)
    dark = scene(0.6, 20, 190, 40)
    bars = scene(2.5, 200, 30, 6)
    bars_f = bars.float() + 0.25
    torch.cuda.synchronize()
    u8_ms, u8_rate = copy_rate(dark)
    f32_ms, f32_rate = copy_rate(bars_f)
    frames = "%d x %dx%d" % (B, W, H)
    lines = [{"op": "device copy u8 (the yardstick)", "frames": frames, "call_ms": round(u8_ms, 4), "GBps": round(u8_rate / 1e9, 1)},
             {"op": "device copy f32", "frames": frames, "call_ms": round(f32_ms, 4), "GBps": round(f32_rate / 1e9, 1)}]
    for ln in lines:
        print(json.dumps(ln), flush=True)

    def case(name, fn, ideal_bytes, rate, extra=None):
        call_ms, kernels = timed(ops, fn)
        copy_ms = ideal_bytes / rate * 1e3
        ln = {"op": name, "frames": frames, "call_ms": round(call_ms, 4), "ms_per_frame": round(call_ms / B, 5), "kernels_ms": kernels,
              "ideal_bytes": int(ideal_bytes), "copy_ms_same_bytes": round(copy_ms, 4), "times_copy": round(call_ms / copy_ms, 2)}
        ln.update(extra or {})
        lines.append(ln)
        print(json.dumps(ln), flush=True)

    def same(got, want, what):
        g, w = got.cpu().numpy()[0], want
        if g.shape != w.shape or not np.array_equal(g.view(np.int32), w.view(np.int32)):
            raise SystemExit("%s differs from tests/hough_ref.py" % what)

    # ---- the binary polar detector: GLOBAL_OTSU, vote, relaxed NMS (radius 1), the counts at the peaks ----
    otsu = binary.ConfigThreshold.global_(binary.ThresholdType.GLOBAL_OTSU)
    bw = ops.threshold(dark, otsu)
    share = float((bw != 0).float().mean())
    crop = bw[:1, :180, :320].contiguous()
    same(ops.houghBinaryPolar(crop), R.hough_binary(crop.cpu().numpy()[0], R.Polar(2.0, 180)), "binary vote")
    bins, _ = ops.houghPolarBins(W, H, 2.0)
    T = B * 180 * bins
    transform = torch.empty((B, 180, bins), dtype=torch.float32, device="cuda")
    threshold = float(np.float32(max(0.001 * 180 * bins, 1.0)))
    case("binary: threshold GLOBAL_OTSU", lambda: ops.threshold(dark, otsu, out=bw), 3 * P, u8_rate)
    case("binary: vote polar 180 x %d" % bins, lambda: ops.houghBinaryPolar(bw, out=transform), P + 4 * T, u8_rate, {"edge_pixel_share": round(share, 5)})
    xy, n = ops.nonmaxRelaxed(transform, 1, threshold, cap=4096)
    peaks = float(n.float().mean())
    case("binary: relaxed NMS radius 1", lambda: ops.nonmaxRelaxed(transform, 1, threshold, cap=4096), 4 * T, f32_rate, {"peaks_per_frame": round(peaks, 1)})
    xyc = xy.contiguous()
    case("binary: counts at the peaks", lambda: ops.meanShiftPeak(transform, xyc, n, radius=0), 16 * B * peaks, f32_rate)

    def binary_detector():
        ops.threshold(dark, otsu, out=bw)
        ops.houghBinaryPolar(bw, out=transform)
        p, c = ops.nonmaxRelaxed(transform, 1, threshold, cap=4096)
        ops.meanShiftPeak(transform, p, c, radius=0)
    case("binary: whole detector (device stages)", binary_detector, 3 * P + P + 8 * T, u8_rate, {"edge_pixel_share": round(share, 5)})
    del dark, bw, transform

    # ---- the gradient foot-of-norm detector: Prewitt, intensityAbs, crude suppression, FIXED threshold, vote, strict NMS, mean shift ----
    fixed = binary.ConfigThreshold.fixed(30.0)
    fixed.down = False
    for name, src, db, rate in (("u8", bars, 2, u8_rate), ("f32", bars_f, 4, f32_rate)):
        sb = src.element_size()
        dx, dy = ops.prewitt(src, "EXTENDED")
        inten = ops.intensity(device.INTENSITY_ABS, dx, dy)
        supp = ops.edgeNonMaxCrude4(inten, dx, dy)
        edges = ops.threshold(supp, fixed)
        share = float((edges != 0).float().mean())
        transform = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
        counts = torch.empty((B,), dtype=torch.int32, device="cuda")
        c = (slice(0, 1), slice(0, 180), slice(0, 320))
        got, _ = ops.houghGradientFoot(dx[c].contiguous(), dy[c].contiguous(), edges[c].contiguous())
        same(got, R.hough_gradient(dx[c].cpu().numpy()[0], dy[c].cpu().numpy()[0], edges[c].cpu().numpy()[0], R.FootOfNorm(5)), "gradient vote " + name)
        ops.houghGradientFoot(dx, dy, edges, out=transform, cap=GRADIENT_CAP, counts=counts)
        most = int(counts.max())
        if most > GRADIENT_CAP:
            raise SystemExit("a frame has %d edge pixels, more than the cap of %d" % (most, GRADIENT_CAP))
        case("gradient %s: prewitt EXTENDED" % name, lambda: ops.prewitt(src, "EXTENDED", dx, dy), (sb + 2 * db) * P, rate)
        case("gradient %s: intensityAbs" % name, lambda: ops.intensity(device.INTENSITY_ABS, dx, dy, inten), (2 * db + 4) * P, rate)
        case("gradient %s: nonMaxSuppressionCrude4" % name, lambda: ops.edgeNonMaxCrude4(inten, dx, dy, supp), (8 + 2 * db) * P, rate)
        case("gradient %s: threshold FIXED" % name, lambda: ops.threshold(supp, fixed, out=edges), 5 * P, rate)
        case("gradient %s: vote foot of norm (cap %d)" % (name, GRADIENT_CAP), lambda: ops.houghGradientFoot(dx, dy, edges, out=transform, cap=GRADIENT_CAP, counts=counts),
             (1 + 4) * P + 2 * db * share * P, rate, {"edge_pixel_share": round(share, 5), "most_edge_pixels_in_a_frame": most})
        xy, n = ops.nonmax(transform, 2, 5.0, 0, cap=4096)
        peaks = float(n.float().mean())
        case("gradient %s: strict NMS radius 2" % name, lambda: ops.nonmax(transform, 2, 5.0, 0, cap=4096), 4 * P, rate, {"peaks_per_frame": round(peaks, 1)})
        case("gradient %s: mean shift radius 3" % name, lambda: ops.meanShiftPeak(transform, xy, n, radius=3), 16 * B * min(peaks, 4096), rate)

        def gradient_detector():
            ops.prewitt(src, "EXTENDED", dx, dy)
            ops.intensity(device.INTENSITY_ABS, dx, dy, inten)
            ops.edgeNonMaxCrude4(inten, dx, dy, supp)
            ops.threshold(supp, fixed, out=edges)
            ops.houghGradientFoot(dx, dy, edges, out=transform, cap=GRADIENT_CAP, counts=counts)
            p, k = ops.nonmax(transform, 2, 5.0, 0, cap=4096)
            ops.meanShiftPeak(transform, p, k, radius=3)
        case("gradient %s: whole detector (device stages)" % name, gradient_detector, (sb + 4 * db + 4 + 8 + 5 + 1 + 4 + 4) * P, rate, {"edge_pixel_share": round(share, 5)})
        del dx, dy, inten, supp, edges, transform
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
