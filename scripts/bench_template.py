#!/usr/bin/env python3
"""Side measurement of the template matching intensity (FactoryTemplateMatching.createIntensity: SAD, SSE, NCC on GrayU8 / GrayF32) on 64
device-resident 1920x1080 frames (bench.py is not involved).

Frames are uniform noise (uint8 0..255, float32 [0, 255)); the template is a crop of frame 0, shared by the batch.  Cases: templates of 16x16,
32x32 and 64x64, the three scores, both pixel types, unmasked, plus one masked row (NCC, GrayF32, 32x32).  Per case: the median over REPS
calls of the time between two device events around one call (after WARM calls), the template-pixel comparisons per second,
(W-tw+1) * (H-th+1) * tw * th * frames over that time (NCC reads every pair twice; it is counted once), and the ctx profiler's ms per kernel.
bhip_sobel_dev_u8_s16 (k_sobel_u8) is timed on the same frames in the same run as the streaming yardstick.
A 256 x 64 crop is checked against tests/template_ref.py for every score and type before anything is timed.  One JSON line per case, printed
and written to profiles/bench_template.jsonl (--out FILE: elsewhere).  --counters: one call of the 32x32 GrayU8 SAD case only and nothing
written (for a profiler run)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import template_ref  # noqa: E402

B, W, H = 64, 1920, 1080
REPS, WARM = 20, 2
OUT = os.path.join(ROOT, "profiles", "bench_template.jsonl")
SHORT = {template_ref.SAD: "SAD", template_ref.SSE: "SSE", template_ref.NCC: "NCC"}


def make_frames(dtype):
    gen = torch.Generator(device="cuda").manual_seed(23)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (B, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    return torch.rand((B, H, W), dtype=torch.float32, device="cuda", generator=gen) * 255


def make_mask(size, dtype):
    gen = torch.Generator(device="cuda").manual_seed(29)
    m = torch.randint(0, 3, (size, size), device="cuda", generator=gen)
    return m.to(dtype)


def check_against_reference(ops, frames):
    crop = frames[:1, 500:564, 700:956].contiguous()
    tpl = crop[0, 20:36, 100:116].contiguous()
    mask = make_mask(16, frames.dtype)
    for score in template_ref.SCORES:
        for m in (None, mask):
            got = ops.templateIntensity(crop, tpl, m, score)
            ops.ctx.synchronize()
            want = template_ref.intensity(crop[0].cpu().numpy(), tpl.cpu().numpy(), None if m is None else m.cpu().numpy(), score)
            if not np.array_equal(got[0].cpu().numpy().view(np.uint32), want.view(np.uint32)):
                raise SystemExit("template intensity differs from tests/template_ref.py: %s %s" % (score, frames.dtype))


def timed(ops, fn):
    for _ in range(WARM):
        fn()
    ops.ctx.synchronize()
    times = []
    for _ in range(REPS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    ops.ctx.profile(True)
    ops.ctx.profileReset()
    fn()
    ops.ctx.synchronize()
    prof = ops.ctx.profileReport()
    ops.ctx.profile(False)
    return statistics.median(times), min(times), max(times), {tag: round(v["ms"], 4) for tag, v in prof.items()}


def main():
    counters = "--counters" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    ops = DeviceImageOps(device=0)
    frames = {"u8": make_frames(torch.uint8), "f32": make_frames(torch.float32)}
    torch.cuda.synchronize()
    out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    if counters:
        tpl = frames["u8"][0, 300:332, 400:432].contiguous()
        ops.templateIntensity(frames["u8"], tpl, None, template_ref.SAD, out=out)
        ops.ctx.synchronize()
        print("one call of the 32x32 GrayU8 SAD case done")
        return
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    f = open(out_path, "w")

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        f.write(s + "\n")
        f.flush()

    dx, dy = ops.sobel(frames["u8"], 0)
    sobel_ms, _, _, sobel_kernels = timed(ops, lambda: ops.sobel(frames["u8"], 0, dx, dy))
    emit({"op": "sobel u8 -> s16 (yardstick)", "frames": "%d x %dx%d" % (B, W, H), "call_ms": round(sobel_ms, 4), "kernels_ms": sobel_kernels})
    for kind in ("u8", "f32"):
        check_against_reference(ops, frames[kind])
    cases = [(kind, size, score, False) for kind in ("u8", "f32") for score in template_ref.SCORES for size in (16, 32, 64)]
    cases.append(("f32", 32, template_ref.NCC, True))
    for kind, size, score, masked in cases:
        fr = frames[kind]
        tpl = fr[0, 300:300 + size, 400:400 + size].contiguous()
        mask = make_mask(size, fr.dtype) if masked else None
        med, lo, hi, kernels = timed(ops, lambda: ops.templateIntensity(fr, tpl, mask, score, out=out))
        comparisons = (W - size + 1) * (H - size + 1) * size * size * B
        emit({"op": "template %s %s %dx%d%s" % (SHORT[score], kind, size, size, " masked" if masked else ""), "frames": "%d x %dx%d" % (B, W, H),
              "call_ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "reps": REPS, "ms_per_frame": round(med / B, 4),
              "comparisons_per_s": float("%.4g" % (comparisons / (med * 1e-3))), "kernels_ms": kernels, "ratio_to_sobel_u8": round(med / sobel_ms, 1)})
    f.close()


if __name__ == "__main__":
    main()
