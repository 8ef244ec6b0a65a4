#!/usr/bin/env python3
"""Side measurement of the dense KLT optical flow (FactoryDenseOpticalFlow.flowKlt) on device-resident pairs (bench.py is not involved).

    bench_flow.py [--image-type f32|u8] [--radius R] [--size WxH] [--batch B] [--form auto|lane|wave|both] [--scales 1,2,4]

Pairs: a Gaussian-blurred noise texture; the second frame is the first moved by a sub-pixel shift (bilinear samples of one larger texture) with
a flat patch in both frames and a patch that only the second frame has.  Per form of the track stage (--form both, the default: lane per pixel
and wave per pixel, alternating, in this order and again in reverse; the launcher is chosen by the `form` argument of the C ABI, not by a
switch in the library): ms per call and per pair by device events around REPS calls after WARM calls, pixels per second, the ctx profiler's
ms per kernel (track stage, reduce stage, pyramids, gradients; from a separate set of calls), the mean Lucas-Kanade iterations per pixel, and
the share of invalid pixels.  The two forms' flows are compared bit for bit, and a 96 x 40 crop is checked against tests/flow_ref.py before
anything is timed.  One JSON line per form and one with their ratio, printed and appended to profiles/bench_flow.jsonl."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from boofcv_amd import _lib, api  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402

REPS, WARM = 10, 3
OUT = os.path.join(ROOT, "profiles", "bench_flow.jsonl")
FORMS = {"auto": _lib.BHIP_FLOW_FORM_AUTO, "lane": _lib.BHIP_FLOW_FORM_LANE, "wave": _lib.BHIP_FLOW_FORM_WAVE}


def make_pairs(ops, B, W, H, u8):
    gen = torch.Generator(device="cuda").manual_seed(23)
    m = 16
    noise = torch.rand((B, H + 2 * m, W + 2 * m), dtype=torch.float32, device="cuda", generator=gen) * 255
    tex = ops.gaussian(noise, -1, 3)
    ops.ctx.synchronize()
    lo, hi = tex.amin(dim=(1, 2), keepdim=True), tex.amax(dim=(1, 2), keepdim=True)
    tex = (tex - lo) / (hi - lo) * 255
    sx, sy = 0.6, 0.4   # dst(x, y) = tex(x - sx, y - sy): a flow of (+0.6, +0.4)
    a = tex[:, m - 1:m - 1 + H, m - 1:m - 1 + W]
    b = tex[:, m - 1:m - 1 + H, m:m + W]
    c = tex[:, m:m + H, m - 1:m - 1 + W]
    d = tex[:, m:m + H, m:m + W]
    src = d.clone()
    dst = (sx * sy) * a + ((1 - sx) * sy) * b + (sx * (1 - sy)) * c + ((1 - sx) * (1 - sy)) * d
    src[:, H // 8:H // 8 + H // 6, W // 8:W // 8 + W // 6] = 40
    dst[:, H // 8:H // 8 + H // 6, W // 8:W // 8 + W // 6] = 40
    dst[:, H // 2:H // 2 + H // 8, W // 2:W // 2 + W // 8] = 250
    if u8:
        src, dst = src.round().clamp(0, 255).to(torch.uint8), dst.round().clamp(0, 255).to(torch.uint8)
    torch.cuda.synchronize()
    return src.contiguous(), dst.contiguous()


def check_against_reference(ops, src, dst, cfg, radius, u8, form):
    import flow_ref
    import klt_ref
    from oracle import pyoracle
    pyoracle.build()
    H, W = src.shape[1:]
    y0, x0 = H // 8 - 10, W // 8 - 10    # a crop over the corner of the flat patch
    s, d = src[:1, y0:y0 + 40, x0:x0 + 96].contiguous(), dst[:1, y0:y0 + 40, x0:x0 + 96].contiguous()
    got = ops.denseFlowKlt(s, d, cfg, radius, form=form)
    ops.ctx.synchronize()
    kc = klt_ref.KltConfig(cfg.config.maxPerPixelError, cfg.config.maxIterations, cfg.config.minDeterminant, cfg.config.minPositionDelta)
    want, rec = flow_ref.dense_flow_klt(pyoracle, s[0].cpu().numpy(), d[0].cpu().numpy(), cfg.pyramidScaling, radius, kc, u8)
    if not flow_ref.same_bits(got[0].cpu().numpy(), want):
        raise SystemExit("the flow differs from tests/flow_ref.py")
    return dict(zip(flow_ref.CLASS_NAMES, (int(v) for v in np.bincount(flow_ref.classify(rec, radius).reshape(-1), minlength=5))))


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
    return start.elapsed_time(stop) / REPS


def kernels(ops, fn):
    ops.ctx.profile(True)
    ops.ctx.profileReset()
    for _ in range(REPS):
        fn()
    ops.ctx.synchronize()
    prof = ops.ctx.profileReport()
    ops.ctx.profile(False)
    return {tag: round(v["ms"] / REPS, 4) for tag, v in prof.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--image-type", choices=("f32", "u8"), default="f32")
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--form", choices=("auto", "lane", "wave", "both"), default="both")
    ap.add_argument("--scales", default="1,2,4")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    u8 = a.image_type == "u8"
    cfg = api.PkltConfig(pyramidScaling=[int(v) for v in a.scales.split(",")])
    ops = DeviceImageOps(device=0)
    src, dst = make_pairs(ops, a.batch, W, H, u8)
    forms = ["lane", "wave"] if a.form == "both" else [a.form]
    out = {f: torch.empty((a.batch, H, W, 2), dtype=torch.float32, device="cuda") for f in forms}
    classes = {f: check_against_reference(ops, src, dst, cfg, a.radius, u8, FORMS[f]) for f in forms}
    run = {f: (lambda f=f: ops.denseFlowKlt(src, dst, cfg, a.radius, out=out[f], form=FORMS[f])) for f in forms}
    # alternate the forms, forwards and backwards, so that a drift of the machine falls on both
    call_ms = {f: [] for f in forms}
    for order in (forms, forms[::-1]):
        for f in order:
            call_ms[f].append(timed(ops, run[f]))
    lines = []
    for f in forms:
        run[f]()
        pixels, iterations = ops.denseFlowStats()
        k = kernels(ops, run[f])
        ms = min(call_ms[f])
        track = sum(v for tag, v in k.items() if tag.startswith("k_flow_track"))
        flow = out[f]
        lines.append({"op": "flowKlt %s radius %d scales %s, track stage: %s per pixel" % (a.image_type, a.radius, cfg.pyramidScaling, f),
                      "pairs": "%d x %dx%d" % (a.batch, W, H), "call_ms": round(ms, 3), "call_ms_runs": [round(v, 3) for v in call_ms[f]],
                      "ms_per_pair": round(ms / a.batch, 4), "pixels_per_s": float("%.4g" % (a.batch * W * H / (ms * 1e-3))),
                      "track_stage_ms": round(track, 4), "reduce_stage_ms": k.get("k_flow_reduce"), "kernels_ms": k,
                      "mean_iterations_per_pixel": round(iterations / max(pixels, 1), 3),
                      "invalid_share": round(float(torch.isnan(flow[..., 0]).float().mean()), 4), "checked_crop_classes": classes[f]})
    if len(forms) == 2:
        same = bool((out["lane"].view(torch.int32) == out["wave"].view(torch.int32)).all())
        if not same:
            raise SystemExit("the two forms differ")
        lines.append({"op": "flowKlt %s radius %d: wave per pixel over lane per pixel" % (a.image_type, a.radius), "pairs": lines[0]["pairs"],
                      "call_ms_ratio": round(lines[1]["call_ms"] / lines[0]["call_ms"], 3),
                      "track_stage_ratio": round(lines[1]["track_stage_ms"] / lines[0]["track_stage_ms"], 3), "flows_identical": same})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
