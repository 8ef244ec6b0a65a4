#!/usr/bin/env python3
"""Side measurement of the Horn-Schunck dense optical flow (FactoryDenseOpticalFlow.hornSchunck) on device-resident pairs (bench.py is not
involved).

    bench_hornschunck.py [--size WxH] [--batch B] [--alpha A] [--iterations N] [--out FILE]

Pairs: bench_flow.py's (a Gaussian-blurred noise texture, the second frame moved by a sub-pixel shift, a flat patch), 1920 x 1080, GrayF32 and
GrayU8, at the default ConfigHornSchunck (alpha = 20, numIterations = 1000).  For itersPerLaunch = 1, 2, 4, .. BHIP_FLOW_HS_MAX_FUSED and 0 (the
library's choice): ms per call and per pair by device events around REPS calls after WARM calls -- the depths alternate, in this order and
again in reverse, so that a drift of the machine falls on all of them; both figures are kept (their difference is the run-to-run spread the
choice of 0 is judged by) -- and the ctx profiler's ms per kernel from a separate call.  Every depth's flow is compared bit for bit with depth
1's, and a 130 x 61 crop is checked against tests/hornschunck_ref.py before anything is timed.

The depth-1 row is the launch-per-iteration form.  Its `sweep_bytes_estimate` is an ESTIMATE, not a measurement: 28 B per pixel and iteration
(flow in 8, three derivatives 12, flow out 8) times the halo factor of a 112 x 48 tile with a one-pixel halo; `sweep_gbps_if_estimate_holds`
divides it by the MEASURED time of the iteration kernel.  One JSON line per image type and depth, printed and appended to
profiles/bench_hornschunck.jsonl (or --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from boofcv_amd import _lib  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
from bench_flow import make_pairs  # noqa: E402

REPS, WARM = 3, 1
OUT = os.path.join(ROOT, "profiles", "bench_hornschunck.jsonl")
K, TW, TH = _lib.BHIP_FLOW_HS_MAX_FUSED, _lib.BHIP_FLOW_HS_TILE_WIDTH, _lib.BHIP_FLOW_HS_TILE_HEIGHT


def check_against_reference(ops, src, dst, u8):
    import hornschunck_ref
    import flow_ref
    H, W = src.shape[1:]
    y0, x0 = H // 8 - 10, W // 8 - 10    # a crop over the corner of the flat patch
    s, d = src[:1, y0:y0 + 61, x0:x0 + 130].contiguous(), dst[:1, y0:y0 + 61, x0:x0 + 130].contiguous()
    want, _ = hornschunck_ref.horn_schunck(s[0].cpu().numpy(), d[0].cpu().numpy(), 20.0, 2 * K + 3, u8)
    for depth in (0, 1, K):
        got = ops.denseFlowHornSchunck(s, d, 20.0, 2 * K + 3, itersPerLaunch=depth)
        ops.ctx.synchronize()
        if not flow_ref.same_bits(got[0].cpu().numpy(), want):
            raise SystemExit("the flow differs from tests/hornschunck_ref.py at depth %d" % depth)


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
    fn()
    ops.ctx.synchronize()
    prof = ops.ctx.profileReport()
    ops.ctx.profile(False)
    return {tag: round(v["ms"], 4) for tag, v in prof.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=20.0)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    ops = DeviceImageOps(device=0)
    depths = [d for d in (1, 2, 4, 8, 16, 32) if d <= K] + [0]
    lines = []
    for u8 in (False, True):
        src, dst = make_pairs(ops, a.batch, W, H, u8)
        check_against_reference(ops, src, dst, u8)
        out = {d: torch.empty((a.batch, H, W, 2), dtype=torch.float32, device="cuda") for d in depths}
        run = {d: (lambda d=d: ops.denseFlowHornSchunck(src, dst, a.alpha, a.iterations, out=out[d], itersPerLaunch=d)) for d in depths}
        call_ms = {d: [] for d in depths}
        for order in (depths, depths[::-1]):
            for d in order:
                call_ms[d].append(timed(ops, run[d]))
        for d in depths:
            if not bool((out[d].view(torch.int32) == out[1].view(torch.int32)).all()):
                raise SystemExit("depth %d differs from depth 1" % d)
        for d in depths:
            k = kernels(ops, run[d])
            ms = min(call_ms[d])
            line = {"op": "hornSchunck %s alpha %g, %d iterations, itersPerLaunch %d" % ("u8" if u8 else "f32", a.alpha, a.iterations, d),
                    "pairs": "%d x %dx%d" % (a.batch, W, H), "itersPerLaunch": d, "call_ms": round(ms, 3), "call_ms_runs": [round(v, 3) for v in call_ms[d]],
                    "ms_per_pair": round(ms / a.batch, 3), "us_per_pair_and_iteration": round(1e3 * ms / a.batch / max(a.iterations, 1), 3), "kernels_ms": k,
                    "flows_identical_to_depth_1": True, "nan_share": round(float(torch.isnan(out[d]).float().mean()), 6)}
            if d == 1:
                est = 28.0 * W * H * ((TW + 2) * (TH + 2) / (TW * TH))
                line["sweep_bytes_estimate"] = round(est)
                line["sweep_gbps_if_estimate_holds"] = round(est * a.batch * a.iterations / (k.get("k_hs_iterate", float("nan")) * 1e-3) / 1e9, 1)
            lines.append(line)
        best = min((ln for ln in lines[-len(depths):] if ln["itersPerLaunch"]), key=lambda ln: ln["call_ms"])
        lines.append({"op": "hornSchunck %s: the depth 0 chooses against the fastest forced depth" % ("u8" if u8 else "f32"), "pairs": best["pairs"],
                      "fastest_forced_depth": best["itersPerLaunch"], "fastest_forced_ms_per_pair": best["ms_per_pair"], "auto_ms_per_pair": lines[-1]["ms_per_pair"],
                      "auto_over_fastest": round(lines[-1]["call_ms"] / best["call_ms"], 4)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
