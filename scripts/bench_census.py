#!/usr/bin/env python3
"""Side measurement of the census transform and of census block matching on 64 device-resident 1920x1080 pairs (bench.py is not involved).
The protocol and the pairs are scripts/bench_disparity.py's.

Transform: one call per output type on the left frames -- BLOCK_3_3 (GrayU8), BLOCK_5_5 (GrayS32), BLOCK_7_7 and CIRCLE_9 (GrayS64) -- with
ms per call and the share of the 6.29 TB/s measured copy rate that the byte floor, 1 B read + 1 / 4 / 8 B written per pixel,
reaches.  Block matching: the default ConfigDisparityBM (range 100, 7x7 region, sub-pixel GrayF32 output, right-to-left and texture checks)
with errorType = CENSUS for the three word sizes (BLOCK_3_3, BLOCK_5_5, BLOCK_7_7) and CIRCLE_9: ms per call (device events around REPS calls,
and the ctx profiler's ms per kernel).  Every line carries the SAD default case timed in the same run and the ratio to it.
A 256 x 64 crop of one pair is checked against tests/census_ref.py before anything is timed.  One JSON line per case, printed and written to
profiles/bench_census.jsonl."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from boofcv_amd import api  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import bench_disparity as bd  # noqa: E402
import census_ref  # noqa: E402
import disparity_ref  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "bench_census.jsonl")
B, W, H = bd.B, bd.W, bd.H


def check_transform(ops, left, variant):
    crop = left[:1, 500:564, 700:956].contiguous()
    got = ops.census(crop, census_ref.VARIANTS.index(variant))
    ops.ctx.synchronize()
    want = census_ref.census_variant(crop[0].cpu().numpy(), variant)
    g = got[0].cpu().numpy()
    if g.dtype != want.dtype or not np.array_equal(g, want):
        raise SystemExit("the census transform %s differs from tests/census_ref.py" % variant)


def check_matching(ops, left, right, cfg, variant):
    l, r = left[:1, 500:564, 700:956].contiguous(), right[:1, 500:564, 700:956].contiguous()
    got = ops.disparityBMCensus(l, r, cfg, variant=census_ref.VARIANTS.index(variant), subpixel=True)
    ops.ctx.synchronize()
    want, cls = census_ref.block_match(l[0].cpu().numpy(), r[0].cpu().numpy(), variant, cfg.minDisparity, cfg.rangeDisparity, cfg.regionRadiusX,
                                       cfg.regionRadiusY, cfg.maxPerPixelError, cfg.validateRtoL, cfg.texture, True)
    if not np.array_equal(got[0].cpu().numpy().view(np.uint32), want.view(np.uint32)):
        raise SystemExit("census block matching %s differs from tests/census_ref.py" % variant)
    return dict(zip(disparity_ref.CLASS_NAMES, disparity_ref.class_counts(cls)))


def main():
    ops = DeviceImageOps(device=0)
    left, right = bd.make_pairs(ops)
    cfg = api.ConfigDisparityBM()
    bd.check_against_reference(ops, left, right, cfg, True)
    disp = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    sad_ms, sad_kernels = bd.timed(ops, lambda: ops.disparityBM(left, right, cfg, subpixel=True, out=disp))
    sad = {"sad_default_ms": round(sad_ms, 3), "sad_default_kernels_ms": sad_kernels}
    lines = []
    for variant in ("BLOCK_3_3", "BLOCK_5_5", "BLOCK_7_7", "CIRCLE_9"):
        check_transform(ops, left, variant)
        v = census_ref.VARIANTS.index(variant)
        out = ops.census(left, v)
        call_ms, kernels = bd.timed(ops, lambda: ops.census(left, v, out=out))
        floor_bytes = (1 + out.element_size()) * B * W * H
        lines.append(dict({"op": "census %s u8 -> %s" % (variant, str(out.dtype).replace("torch.", "")), "frames": "%d x %dx%d" % (B, W, H),
                           "call_ms": round(call_ms, 4), "kernels_ms": kernels, "byte_floor_bytes": floor_bytes,
                           "byte_floor_share_of_copy_rate": round(floor_bytes / (call_ms * 1e-3) / bd.COPY_RATE, 4),
                           "ratio_to_sad_default": round(call_ms / sad_ms, 4)}, **sad))
        del out
    for variant in ("BLOCK_3_3", "BLOCK_5_5", "BLOCK_7_7", "CIRCLE_9"):
        classes = check_matching(ops, left, right, cfg, variant)
        v = census_ref.VARIANTS.index(variant)
        call_ms, kernels = bd.timed(ops, lambda: ops.disparityBMCensus(left, right, cfg, variant=v, subpixel=True, out=disp))
        lines.append(dict({"op": "blockMatch CENSUS %s u8: default: range 100, 7x7, sub-pixel F32" % variant, "pairs": "%d x %dx%d" % (B, W, H),
                           "call_ms": round(call_ms, 3), "ms_per_pair": round(call_ms / B, 4), "kernels_ms": kernels,
                           "block_comparisons_per_s": float("%.4g" % (B * W * H * cfg.rangeDisparity / (call_ms * 1e-3))),
                           "ratio_to_sad_default": round(call_ms / sad_ms, 3), "checked_crop_classes": classes}, **sad))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
