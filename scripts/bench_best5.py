#!/usr/bin/env python3
"""Side measurement of five-region block matching (FactoryStereoDisparity.blockMatchBest5 on GrayU8 pairs) against plain block matching, on
the 64 device-resident 1920x1080 pairs and with the protocol of scripts/bench_disparity.py (bench.py is not involved).

Cases, timed in the same run: plain SAD block matching with the default ConfigDisparityBM (range 100, 7x7 region, sub-pixel GrayF32 output,
right-to-left and texture checks), Best5 SAD with the default ConfigDisparityBMBest5 (the same fields), and Best5 on the census BLOCK_5_5
images.  Per case: ms per call (device events around REPS calls), the ctx profiler's ms per kernel, and for the Best5 cases the ratio of the
call and of the two matching kernels to the plain SAD case.  A 256 x 64 crop of one pair is checked against tests/best5_ref.py (and the plain
case against tests/disparity_ref.py) before anything is timed.  One JSON line per case, printed and written to profiles/bench_best5.jsonl."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import boofcv_amd as b  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
import best5_ref  # noqa: E402
import disparity_ref  # noqa: E402
from bench_disparity import B, H, W, check_against_reference, make_pairs, timed  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "bench_best5.jsonl")


def check_best5(ops, left, right, cfg, variant):
    l, r = left[:1, 500:564, 700:956].contiguous(), right[:1, 500:564, 700:956].contiguous()
    got = ops.disparityBM5(l, r, cfg, variant=None if variant is None else b.CensusVariants[variant], subpixel=True)
    ops.ctx.synchronize()
    want, cls = best5_ref.block_match_best5(l[0].cpu().numpy(), r[0].cpu().numpy(), cfg.minDisparity, cfg.rangeDisparity, cfg.regionRadiusX, cfg.regionRadiusY,
                                            cfg.maxPerPixelError, cfg.validateRtoL, cfg.texture, True, variant)
    if not np.array_equal(got[0].cpu().numpy().view(np.uint32), want.view(np.uint32)):
        raise SystemExit("blockMatchBest5 differs from tests/best5_ref.py")
    return dict(zip(disparity_ref.CLASS_NAMES, disparity_ref.class_counts(cls)))


def matching_ms(kernels):
    """the right-to-left and the selection kernel: what the cost and selection stages take"""
    return sum(v for k, v in kernels.items() if k.startswith("k_disparity_bm") or k == "k_disparity_rtol")


def main():
    ops = DeviceImageOps(device=0)
    left, right = make_pairs(ops)
    out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    lines = []
    plain_cfg = b.ConfigDisparityBM()
    classes = check_against_reference(ops, left, right, plain_cfg, True)
    plain_ms, plain_kernels = timed(ops, lambda: ops.disparityBM(left, right, plain_cfg, subpixel=True, out=out))
    lines.append({"op": "blockMatch SAD u8: default (range 100, 7x7, sub-pixel F32)", "pairs": "%d x %dx%d" % (B, W, H), "call_ms": round(plain_ms, 3),
                  "ms_per_pair": round(plain_ms / B, 4), "kernels_ms": plain_kernels, "checked_crop_classes": classes})
    cfg = b.ConfigDisparityBMBest5()
    for name, variant in (("blockMatchBest5 SAD u8: default (range 100, 7x7 sub-blocks, sub-pixel F32)", None),
                          ("blockMatchBest5 CENSUS BLOCK_5_5: default (range 100, 7x7 sub-blocks, sub-pixel F32)", "BLOCK_5_5")):
        classes = check_best5(ops, left, right, cfg, variant)
        v = None if variant is None else b.CensusVariants[variant]
        call_ms, kernels = timed(ops, lambda: ops.disparityBM5(left, right, cfg, variant=v, subpixel=True, out=out))
        lines.append({"op": name, "pairs": "%d x %dx%d" % (B, W, H), "call_ms": round(call_ms, 3), "ms_per_pair": round(call_ms / B, 4), "kernels_ms": kernels,
                      "ratio_to_plain_sad_call": round(call_ms / plain_ms, 2),
                      "ratio_to_plain_sad_matching_kernels": round(matching_ms(kernels) / matching_ms(plain_kernels), 2),
                      "block_comparisons_per_s": float("%.4g" % (3.0 * B * W * H * cfg.rangeDisparity / (call_ms * 1e-3))), "checked_crop_classes": classes})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            f.write(s + "\n")


if __name__ == "__main__":
    main()
