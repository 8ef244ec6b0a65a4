#!/usr/bin/env python3
"""Side measurement of SIFT detect + describe (FactoryDetectDescribe.sift) on device-resident frames (bench.py is not involved).

    bench_sift_describe.py [--size WxH] [--batch B] [--cap N] [--out FILE]

Frames: the seeded noise texture of scripts/bench_sift.py (blurred with sigma 2, stretched to 0 .. 255), 16 frames of 1920 x 1080, GrayF32,
at the default ConfigCompleteSift.  In one run: ms per batch by device events around REPS calls after WARM calls of detect + describe
(bhip_csift_dev_f32) and of the detector alone (bhip_sift_detect_dev_f32), into preallocated buffers, in that order and again in reverse so
that a drift of the machine falls on both (both figures are kept: their difference is the run-to-run spread); the difference of the two is
what orientation and description add.  Then the ctx profiler's ms per kernel from a separate call of each, the features per frame and the
angles per detection (the run lengths of equal ScalePoints).  Before anything is timed a 304 x 72 crop is checked against
tests/sift_describe_ref.py (counts, ScalePoints and order exactly; angles and descriptor elements within 1e-12), and two calls on the full
frames are compared bit for bit.  One JSON line per measurement, printed and appended to profiles/bench_sift_describe.jsonl (or --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from boofcv_amd import sift  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
from bench_sift import kernels, make_frames  # noqa: E402

REPS, WARM = 20, 2
OUT = os.path.join(ROOT, "profiles", "bench_sift_describe.jsonl")


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


def check_against_reference(ops, frames):
    import sift_describe_ref as dr
    import sift_ref
    crop = frames[:1, 100:172, 200:504].contiguous()
    res = dr.complete(sift_ref.ConfigSS(), sift_ref.ConfigDet(), dr.Orientation(), dr.Describe(), crop[0].cpu().numpy())
    x, y, s, o, w, d, n = (v.cpu().numpy() for v in ops.siftDetectDescribe(crop, cap=4096))
    k = int(n[0])
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    same = k == len(res["x"]) and np.array_equal(bits(x[0, :k]), bits(res["x"])) and np.array_equal(bits(y[0, :k]), bits(res["y"])) \
        and np.array_equal(bits(s[0, :k]), bits(res["scale"])) and np.array_equal(w[0, :k], res["white"])
    if not same or k < 20:
        raise SystemExit("the crop's features differ from tests/sift_describe_ref.py")
    ea, ed = float(dr.angle_dist(o[0, :k], res["orientation"]).max()), float(np.abs(d[0, :k] - res["desc"]).max())
    if ea > 1e-12 or ed > 1e-12:
        raise SystemExit("the crop's angles / descriptors differ from tests/sift_describe_ref.py: %g rad, %g" % (ea, ed))
    return k, ea, ed


def run_lengths(x, y, s):
    """angles per detection of one frame's records: runs of equal ScalePoints"""
    if len(x) == 0:
        return {}
    new = np.ones(len(x), bool)
    new[1:] = (x[1:] != x[:-1]) | (y[1:] != y[:-1]) | (s[1:] != s[:-1])
    runs = np.diff(np.append(np.nonzero(new)[0], len(x)))
    return {int(k): int(v) for k, v in zip(*np.unique(runs, return_counts=True))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--cap", type=int, default=32768)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    B, cap = a.batch, a.cap
    ops = DeviceImageOps(device=0)
    L = ops.L
    cfg, dc = sift._cfg(None, None), sift._desc_cfg()
    frames = make_frames(ops, B, W, H, False)
    crop_features, crop_angle_err, crop_desc_err = check_against_reference(ops, frames)
    p = lambda t: C.c_void_p(t.data_ptr())
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    outs = [(f64(4, B, cap), torch.zeros((B, cap), dtype=torch.uint8, device="cuda"), f64(B, cap, 128), torch.zeros((B,), dtype=torch.int32, device="cuda")) for _ in range(2)]
    det = (f64(3, B, cap), torch.zeros((B, cap), dtype=torch.uint8, device="cuda"), torch.zeros((B, cap, 4), dtype=torch.int16, device="cuda"),
           torch.zeros((B,), dtype=torch.int32, device="cuda"))

    def describe(k=0):
        v, wh, d, n = outs[k]
        assert L.bhip_csift_dev_f32(ops.ctx._h, C.byref(cfg), C.byref(dc), p(frames), W * H, W, W, H, B, p(v[0]), p(v[1]), p(v[2]), p(v[3]), p(wh), p(d), p(n), cap) == 0

    def detect():
        v, wh, where, n = det
        assert L.bhip_sift_detect_dev_f32(ops.ctx._h, C.byref(cfg), p(frames), W * H, W, W, H, B, p(v[0]), p(v[1]), p(v[2]), p(wh), p(where), p(n), cap) == 0

    describe(0)
    describe(1)
    ops.ctx.synchronize()
    counts = outs[0][3].cpu().tolist()
    if max(counts) > cap:
        raise SystemExit("cap %d is below the largest feature count %d" % (cap, max(counts)))
    identical = all(torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v) for u, v in zip(outs[0], outs[1]))
    if not identical:
        raise SystemExit("two calls on the same frames differ")
    variants = [("detect + describe", describe), ("detector alone", detect)]
    ms = {i: [] for i in range(len(variants))}
    for order in (range(len(variants)), reversed(range(len(variants)))):
        for i in order:
            ms[i].append(timed(ops, variants[i][1]))
    ops.ctx.synchronize()
    v = outs[0][0].cpu().numpy()
    per = {}
    for b in range(B):
        for k, c in run_lengths(v[0, b, :counts[b]], v[1, b, :counts[b]], v[2, b, :counts[b]]).items():
            per[k] = per.get(k, 0) + c
    detections = det[3].cpu().tolist()
    frames_s = "%d x %dx%d" % (B, W, H)
    lines = []
    for i, (what, fn) in enumerate(variants):
        lines.append({"op": "sift %s f32" % what, "frames": frames_s, "ms_per_batch": round(min(ms[i]), 3), "ms_per_batch_runs": [round(t, 3) for t in ms[i]],
                      "kernels_ms": kernels(ops, fn), "cap": cap})
    both, alone = min(ms[0]), min(ms[1])
    new = {k: t for k, t in lines[0]["kernels_ms"].items() if k.startswith(("k_sift_orient", "k_sift_angle_scan", "k_sift_describe"))}
    lines.append({"op": "sift orientation + description f32: what they add to the detector", "frames": frames_s, "detect_describe_ms": round(both, 3),
                  "detector_ms": round(alone, 3), "added_ms": round(both - alone, 3), "added_over_detector": round((both - alone) / alone, 4),
                  "new_kernels_ms": new, "new_kernels_sum_ms": round(sum(new.values()), 3),
                  "features_per_frame_min_max": [min(counts), max(counts)], "features_total": int(sum(counts)),
                  "detections_per_frame_min_max": [min(detections), max(detections)], "detections_with_angles_by_angle_count": {str(k): per[k] for k in sorted(per)},
                  "two_calls_identical": True, "crop_check": {"features": crop_features, "max_angle_error_rad": crop_angle_err, "max_descriptor_error": crop_desc_err}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
