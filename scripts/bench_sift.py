#!/usr/bin/env python3
"""Side measurement of the SIFT detector (FactoryInterestPoint.sift) on device-resident frames (bench.py is not involved).

    bench_sift.py [--size WxH] [--batch B] [--out FILE]

Frames: a seeded noise texture blurred with sigma 2 and stretched to 0 .. 255, 16 frames of 1920 x 1080, GrayF32 and GrayU8, at the default
ConfigSiftScaleSpace / ConfigSiftDetector.  In one run, for the scale space alone (DeviceImageOps.siftScaleSpace's C call into preallocated
buffers) and for the whole detector (siftDetect's), each with the fused level kernel and with BHIP_SIFT_TWO_PASS=1 (the chain of the
normalised-convolution launchers plus a subtract; the flag is read on every call, so the two forms alternate inside one process): ms per
batch by device events around REPS calls after WARM calls, the four variants in order and again in reverse so that a drift of the machine
falls on all of them (both figures are kept: their difference is the run-to-run spread).  Then the ctx profiler's ms per kernel from a
separate call of each, and the time of a device-to-device copy that moves the scale space's algorithmic bytes (per octave pixel: 8 for the
first image, 12 for each of the numScales+2 levels: 4 read, 8 written).  Before anything is timed a 304 x 72 crop is checked against
tests/sift_ref.py, and the fused and two-pass outputs of the full frames are compared bit for bit.  One JSON line per image type and
variant, printed and appended to profiles/bench_sift.jsonl (or --out)."""
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
from boofcv_amd import sift  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402

REPS, WARM = 40, 2
OUT = os.path.join(ROOT, "profiles", "bench_sift.jsonl")
FLAG = "BHIP_SIFT_TWO_PASS"


def make_frames(ops, batch, W, H, u8):
    g = torch.Generator(device="cuda").manual_seed(1234)
    t = ops.gaussian(torch.rand((batch, H, W), generator=g, device="cuda", dtype=torch.float32), 2.0, -1)
    lo, hi = t.amin(), t.amax()
    t = ((t - lo) * (255.0 / (hi - lo))).contiguous()
    return t.floor().to(torch.uint8) if u8 else t


def two_pass(on):
    os.environ[FLAG] = "1" if on else "0"


def check_against_reference(ops, frames):
    import sift_ref
    crop = frames[:1, 100:172, 200:504].contiguous()
    img = crop[0].cpu().numpy()
    ss, det = sift_ref.ConfigSS(), sift_ref.ConfigDet()
    space = sift_ref.scale_space(ss, img)
    xy, scale, white, where = sift_ref.detect(ss, det, None, None, space)
    for on in (False, True):
        two_pass(on)
        x, y, s, w, wh, n = (v.cpu().numpy() for v in ops.siftDetect(crop, cap=4096))
        k = int(n[0])
        same = k == len(scale) and np.array_equal(x[0, :k].view(np.uint64), xy[:, 0].view(np.uint64)) and np.array_equal(y[0, :k].view(np.uint64), xy[:, 1].view(np.uint64)) \
            and np.array_equal(s[0, :k].view(np.uint64), scale.view(np.uint64)) and np.array_equal(w[0, :k], white) and np.array_equal(wh[0, :k], where)
        sc, dg, dims = ops.siftScaleSpace(crop)
        imgs = ops.siftImages(sc[0].cpu().numpy(), dims, 6)
        same = same and all(np.array_equal(imgs[o][i].view(np.uint32), space[o][1][i].view(np.uint32)) for o in range(len(space)) for i in range(6))
        if not same:
            raise SystemExit("the crop differs from tests/sift_ref.py (%s)" % ("two-pass" if on else "fused"))


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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--cap", type=int, default=65536)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    B = a.batch
    ops = DeviceImageOps(device=0)
    L = ops.L
    cfg = sift._cfg(None, None)
    dims, sf, df = ops.siftLayout(W, H)
    ns = cfg.numScales
    alg_bytes = B * sum(w * h * (8 + 12 * (ns + 2)) for w, h in dims)
    p = lambda t: C.c_void_p(t.data_ptr())
    lines = []
    for u8 in (False, True):
        frames = make_frames(ops, B, W, H, u8)
        check_against_reference(ops, frames)
        sfn = L.bhip_sift_scale_space_dev_u8 if u8 else L.bhip_sift_scale_space_dev_f32
        dfn = L.bhip_sift_detect_dev_u8 if u8 else L.bhip_sift_detect_dev_f32
        scale = {v: torch.zeros((B, sf), dtype=torch.float32, device="cuda") for v in (False, True)}
        dog = {v: torch.zeros((B, df), dtype=torch.float32, device="cuda") for v in (False, True)}
        det = {v: (torch.zeros((3, B, a.cap), dtype=torch.float64, device="cuda"), torch.zeros((B, a.cap), dtype=torch.uint8, device="cuda"),
                   torch.zeros((B, a.cap, 4), dtype=torch.int16, device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda")) for v in (False, True)}

        def space(on):
            two_pass(on)
            assert sfn(ops.ctx._h, C.byref(cfg), p(frames), W * H, W, W, H, B, p(scale[on]), p(dog[on])) == 0

        def detect(on):
            two_pass(on)
            xyz, wh, where, n = det[on]
            assert dfn(ops.ctx._h, C.byref(cfg), p(frames), W * H, W, W, H, B, p(xyz[0]), p(xyz[1]), p(xyz[2]), p(wh), p(where), p(n), a.cap) == 0

        variants = [("scale space", False, space), ("scale space", True, space), ("detector", False, detect), ("detector", True, detect)]
        ms = {i: [] for i in range(len(variants))}
        for order in (range(len(variants)), reversed(range(len(variants)))):
            for i in order:
                ms[i].append(timed(ops, lambda i=i: variants[i][2](variants[i][1])))
        identical = all(torch.equal(b[False].view(torch.int32), b[True].view(torch.int32)) for b in (scale, dog)) and \
            all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y) for x, y in zip(det[False], det[True]))
        if not identical:
            raise SystemExit("the fused and the two-pass outputs differ")
        counts = det[False][3].cpu().tolist()
        for i, (what, on, fn) in enumerate(variants):
            lines.append({"op": "sift %s %s, %s" % (what, "u8" if u8 else "f32", "two-pass (BHIP_SIFT_TWO_PASS=1)" if on else "fused level kernel"),
                          "frames": "%d x %dx%d" % (B, W, H), "octaves": dims, "ms_per_batch": round(min(ms[i]), 3), "ms_per_batch_runs": [round(v, 3) for v in ms[i]],
                          "kernels_ms": kernels(ops, lambda: fn(on)), "outputs_identical_fused_two_pass": True,
                          "detections_per_frame_min_max": [min(counts), max(counts)], "cap": a.cap})
        fused, chain = min(ms[0]), min(ms[1])
        lines.append({"op": "sift scale space %s: fused level kernel against the two-pass chain" % ("u8" if u8 else "f32"), "frames": "%d x %dx%d" % (B, W, H),
                      "fused_ms": round(fused, 3), "two_pass_ms": round(chain, 3), "two_pass_over_fused": round(chain / fused, 4),
                      "detector_fused_ms": round(min(ms[2]), 3), "detector_two_pass_ms": round(min(ms[3]), 3)})
        del scale, dog, det
    # a device copy that moves the scale space's algorithmic bytes: half of them read, half written
    src = torch.zeros((alg_bytes // 8,), dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    copy_ms = [timed(ops, lambda: dst.copy_(src)) for _ in range(2)]
    lines.append({"op": "device copy of the scale space's algorithmic bytes", "frames": "%d x %dx%d" % (B, W, H), "algorithmic_bytes": alg_bytes,
                  "copy_ms": round(min(copy_ms), 3), "copy_ms_runs": [round(v, 3) for v in copy_ms], "copy_gbps": round(alg_bytes / (min(copy_ms) * 1e-3) / 1e9, 1)})
    two_pass(False)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for ln in lines:
            s = json.dumps(ln)
            print(s, flush=True)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
