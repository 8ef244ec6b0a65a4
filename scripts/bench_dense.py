#!/usr/bin/env python3
"""Side measurement of the dense descriptors (FactoryDescribeImageDense.hog, both variants, and .sift) on device-resident frames (bench.py is not
involved).

    bench_dense.py [--size WxH] [--batch B] [--out FILE]

Frames: the seeded noise texture of scripts/bench_sift.py (blurred with sigma 2, stretched to 0 .. 255), 16 frames of 1920 x 1080, GrayF32 and
GrayU8, for the default fast HOG, the default standard HOG and the default dense SIFT.  Per variant: ms per batch by device events around REPS calls
after WARM calls into preallocated buffers, once in the listed order and once in reverse so that a drift of the machine falls on all (both
figures are kept: their difference is the run-to-run spread); beside it the time of a device-to-device copy of the bytes the call must move --
the frames once, the descriptors once -- timed the same way, and the ratio of the two; then the ctx profiler's ms per kernel from a separate
call.  Before anything is timed, 64 descriptors at fixed spread-out indices of frame 0 are compared with tests/dense_ref.py evaluated on the
descriptor's own window (the Python restatement is too slow for a whole frame): locations exactly, elements within 1e-12; and two calls on the
full frames are compared bit for bit.  One JSON line per variant, printed and appended to profiles/bench_dense.jsonl (or --out)."""
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
from boofcv_amd import dense  # noqa: E402
from boofcv_amd.device import DeviceImageOps  # noqa: E402
from bench_sift import kernels, make_frames  # noqa: E402

REPS, WARM, CHECKED = 10, 2, 64
OUT = os.path.join(ROOT, "profiles", "bench_dense.jsonl")


def timed(ops, fn):
    for _ in range(WARM):
        fn()
    ops.ctx.synchronize()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / REPS


def reference_descriptor(kind, frame, x, y):
    """the descriptor whose location is (x, y), from the window's own pixels and one more on every side that the image has"""
    import dense_ref as dr
    H, W = frame.shape
    u8 = frame.dtype == np.uint8
    if kind == "sift":
        alg = dr.DenseSift()
        left, top, w, h = x - 8, y - 8, 16, 16
    else:
        alg = dr.Hog(fastVariant=(kind == "hog fast"))
        left, top, w, h = x, y, 24, 24
    x0, y0, x1, y1 = max(left - 1, 0), max(top - 1, 0), min(left + w + 1, W), min(top + h + 1, H)
    crop = frame[y0:y1, x0:x1]
    ox, oy = left - x0, top - y0
    if kind == "sift":
        dx, dy = dr.gradient_s16(crop) if u8 else dr.gradient_f32(crop)
        angle, magnitude = alg.precompute_angles(dx, dy)
        return dr.normalize_descriptor(alg.descriptor_raw(angle, magnitude, ox + 8, oy + 8), 0.2)
    findex, sumsq = alg.pixel_features(*dr.gradient_f32(crop))
    if alg.fast:
        cells = alg.cell_histograms(findex[oy:oy + h, ox:ox + w], sumsq[oy:oy + h, ox:ox + w])
        return alg.block_descriptor(cells, 0, 0)
    return dr.normalize_descriptor(alg.std_descriptor_raw(findex, sumsq, ox, oy), 0.2)


def check_against_reference(kind, frame, desc, xy, layout):
    n = len(desc)
    picks = sorted({int(round(i * (n - 1) / (CHECKED - 1))) for i in range(CHECKED)})
    worst, identical = 0.0, True
    for k in picks:
        if tuple(int(v) for v in xy[k]) != layout[k]:
            raise SystemExit("%s: descriptor %d is at %s, the grid says %s" % (kind, k, xy[k].tolist(), layout[k]))
        ref = reference_descriptor(kind, frame, *layout[k])
        worst = max(worst, float(np.abs(ref - desc[k]).max()))
        identical = identical and np.array_equal(ref.view(np.uint64), np.ascontiguousarray(desc[k]).view(np.uint64))
    if worst > 1e-12:
        raise SystemExit("%s: descriptors differ from tests/dense_ref.py by %g" % (kind, worst))
    return len(picks), worst, identical


def main():
    import dense_ref as dr
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    B = a.batch
    ops = DeviceImageOps(device=0)
    frames = {"f32": make_frames(ops, B, W, H, False), "u8": make_frames(ops, B, W, H, True)}
    configs = {"hog fast": dense.ConfigDenseHoG(), "hog standard": dense.ConfigDenseHoG(fastVariant=False), "sift": dense.ConfigDenseSift()}
    layouts = {"hog fast": dr.Hog().layout(W, H)[2], "hog standard": dr.Hog(fastVariant=False).layout(W, H)[2], "sift": dr.DenseSift().layout(W, H)[2]}
    variants = [(kind, t) for kind in configs for t in ("f32", "u8")]
    calls, checks, shapes = {}, {}, {}
    for kind, t in variants:
        src, cfg = frames[t], configs[kind]
        run = (lambda s=src, c=cfg: ops.denseSift(s, c)) if kind == "sift" else (lambda s=src, c=cfg: ops.denseHog(s, c))
        desc, xy, count = run()
        desc2, xy2, count2 = run()
        ops.ctx.synchronize()
        n, dof = desc.shape[1], desc.shape[2]
        if count.cpu().tolist() != [len(layouts[kind])] * B or n != len(layouts[kind]):
            raise SystemExit("%s %s: counts %s, the grid has %d" % (kind, t, count.cpu().tolist()[:4], len(layouts[kind])))
        if not (torch.equal(desc.view(torch.int64), desc2.view(torch.int64)) and torch.equal(xy, xy2)):
            raise SystemExit("%s %s: two calls on the same frames differ" % (kind, t))
        checks[(kind, t)] = check_against_reference("sift" if kind == "sift" else kind, src[0].cpu().numpy(), desc[0].cpu().numpy(), xy[0].cpu().numpy(), layouts[kind])
        del desc2, xy2
        # the timed call writes into the buffers of the first one
        L, h = ops.L, ops.ctx._h
        import ctypes as C
        p = lambda v: C.c_void_p(v.data_ptr())
        if kind == "sift":
            g, rest = dense._sift_args(cfg)
            fn = L.bhip_dense_sift_dev_u8 if t == "u8" else L.bhip_dense_sift_dev_f32
            call = lambda fn=fn, g=g, rest=rest, s=src, d=desc, x=xy, c=count, n=n: fn(h, *g, *rest, p(s), W * H, W, W, H, B, p(d), p(x), p(c), n)
        else:
            fn = L.bhip_dense_hog_dev_u8 if t == "u8" else L.bhip_dense_hog_dev_f32
            call = lambda fn=fn, g=dense._hog_args(cfg), s=src, d=desc, x=xy, c=count, n=n: fn(h, *g, p(s), W * H, W, W, H, B, p(d), p(x), p(c), n, None)
        spare_in, spare_out = torch.empty_like(src), torch.empty_like(desc)
        calls[(kind, t)] = (call, lambda s=src, d=desc, si=spare_in, so=spare_out: (si.copy_(s), so.copy_(d)))
        shapes[(kind, t)] = (n, dof, src.numel() * src.element_size(), desc.numel() * 8)
        if call() != 0:
            raise SystemExit("%s %s: the direct call failed" % (kind, t))
    ms, copy_ms = {v: [] for v in variants}, {v: [] for v in variants}
    for order in (variants, list(reversed(variants))):
        for v in order:
            ms[v].append(timed(ops, calls[v][0]))
            copy_ms[v].append(timed(ops, calls[v][1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for v in variants:
            kind, t = v
            n, dof, in_bytes, out_bytes = shapes[v]
            best, copy = min(ms[v]), min(copy_ms[v])
            checked, worst, identical = checks[v]
            line = {"op": "dense %s %s" % (kind, t), "frames": "%d x %dx%d" % (B, W, H), "descriptors_per_frame": n, "dof": dof,
                    "ms_per_batch": round(best, 3), "ms_per_batch_runs": [round(x, 3) for x in ms[v]],
                    "bytes_in": in_bytes, "bytes_out": out_bytes, "copy_ms": round(copy, 3), "copy_ms_runs": [round(x, 3) for x in copy_ms[v]],
                    "ms_over_copy": round(best / copy, 2), "kernels_ms": kernels(ops, calls[v][0]), "two_calls_identical": True,
                    "reference_check": {"descriptors": checked, "max_element_difference": worst, "bit_identical": bool(identical)}}
            s = json.dumps(line)
            print(s, flush=True)
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
