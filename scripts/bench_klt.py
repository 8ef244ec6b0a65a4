#!/usr/bin/env python3
"""Side measurement of the pyramid KLT tracker on 64 device-resident 1920x1080 sequences (bench.py is not involved).

Every sequence has a scene of its own (uniform noise blurred with gaussian(-1, 3), 64 pixels larger than the frame in both directions); frame k of
a sequence is the 1920x1080 window of its scene moved by whole pixels, so the true motion is known.  Scales 1,2,4, template radius 2.  Tracks are
spawned on the first frame (Shi-Tomasi radius 1, strict non-max of --detect-radius, threshold 1); every timed step is one process() of the 64
next frames.  Reported per step: ctx-profiler ms split into pyramid, gradient, track, re-describe and compaction, the wall time between HIP events,
tracks per second, the mean Lucas-Kanade iteration count per track and the share of SUCCESS tracks that lie within 0.25 px of the true motion.
One JSON line per run, printed and appended to --out (default profiles/bench_klt.jsonl).

--image-type u8 runs the same scenes rounded to bytes through the GrayU8 tracker (uint8 pyramid, int16 Sobel); the line then carries "imageType".
--host-steps N adds N process() calls from page-locked host frames (bhip_klt_process_f32 / _u8: upload, step, synchronise) and reports
"host_steps_per_second" / "host_frames_per_second", the figure a caller with a camera stream sees."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boofcv_amd.device import DeviceImageOps, DeviceKltTracker  # noqa: E402

B, W, H, MARGIN = 64, 1920, 1080, 64
GROUPS = (("track", ("k_klt_track", "k_klt_track_u8")), ("redescribe", ("k_klt_describe", "k_klt_describe_u8")), ("compaction", ("k_klt_compact",)),
          ("gradient", ("k_sobel", "k_sobel_u8")))


def host_steps(ops, trk, frame, n, u8):
    """n process() calls from page-locked host frames on a tracker of the same configuration -> steps per second (wall clock, each call synchronises)"""
    import time
    from boofcv_amd import _lib
    L = ops.L
    h = C.c_void_p()
    cfg = trk.config._c()
    sc = (C.c_int * 3)(1, 2, 4)
    create, process = (L.bhip_klt_create_u8, L.bhip_klt_process_u8) if u8 else (L.bhip_klt_create, L.bhip_klt_process_f32)
    assert create(ops.ctx._h, C.byref(cfg), 2, sc, 3, trk.detectRadius, trk.detectThreshold, trk.detectBorder, W, H, B, C.byref(h)) == 0
    pinned = [frame(k).contiguous().cpu().pin_memory() for k in (0, 1)]
    elem = C.c_uint8 if u8 else C.c_float
    ptrs = [(C.POINTER(elem) * B)(*[C.cast(p[b].data_ptr(), C.POINTER(elem)) for b in range(B)]) for p in pinned]
    assert process(h, ptrs[0], None, None) == 0
    assert L.bhip_klt_spawn(h, -1) == 0
    assert process(h, ptrs[1], None, None) == 0
    t0 = time.perf_counter()
    for k in range(n):
        assert process(h, ptrs[k % 2], None, None) == 0
    dt = time.perf_counter() - t0
    L.bhip_klt_destroy(h)
    return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detect-radius", type=int, default=20, help="non-max radius of the spawn: 20 gives about a thousand tracks per 1080p frame, 3 a dense field")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_klt.jsonl"))
    ap.add_argument("--image-type", choices=("f32", "u8"), default="f32", help="f32: GrayF32 frames; u8: the same scenes rounded to bytes, GrayU8 tracker")
    ap.add_argument("--host-steps", type=int, default=0, help="also time this many process() calls from page-locked host frames")
    a = ap.parse_args()
    u8 = a.image_type == "u8"

    ops = DeviceImageOps(device=0)
    gen = torch.Generator(device="cuda").manual_seed(11)
    scene = ops.gaussian(torch.rand((B, H + MARGIN, W + MARGIN), device="cuda", generator=gen) * 255, -1, 3)
    ops.ctx.synchronize()
    if u8:
        scene = scene.round().clamp(0, 255).to(torch.uint8)
        torch.cuda.synchronize()
    trk = DeviceKltTracker([1, 2, 4], 2, None, detectRadius=a.detect_radius, detectThreshold=1.0, ctx=ops.ctx)

    # the window walks one pixel right and down per frame and turns round before it leaves the scene
    path = [(MARGIN // 2, MARGIN // 2)]
    vx = vy = 1
    for _ in range(a.warmup + 2 * a.steps):
        x, y = path[-1]
        if not 0 <= x + vx <= MARGIN:
            vx = -vx
        if not 0 <= y + 2 * vy <= MARGIN:
            vy = -vy
        path.append((x + vx, y + 2 * vy))

    def frame(k):
        x, y = path[k]
        return scene[:, y:y + H, x:x + W]   # a view: rows are MARGIN floats longer than the frame

    trk.process(frame(0))
    trk.spawn()
    spawned = trk.counts()[0].copy()
    start = [trk.active(b) for b in (0, B - 1)]
    for k in range(1, a.warmup + 1):
        trk.process(frame(k))
    tracks_before = int(trk.counts()[0].sum())
    torch.cuda.synchronize()
    # first the wall time with the profiler off, then the same number of steps with every launch bracketed by events
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(a.warmup + 1, a.warmup + a.steps + 1):
        trk.process(frame(k))
    t1.record()
    torch.cuda.synchronize()
    wall = t0.elapsed_time(t1) / a.steps
    ops.ctx.profile(True)
    ops.ctx.profileReset()
    for k in range(a.warmup + a.steps + 1, a.warmup + 2 * a.steps + 1):
        trk.process(frame(k))
    ops.ctx.synchronize()
    prof = ops.ctx.profileReport()
    ops.ctx.profile(False)
    n_tracked, iters, border = trk.stats()          # of the last step
    tracks_after = int(trk.counts()[0].sum())

    ms = {name: 0.0 for name, _ in GROUPS}
    ms["pyramid"] = 0.0
    for tag, v in prof.items():
        for name, tags in GROUPS:
            if tag in tags:
                ms[name] += v["ms"] / a.steps
                break
        else:
            ms["pyramid"] += v["ms"] / a.steps
    # accuracy: the tracks of two sequences that are still alive, against the known motion
    near = alive = 0
    last = path[a.warmup + 2 * a.steps]
    for b, st in zip((0, B - 1), start):
        now = trk.active(b)
        pos = dict(zip(st["featureId"].tolist(), st["xy"]))
        for i, xy in zip(now["featureId"].tolist(), now["xy"]):
            tx, ty = pos[i][0] - (last[0] - path[0][0]), pos[i][1] - (last[1] - path[0][1])
            alive += 1
            near += abs(xy[0] - tx) < 0.25 and abs(xy[1] - ty) < 0.25
    front = ms["pyramid"] + ms["gradient"]
    tracking = ms["track"] + ms["redescribe"] + ms["compaction"]
    mean_tracks = (tracks_before + tracks_after) / 2
    out = {"bench": "klt", "frames": "%d x %dx%d" % (B, W, H), "scales": [1, 2, 4], "templateRadius": 2, "detectRadius": a.detect_radius, "steps": a.steps,
           "spawned_per_frame": round(float(spawned.mean()), 1), "tracks_before": tracks_before, "tracks_after": tracks_after,
           "ms_per_step": {k: round(v, 4) for k, v in ms.items()}, "front_end_ms": round(front, 4), "tracking_ms": round(tracking, 4),
           "tracking_over_front_end": round(tracking / front, 3) if front > 0 else None, "wall_ms_per_step": round(wall, 4),
           "tracks_per_second": round(mean_tracks / (wall * 1e-3)), "tracks_per_second_tracking_kernels": round(mean_tracks / (tracking * 1e-3)) if tracking > 0 else None,
           "mean_iterations_per_track": round(iters / max(n_tracked, 1), 3), "border_iteration_share": round(border / max(iters, 1), 4),
           "alive_checked": alive, "within_quarter_pixel": round(near / max(alive, 1), 4)}
    if u8:
        out["imageType"] = "u8"
    if a.host_steps > 0:
        sps = host_steps(ops, trk, frame, a.host_steps, u8)
        out["host_steps_per_second"] = round(sps, 2)
        out["host_frames_per_second"] = round(sps * B, 1)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    trk.close()


if __name__ == "__main__":
    main()
