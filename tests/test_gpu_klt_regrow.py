"""GPU: the track table of the pyramid KLT tracker regrows (kltGrow in csrc/cabi_klt.hip) while it holds live tracks, from both call sites:
bhip_klt_add_tracks (case add_tracks) and kltSpawnFrom (case spawn).  A grow copies 19 per-track arrays row by row into a wider table, keeps
the per-sequence counters and appends the new slots to every sequence's unused list; nothing else in the suite does that with tracks in the
table.  DeviceKltTracker with three sequences of different 320x240 frames, scales 1,2,4, template radius 2, GrayF32 and GrayU8, against
tests/klt_ref.py / tests/klt_u8_ref.py with the bit-for-bit comparison of tests/test_gpu_klt.py after every step.

Reference figures next to BHIP_KLT_INITIAL_CAPACITY (1024), GrayF32 / GrayU8 (CPU run of this recipe):
add_tracks: sequence 0 holds 591 / 590 active tracks (600 slots with the just dropped ones: 424 unused) when 700 more are added, sequence 1
holds 26 / 27; 1322 tracks are tracked in the next frame.
spawn: sequence 0 holds 889 / 888 (900 slots: 124 unused) when spawnTracks finds 600 / 592 corners for it; sequences 1 and 2 get 570 + 485 /
571 + 488 new tracks; 2564 / 2559 tracks are tracked in the next frame.  Either way the table goes from 1024 to 1792 slots per sequence.
The preconditions below are asserted from the reference on every run."""
import ctypes as C

import numpy as np
import pytest

import klt_ref as kr
import klt_u8_ref as ku
import test_gpu_klt as tg      # scene, _snapshot, _compare_lists, same(): the F32 file's recipe and its bit comparison
from boofcv_amd import _lib

pytestmark = pytest.mark.gpu
SCALES, DET = tg.SCALES, tg.DET
R, B, FW, FH = 2, 3, 320, 240
CAP = _lib.BHIP_KLT_INITIAL_CAPACITY
SEEDS = [234, 235, 236]                    # one scene per sequence
SHIFTS = [(3, -2), (7, 5), (2, 3)]         # and one motion

# `grow` marks the call that has to regrow the table
PLANS = {
    "add_tracks": [("process", 0), ("add", {0: 600, 1: 40}), ("process", 1), ("add", {0: 700, 2: 5}, "grow"), ("process", 2), ("process", 3),
                   ("drop",), ("process", 4)],
    "spawn": [("process", 0), ("add", {0: 900, 1: 40}), ("process", 1), ("spawn", "grow"), ("process", 2), ("process", 3), ("drop",), ("process", 4)],
}
MIN_ACTIVE = {"add_tracks": 500, "spawn": 800}


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd import device
    return device, torch


def _frames(orc, b, u8):
    """five 320x240 windows of sequence b's scene: the window moves by SHIFTS[b], then by a pixel or two more each frame.  Sequences 1 and 2
    are textured in a part of the scene only (the rest is flat: no corners, zero determinants), which keeps the reference run short."""
    sc = tg._scene(orc, SEEDS[b]).copy()
    if b == 1:
        sc[:, 200:] = 128
    if b == 2:
        sc[:160, :] = 128
    sx, sy = SHIFTS[b]
    moves = [(0, 0), (sx, sy), (sx + 1, sy + 1), (sx + 2, sy), (sx + 2, sy + 1)]
    out = [np.ascontiguousarray(sc[20 + my:20 + FH + my, 20 + mx:20 + FW + mx]) for mx, my in moves]
    if u8:
        out = [np.clip(np.rint(f), 0, 255).astype(np.uint8) for f in out]
    return out


def _points(step, counts):
    """addTrack requests of one step: in-frame positions with fractional parts, the sequences interleaved (fixed seed)"""
    rng = np.random.default_rng(4000 + step)
    seq = np.concatenate([np.full(n, s, np.int32) for s, n in sorted(counts.items())])
    xy = rng.uniform((0.0, 0.0), (float(FW), float(FH)), size=(len(seq), 2))
    assert ((xy >= 0) & (xy < (FW, FH))).all() and (xy != np.floor(xy)).all()
    order = rng.permutation(len(seq))
    return seq[order], xy[order]


def _drop_by_id(ref, fid):
    """bhip_klt_drop_tracks' rule on the reference: the first active track with that featureId (added tracks all carry -1)"""
    ids = [t.featureId for t in ref.active]
    return fid in ids and ref.dropTrack(ref.active[ids.index(fid)])


_ref_cache = {}


def _reference(orc, case, u8):
    """the plan on three single-sequence reference trackers -> one record per step: the inputs the device run repeats, the lists after the
    step, and the figures the preconditions are stated on.  klt_ref.Thrown propagates: such inputs are not allowed."""
    key = (case, u8)
    if key in _ref_cache:
        return _ref_cache[key]
    make = ku.PointTrackerKltPyramidU8 if u8 else kr.PointTrackerKltPyramid
    refs = [make(orc, SCALES, R, kr.KltConfig(), DET["detectRadius"], DET["detectThreshold"], DET["detectBorder"]) for _ in range(B)]
    frames = [_frames(orc, b, u8) for b in range(B)]
    steps = []
    for i, op in enumerate(PLANS[case]):
        rec = dict(op=op[0], grow="grow" in op, before=[len(r.active) for r in refs])
        # slots the device has left: the tracks the last process() dropped return to the unused list only at the next process()
        rec["held"] = [len(r.active) + len(r.dropped) for r in refs]
        if op[0] == "process":
            t0 = [(r.klt.iterations, r.klt.borderIterations) for r in refs]
            for b in range(B):
                refs[b].process(frames[b][op[1]])
            rec["frame"] = op[1]
            rec["stats"] = (sum(rec["before"]), sum(r.klt.iterations - t[0] for r, t in zip(refs, t0)), sum(r.klt.borderIterations - t[1] for r, t in zip(refs, t0)))
        elif op[0] == "add":
            rec["seq"], rec["xy"] = _points(i, op[1])
            rec["asked"] = [op[1].get(b, 0) for b in range(B)]
            for s, (x, y) in zip(rec["seq"], rec["xy"]):
                assert refs[s].addTrack(x, y) is not None
        elif op[0] == "spawn":
            for r in refs:
                r.spawnTracks()
            rec["asked"] = [len(r.spawned) for r in refs]
        else:
            ids = [t.featureId for t in refs[0].active]
            rec["ids"] = [ids[0], ids[len(ids) // 2], ids[-1]]
            assert all(_drop_by_id(refs[0], fid) for fid in rec["ids"])
        rec["lists"] = [tg._snapshot(r) for r in refs]
        steps.append(rec)
    _ref_cache[key] = frames, steps
    return _ref_cache[key]


def _preconditions(case, steps):
    """the reference side shows that the growing call finds a table with live tracks in it and asks for more slots than it has"""
    grow = [s for s in steps if s["grow"]]
    assert len(grow) == 1
    g = grow[0]
    assert g["before"][0] >= MIN_ACTIVE[case], g["before"]
    assert g["asked"][0] > CAP - g["before"][0], (g["asked"], g["before"])
    assert g["asked"][0] > CAP - g["held"][0]                      # also with the slots of the just dropped tracks still out
    assert g["before"][1] >= 10                                    # another sequence has live tracks of its own
    if case == "spawn":
        assert g["asked"][1] + g["asked"][2] >= 100, g["asked"]    # and their lists move too
    for s in steps:                                                # no step before it can have grown the table
        if s is g:
            break
        if s["op"] in ("add", "spawn"):
            assert all(a <= CAP - h for a, h in zip(s["asked"], s["held"])), (s["asked"], s["held"])
    after = steps[steps.index(g) + 1]
    assert after["op"] == "process" and after["stats"][0] > CAP and after["stats"][2] > 100   # the grown table tracks, border form included


def _slots(trk, u8):
    """slots per sequence of the device table (bhip_klt_dev_view)"""
    n = C.c_int(0)
    view = trk.L.bhip_klt_dev_view_u8 if u8 else trk.L.bhip_klt_dev_view
    assert view(trk._h, None, None, None, None, None, None, None, None, C.byref(n), None) == 0
    return n.value


def _capture(trk, seqs):
    """ids, positions and the per-layer templates (desc, derivX, derivY; Gxx, Gyy, Gxy) of every active track of these sequences"""
    out = {}
    for b in seqs:
        act = trk.active(b)
        out[b] = dict(featureId=act["featureId"].copy(), xy=act["xy"].copy(), layers=[tuple(a.copy() for a in trk.templates(b, l, 0)) for l in range(len(SCALES))])
    return out


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _unchanged_across_grow(before, after):
    """the tracks that existed before the growing call: same ids, same position bits, templates bit-identical (NaN-marked ones included)"""
    nan_rows = 0
    for b, old in before.items():
        new = after[b]
        n = len(old["featureId"])
        assert n > 0 and len(new["featureId"]) >= n
        assert np.array_equal(new["featureId"][:n], old["featureId"])
        assert np.array_equal(_u32(new["xy"][:n]), _u32(old["xy"]))
        for l, ((t0, g0), (t1, g1)) in enumerate(zip(old["layers"], new["layers"])):
            assert t0.shape[0] == n and np.array_equal(_u32(t1[:n]), _u32(t0)), (b, l)
            assert np.array_equal(_u32(g1[:n]), _u32(g0)), (b, l)
            nan_rows += int(np.isnan(t0).any(axis=(1, 2)).sum())
    assert nan_rows >= 20      # border templates are among the rows that moved


@pytest.mark.parametrize("u8", [False, True], ids=["GrayF32", "GrayU8"])
@pytest.mark.parametrize("case", list(PLANS))
def test_table_grows_with_live_tracks(dev, api, orc, case, u8):
    device, torch = dev
    frames, steps = _reference(orc, case, u8)
    _preconditions(case, steps)
    trk = device.DeviceKltTracker(SCALES, R, api.KltConfig(), **DET)
    for i, s in enumerate(steps):
        before = _capture(trk, (0, 1)) if s["grow"] else None
        if s["grow"]:
            assert _slots(trk, u8) == CAP                          # nothing has grown the table yet
        if s["op"] == "process":
            trk.process(torch.from_numpy(np.stack([frames[b][s["frame"]] for b in range(B)])).cuda())
            assert trk.stats() == s["stats"], (i, trk.stats(), s["stats"])   # the same Lucas-Kanade iterations, the same number in the border form
        elif s["op"] == "add":
            assert trk.addTracks(s["seq"], s["xy"]).all()
        elif s["op"] == "spawn":
            trk.spawn()
        else:
            assert trk.dropTracks([0, 0, 0], s["ids"]).all()
        if s["grow"]:
            assert _slots(trk, u8) > CAP
            _unchanged_across_grow(before, _capture(trk, (0, 1)))
        a, sp, d = trk.counts()
        for b in range(B):
            got = trk.active(b), trk.spawned(b), trk.dropped(b)
            assert (a[b], sp[b], d[b]) == tuple(len(x["featureId"]) for x in got), (i, b)
            tg._compare_lists(got[0], got[1], got[2], s["lists"][b])
    trk.close()


def test_list_comparison_notices_a_permuted_track(orc):
    """(no device call) the comparison the cases rest on fails when two tracks of a reference snapshot change places, or one position
    changes in its last bit: what a wrong row pitch or a wrong slot in a regrown table would look like from outside"""
    _, steps = _reference(orc, "add_tracks", False)
    snap = steps[-2]["lists"][0]               # after the three dropTracks calls: no new tracks, the tracks frame 3 dropped still listed
    act, spw, drp, err = snap
    assert len(act) > 1000 and not spw and len(drp) > 0

    def as_got(a):
        return dict(featureId=np.array([t[0] for t in a], np.int64), xy=np.array([t[1:3] for t in a], np.float32).reshape(-1, 2),
                    fault=np.zeros(len(a), np.int32), error=np.array(err, np.float32))

    none = dict(featureId=np.zeros(0, np.int64), xy=np.zeros((0, 2), np.float32))
    dropped = dict(featureId=np.array([t[0] for t in drp], np.int64), xy=np.array([t[1:3] for t in drp], np.float32).reshape(-1, 2),
                   fault=np.array([t[3] for t in drp], np.int32))
    tg._compare_lists(as_got(act), none, dropped, snap)
    swapped = list(act)
    swapped[3], swapped[700] = swapped[700], swapped[3]
    with pytest.raises(AssertionError):
        tg._compare_lists(as_got(swapped), none, dropped, snap)
    nudged = as_got(act)
    nudged["xy"][900, 1] = np.nextafter(nudged["xy"][900, 1], np.float32(1e9))
    with pytest.raises(AssertionError):
        tg._compare_lists(nudged, none, dropped, snap)
    with pytest.raises(AssertionError):
        tg._compare_lists(as_got(act), none, dict(dropped, fault=dropped["fault"] + 1), snap)
