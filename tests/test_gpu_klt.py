"""GPU: the pyramid KLT tracker (klt.hip behind bhip_klt_* / api.KltTracker / api.PointTrackerKltPyramid / device.DeviceKltTracker) and the
EXTENDED-border Sobel, bit for bit against tests/klt_ref.py.  There is no tolerance anywhere: floats are compared through their uint32 words
(NaN patterns through np.isnan masks), because no operation on the path is allowed to differ from the single-threaded Java arithmetic.

Inputs of the end-to-end cases: scene = gaussian_blur(noise_image(360, 280, 234, 0, 255), -1, 3); frame 0 = scene[20:260, 20:340]; later frames are the
same window moved by whole pixels, so the true motion is known.  Scales 1,2,4; spawn = Shi-Tomasi radius 1, strict non-max radius 3, threshold 1,
border 0.  Before anything is compared the reference side must show what the case is there to exercise (enough successes near the true motion,
NaN-marked border templates, border-form iterations, every fault code) -- see _conditions()."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import klt_ref as kr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SCALES = [1, 2, 4]
DET = dict(detectRadius=3, detectThreshold=1.0, detectBorder=0)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd import device
    return device, torch


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """float32 arrays equal bit for bit, NaN where and only where the other has NaN"""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


# ---------------------------------------------------------------------------------------------------------------- EXTENDED Sobel
SOBEL_SHAPES = [(37, 23), (256, 9), (261, 35), (3, 3), (1, 5)]   # the shapes of test_gpu_corners_u8.GRAD_CASES


def _img(orc, w, h, seed):
    return orc.noise_image(w, h, seed, 0, 255).array().copy()


@pytest.mark.parametrize("shape", SOBEL_SHAPES)
@pytest.mark.parametrize("sub", [False, True])
def test_sobel_extended_host(api, orc, shape, sub):
    W, H = shape
    img = _img(orc, W, H, 11 + W)
    want = kr.sobel_extended(orc, img)
    src = api.GrayF32.wrap(img)
    X, Y = api.GrayF32(W, H), api.GrayF32(W, H)
    if sub:   # views with odd offsets and stride > width
        big = api.GrayF32(W + 5, H + 3)
        src = big.subimage(1, 2, 1 + W, 2 + H)
        src.array()[:, :] = img
        bx, by = api.GrayF32(W + 7, H + 4), api.GrayF32(W + 7, H + 4)
        X, Y = bx.subimage(3, 1, 3 + W, 1 + H), by.subimage(3, 1, 3 + W, 1 + H)
    api.GradientSobel.process(src, X, Y, api.BorderType.EXTENDED)
    assert same(X.array(), want[0]) and same(Y.array(), want[1])
    # borders null and ImageBorderValue(0) on the same input give what they gave before (the oracle's gradient)
    for border, zero in ((None, False), (0, True)):
        X.array()[:, :] = 1234
        Y.array()[:, :] = -77
        api.GradientSobel.process(src, X, Y, border)
        gx, gy = orc.gradient("sobel", orc.Gray.from_array(img), zero)
        ex, ey = gx.array().copy(), gy.array().copy()
        if not zero:
            frame = np.ones((H, W), bool)
            if H > 2 and W > 2:
                frame[1:-1, 1:-1] = False
            ex[frame], ey[frame] = 1234, -77
        assert same(X.array(), ex) and same(Y.array(), ey)
    with pytest.raises(RuntimeError):   # the three-tap gradient has another border construction: not on the GPU
        api.GradientThree.process(src, X, Y, api.BorderType.EXTENDED)


@pytest.mark.parametrize("shape", SOBEL_SHAPES)
def test_sobel_extended_device(dev, orc, shape):
    device, torch = dev
    ops = device.DeviceImageOps(device=0)
    W, H = shape
    imgs = np.stack([_img(orc, W, H, 40 + W + b) for b in range(3)])
    want = [kr.sobel_extended(orc, im) for im in imgs]
    t = torch.from_numpy(imgs).cuda()
    dx, dy = ops.sobel(t, border="EXTENDED")
    ops.ctx.synchronize()
    for b in range(3):
        assert same(dx[b].cpu().numpy(), want[b][0]) and same(dy[b].cpu().numpy(), want[b][1])
    # strided views: rows of a wider buffer (the general kernel), outputs too
    big = torch.zeros((3, H + 2, W + 6), device="cuda")
    big[:, 1:1 + H, 3:3 + W] = t
    ox, oy = torch.zeros((3, H, W + 5), device="cuda"), torch.zeros((3, H, W + 5), device="cuda")
    torch.cuda.synchronize()
    ops.sobel(big[:, 1:1 + H, 3:3 + W], border="EXTENDED", dx=ox[:, :, 2:2 + W], dy=oy[:, :, 2:2 + W])
    ops.ctx.synchronize()
    for b in range(3):
        assert same(ox[b, :, 2:2 + W].cpu().numpy(), want[b][0]) and same(oy[b, :, 2:2 + W].cpu().numpy(), want[b][1])
    # borders None / 0 unchanged
    for border, zero in ((None, False), (0, True)):
        dx, dy = ops.sobel(t, border=border)
        ops.ctx.synchronize()
        for b in range(3):
            gx, gy = orc.gradient("sobel", orc.Gray.from_array(imgs[b]), zero)
            assert same(dx[b].cpu().numpy(), gx.array()) and same(dy[b].cpu().numpy(), gy.array())


# ---------------------------------------------------------------------------------------------------------------- stage level
SW, SH = 40, 50


def _positions(r, W, H):
    """fully inside, every edge and corner, exactly on the allowed* and outside* bounds, integer and fractional"""
    aL, aR, aT, aB = r, W - r - 1, r, H - r - 1
    oL, oR, oT, oB = -r, W + r - 1, -r, H + r - 1
    xs = [W / 2, 20.6, aL, aR, aL - 0.5, aR + 0.5, aL + 0.25, aR - 0.25, oL, oR, oL + 0.3, oR - 0.3, oL - 0.01, oR + 0.01, 0, W - 1, 0.75, W - 1.75]
    ys = [H / 2, 25.1, aT, aB, aT - 0.5, aB + 0.5, aT + 0.25, aB - 0.25, oT, oB, oT + 0.3, oB - 0.3, oT - 0.01, oB + 0.01, 0, H - 1, 0.75, H - 1.75]
    pts = [(x, H / 2) for x in xs] + [(W / 2, y) for y in ys] + [(x, y) for x, y in zip(xs, ys)] + [(x, y) for x, y in zip(xs, reversed(ys))]
    return np.array(pts, np.float32)


def _stage_images(orc, sub, api):
    img = orc.noise_image(SW, SH, 234, 0, 100).array().copy()
    dx, dy = kr.sobel_extended(orc, img)
    if not sub:
        return img, dx, dy, api.GrayF32.wrap(img), api.GrayF32.wrap(dx), api.GrayF32.wrap(dy)
    views = []
    for a, (px, py) in ((img, (3, 2)), (dx, (5, 1)), (dy, (5, 1))):   # derivX / derivY share startIndex and stride; the image has its own
        big = api.GrayF32(SW + 9, SH + 4)
        v = big.subimage(px, py, px + SW, py + SH)
        v.array()[:, :] = a
        views.append(v)
    return (img, dx, dy) + tuple(views)


def _ref_describe(img, dx, dy, cfg, r, xy):
    t = kr.KltTracker(cfg)
    t.setImage(img, dx, dy)
    feats, oks = [], []
    for x, y in xy:
        f = kr.KltFeature(r)
        f.setPosition(x, y)
        try:
            oks.append(1 if t.setDescription(f) else 0)
        except kr.Thrown:
            oks.append(2)
        feats.append(f)
    return feats, np.array(oks, np.uint8)


STAGE_CONFIGS = {
    "default": dict(),
    "unit_test": dict(maxPerPixelError=10, maxIterations=30, minDeterminant=0.01, minPositionDelta=0.001),
    "one_iteration": dict(maxIterations=1),
    "fifty_iterations": dict(maxIterations=50, minPositionDelta=1e-6),
    "det_zero": dict(minDeterminant=0.0),
    "det_large": dict(minDeterminant=1e7),
    "small_error": dict(maxPerPixelError=0.5),
}


OFFSETS = [(0.3, -0.2), (-1.3, 1.2), (2.6, 2.1), (-4.5, 3.0), (9.0, -7.0)]


def _stage_reference(orc, r, kw):
    """klt_ref on the stage-level inputs: the described features, and every one of them tracked from displaced starts (from the reference's
    own templates, so that a description mismatch cannot hide in the tracking comparison)"""
    img = orc.noise_image(SW, SH, 234, 0, 100).array().copy()
    dx, dy = kr.sobel_extended(orc, img)
    xy = _positions(r, SW, SH)
    cfg = kr.KltConfig(**kw)
    feats, want_ok = _ref_describe(img, dx, dy, cfg, r, xy)
    ref = kr.KltTracker(cfg)
    ref.setImage(img)
    rows, starts, want = [], [], []
    for i, f in enumerate(feats):
        if want_ok[i] == 2:
            continue
        for ox, oy in OFFSETS:
            g = kr.KltFeature(r)
            g.desc, g.derivX, g.derivY, g.Gxx, g.Gyy, g.Gxy = f.desc, f.derivX, f.derivY, f.Gxx, f.Gyy, f.Gxy
            g.setPosition(F(xy[i, 0]) + F(ox), F(xy[i, 1]) + F(oy))
            starts.append((g.x, g.y))
            try:
                fault = ref.track(g)
            except kr.Thrown:
                fault = 5
            rows.append(f)
            want.append((fault, g.x, g.y, ref.error))
    seen = collections.Counter(w[0] for w in want)
    return dict(xy=xy, feats=feats, ok=want_ok, rows=rows, starts=np.array(starts, np.float32), want=want, seen=seen)


def _stage_conditions(cfgname, R):
    """the reference side shows what the case is there for"""
    n_nan = sum(1 for f, ok in zip(R["feats"], R["ok"]) if ok != 2 and np.isnan(f.desc).any())
    assert n_nan >= 20                                                        # border templates
    if cfgname == "default":
        assert (R["ok"] == 1).sum() >= 20 and (R["ok"] == 0).sum() >= 4
        assert R["seen"][kr.SUCCESS] >= 50 and R["seen"][kr.OUT_OF_BOUNDS] >= 5, R["seen"]
    if cfgname == "det_large":
        assert R["seen"][kr.FAILED] >= 50, R["seen"]
    if cfgname == "small_error":
        assert R["seen"][kr.LARGE_ERROR] >= 20, R["seen"]


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("cfgname", list(STAGE_CONFIGS))
@pytest.mark.parametrize("r", [1, 2, 3, 7])
def test_stage_level_set_description_and_track(api, orc, r, cfgname, sub):
    kw = STAGE_CONFIGS[cfgname]
    R = _stage_reference(orc, r, kw)
    _stage_conditions(cfgname, R)
    _, _, _, gi, gx, gy = _stage_images(orc, sub, api)
    trk = api.KltTracker(api.KltConfig(**kw))
    trk.setImage(gi, gx, gy)
    d, ddx, ddy, G, ok = trk.setDescriptionAll(R["xy"], r)
    assert np.array_equal(ok, R["ok"]), (ok, R["ok"])      # 2 = the reference throws here: the library reports it instead of reading
    for i, f in enumerate(R["feats"]):
        if R["ok"][i] == 2 or (R["ok"][i] == 0 and not np.isnan(f.desc).any() and not f.desc.any()):
            continue   # thrown, or fully outside: the reference leaves the feature as it was
        vis = ~np.isnan(f.desc.reshape(-1))
        assert same(d[i], f.desc.reshape(-1)), i
        assert same(ddx[i][vis], f.derivX.reshape(-1)[vis]) and same(ddy[i][vis], f.derivY.reshape(-1)[vis]), i
        assert same(G[i], [f.Gxx, f.Gyy, f.Gxy]), i
    rows = R["rows"]
    tD = np.stack([f.desc.reshape(-1) for f in rows])
    tX = np.stack([f.derivX.reshape(-1) for f in rows])
    tY = np.stack([f.derivY.reshape(-1) for f in rows])
    tG = np.array([[f.Gxx, f.Gyy, f.Gxy] for f in rows], np.float32)
    got_xy, got_fault, got_err = trk.trackAll(R["starts"], r, tD, tX, tY, tG)
    for k, (fault, x, y, err) in enumerate(R["want"]):
        assert got_fault[k] == fault, (k, got_fault[k], fault)
        if fault == 5:
            continue
        assert same(got_xy[k], [x, y]), (k, got_xy[k], x, y)     # the position has moved also when a fault is returned
        if fault in (kr.SUCCESS, kr.LARGE_ERROR):
            assert same(got_err[k], err), (k, got_err[k], err)


def test_single_feature_classes(api, orc):
    """api.KltTracker / api.PyramidKltTracker (setImage, setDescription, track, getError) on the reference's own unit-test scene"""
    rand = orc.JavaRandom(234)
    img = rand.fillUniform(orc.Gray(50, 60), 0, 10).array().copy()
    img[22:42, 20:40] = 100
    pyr = api.FactoryPyramid.discreteGaussian(SCALES, -1, 2).process(api.GrayF32.wrap(img))
    dX, dY = [], []
    for l in range(3):
        lay = pyr.getLayer(l)
        x, y = api.GrayF32(lay.width, lay.height), api.GrayF32(lay.width, lay.height)
        api.GradientSobel.process(lay, x, y, api.BorderType.EXTENDED)
        dX.append(x)
        dY.append(y)
    cfg = dict(maxPerPixelError=10, maxIterations=30, minDeterminant=0.01, minPositionDelta=0.001)
    t = api.PyramidKltTracker(api.KltTracker(api.KltConfig(**cfg)))
    t.setImage(pyr, dX, dY)
    layers, rx, ry = kr.pyramid_gradient(orc, img, SCALES)
    ref = kr.PyramidKltTracker(kr.KltTracker(kr.KltConfig(**cfg)), SCALES)
    ref.setImage(layers, rx, ry)
    for l in range(3):
        assert same(pyr.getLayer(l).array(), layers[l]) and same(dX[l].array(), rx[l]) and same(dY[l].array(), ry[l])
    for start, moved in (((20, 22), (20 - 1.3, 22 + 1.2)), ((20, 22), (20 - 5.4, 22 + 5.3)), ((48, 55), (50, 57)), ((1, 1), (2.5, 0.5))):
        f, g = api.PyramidKltFeature(3, 2), kr.PyramidKltFeature(3, 2)
        f.setPosition(*start)
        g.setPosition(*start)
        assert t.setDescription(f) == ref.setDescription(g)
        for l in range(3):
            assert same(f.desc[l].desc.array(), g.desc[l].desc) and same([f.desc[l].Gxx, f.desc[l].Gyy, f.desc[l].Gxy], [g.desc[l].Gxx, g.desc[l].Gyy, g.desc[l].Gxy])
        f.setPosition(*moved)
        g.setPosition(*moved)
        fault = ref.track(g)
        assert t.track(f) == fault
        assert same([f.x, f.y], [g.x, g.y])
        for l in range(3):   # the per-layer positions move even where the track faults
            assert same([f.desc[l].x, f.desc[l].y], [g.desc[l].x, g.desc[l].y])
        if fault == kr.SUCCESS:
            assert same(t.getError(), ref.getError())


# ---------------------------------------------------------------------------------------------------------------- end to end
_scene_cache = {}


def _scene(orc, seed=234):
    if seed not in _scene_cache:
        _scene_cache[seed] = orc.gaussian_blur(orc.noise_image(360, 280, seed, 0, 255), -1, 3).array().copy()
    return _scene_cache[seed]


def _frames(orc, shift):
    """frame 0 and three more: the window moved by `shift`, then by a pixel or two more each frame"""
    sx, sy = shift
    sc = _scene(orc)
    moves = [(0, 0), (sx, sy), (sx + 1, sy + 1), (sx + 2, sy)]
    return [np.ascontiguousarray(sc[20 + my:260 + my, 20 + mx:340 + mx]) for mx, my in moves], moves


def _snapshot(trk):
    """(active, spawned, dropped) of a klt_ref tracker as comparable tuples"""
    act = [(t.featureId, float(t.px), float(t.py)) for t in trk.active]
    spw = [(t.featureId, float(t.px), float(t.py)) for t in trk.spawned]
    drp = [(t.featureId, float(t.px), float(t.py), t.fault) for t in trk.dropped]
    err = [t.error for t in trk.active]
    return act, spw, drp, err


def _compare_lists(got_active, got_spawned, got_dropped, snap, errors=True):
    act, spw, drp, err = snap
    assert [int(i) for i in got_active["featureId"]] == [a[0] for a in act]
    assert same(got_active["xy"], np.array([a[1:] for a in act], np.float32).reshape(-1, 2))
    assert [int(i) for i in got_spawned["featureId"]] == [a[0] for a in spw]
    assert same(got_spawned["xy"], np.array([a[1:] for a in spw], np.float32).reshape(-1, 2))
    assert [int(i) for i in got_dropped["featureId"]] == [a[0] for a in drp]
    assert same(got_dropped["xy"], np.array([a[1:3] for a in drp], np.float32).reshape(-1, 2))
    assert [int(f) for f in got_dropped["fault"]] == [a[3] for a in drp]
    assert not got_active["fault"].any()
    if errors:
        assert same(got_active["error"], np.array(err, np.float32))


def _run_reference(orc, shift, r, cfg_kw):
    """klt_ref over the four frames: spawn on frame 0, process 1..3, a second spawn (with live tracks: the exclusion list) after frame 2.
    -> per-step snapshots and the figures the conditions are stated on.  klt_ref raising Thrown fails the test: such inputs are not allowed."""
    frames, moves = _frames(orc, shift)
    trk = kr.PointTrackerKltPyramid(orc, SCALES, r, kr.KltConfig(**cfg_kw), DET["detectRadius"], DET["detectThreshold"], DET["detectBorder"])
    steps = []
    trk.process(frames[0])
    trk.spawnTracks()
    steps.append(_snapshot(trk))
    info = dict(spawned=len(trk.active), nan=sum(any(np.isnan(d.desc).any() for d in t.desc) for t in trk.active),
                described=all(t.described for t in trk.active))
    start = {t.featureId: (float(t.x), float(t.y)) for t in trk.active}
    for k in (1, 2, 3):
        trk.process(frames[k])
        if k == 1:
            faults = collections.Counter([t.fault for t in trk.dropped] + [kr.SUCCESS] * len(trk.active))
            ok = [t for t in trk.active] + [t for t in trk.dropped if t.fault == kr.SUCCESS]
            near = sum(abs(float(t.x) - (start[t.featureId][0] - moves[1][0])) < 0.25 and abs(float(t.y) - (start[t.featureId][1] - moves[1][1])) < 0.25
                       for t in ok)
            info.update(faults=faults, near=near, iterations=trk.klt.iterations, borderIterations=trk.klt.borderIterations)
        steps.append(_snapshot(trk))
        if k == 2:
            trk.spawnTracks()
            info["respawned"] = len(trk.spawned)
            steps.append(_snapshot(trk))
    return frames, steps, info


CASES = {
    # name: (shift, templateRadius, KltConfig overrides)
    "still_r2": ((0, 0), 2, {}),
    "small_r2": ((3, -2), 2, {}),
    "small_r3": ((3, -2), 3, {}),
    "medium_r2": ((7, 5), 2, {}),
    "medium_r2_large_error": ((7, 5), 2, dict(maxPerPixelError=2)),
    "large_r2": ((13, -9), 2, {}),
}
_ref_cache = {}


def _reference(orc, name):
    if name not in _ref_cache:
        shift, r, kw = CASES[name]
        _ref_cache[name] = _run_reference(orc, shift, r, kw)
    return _ref_cache[name]


def _conditions(name, info):
    """what the reference side must show before a comparison means anything (set well under the figures a CPU run of this recipe gives:
    1071 spawned tracks, 152 / 208 of them with a NaN-marked template at radius 2 / 3, and for frame 1
    (3,-2) r2: 1067 SUCCESS all within 0.25 px, 12673 iterations of which 1812 border form; (7,5) r2: FAILED 2, OUT_OF_BOUNDS 41, DRIFTED 15;
    (7,5) r2 with maxPerPixelError 2: LARGE_ERROR 390, OUT_OF_BOUNDS 26, DRIFTED 6, FAILED 2)"""
    f = info["faults"]
    assert info["spawned"] >= 1000 and info["described"]
    assert info["nan"] >= 100                                                   # (b) tracks with NaN-marked templates are compared
    if name != "still_r2":
        assert info["borderIterations"] >= 1000, info["borderIterations"]      # (b) the border form runs
    if name == "small_r2":                                                      # (a) the yardstick tracks
        assert f[kr.SUCCESS] >= 1000 and info["near"] >= 0.95 * f[kr.SUCCESS], (f, info["near"])
    if name == "medium_r2":                                                     # (c)
        assert f[kr.FAILED] >= 1 and f[kr.OUT_OF_BOUNDS] >= 1 and f[kr.DRIFTED] >= 1, f
        assert f[kr.LARGE_ERROR] == 0
    if name == "medium_r2_large_error":                                         # (d) all five outcomes in one case
        assert f[kr.LARGE_ERROR] >= 100 and f[kr.SUCCESS] >= 1 and f[kr.FAILED] >= 1 and f[kr.OUT_OF_BOUNDS] >= 1 and f[kr.DRIFTED] >= 1, f
    assert info["respawned"] >= 1                                               # the second spawn finds room next to the live tracks


def _run_device(dev, frames_per_seq, r, cfg_kw, api):
    """DeviceKltTracker over B sequences -> per-step (active, spawned, dropped) of every sequence, same steps as _run_reference"""
    device, torch = dev
    trk = device.DeviceKltTracker(SCALES, r, api.KltConfig(**cfg_kw), **DET)
    B = len(frames_per_seq)
    steps = []

    def snap():
        a, s, d = trk.counts()
        out = [(trk.active(b), trk.spawned(b), trk.dropped(b)) for b in range(B)]
        for b in range(B):
            assert (a[b], s[b], d[b]) == tuple(len(x["featureId"]) for x in out[b])
        steps.append(out)

    def push(k):
        trk.process(torch.from_numpy(np.stack([f[k] for f in frames_per_seq])).cuda())

    push(0)
    trk.spawn()
    snap()
    for k in (1, 2, 3):
        push(k)
        if k == 1:
            stats = trk.stats()
        snap()
        if k == 2:
            trk.spawn()
            snap()
    trk.close()
    return steps, stats


@pytest.mark.parametrize("name", list(CASES))
def test_device_tracker_matches_reference(dev, api, orc, name):
    shift, r, kw = CASES[name]
    frames, ref_steps, info = _reference(orc, name)
    _conditions(name, info)
    got, stats = _run_device(dev, [frames], r, kw, api)
    assert len(got) == len(ref_steps) == 5
    assert stats == (info["spawned"], info["iterations"], info["borderIterations"])   # the same Lucas-Kanade iterations, the same number in the border form
    for k, (g, want) in enumerate(zip(got, ref_steps)):
        # every spawned track is compared in every frame: the lists are compared whole, in order (e)
        _compare_lists(g[0][0], g[0][1], g[0][2], want)


def test_three_sequences_in_one_tracker_equal_three_single_runs(dev, api, orc):
    names = ["small_r2", "medium_r2", "large_r2"]
    refs = [_reference(orc, n) for n in names]
    for n, (_, _, info) in zip(names, refs):
        _conditions(n, info)
    got, stats = _run_device(dev, [r[0] for r in refs], 2, {}, api)
    assert stats == tuple(sum(r[2][key] for r in refs) for key in ("spawned", "iterations", "borderIterations"))
    for k in range(5):
        for b in range(3):
            _compare_lists(got[k][b][0], got[k][b][1], got[k][b][2], refs[b][1][k])


def test_pyramid_and_gradients_of_the_tracker(dev, api, orc):
    """the buffers the tracker works on are the reference's pyramid and EXTENDED Sobel layers"""
    device, torch = dev
    frames, _ = _frames(orc, (3, -2))
    trk = device.DeviceKltTracker(SCALES, 2, None, **DET)
    trk.process(torch.from_numpy(np.stack([frames[0], frames[1]])).cuda())
    for b in range(2):
        layers, dx, dy = kr.pyramid_gradient(orc, frames[b], SCALES)
        for l in range(3):
            assert same(trk.layer(b, l, 0), layers[l]) and same(trk.layer(b, l, 1), dx[l]) and same(trk.layer(b, l, 2), dy[l])
    trk.close()


def _as_lists(trk):
    def pack(tracks):
        return dict(featureId=np.array([t.featureId for t in tracks], np.int64), xy=np.array([[t.x, t.y] for t in tracks], np.float32).reshape(-1, 2),
                    fault=np.array([t.fault for t in tracks], np.int32), error=np.zeros(len(tracks), np.float32))
    return pack(trk.getActiveTracks()), pack(trk.getNewTracks()), pack(trk.getDroppedTracks())


def test_point_tracker_class(api, orc):
    """api.PointTrackerKltPyramid (host frames, one sequence): the same run as the device class, then addTrack, dropTrack, dropAllTracks, reset"""
    name = "small_r2"
    shift, r, kw = CASES[name]
    frames, ref_steps, info = _reference(orc, name)
    _conditions(name, info)
    cfg = api.ConfigGeneralDetector(radius=DET["detectRadius"], threshold=DET["detectThreshold"])
    trk = api.PointTrackerKltPyramid(api.KltConfig(**kw), r, SCALES, cfg, detectBorder=DET["detectBorder"])
    ref = kr.PointTrackerKltPyramid(orc, SCALES, r, kr.KltConfig(**kw), DET["detectRadius"], DET["detectThreshold"], DET["detectBorder"])
    assert trk.getActiveTracks() == [] and trk.getInactiveTracks() == []

    def check():
        _compare_lists(*_as_lists(trk), _snapshot(ref), errors=False)

    for k in range(4):
        trk.process(api.GrayF32.wrap(frames[k]))
        ref.process(frames[k])
        if k in (0, 2):
            trk.spawnTracks()
            ref.spawnTracks()
        check()
        assert len(trk.getAllTracks()) == len(ref.active)
    # addTrack: inside the frame -> appended whatever the texture; outside -> None
    assert trk.addTrack(-3.0, 10.0) is None and ref.addTrack(-3.0, 10.0) is None
    assert trk.addTrack(100.25, 2000.0) is None
    for x, y in ((100.25, 80.5), (0.5, 0.5), (318.9, 238.9)):
        assert trk.addTrack(x, y) is not None and ref.addTrack(x, y) is not None
    check()
    # dropTrack by featureId, first / middle / last and one that is not there
    act = trk.getActiveTracks()
    for idx in (0, len(act) // 2, len(act) - 4):
        assert trk.dropTrack(act[idx]) and ref.dropTrack(ref.active[[t.featureId for t in ref.active].index(act[idx].featureId)])
    assert not trk.dropTrack(act[0])
    check()
    trk.process(api.GrayF32.wrap(frames[1]))
    ref.process(frames[1])
    check()
    trk.dropAllTracks()
    ref.dropAllTracks()
    check()
    trk.spawnTracks()
    ref.spawnTracks()
    check()                      # featureIds continue
    trk.reset()
    ref.reset()
    trk.spawnTracks()
    ref.spawnTracks()
    check()                      # featureIds start at 0 again
    assert trk.getNewTracks()[0].featureId == 0
    trk.close()


def test_spawn_with_max_features_uses_select_n_best(api, orc):
    """ConfigGeneralDetector.maxFeatures > 0: GeneralFeatureDetector with the exclusion list and SelectNBestFeatures, composed on the host"""
    frames, _ = _frames(orc, (3, -2))
    cfg = api.ConfigGeneralDetector(radius=3, threshold=1.0, maxFeatures=300)
    trk = api.PointTrackerKltPyramid(None, 2, SCALES, cfg, detectBorder=0)
    ref = kr.PointTrackerKltPyramid(orc, SCALES, 2, None, 3, 1.0, 0, maxFeatures=300)
    for k in range(3):
        trk.process(api.GrayF32.wrap(frames[k]))
        ref.process(frames[k])
        trk.spawnTracks()
        ref.spawnTracks()
        got, want = _as_lists(trk), _snapshot(ref)
        # the kept SET is compared (the order quick-select leaves the corners in, and with it the featureId of each, is unpinned)
        assert sorted(map(tuple, got[0]["xy"].tolist())) == sorted((a[1], a[2]) for a in want[0]) and len(want[0]) <= 300
        assert sorted(map(tuple, got[1]["xy"].tolist())) == sorted((a[1], a[2]) for a in want[1])
    assert len(ref.active) > 250
    trk.close()


def test_exclude_list_of_general_feature_detector(api, orc):
    img = _img(orc, 80, 60, 9)
    dx, dy = kr.sobel_extended(orc, img)
    det = api.GeneralFeatureDetector(api.FactoryIntensityPointAlg.shiTomasi(1, False, api.GrayF32), api.FactoryFeatureExtractor.nonmax(api.ConfigExtract(2, 1.0, 0)))
    det.process(api.GrayF32.wrap(img), api.GrayF32.wrap(dx), api.GrayF32.wrap(dy))
    base = [(p.x, p.y) for p in det.getMaximums()]
    assert base == [tuple(int(v) for v in p) for p in kr.detect(orc, dx, dy, None, 2, 1.0, 1)] and len(base) > 20
    excl = [api.Point2D_I16(*base[3]), api.Point2D_I16(*base[10])]
    det.setExcludeMaximum(excl)
    det.process(api.GrayF32.wrap(img), api.GrayF32.wrap(dx), api.GrayF32.wrap(dy))
    got = [(p.x, p.y) for p in det.getMaximums()]
    assert got == [tuple(int(v) for v in p) for p in kr.detect(orc, dx, dy, [base[3], base[10]], 2, 1.0, 1)]
    assert base[3] not in got and base[10] not in got
    det.setMaxFeatures(2)        # numSelectMax = maxFeatures - exclude.size <= 0: nothing is detected
    det.process(api.GrayF32.wrap(img), api.GrayF32.wrap(dx), api.GrayF32.wrap(dy))
    assert det.getMaximums() == []


# ---------------------------------------------------------------------------------------------------------------- handle lifetime
def test_klt_handle_lifetime():
    """context destroyed before its tracker, destroy twice (tests/test_handle_lifetime.py is the model), in a child process"""
    code = """
import ctypes as C, numpy as np, torch
from boofcv_amd import _lib
L = _lib.load()
c = C.c_void_p(); k = C.c_void_p()
assert L.bhip_ctx_create(0, C.byref(c)) == 0
scales = (C.c_int * 3)(1, 2, 4)
assert L.bhip_klt_create(c, None, 2, scales, 3, 3, 1.0, 0, 160, 120, 2, C.byref(k)) == 0
assert L.bhip_klt_spawn(k, -1) == _lib.BHIP_ERR_INVALID            # before the first process()
assert L.bhip_klt_create(c, None, 9, scales, 3, 3, 1.0, 0, 160, 120, 2, C.byref(C.c_void_p())) == _lib.BHIP_ERR_UNSUPPORTED
frames = (torch.rand((2, 120, 160), device="cuda:0") * 100).contiguous()
torch.cuda.synchronize()
assert L.bhip_klt_process_dev_f32(k, C.c_void_p(frames.data_ptr()), 120 * 160, 160) == 0
assert L.bhip_klt_spawn(k, 5) == _lib.BHIP_ERR_UNSUPPORTED
assert L.bhip_klt_spawn(k, -1) == 0
a = (C.c_int * 2)()
assert L.bhip_klt_counts(k, a, None, None) == 0 and a[0] > 10 and a[1] > 10
assert L.bhip_ctx_destroy(c) == 0                                  # context first: the tracker becomes an inert shell
assert L.bhip_klt_counts(k, a, None, None) == _lib.BHIP_ERR_INVALID
assert L.bhip_klt_process_dev_f32(k, C.c_void_p(frames.data_ptr()), 120 * 160, 160) == _lib.BHIP_ERR_INVALID
assert L.bhip_klt_spawn(k, -1) == _lib.BHIP_ERR_INVALID
assert L.bhip_klt_destroy(k) == 0
assert L.bhip_klt_destroy(k) == _lib.BHIP_ERR_INVALID
assert L.bhip_ctx_destroy(c) == _lib.BHIP_ERR_INVALID
print("ok", a[0], a[1])
"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok")
