"""GPU: the pyramid KLT tracker on GrayU8 frames -- the GrayU8 down-convolution and pyramid, the EXTENDED-border GrayU8 -> GrayS16 Sobel, the
typed tracker kernels and the GrayU8 tracker objects -- bit for bit against tests/klt_u8_ref.py.  Every comparison is exact: integers with
array_equal, floats through their uint32 words (NaN through np.isnan masks), as in test_gpu_klt.py.

The scenes of the whole-tracker cases are klt_u8_ref.CASES; what they exercise (no position where the reference throws, border-form iterations,
NaN-marked templates, every KltTrackFault) is stated by the reference alone in test_klt_u8_reference.py, with the figures pinned there.

Full-size case: 1920 x 1080, 8 frames, spawn on frames 0 and 4 (detect radius 20: about 1200 tracks, 188 k Lucas-Kanade iterations).  Wall time of
test_full_size_sequence on an MI355X host: 3.8 s, nearly all of it the numpy reference (the eight device steps together take a few milliseconds)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import corner_ref
import klt_ref as kr
import klt_u8_ref as ku
import test_gpu_klt as tg      # the F32 file's stage-level recipe (positions, offsets, configs) and its bit comparison

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
same = tg.same
K5 = np.array([1, 4, 7, 4, 1], np.int32)


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd import device
    return device, torch


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(a, b))


def _view(api, cls, arr, pad_x, pad_y, fill=0):
    """`arr` as a sub-image with an odd offset inside a wider, taller image (stride > width)"""
    h, w = arr.shape
    big = cls(w + 2 * pad_x + 1, h + pad_y + 2)
    big.data[:] = fill
    v = big.subimage(pad_x, pad_y, pad_x + w, pad_y + h)
    v.array()[:, :] = arr
    return v


# ---------------------------------------------------------------------------------------------------------------- down convolution
CONV_SIZES = [(37, 23), (256, 9), (261, 35), (16, 21), (9, 9), (7, 8), (5, 12), (3, 10)]   # (W, H)


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("skip", [1, 2, 3, 4])
def test_conv_down_u8_stage_level(api, skip, sub):
    """bhip_conv_down_norm_h_u8 / _v_u8 for radii 1..3 (and radius 4 with skip 3: the off-grid interior that leaves a pixel unwritten); where
    the reference's loops leave the row (klt_u8_ref raises) the library answers BHIP_ERR_INVALID"""
    checked = refused = 0
    for radius in (1, 2, 3, 4):
        if radius == 4 and skip != 3:
            continue
        kernel = corner_ref.gaussian_kernel_s32(radius).astype(np.int32)
        for W, H in CONV_SIZES:
            img = _u8((H, W), 31 * W + H + skip)
            for axis, fn in ((1, api.ConvolveImageDownNormalized.horizontal), (0, api.ConvolveImageDownNormalized.vertical)):
                shape = (H, W // skip) if axis == 1 else (H // skip, W)
                if shape[0] == 0 or shape[1] == 0:
                    continue
                before = np.full(shape, 77, np.uint8)      # pixels the reference does not write keep the caller's values
                src = _view(api, api.GrayU8, img, 3, 1) if sub else api.GrayU8.wrap(img)
                dst = _view(api, api.GrayU8, before, 5, 2) if sub else api.GrayU8.wrap(before.copy())
                try:
                    want = ku.conv_down_norm_u8(img, kernel, skip, axis, out=before.copy())
                except ValueError:
                    with pytest.raises(api.IllegalArgumentException):
                        fn(kernel, src, dst, skip)
                    refused += 1
                    continue
                fn(kernel, src, dst, skip)
                assert eq(dst.array(), want), (radius, W, H, axis)
                checked += 1
    assert checked >= 20


def test_conv_down_u8_rejects_what_the_reference_rejects(api):
    src, k = api.GrayU8(20, 20), K5
    for fn, dst, skip in ((api.ConvolveImageDownNormalized.horizontal, api.GrayU8(20, 20), 0), (api.ConvolveImageDownNormalized.horizontal, api.GrayU8(9, 20), 2),
                          (api.ConvolveImageDownNormalized.vertical, api.GrayU8(20, 9), 2)):
        with pytest.raises(api.IllegalArgumentException):
            fn(k, src, dst, skip)
    with pytest.raises(api.IllegalArgumentException):   # Java: ArithmeticException (/ by zero)
        api.ConvolveImageDownNormalized.horizontal(np.array([1, 0, -1], np.int32), src, api.GrayU8(10, 20), 2)


# ---------------------------------------------------------------------------------------------------------------- pyramid
PYR_SHAPES = tg.SOBEL_SHAPES + [(640, 480), (1920, 1080)]
SCALE_SETS = [(1, 2, 4), (2, 4), (1, 3), (1, 2, 4, 8)]


@pytest.mark.parametrize("scales", SCALE_SETS)
@pytest.mark.parametrize("shape", PYR_SHAPES)
def test_pyramid_u8_host(api, shape, scales):
    W, H = shape
    img = _u8((H, W), 7 * W + H)
    want = ku.pyramid_u8(img, scales)
    for src in (api.GrayU8.wrap(img), _view(api, api.GrayU8, img, 3, 1)):
        pyr = api.FactoryPyramid.discreteGaussian(scales, -1, 2, imageType=api.GrayU8).process(src)
        assert pyr.getNumLayers() == len(scales)
        for l in range(len(scales)):
            assert eq(pyr.getLayer(l).array(), want[l]), (shape, scales, l)


def test_pyramid_u8_narrow_layer(api):
    img = _u8((30, 9), 6)
    want = ku.pyramid_u8(img, (1, 2, 4))
    assert want[1].shape[1] == 5 and want[2].shape[1] == 3        # kernel.width >= image.width in the second step: both passes naive
    pyr = api.FactoryPyramid.discreteGaussian((1, 2, 4), -1, 2, imageType=api.GrayU8).process(api.GrayU8.wrap(img))
    for l in range(3):
        assert eq(pyr.getLayer(l).array(), want[l])
    with pytest.raises(api.IllegalArgumentException):   # a pyramid built for one image type refuses the other
        pyr.process(api.GrayF32(9, 30))


@pytest.mark.parametrize("scales", SCALE_SETS)
@pytest.mark.parametrize("shape", [(37, 23), (261, 35), (640, 480), (1920, 1080)])
def test_pyramid_u8_device(dev, shape, scales):
    device, torch = dev
    ops = device.DeviceImageOps(device=0)
    W, H = shape
    B = 3 if W < 1000 else 2
    imgs = np.stack([_u8((H, W), 11 * W + b) for b in range(B)])
    want = [ku.pyramid_u8(im, scales) for im in imgs]
    t = torch.from_numpy(imgs).cuda()
    big = torch.zeros((B, H + 3, W + 7), dtype=torch.uint8, device="cuda")
    big[:, 1:1 + H, 3:3 + W] = t
    torch.cuda.synchronize()
    for src in (t, big[:, 1:1 + H, 3:3 + W]):                    # dense, and rows of a wider buffer at an odd offset
        layers = ops.pyramid(K5, scales, src)
        ops.ctx.synchronize()
        assert len(layers) == len(scales)
        for b in range(B):
            for l in range(len(scales)):
                assert eq(layers[l][b].cpu().numpy(), want[b][l]), (shape, scales, b, l)


# ---------------------------------------------------------------------------------------------------------------- EXTENDED Sobel
@pytest.mark.parametrize("shape", PYR_SHAPES)
@pytest.mark.parametrize("sub", [False, True])
def test_sobel_u8_extended_host(api, shape, sub):
    W, H = shape
    img = _u8((H, W), 13 + W)
    want = ku.sobel_extended_u8(img)
    src = _view(api, api.GrayU8, img, 1, 2, fill=255) if sub else api.GrayU8.wrap(img)   # what surrounds a view must not leak in
    X = _view(api, api.GrayS16, np.zeros((H, W), np.int16), 3, 1) if sub else api.GrayS16(W, H)
    Y = _view(api, api.GrayS16, np.zeros((H, W), np.int16), 3, 1) if sub else api.GrayS16(W, H)
    api.GradientSobel.process(src, X, Y, api.BorderType.EXTENDED)
    assert eq(X.array(), want[0]) and eq(Y.array(), want[1])
    # borders null and ImageBorderValue(0) on the same input are what they were (corner_ref)
    for border, full in ((None, False), (0, True)):
        X.array()[:, :] = 1234
        Y.array()[:, :] = -77
        api.GradientSobel.process(src, X, Y, border)
        ex, ey = corner_ref.gradient_u8("sobel", img, full, np.full((H, W), 1234, np.int16), np.full((H, W), -77, np.int16))
        assert eq(X.array(), ex) and eq(Y.array(), ey)
    with pytest.raises(RuntimeError):   # the three-tap gradient keeps refusing EXTENDED, for both image types
        api.GradientThree.process(src, X, Y, api.BorderType.EXTENDED)


@pytest.mark.parametrize("shape", PYR_SHAPES)
def test_sobel_u8_extended_device(dev, shape):
    device, torch = dev
    ops = device.DeviceImageOps(device=0)
    W, H = shape
    B = 3 if W < 1000 else 2
    imgs = np.stack([_u8((H, W), 40 + W + b) for b in range(B)])
    want = [ku.sobel_extended_u8(im) for im in imgs]
    t = torch.from_numpy(imgs).cuda()
    dx, dy = ops.sobel(t, border="EXTENDED")
    ops.ctx.synchronize()
    for b in range(B):
        assert eq(dx[b].cpu().numpy(), want[b][0]) and eq(dy[b].cpu().numpy(), want[b][1])
    big = torch.full((B, H + 2, W + 7), 255, dtype=torch.uint8, device="cuda")
    big[:, 1:1 + H, 3:3 + W] = t
    ox = torch.zeros((B, H, W + 5), dtype=torch.int16, device="cuda")
    oy = torch.zeros((B, H, W + 5), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ops.sobel(big[:, 1:1 + H, 3:3 + W], border="EXTENDED", dx=ox[:, :, 1:1 + W], dy=oy[:, :, 1:1 + W])
    ops.ctx.synchronize()
    for b in range(B):
        assert eq(ox[b, :, 1:1 + W].cpu().numpy(), want[b][0]) and eq(oy[b, :, 1:1 + W].cpu().numpy(), want[b][1])
        assert not ox[b, :, 0].any() and not ox[b, :, 1 + W:].any()
    for border, full in ((None, False), (0, True)):
        dx, dy = ops.sobel(t, border=border)
        ops.ctx.synchronize()
        for b in range(B):
            ex, ey = corner_ref.gradient_u8("sobel", imgs[b], full)
            assert eq(dx[b].cpu().numpy(), ex) and eq(dy[b].cpu().numpy(), ey)
    with pytest.raises(RuntimeError):
        ops.three(t, border="EXTENDED")


# ---------------------------------------------------------------------------------------------------------------- stage level
SW, SH = tg.SW, tg.SH


def _stage_arrays(orc):
    img = np.floor(orc.noise_image(SW, SH, 234, 0, 100).array()).astype(np.uint8)
    dx, dy = ku.sobel_extended_u8(img)
    return img, dx, dy


def _stage_reference_u8(orc, r, kw):
    """test_gpu_klt._stage_reference on the float copies of the GrayU8 image and its GrayS16 derivatives"""
    img, dx, dy = (a.astype(np.float32) for a in _stage_arrays(orc))
    xy = tg._positions(r, SW, SH)
    cfg = kr.KltConfig(**kw)
    feats, want_ok = tg._ref_describe(img, dx, dy, cfg, r, xy)
    ref = kr.KltTracker(cfg)
    ref.setImage(img)
    rows, starts, want = [], [], []
    for i, f in enumerate(feats):
        if want_ok[i] == 2:
            continue
        for ox, oy in tg.OFFSETS:
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
    return dict(xy=xy, feats=feats, ok=want_ok, rows=rows, starts=np.array(starts, np.float32), want=want)


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("cfgname", list(tg.STAGE_CONFIGS))
@pytest.mark.parametrize("r", [1, 2, 3, 7])
def test_stage_level_cross_type_identity(api, orc, r, cfgname, sub):
    """bhip_klt_set_description_u8 / bhip_klt_track_u8 on a GrayU8 image with GrayS16 derivatives == bhip_klt_set_description_f32 /
    bhip_klt_track_f32 on the float32 copies of the same arrays, in every output bit; and both == klt_u8_ref"""
    kw = tg.STAGE_CONFIGS[cfgname]
    img, dx, dy = _stage_arrays(orc)
    R = _stage_reference_u8(orc, r, kw)
    assert sum(1 for f, ok in zip(R["feats"], R["ok"]) if ok != 2 and np.isnan(f.desc).any()) >= 20      # border templates are among them
    if sub:
        gi, gx, gy = _view(api, api.GrayU8, img, 3, 2), _view(api, api.GrayS16, dx, 5, 1), _view(api, api.GrayS16, dy, 5, 1)
    else:
        gi, gx, gy = api.GrayU8.wrap(img), api.GrayS16.wrap(dx), api.GrayS16.wrap(dy)
    fi, fx, fy = (api.GrayF32.wrap(a.astype(np.float32)) for a in (img, dx, dy))
    ti, tf = api.KltTracker(api.KltConfig(**kw)), api.KltTracker(api.KltConfig(**kw))
    ti.setImage(gi, gx, gy)
    tf.setImage(fi, fx, fy)
    got_i, got_f = ti.setDescriptionAll(R["xy"], r), tf.setDescriptionAll(R["xy"], r)
    for a, b in zip(got_i[:4], got_f[:4]):      # desc, derivX, derivY, G
        assert same(a, b)
    assert np.array_equal(got_i[4], got_f[4]) and np.array_equal(got_i[4], R["ok"])
    d, ddx, ddy, G, ok = got_i
    for i, f in enumerate(R["feats"]):
        if R["ok"][i] == 2 or (R["ok"][i] == 0 and not np.isnan(f.desc).any() and not f.desc.any()):
            continue
        vis = ~np.isnan(f.desc.reshape(-1))
        assert same(d[i], f.desc.reshape(-1)), i
        assert same(ddx[i][vis], f.derivX.reshape(-1)[vis]) and same(ddy[i][vis], f.derivY.reshape(-1)[vis]), i
        assert same(G[i], [f.Gxx, f.Gyy, f.Gxy]), i
    rows = R["rows"]
    tD = np.stack([f.desc.reshape(-1) for f in rows])
    tX = np.stack([f.derivX.reshape(-1) for f in rows])
    tY = np.stack([f.derivY.reshape(-1) for f in rows])
    tG = np.array([[f.Gxx, f.Gyy, f.Gxy] for f in rows], np.float32)
    xy_i, fault_i, err_i = ti.trackAll(R["starts"], r, tD, tX, tY, tG)
    xy_f, fault_f, err_f = tf.trackAll(R["starts"], r, tD, tX, tY, tG)
    assert np.array_equal(fault_i, fault_f)
    ok_rows = fault_i != 5
    assert same(xy_i[ok_rows], xy_f[ok_rows])
    done = (fault_i == kr.SUCCESS) | (fault_i == kr.LARGE_ERROR)
    assert same(err_i[done], err_f[done])
    for k, (fault, x, y, err) in enumerate(R["want"]):
        assert fault_i[k] == fault, (k, fault_i[k], fault)
        if fault == 5:
            continue
        assert same(xy_i[k], [x, y]), (k, xy_i[k], x, y)
        if fault in (kr.SUCCESS, kr.LARGE_ERROR):
            assert same(err_i[k], err), (k, err_i[k], err)


def test_stage_level_refuses_mixed_types(api):
    t = api.KltTracker()
    with pytest.raises(RuntimeError):
        t.setImage(api.GrayU8(8, 8), api.GrayF32(8, 8), api.GrayF32(8, 8))
    with pytest.raises(RuntimeError):
        t.setImage(api.GrayS16(8, 8))


# ---------------------------------------------------------------------------------------------------------------- whole tracker
def _snapshot(trk):
    """everything the comparison looks at, copied out of a klt_u8_ref tracker"""
    L = len(trk.scales)
    act = [(t.featureId, float(t.px), float(t.py)) for t in trk.active]
    spw = [(t.featureId, float(t.px), float(t.py)) for t in trk.spawned]
    drp = [(t.featureId, float(t.px), float(t.py), t.fault) for t in trk.dropped]
    err = [t.error for t in trk.active]
    tmpl = [[(d.desc.reshape(-1).copy(), d.derivX.reshape(-1).copy(), d.derivY.reshape(-1).copy(), (d.Gxx, d.Gyy, d.Gxy)) if getattr(d, "written", False) else None
             for d in t.desc] for t in trk.active]
    layers = [a.copy() for a in trk.layersU8], [a.copy() for a in trk.derivXS16], [a.copy() for a in trk.derivYS16]
    return dict(lists=(act, spw, drp, err), tmpl=tmpl, layers=layers, L=L)


def _reference_steps(orc, name):
    steps = {}
    fr, trk, info = ku.run_case(orc, name, on_step=lambda label, t: steps.__setitem__(label, _snapshot(t)))
    return fr, steps, info


_ref_cache = {}


def _reference(orc, name):
    if name not in _ref_cache:
        _ref_cache[name] = _reference_steps(orc, name)
    return _ref_cache[name]


def _compare_templates(trk, b, snap):
    """every written layer of every active track: desc (NaN where the patch left the image), derivX / derivY where desc is defined, G"""
    n_cmp = 0
    for l in range(snap["L"]):
        t, G = trk.templates(b, l, 0)
        assert len(t) == len(snap["tmpl"])
        for i, per_layer in enumerate(snap["tmpl"]):
            if per_layer[l] is None:
                continue
            d, dx, dy, g = per_layer[l]
            vis = ~np.isnan(d)
            assert same(t[i, 0], d), (l, i)
            assert same(t[i, 1][vis], dx[vis]) and same(t[i, 2][vis], dy[vis]), (l, i)
            assert same(G[i], g), (l, i)
            n_cmp += 1
    return n_cmp


def _drive_device(dev, api, orc, names, errors=True):
    """DeviceKltTracker with one sequence per case of `names` (same radius and configuration), stepped as klt_u8_ref.run_case steps the
    reference, compared after every operation"""
    device, torch = dev
    refs = [_reference(orc, n) for n in names]
    shift, r, kw, _ = ku.CASES[names[0]]
    assert all(ku.CASES[n][1] == r and ku.CASES[n][2] == kw for n in names)
    B = len(names)
    trk = device.DeviceKltTracker(ku.SCALES, r, api.KltConfig(**kw), **ku.DET)
    compared = 0

    def check(label, templates=True):
        nonlocal compared
        a, s, d = trk.counts()
        for b in range(B):
            snap = refs[b][1][label]
            got = trk.active(b), trk.spawned(b), trk.dropped(b)
            assert (a[b], s[b], d[b]) == tuple(len(x["featureId"]) for x in got)
            tg._compare_lists(got[0], got[1], got[2], snap["lists"], errors=errors)
            if templates:
                compared += _compare_templates(trk, b, snap)

    def process(k):
        trk.process(torch.from_numpy(np.stack([refs[b][0][k] for b in range(B)])).cuda())
        label = "process%d" % k
        if k > 0:
            want = tuple(sum(refs[b][2]["stats%d" % k][i] for b in range(B)) for i in range(3))
            assert trk.stats() == want, (label, trk.stats(), want)
        for b in range(B):   # the buffers the tracker works on: getLayer / bhip_klt_fetch_layer_u8 / _s16
            lay, dx, dy = refs[b][1][label]["layers"]
            for l in range(len(ku.SCALES)):
                assert eq(trk.layer(b, l, 0), lay[l]) and eq(trk.layer(b, l, 1), dx[l]) and eq(trk.layer(b, l, 2), dy[l])
        check(label)

    process(0)
    trk.spawn()
    check("spawn0")
    ok = trk.addTracks([b for b in range(B) for _ in ku.ADDED], [p for _ in range(B) for p in ku.ADDED])
    assert ok.all()
    assert not trk.addTracks([0], [(-3.0, 10.0)])[0] and not trk.addTracks([B - 1], [(100.25, 2000.0)])[0]   # outside the frame: null
    check("add")
    process(1)
    process(2)
    trk.spawn()
    check("spawn2")
    seqs = [b for b in range(B) for _ in range(3)]
    ids = [i for b in range(B) for i in refs[b][2]["drop_ids"]]
    assert trk.dropTracks(seqs, ids).all()
    assert not trk.dropTracks([0], [ids[0]])[0]
    check("drop")
    process(3)
    trk.dropAllTracks()
    check("dropAll", templates=False)
    trk.spawn()
    check("spawn3")
    trk.reset()
    check("reset", templates=False)
    trk.spawn()
    check("spawn4")
    for b in range(B):
        assert int(trk.spawned(b)["featureId"][0]) == 0     # featureIds start again after reset
    trk.close()
    return compared


@pytest.mark.parametrize("name", list(ku.CASES))
def test_device_tracker_u8_matches_reference(dev, api, orc, name):
    assert _drive_device(dev, api, orc, [name]) >= 3000      # (track, layer) templates compared


def test_two_sequences_in_one_u8_tracker(dev, api, orc):
    assert _drive_device(dev, api, orc, ["small_r2", "large_r2"]) >= 6000


def _as_lists(trk):
    return tg._as_lists(trk)


@pytest.mark.parametrize("name", ["medium_r3", "medium_r2_large_error"])
def test_point_tracker_class_on_u8_host_frames(api, orc, name):
    """api.PointTrackerKltPyramid from FactoryPointTracker.klt(..., GrayU8, GrayS16 / None), host frames (also as sub-image views)"""
    shift, r, kw, _ = ku.CASES[name]
    fr, steps, info = _reference(orc, name)
    cfg = api.ConfigGeneralDetector(radius=ku.DET["detectRadius"], threshold=ku.DET["detectThreshold"])
    pk = api.PkltConfig(r, ku.SCALES)
    pk.config = api.KltConfig(**kw)
    trk = api.FactoryPointTracker.klt(pk, cfg, imageType=api.GrayU8, derivType=api.GrayS16 if name == "medium_r3" else None)
    assert trk.imageType is api.GrayU8 and trk.templateRadius == r
    trk.close()
    trk = api.PointTrackerKltPyramid(api.KltConfig(**kw), r, ku.SCALES, cfg, detectBorder=ku.DET["detectBorder"], imageType=api.GrayU8)

    def check(label):
        tg._compare_lists(*_as_lists(trk), steps[label]["lists"], errors=False)

    def process(k):
        img = api.GrayU8.wrap(fr[k]) if k % 2 == 0 else _view(api, api.GrayU8, fr[k], 3, 1, fill=255)
        trk.process(img)
        lay, dx, dy = steps["process%d" % k]["layers"]
        for l in range(len(ku.SCALES)):
            a, x, y = trk.getLayer(l, 0), trk.getLayer(l, 1), trk.getLayer(l, 2)
            assert isinstance(a, api.GrayU8) and isinstance(x, api.GrayS16) and isinstance(y, api.GrayS16)
            assert eq(a.array(), lay[l]) and eq(x.array(), dx[l]) and eq(y.array(), dy[l])
        check("process%d" % k)

    process(0)
    trk.spawnTracks()
    check("spawn0")
    for x, y in ku.ADDED:
        assert trk.addTrack(x, y) is not None
    assert trk.addTrack(-3.0, 10.0) is None
    check("add")
    process(1)
    process(2)
    trk.spawnTracks()
    check("spawn2")
    by_id = {t.featureId: t for t in trk.getActiveTracks()}
    for i in info["drop_ids"]:
        assert trk.dropTrack(by_id[i])
    assert not trk.dropTrack(by_id[info["drop_ids"][0]])
    check("drop")
    process(3)
    trk.dropAllTracks()
    check("dropAll")
    trk.spawnTracks()
    check("spawn3")
    trk.reset()
    check("reset")
    trk.spawnTracks()
    check("spawn4")
    # a tracker that has seen GrayU8 frames refuses a GrayF32 one, in the reference's IllegalArgumentException style
    with pytest.raises(api.IllegalArgumentException):
        trk.process(api.GrayF32(ku.FRAME_W, ku.FRAME_H))
    trk.close()


def test_u8_spawn_with_max_features_uses_s16_intensity(api, orc):
    """maxFeatures > 0: GeneralFeatureDetector on the GrayS16 derivatives with SelectNBestFeatures, composed on the host (kept SET compared)"""
    fr, _ = ku.frames(orc, (3, -2))
    cfg = api.ConfigGeneralDetector(radius=3, threshold=1.0, maxFeatures=150)
    trk = api.PointTrackerKltPyramid(None, 2, ku.SCALES, cfg, detectBorder=0, imageType=api.GrayU8)
    ref = ku.PointTrackerKltPyramidU8(orc, ku.SCALES, 2, None, 3, 1.0, 0, maxFeatures=150)
    for k in range(2):
        trk.process(api.GrayU8.wrap(fr[k]))
        ref.process(fr[k])
        trk.spawnTracks()
        ref.spawnTracks()
        got = _as_lists(trk)
        assert sorted(map(tuple, got[0]["xy"].tolist())) == sorted((float(t.px), float(t.py)) for t in ref.active) and len(ref.active) <= 150
    assert len(ref.active) > 100
    trk.close()


def test_factory_keeps_refusing_other_type_pairs(api):
    for imageType, derivType in ((api.GrayS16, None), (api.GrayU8, api.GrayF32), (api.GrayF32, api.GrayS16), (api.GrayS32, api.GrayS32)):
        with pytest.raises(RuntimeError, match="Java path"):
            api.FactoryPointTracker.klt(None, None, imageType=imageType, derivType=derivType)
    with pytest.raises(RuntimeError, match="Java path"):
        api.PointTrackerKltPyramid(None, 2, ku.SCALES, None, imageType=api.GrayU8).process(api.GrayS16(32, 32))


def test_device_tracker_refuses_the_other_dtype(dev, api, orc):
    device, torch = dev
    fr, _ = ku.frames(orc, (3, -2))
    trk = device.DeviceKltTracker(ku.SCALES, 2, None, **ku.DET)
    trk.process(torch.from_numpy(fr[0][None]).cuda())
    with pytest.raises(api.IllegalArgumentException):
        trk.process(torch.from_numpy(fr[0][None].astype(np.float32)).cuda())
    trk.close()


# ---------------------------------------------------------------------------------------------------------------- full size
def test_full_size_sequence(dev, api, orc):
    """1920 x 1080, eight frames, spawns on frames 0 and 4; every list, error and iteration count against the reference"""
    device, torch = dev
    W, H, N = 1920, 1080, 8
    sc = orc.gaussian_blur(orc.noise_image(W + 40, H + 40, 99, 0, 255), -1, 3).array()
    sc = np.clip(np.rint(sc), 0, 255).astype(np.uint8)
    sc[300:380, 500:620] = 255
    moves = [(0, 0), (2, -1), (3, 1), (5, 2), (6, 0), (4, -2), (7, 3), (9, 4)]
    fr = [np.ascontiguousarray(sc[20 + my:20 + H + my, 20 + mx:20 + W + mx]) for mx, my in moves]
    det = dict(detectRadius=20, detectThreshold=1.0, detectBorder=0)
    ref = ku.PointTrackerKltPyramidU8(orc, ku.SCALES, 2, None, **det)
    trk = device.DeviceKltTracker(ku.SCALES, 2, None, **det)
    total_iterations = 0
    for k in range(N):
        it0, bd0, n0 = ref.klt.iterations, ref.klt.borderIterations, len(ref.active)
        ref.process(fr[k])
        trk.process(torch.from_numpy(fr[k][None]).cuda())
        assert trk.stats() == (n0, ref.klt.iterations - it0, ref.klt.borderIterations - bd0)
        total_iterations += ref.klt.iterations - it0
        if k in (0, 4):
            ref.spawnTracks()
            trk.spawn()
        tg._compare_lists(trk.active(0), trk.spawned(0), trk.dropped(0), tg._snapshot(ref))
    assert len(ref.active) >= 1000 and total_iterations >= 100000      # a CPU run of the reference: 1206 tracks at the end, 187814 iterations
    for l in range(3):
        assert eq(trk.layer(0, l, 0), ref.layersU8[l]) and eq(trk.layer(0, l, 1), ref.derivXS16[l]) and eq(trk.layer(0, l, 2), ref.derivYS16[l])
    trk.close()


# ---------------------------------------------------------------------------------------------------------------- handles
def test_u8_handle_and_type_errors():
    """status codes on live and already-destroyed handles through the registry, in a child process (as test_gpu_klt.test_klt_handle_lifetime)"""
    code = """
import ctypes as C, numpy as np, torch
from boofcv_amd import _lib
L = _lib.load()
INV = _lib.BHIP_ERR_INVALID
c = C.c_void_p(); k8 = C.c_void_p(); kf = C.c_void_p()
assert L.bhip_ctx_create(0, C.byref(c)) == 0
scales = (C.c_int * 3)(1, 2, 4)
assert L.bhip_klt_create_u8(c, None, 2, scales, 3, 3, 1.0, 0, 160, 120, 2, C.byref(k8)) == 0
assert L.bhip_klt_create(c, None, 2, scales, 3, 3, 1.0, 0, 160, 120, 2, C.byref(kf)) == 0
assert L.bhip_klt_create_u8(c, None, 9, scales, 3, 3, 1.0, 0, 160, 120, 2, C.byref(C.c_void_p())) == _lib.BHIP_ERR_UNSUPPORTED
assert L.bhip_klt_spawn(k8, -1) == INV                                 # before the first process()
f8 = (torch.rand((2, 120, 160), device="cuda:0") * 255).to(torch.uint8).contiguous()
ff = f8.to(torch.float32).contiguous()
torch.cuda.synchronize()
p8, pf = C.c_void_p(f8.data_ptr()), C.c_void_p(ff.data_ptr())
# a handle made for one pixel type refuses the other type's calls
assert L.bhip_klt_process_dev_u8(kf, p8, 120 * 160, 160) == INV
assert L.bhip_klt_process_dev_f32(k8, pf, 120 * 160, 160) == INV
assert L.bhip_klt_process_dev_u8(k8, p8, 120 * 160, 159) == INV        # stride < width
assert L.bhip_klt_process_dev_u8(k8, p8, 120 * 160, 160) == 0
assert L.bhip_klt_process_dev_f32(kf, pf, 120 * 160, 160) == 0
buf8 = np.zeros(160 * 120, np.uint8); buf16 = np.zeros(160 * 120, np.int16); buff = np.zeros(160 * 120, np.float32)
assert L.bhip_klt_fetch_layer_u8(kf, 0, 0, buf8.ctypes.data_as(_lib._u8p)) == INV
assert L.bhip_klt_fetch_layer_s16(kf, 0, 0, 1, buf16.ctypes.data_as(_lib._i16p)) == INV
assert L.bhip_klt_fetch_layer(k8, 0, 0, 0, buff.ctypes.data_as(_lib._fp)) == INV
assert L.bhip_klt_fetch_layer_s16(k8, 0, 0, 0, buf16.ctypes.data_as(_lib._i16p)) == INV     # which 0 is the image: a GrayU8
assert L.bhip_klt_fetch_layer_u8(k8, 1, 0, buf8.ctypes.data_as(_lib._u8p)) == 0
assert np.array_equal(buf8.reshape(120, 160), f8[1].cpu().numpy())     # layer 0 at scale 1 is the frame
n = C.c_int(); e = C.c_longlong()
assert L.bhip_klt_dev_view_u8(kf, None, None, None, None, None, None, None, None, C.byref(n), C.byref(e)) == INV
assert L.bhip_klt_dev_view(k8, None, None, None, None, None, None, None, None, C.byref(n), C.byref(e)) == INV
pyr = C.c_void_p()
assert L.bhip_klt_dev_view_u8(k8, None, None, None, None, None, C.byref(pyr), None, None, C.byref(n), C.byref(e)) == 0
assert pyr.value and n.value >= 1024 and e.value == 160 * 120 + 80 * 60 + 40 * 30
assert L.bhip_klt_spawn(k8, 5) == _lib.BHIP_ERR_UNSUPPORTED
assert L.bhip_klt_spawn(k8, -1) == 0
a = (C.c_int * 2)()
assert L.bhip_klt_counts(k8, a, None, None) == 0 and a[0] > 10 and a[1] > 10
assert L.bhip_ctx_destroy(c) == 0                                      # context first: the trackers become inert shells
assert L.bhip_klt_counts(k8, a, None, None) == INV
assert L.bhip_klt_process_dev_u8(k8, p8, 120 * 160, 160) == INV
assert L.bhip_klt_fetch_layer_u8(k8, 0, 0, buf8.ctypes.data_as(_lib._u8p)) == INV
assert L.bhip_klt_spawn(k8, -1) == INV
assert L.bhip_klt_destroy(k8) == 0
assert L.bhip_klt_destroy(k8) == INV
assert L.bhip_klt_destroy(kf) == 0
assert L.bhip_ctx_destroy(c) == INV
print("ok", a[0], a[1])
"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("ok")
