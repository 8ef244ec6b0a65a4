"""CPU checks of the dense KLT optical flow reference (flow_ref.py) and of the Python mirror (api.FactoryDenseOpticalFlow, ImageFlow): the
vectorised tracker against klt_ref's tracker run pixel by pixel, the order-free form of checkNeighbors against the literal loop, the
reference's own tests re-expressed (FT: = main/boofcv-feature/src/test/java/boofcv/), and the mirror's factory rules."""
import numpy as np
import pytest

import flow_ref as fr
import klt_ref as kr
import klt_u8_ref as ku

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- tracker check
def _pixel_by_pixel(layers0, dx0, dy0, layers1, scales, radius, cfg):
    """DenseOpticalFlowKlt.process :78-92 with klt_ref's tracker, one pixel at a time"""
    H, W = layers0[0].shape
    klt = kr.KltTracker(cfg)
    tracker = kr.PyramidKltTracker(klt, scales)
    feature = kr.PyramidKltFeature(len(scales), radius)
    rec = dict(fault=np.zeros((H, W), np.int32), error=np.zeros((H, W), np.float32), dx=np.zeros((H, W), np.float32), dy=np.zeros((H, W), np.float32))
    for y in range(H):
        for x in range(W):
            tracker.setImage(layers0, dx0, dy0)
            feature.setPosition(x, y)
            try:
                if not tracker.setDescription(feature):
                    rec["fault"][y, x] = fr.NO_DESCRIPTION
                    continue
                tracker.setImage(layers1)
                fault = tracker.track(feature)
            except kr.Thrown:
                rec["fault"][y, x] = fr.THROWS
                continue
            rec["fault"][y, x] = fault
            if fault == kr.SUCCESS:
                rec["error"][y, x] = tracker.getError()
                rec["dx"][y, x] = feature.x - F(x)
                rec["dy"][y, x] = feature.y - F(y)
    return rec


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_track_all_equals_the_tracker_run_pixel_by_pixel(orc, u8):
    W, H, scales, radius = 24, 18, (1, 2), 2
    src, dst = fr.scene(W, H, 77, flat=(2, 2, 11, 10), occluder=(15, 9, 6, 6))
    if u8:
        src, dst = np.rint(src).astype(np.uint8), np.rint(dst).astype(np.uint8)
    l0, gx, gy, l1 = fr.pyramids(orc, src, dst, scales, u8)
    cfg = kr.KltConfig(maxPerPixelError=12.0)
    got = fr.track_all(l0, gx, gy, l1, scales, radius, cfg)
    f32 = lambda v: [np.ascontiguousarray(a, np.float32) for a in v]
    want = _pixel_by_pixel(f32(l0), f32(gx), f32(gy), f32(l1), scales, radius, cfg)
    assert np.array_equal(got["fault"], want["fault"])
    for k in ("error", "dx", "dy"):
        assert fr.same_bits(got[k], want[k]), k
    counts = np.bincount(got["fault"].reshape(-1), minlength=7)
    assert counts[fr.SUCCESS] > 100 and counts[fr.NO_DESCRIPTION] > 5 and counts[fr.LARGE_ERROR] > 5, counts   # the scene exercises the branches


# ---------------------------------------------------------------------------------------------------------------- fold check
SCORES = np.array([0.5, 1.25, 2.0, 3.5, 7.0], np.float32)


def _table(seed, H=17, W=23, fail=0.3):
    """a synthetic record table full of ties: scores from five values; flows (a, b) / (b, a) / (-a, b), which have equal motion"""
    rng = np.random.RandomState(seed)
    a, b = F(0.75), F(-1.5)
    flows = np.array([(a, b), (b, a), (-a, b), (F(0.25), F(0.5)), (F(2), F(0)), (F(0), F(0))], np.float32)
    pick = rng.randint(0, len(flows), (H, W))
    ok = rng.rand(H, W) >= fail
    return dict(fault=np.where(ok, fr.SUCCESS, rng.randint(1, 7, (H, W))).astype(np.int32), error=np.where(ok, SCORES[rng.randint(0, 5, (H, W))], 0).astype(np.float32),
                dx=np.where(ok, flows[pick, 0], 0).astype(np.float32), dy=np.where(ok, flows[pick, 1], 0).astype(np.float32))


def _tables():
    out = [("random %d" % s, _table(s)) for s in range(4)]
    t = _table(10)
    t["fault"][:] = fr.FAILED
    t["error"][:] = 0; t["dx"][:] = 0; t["dy"][:] = 0
    out.append(("all failed", t))
    t = _table(11, fail=0.0)
    t["error"][:] = SCORES[2]; t["dx"][:] = F(0.75); t["dy"][:] = F(-1.5)
    out.append(("all equal", t))
    # a later neighbour's score equal, bit for bit, to a centre's score * 0.7f: the centre keeps its own flow only through the motion test
    t = _table(12, fail=0.0)
    t["error"][:] = SCORES[3]
    s07 = SCORES[3] * fr.MAGIC_ADJUSTMENT
    for (y, x), (fx, fy) in (((5, 5), (F(0.1), F(0.1))), ((5, 12), (F(3), F(3))), ((11, 7), (F(0.75), F(-1.5)))):
        t["error"][y, x + 1] = s07          # the pixel after (y, x)
        t["dx"][y, x], t["dy"][y, x] = F(0.75), F(-1.5)
        t["dx"][y, x + 1], t["dy"][y, x + 1] = fx, fy   # less / more / equal motion
    out.append(("0.7f tie", t))
    return out


def test_the_reduction_equals_the_sequential_pass_on_tables_full_of_ties():
    seen = np.zeros(5, np.int64)
    for radius in (1, 2, 3):
        for name, t in _tables():
            held = np.random.RandomState(radius).rand(*t["fault"].shape, 2).astype(np.float32)   # what the caller's ImageFlow held: y survives
            for flow in (None, held):
                a, b = fr.assign_sequential(t, radius, flow), fr.assign_reduce(t, radius, flow)
                assert fr.same_bits(a, b), (name, radius)
            cls = fr.classify(t, radius)
            seen += np.bincount(cls.reshape(-1), minlength=5)
            inv = np.isnan(a[:, :, 0])
            assert np.array_equal(inv, cls == fr.INVALID)
            assert np.array_equal(a[inv, 1], held[inv, 1])
            if name == "all failed":
                assert inv.all()
            if name == "0.7f tie":
                assert a[5, 5, 0] == F(0.1) and a[5, 12, 0] == F(0.75) and a[11, 7, 0] == F(0.75)   # less motion wins, more and equal do not
                assert cls[5, 5] == fr.TIE
    assert (seen >= 10).all(), dict(zip(fr.CLASS_NAMES, seen))


# ---------------------------------------------------------------------------------------------------------------- the reference's tests
def _rect(img, value, x0, y0, w, h):   # ImageMiscOps.fillRectangle
    img[y0:y0 + h, x0:x0 + w] = value


def _klt(orc, img0, img1, scales, radius, cfg=None, flow=None):
    return fr.dense_flow_klt(orc, img0, img1, scales, radius, cfg, flow=flow)[0]


def test_reference_positive_and_negative(orc):   # FT:alg/flow/TestDenseOpticalFlowKlt.java:44-144
    cfg = kr.KltConfig(maxPerPixelError=15)
    img0, img1 = np.zeros((40, 30), np.float32), np.zeros((40, 30), np.float32)
    _rect(img0, 50, 10, 12, 2, 2)
    _rect(img1, 50, 11, 13, 2, 2)
    flow = _klt(orc, img0, img1, (1, 2), 3, cfg)
    assert np.isnan(flow[0, 0, 0]) and np.isnan(flow[39, 29, 0])   # no texture in the image so KLT can't do anything
    for x, y in ((10, 12), (11, 12), (10, 13), (11, 13)):           # there is texture at the target
        assert not np.isnan(flow[y, x, 0])
        assert abs(flow[y, x, 0] - 1) <= 0.05 and abs(flow[y, x, 1] - 1) <= 0.05
    img0, img1 = np.zeros((40, 30), np.float32), np.zeros((40, 30), np.float32)
    _rect(img0, 200, 7, 9, 5, 5)
    flow = _klt(orc, img0, img1, (1, 2), 3, cfg)
    assert np.isnan(flow[:, :, 0]).mean() >= 0.90


@pytest.fixture(scope="module")
def general(orc):
    """GeneralDenseOpticalFlowChecks :49-62 for TestFlowKlt_to_DenseOpticalFlow: flowKlt(null, 2, GrayF32, null), Random(234), fillUniform 0..256"""
    orig = orc.JavaRandom(234).fillUniform(orc.Gray(20, 25), 0, 256).array().copy()
    shift = lambda dx, dy: np.roll(np.roll(orig, dx, 1), dy, 0)   # :198-220: the wrap-around shift
    run = lambda a, b: _klt(orc, a, b, (1, 2, 4), 2)
    return orig, shift, run


def test_reference_process_edges(general):   # FT:abst/flow/GeneralDenseOpticalFlowChecks.java:86-126
    orig, shift, run = general
    H, W = orig.shape
    valid = ~np.isnan(run(orig, shift(1, 0))[:, :, 0])
    assert valid[0].sum() >= W // 3 and valid[H - 2].sum() >= W // 3
    valid = ~np.isnan(run(orig, shift(0, 1))[:, :, 0])
    assert valid[:, 0].sum() >= H // 3 and valid[:, W - 2].sum() >= H // 3


@pytest.mark.parametrize("dx,dy", [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
def test_reference_planar_motion(general, dx, dy):   # :131-162
    orig, shift, run = general
    flow = run(orig, shift(dx, dy))
    assert not np.isnan(flow[10, 10, 0])
    assert abs(flow[10, 10, 0] - dx) <= 0.2 and abs(flow[10, 10, 1] - dy) <= 0.2


def test_reference_sub_image_and_input_size(general, orc):   # :167-210, through the mirror's sub-image path on the reference's arithmetic
    orig, shift, run = general
    a = run(orig, shift(1, -1))
    big0, big1 = np.full((31, 29), 7, np.float32), np.full((31, 29), 9, np.float32)
    big0[3:28, 5:25], big1[3:28, 5:25] = orig, shift(1, -1)
    b = run(big0[3:28, 5:25], big1[3:28, 5:25])
    assert fr.same_bits(a, b)
    assert run(np.zeros((35, 40), np.float32), np.zeros((35, 40), np.float32)).shape == (35, 40, 2)   # checkChangeInputSize: it does not blow up


# ---------------------------------------------------------------------------------------------------------------- the mirror
class NoGpu:
    _h = None


def test_image_flow_behaves_like_the_reference():   # F:struct/flow/ImageFlow.java
    from boofcv_amd import api
    f = api.ImageFlow(4, 3)
    assert f.data.shape == (3, 4, 2) and f.data.dtype == np.float32 and not f.data.any()
    assert f.isValid(0, 0) and f.get(3, 2).isValid()
    f.get(1, 2).set(1.5, -2.0)
    assert tuple(f.data[2, 1]) == (1.5, -2.0) and f.get(1, 2).getX() == 1.5 and f.get(1, 2).y == -2.0
    f.invalidateAll()                                    # x only
    assert np.isnan(f.data[:, :, 0]).all() and f.data[2, 1, 1] == -2.0 and not f.isValid(1, 2)
    f.get(0, 0).markInvalid()
    with pytest.raises(api.IllegalArgumentException):
        f.get(4, 0)
    with pytest.raises(api.IllegalArgumentException):
        f.get(0, -1)
    g = api.ImageFlow(4, 3)
    g.setTo(f)
    assert fr.same_bits(g.data, f.data)
    f.fillZero()
    assert not f.data.any()
    f.get(3, 2).set(5, 6)                                # flat index 11
    f.reshape(6, 4)                                      # grows: the elements it had keep their flat index, new ones are (0, 0)
    assert f.data.shape == (4, 6, 2) and tuple(f.data[1, 5]) == (5, 6) and not f.data[2:].any()
    f.reshape(2, 2)
    assert (f.getWidth(), f.getHeight(), f.data.shape) == (2, 2, (2, 2, 2))


def test_factory_defaults_and_refusals():   # F:factory/flow/FactoryDenseOpticalFlow.java:61-82
    from boofcv_amd import api
    alg = api.FactoryDenseOpticalFlow.flowKlt(None, 3, api.GrayF32, None, ctx=NoGpu())
    assert isinstance(alg, api.DenseOpticalFlow) and alg.getInputType() is api.GrayF32
    assert alg.config.pyramidScaling == [1, 2, 4] and alg.config.config.maxIterations == 15 and alg.radius == 3
    cfg = api.PkltConfig(templateRadius=5, pyramidScaling=(1, 2))
    alg = api.FactoryDenseOpticalFlow.flowKlt(cfg, 2, api.GrayU8, api.GrayS16, ctx=NoGpu())
    assert alg.radius == 2 and alg.config is cfg and alg.getInputType() is api.GrayU8   # templateRadius is not read
    api.FactoryDenseOpticalFlow.flowKlt(None, 1, api.GrayU8, None, ctx=NoGpu())
    api.FactoryDenseOpticalFlow.flowKlt(None, 1, api.GrayF32, api.GrayF32, ctx=NoGpu())
    for it, dt in ((api.GrayU8, api.GrayS32), (api.GrayU8, api.GrayF32), (api.GrayF32, api.GrayS16), (api.GrayS16, None), (api.GrayS16, api.GrayS16),
                   (api.PlanarType(3, api.GrayF32), None), (api.InterleavedType(3, api.GrayF32), None)):
        with pytest.raises(RuntimeError, match="use the Java path") as e:
            api.FactoryDenseOpticalFlow.flowKlt(None, 2, it, dt, ctx=NoGpu())
        assert not isinstance(e.value, api.IllegalArgumentException)
    for name in ("region", "hornSchunck", "hornSchunckPyramid", "broxWarping"):
        with pytest.raises(RuntimeError, match="use the Java path"):
            getattr(api.FactoryDenseOpticalFlow, name)(None, api.GrayF32)


def test_process_checks_its_arguments_and_keeps_y_of_invalid_pixels():
    from boofcv_amd import api
    alg = api.FactoryDenseOpticalFlow.flowKlt(None, 2, api.GrayF32, None, ctx=NoGpu())
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayU8(6, 5), api.GrayU8(6, 5), api.ImageFlow(6, 5))
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayF32(6, 5), api.GrayF32(6, 4), api.ImageFlow(6, 5))
    with pytest.raises(api.IllegalArgumentException):   # the deviation: the Java does not check the flow's size
        alg.process(api.GrayF32(6, 5), api.GrayF32(6, 5), api.ImageFlow(5, 6))
    # what the library returns for a new ImageFlow is merged into what the caller's flow held: y of an invalid pixel survives, as in Java
    fresh = np.zeros((5, 6, 2), np.float32)
    fresh[:, :, 0] = np.nan
    fresh[1:4, 2:5] = (0.5, -0.25)
    alg._run = lambda source, destination: fresh.copy()
    flow = api.ImageFlow(6, 5)
    flow.data[...] = np.arange(60, dtype=np.float32).reshape(5, 6, 2)
    held = flow.data.copy()
    alg.process(api.GrayF32(6, 5), api.GrayF32(6, 5), flow)
    want = fresh.copy()
    want[0, :, 1] = held[0, :, 1]; want[4, :, 1] = held[4, :, 1]; want[:, :2, 1] = held[:, :2, 1]; want[:, 5, 1] = held[:, 5, 1]
    assert fr.same_bits(flow.data, want)
    assert fr.same_bits(flow.data, fr.assign_reduce(dict(fault=np.where(np.isnan(fresh[:, :, 0]), fr.FAILED, fr.SUCCESS), error=np.ones((5, 6), np.float32),
                                                         dx=np.nan_to_num(fresh[:, :, 0]), dy=fresh[:, :, 1]), 0, held))
