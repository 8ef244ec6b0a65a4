"""CPU checks of the Horn-Schunck reference (hornschunck_ref.py) and of the Python mirror (boofcv_amd.hornschunck): the reference's own tests
re-expressed (FT: = main/boofcv-feature/src/test/java/boofcv/), the rule forms against the routines as written, the four deviations, and the
mirror's factory rules and argument checks, which fail before anything reaches C."""
import numpy as np
import pytest

import flow_ref as fr
import hornschunck_ref as hs

F = np.float32
W, H = 20, 30   # ChecksHornSchunck :42-43


# ---------------------------------------------------------------------------------------------------------------- the reference's tests
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_reference_process_known_answer(u8):   # FT:alg/flow/ChecksHornSchunck.java:55-75, createAlg: (0.2f, 1)
    dt = np.uint8 if u8 else np.float32
    image1, image2 = np.zeros((H, W), dt), np.zeros((H, W), dt)
    image1[0:30, 10:30] = 100   # fillRectangle(image, 100, x0, 0, 20, 30), clipped to the image
    image2[0:30, 11:31] = 100
    flow, _ = hs.horn_schunck(image1, image2, 0.2, 1, u8)
    for y in range(H - 1):
        assert flow[y, 9, 0] > 0.9
        assert abs(flow[y, 10, 1]) < 0.1
        assert flow[y, 10, 0] > 0.9
        assert abs(flow[y, 11, 1]) < 0.1


def _uniform_pair(orc, u8):
    """two images of fillUniform(image, rand, 0, 200) from one java.util.Random(234) (:40, :96-97)"""
    rand = orc.JavaRandom(234)
    if not u8:
        return [rand.fillUniform(orc.Gray(W, H), 0, 200).array().copy() for _ in range(2)]
    return [np.array([rand.nextInt(200) for _ in range(W * H)], np.uint8).reshape(H, W) for _ in range(2)]   # (byte)(rand.nextInt(range) + min)


def _expected(image1, image2, samples):
    """computeExpected :161-186: the eight-sample sum, signs +, -, ..., coordinates clamped, total *= 0.25"""
    imgs = (image1.astype(np.float32), image2.astype(np.float32))
    ys, xs = np.mgrid[0:H, 0:W]
    total = np.zeros((H, W), np.float32)
    for i, (dx, dy, k) in enumerate(samples):
        s = F(1) if i % 2 == 0 else F(-1)
        total = total + s * imgs[k][np.minimum(ys + dy, H - 1), np.minimum(xs + dx, W - 1)]
    return (total.astype(np.float64) * 0.25).astype(np.float32)


SAMPLES = {   # :79-88, :107-116, :135-144
    0: ((1, 0, 0), (0, 0, 0), (1, 1, 0), (0, 1, 0), (1, 0, 1), (0, 0, 1), (1, 1, 1), (0, 1, 1)),
    1: ((0, 1, 0), (0, 0, 0), (1, 1, 0), (1, 0, 0), (0, 1, 1), (0, 0, 1), (1, 1, 1), (1, 0, 1)),
    2: ((0, 0, 1), (0, 0, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (1, 1, 1), (1, 1, 0)),
}


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_reference_derivatives_against_the_eight_sample_sum(orc, u8):   # ChecksHornSchunck.computeDerivX / Y / T :77-159, tolerance 1
    image1, image2 = _uniform_pair(orc, u8)
    assert image1.std() > 20 and not np.array_equal(image1, image2)
    found = (hs.derivatives_u8 if u8 else hs.derivatives_f32)(image1, image2)
    for which, name in enumerate(("derivX", "derivY", "derivT")):
        want = _expected(image1, image2, SAMPLES[which])
        assert np.abs(found[which].astype(np.float32) - want).max() <= 1, name


def test_reference_average_flow(orc):   # FT:alg/flow/TestHornSchunck.java:35-86, tolerance 1e-4
    rand = orc.JavaRandom(123)
    flow = np.zeros((35, 30, 2), np.float32)
    for y in range(35):
        for x in range(30):
            flow[y, x, 0] = F(rand.nextFloat()) * F(2)
            flow[y, x, 1] = F(rand.nextFloat()) * F(2)
    found = hs.average(flow)
    p = np.pad(flow, ((1, 1), (1, 1), (0, 0)), "edge")
    expected = np.zeros_like(flow)
    for (dx, dy), coef in (((1, 0), hs.C_SIDE), ((-1, 0), hs.C_SIDE), ((0, 1), hs.C_SIDE), ((0, -1), hs.C_SIDE),
                           ((1, 1), hs.C_DIAG), ((-1, 1), hs.C_DIAG), ((1, -1), hs.C_DIAG), ((-1, -1), hs.C_DIAG)):   # computeAverage :62-74
        expected = expected + p[1 + dy:36 + dy, 1 + dx:31 + dx] * coef
    assert np.abs(found.astype(np.float64) - expected).max() <= 1e-4
    # the one clamped expression is borderAverageFlow + innerAverageFlow as written, bit for bit
    assert fr.same_bits(found, hs.average_as_written(flow))


# ---------------------------------------------------------------------------------------------------------------- rule forms and deviations
def test_border_deriv_t_of_u8_through_float_equals_the_integer_form():
    """HornSchunck_U8.borderDerivT goes through float and (short); over every sum of four differences, -1020 .. 1020, that is (d0+d1+d2+d3)/4 in int"""
    for s in range(-1020, 1021):
        d0 = max(-255, min(255, s))   # four differences in -255 .. 255 that sum to s
        d1 = max(-255, min(255, s - d0))
        d2 = max(-255, min(255, s - d0 - d1))
        d3 = s - d0 - d1 - d2
        assert -255 <= d3 <= 255
        want = abs(s) // 4 * (1 if s >= 0 else -1)
        assert int(hs.border_deriv_t_u8(d0, d1, d2, d3)) == want, s
        assert int(hs._trunc_div(np.int32(s), 4)) == want, s


def _as_written_f32(a, b):
    """HornSchunck_F32.computeDerivX / Y / T with their loops, on dense images (so :114's image2.stride is image1's)"""
    h, w = a.shape[0] - 1, a.shape[1] - 1
    dX, dY, dT = (np.full(a.shape, 77, np.float32) for _ in range(3))   # 77: what a reused array might hold
    for y in range(h):
        for x in range(w):
            dX[y, x] = F(0.25) * ((a[y, x + 1] - a[y, x]) + (a[y + 1, x + 1] - a[y + 1, x]) + (b[y, x + 1] - b[y, x]) + (b[y + 1, x + 1] - b[y + 1, x]))
            dY[y, x] = F(0.25) * ((a[y + 1, x] - a[y, x]) + (a[y + 1, x + 1] - a[y, x + 1]) + (b[y + 1, x] - b[y, x]) + (b[y + 1, x + 1] - b[y, x + 1]))
            dT[y, x] = F(0.25) * ((b[y, x] - a[y, x]) + (b[y, x + 1] - a[y, x + 1]) + (b[y + 1, x] - a[y + 1, x]) + (b[y + 1, x + 1] - a[y + 1, x + 1]))
    dX[:, w] = 0
    for x in range(w):
        dX[h, x] = F(0.5) * ((a[h, x + 1] - a[h, x]) + (b[h, x + 1] - b[h, x]))
        dY[h, x] = 0
    for y in range(h):
        dY[y, w] = F(0.5) * ((a[y + 1, w] - a[y, w]) + (b[y + 1, w] - b[y, w]))

    def t(x, y):
        x, y = min(x, w), min(y, h)
        return b[y, x] - a[y, x]

    for x, y in [(w, y) for y in range(h + 1)] + [(x, h) for x in range(w)]:
        dT[y, x] = F(0.25) * (t(x, y) + t(x + 1, y) + t(x, y + 1) + t(x + 1, y + 1))
    return dX, dY, dT


@pytest.mark.parametrize("shape", [(30, 20), (1, 1), (1, 9), (9, 1), (2, 2)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_derivative_rules_equal_the_loops_and_the_unwritten_corner_is_zero(shape):
    rng = np.random.RandomState(3)
    a, b = (rng.rand(*shape) * 200).astype(np.float32), (rng.rand(*shape) * 200).astype(np.float32)
    got, want = hs.derivatives_f32(a, b), _as_written_f32(a, b)
    assert want[1][-1, -1] == 77, "the reference never writes derivY(w, h)"
    want[1][-1, -1] = 0   # deviation 1: the value for a freshly constructed instance
    for g, w_, name in zip(got, want, ("derivX", "derivY", "derivT")):
        assert fr.same_bits(g, w_), name
    # GrayU8: the integer taps are the float taps where those are exact (whole numbers, sums below 2^24), up to the truncation
    a8, b8 = a.astype(np.uint8), b.astype(np.uint8)
    gi = hs.derivatives_u8(a8, b8)
    gf = _as_written_f32(a8.astype(np.float32), b8.astype(np.float32))
    gf[1][-1, -1] = 0
    for g, f_, name in zip(gi, gf, ("derivX", "derivY", "derivT")):
        assert g.dtype == np.int16 and np.array_equal(g, np.trunc(f_).astype(np.int16)), name


def test_deriv_t_reads_image1_whatever_the_strides_are():
    """deviation 2: :114 reads image1.data[index1+1+image2.stride]; on sub-images with different strides that is another pixel.  The rule form has
    no stride: views with different strides give the dense result."""
    rng = np.random.RandomState(4)
    a, b = (rng.rand(7, 9) * 200).astype(np.float32), (rng.rand(7, 9) * 200).astype(np.float32)
    big_a, big_b = np.full((7, 14), 5, np.float32), np.full((7, 11), 6, np.float32)
    big_a[:, 2:11], big_b[:, 1:10] = a, b
    for g, w_ in zip(hs.derivatives_f32(big_a[:, 2:11], big_b[:, 1:10]), hs.derivatives_f32(a, b)):
        assert fr.same_bits(g, w_)


def test_no_iterations_give_the_zero_flow_and_nan_spreads_one_pixel_per_iteration():
    src, dst = fr.scene(24, 18, 9, flat=(8, 6, 6, 5))
    for n in (0, -3):   # deviation 4
        flow, _ = hs.horn_schunck(src, dst, 20.0, n)
        assert flow.shape == (18, 24, 2) and not flow.any()
    nan = [np.isnan(hs.horn_schunck(src, dst, 0.0, n)[0][:, :, 0]) for n in (1, 2, 3)]   # alpha = 0 on the flat patch: 0/0
    assert nan[0].sum() > 0 and not nan[0][:6].any()
    for before, after in zip(nan, nan[1:]):
        grown = np.pad(before, 1)[:, :]
        spread = np.zeros_like(before)
        for dy in range(3):
            for dx in range(3):
                spread |= grown[dy:dy + 18, dx:dx + 24]
        assert np.array_equal(after, spread | before) and after.sum() > before.sum()


# ---------------------------------------------------------------------------------------------------------------- the mirror
class NoGpu:
    _h = None


def test_factory_defaults_and_refusals():   # F:factory/flow/FactoryDenseOpticalFlow.java:122-138
    from boofcv_amd import api, hornschunck as m
    cfg = m.ConfigHornSchunck()
    assert (cfg.alpha, cfg.numIterations) == (20.0, 1000)
    alg = m.FactoryDenseOpticalFlowHornSchunck.hornSchunck(None, api.GrayF32, ctx=NoGpu())
    assert isinstance(alg, m.DenseOpticalFlowHornSchunck) and alg.getInputType() is api.GrayF32 and (alg.alpha, alg.numIterations) == (20.0, 1000)
    alg = m.FactoryDenseOpticalFlowHornSchunck.hornSchunck(m.ConfigHornSchunck(0.2, 1), api.GrayU8, ctx=NoGpu())
    assert alg.getInputType() is api.GrayU8 and (alg.alpha, alg.numIterations) == (0.2, 1)
    for it in (api.GrayS16, api.GrayS32, api.PlanarType(3, api.GrayF32), api.InterleavedType(3, api.GrayF32), api.Planar):
        with pytest.raises(RuntimeError, match="use the Java path") as e:
            m.FactoryDenseOpticalFlowHornSchunck.hornSchunck(None, it, ctx=NoGpu())
        assert not isinstance(e.value, api.IllegalArgumentException)
    with pytest.raises(RuntimeError, match="use the Java path"):   # the api package's factory keeps refusing
        api.FactoryDenseOpticalFlow.hornSchunck(None, api.GrayF32)
    assert not hasattr(api, "ConfigHornSchunck")


def test_process_checks_its_arguments_before_anything_reaches_c():
    """with a NoGpu context a call that reached C would fail on the missing handle, not with IllegalArgumentException"""
    from boofcv_amd import api, hornschunck as m
    alg = m.FactoryDenseOpticalFlowHornSchunck.hornSchunck(None, api.GrayF32, ctx=NoGpu())
    flow = api.ImageFlow(6, 5)
    flow.data[...] = 3.5
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayU8(6, 5), api.GrayU8(6, 5), flow)
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayF32(6, 5), api.GrayF32(6, 4), flow)
    with pytest.raises(api.IllegalArgumentException):   # deviation 3: the Java does not check the flow's size
        alg.process(api.GrayF32(6, 5), api.GrayF32(6, 5), api.ImageFlow(5, 6))
    bad = api.GrayF32(6, 5)
    bad.stride = 4   # a view that does not fit its array: refused by the marshaller
    with pytest.raises(api.IllegalArgumentException):
        alg.process(bad, api.GrayF32(6, 5), flow)
    assert (flow.data == 3.5).all()
