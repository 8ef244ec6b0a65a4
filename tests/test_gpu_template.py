"""GPU: template matching (FactoryTemplateMatching.createIntensity / createMatcher: SAD, SSE and NCC on GrayU8 / GrayF32, with and without a
mask), bit for bit against tests/template_ref.py, through the device-batched API (device.py), the host-buffer API (api.py) and the C ABI.
Every comparison is exact; float values are compared as bit patterns.

The kernel's tile is 64 x 16 output pixels per workgroup and it walks the template in chunks of 16 rows (TPL_TW, TPL_TH, TPL_CH in
boofcv_amd/csrc/template.hip): the 300 x 70 image spans five tiles in x and up to five in y, the template heights 16, 17, 20, 32 and 40 are
one full chunk, a chunk and a row, two chunks and two and a half; widths that are no multiple of four take the tail of the column loop.  The
width limit is 160 (BHIP_TEMPLATE_MAX_WIDTH), so the masked GrayU8 SSE case that wraps Java's int (130 columns or more) is kept."""
import ctypes as C
import functools

import numpy as np
import pytest

import template_ref as tr
import view_layouts as vl

pytestmark = pytest.mark.gpu

MAX_WIDTH = 160
DTYPES = ("u8", "f32")
NP = {"u8": np.uint8, "f32": np.float32}
# image (W, H), template (tw, th)
CASES = [
    ((300, 70), (1, 1)),
    ((300, 70), (5, 8)),
    ((300, 70), (8, 5)),
    ((300, 70), (16, 16)),
    ((300, 70), (33, 17)),
    ((300, 70), (70, 3)),       # wider than a tile
    ((300, 70), (3, 40)),       # taller than a tile, three chunks
    ((300, 70), (4, 32)),       # two full chunks
    ((300, 70), (MAX_WIDTH, 20)),   # the limit
    ((67, 21), (5, 8)),
    ((67, 21), (67, 21)),       # the template equals the image: w = h = 1
]
FLAT = (slice(20, 50), slice(100, 180))   # a flat region of the 300 x 70 image


@pytest.fixture(scope="module")
def api():
    from boofcv_amd import api
    return api


@pytest.fixture(scope="module")
def dev():
    import torch
    from boofcv_amd.device import DeviceImageOps
    return DeviceImageOps(device=0), torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def _image(W, H, kind, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "u8":
        img = rng.integers(0, 256, (H, W), dtype=np.uint8)
        img[0, 0], img[0, 1] = 0, 255
    else:
        img = (rng.random((H, W)) * 255).astype(np.float32)
        img[rng.integers(0, H, 6), rng.integers(0, W, 6)] = np.float32(-13.5)
    if (W, H) == (300, 70):
        img[FLAT] = 77
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _template(tw, th, kind, seed=0, image_size=None):
    """a noisy crop of the image (so that there is a good match), or random"""
    rng = np.random.default_rng(2000 + 7 * seed + tw + 1000 * th)
    if image_size is not None and (tw, th) == image_size:
        t = np.array(_image(tw, th, kind, seed))
    elif kind == "u8":
        t = rng.integers(0, 256, (th, tw), dtype=np.uint8)
    else:
        t = (rng.random((th, tw)) * 255).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _mask(tw, th, kind, seed=0):
    rng = np.random.default_rng(3000 + seed + tw + 1000 * th)
    vals = np.array([0, 1, 2, 255], np.uint8) if kind == "u8" else np.array([0, 0.5, 1, 3.25], np.float32)
    m = rng.choice(vals, (th, tw))
    m.reshape(-1)[0] = vals[0]
    m.reshape(-1)[-1] = vals[-1]
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _want(W, H, tw, th, kind, score, masked, seed=0):
    out = tr.intensity(_image(W, H, kind, seed), _template(tw, th, kind, seed, (W, H)), _mask(tw, th, kind, seed) if masked else None, score)
    out.setflags(write=False)
    return out


def _same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    bad = _bits(got) != _bits(want)
    if bad.any():
        ys, xs = np.nonzero(bad)[-2:]
        raise AssertionError("%s: %d values differ; first (x, y) %s: got %r want %r" % (what, int(bad.sum()), (int(xs[0]), int(ys[0])), got[bad][0], want[bad][0]))


def _t(dev, a):
    ops, torch = dev
    return torch.as_tensor(np.array(a), device=ops.device)


# ---- intensity, device form ----
@pytest.mark.parametrize("kind", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_t%dx%d" % (c[0] + c[1]))
def test_intensity_cases(dev, case, kind):
    ops, torch = dev
    (W, H), (tw, th) = case
    img, tpl, mask = _t(dev, _image(W, H, kind)), _t(dev, _template(tw, th, kind, 0, (W, H))), _t(dev, _mask(tw, th, kind))
    for score in tr.SCORES:
        for masked in (False, True):
            got = ops.templateIntensity(img.unsqueeze(0), tpl, mask if masked else None, score)
            ops.ctx.synchronize()
            want = _want(W, H, tw, th, kind, score, masked)
            _same(got[0], want, "%s %s %s masked=%s" % (case, kind, score, masked))
            assert np.isfinite(want).all()
    if (W, H) == (300, 70) and tw <= 33 and th <= 17:
        # NCC of a window inside the flat region: top = 0 over EPS, exactly 0 (and it was compared above)
        assert _want(W, H, tw, th, kind, tr.NCC, True)[25 + th // 2, 110 + tw // 2] == 0


def test_masked_u8_sse_wraps_as_java_int(dev):
    """rows of 140 elements with error 255 and mask 255: 140 * 255 * 65025 > 2^31, the int row total is negative in Java"""
    ops, torch = dev
    image = np.full((6, 200), 255, np.uint8)
    image[:, 150:] = 9
    template = np.zeros((2, 140), np.uint8)
    mask = np.full((2, 140), 255, np.uint8)
    with np.errstate(over="ignore"):
        want = tr.intensity(image, template, mask, tr.SSE)
    assert want[1, 70] < 0
    got = ops.templateIntensity(_t(dev, image).unsqueeze(0), _t(dev, template), _t(dev, mask), tr.SSE)
    ops.ctx.synchronize()
    _same(got[0], want, "wrap")


@pytest.mark.parametrize("kind", DTYPES)
@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per_image"])
def test_batch_of_three(dev, kind, per_image):
    ops, torch = dev
    W, H, tw, th = 131, 37, 9, 18
    imgs = np.stack([_image(W, H, kind, s) for s in range(3)])
    seeds = (0, 1, 2) if per_image else (0, 0, 0)
    tpls = np.stack([_template(tw, th, kind, s) for s in seeds])
    masks = np.stack([_mask(tw, th, kind, s) for s in seeds])
    for score in tr.SCORES:
        for masked in (False, True):
            t, m = (_t(dev, tpls), _t(dev, masks)) if per_image else (_t(dev, tpls[0]), _t(dev, masks[0]))
            got = ops.templateIntensity(_t(dev, imgs), t, m if masked else None, score)
            ops.ctx.synchronize()
            for b in range(3):
                want = tr.intensity(imgs[b], tpls[b], masks[b] if masked else None, score)
                _same(got[b], want, "%s %s masked=%s image %d" % (kind, score, masked, b))


@pytest.mark.parametrize("kind", DTYPES)
@pytest.mark.parametrize("layout", vl.LAYOUTS)
def test_strided_views_and_guard_bands(dev, kind, layout):
    """images, templates, masks and the output are windows of sentinel-filled parents; the output's border is 0 after the masked call too"""
    ops, torch = dev
    W, H, tw, th, B = 70, 23, 7, 18, 2
    tdt = torch.uint8 if kind == "u8" else torch.float32
    imgs = np.stack([_image(W, H, kind, s) for s in range(B)])
    tpls = np.stack([_template(tw, th, kind, s) for s in range(B)])
    masks = np.stack([_mask(tw, th, kind, s) for s in range(B)])
    views = []
    for a, shape in ((imgs, (B, H, W)), (tpls, (B, th, tw)), (masks, (B, th, tw))):
        parent, view = vl.make_view(layout, *shape, tdt, ops.device)
        view.copy_(torch.as_tensor(a, device=ops.device))
        views.append(view)
    for score in tr.SCORES:
        for masked in (False, True):
            parent, out = vl.make_view(layout, B, H, W, torch.float32, ops.device)
            before = vl.snapshot(parent)
            torch.cuda.synchronize()
            got = ops.templateIntensity(views[0], views[1], views[2] if masked else None, score, out=out)
            ops.ctx.synchronize()
            assert got is out
            vl.assert_only_view_written(parent, out, before, "%s %s %s" % (layout, kind, score))
            for b in range(B):
                _same(out[b], tr.intensity(imgs[b], tpls[b], masks[b] if masked else None, score), "%s %s %s masked=%s" % (layout, kind, score, masked))


# ---- the host api and the C ABI ----
@pytest.mark.parametrize("kind", DTYPES)
def test_host_api_on_sub_images(api, kind):
    """TemplateMatchingIntensity on views with a start index and a stride; the same object is reused, so the masked call must clear the border"""
    W, H, tw, th = 67, 21, 5, 8
    cls = api.GrayU8 if kind == "u8" else api.GrayF32

    def view(a, pad):
        h, w = a.shape
        big = np.full((h + 2 * pad, w + 2 * pad + 1), 99, a.dtype)
        big[pad:pad + h, pad:pad + w] = a
        return cls(w + 2 * pad + 1, h + 2 * pad, big.reshape(-1)).subimage(pad, pad, pad + w, pad + h)
    image, tpl, mask = _image(W, H, kind), _template(tw, th, kind), _mask(tw, th, kind)
    for score in tr.SCORES:
        alg = api.FactoryTemplateMatching.createIntensity(score, cls)
        alg.setInputImage(view(image, 3))
        alg.process(view(np.array(_template(9, 4, kind)), 1))    # leaves another border behind
        alg.process(view(tpl, 2), view(mask, 1))
        _same(alg.getIntensity().array(), _want(W, H, tw, th, kind, score, True), "%s %s masked" % (kind, score))
        assert (alg.getBorderX0(), alg.getBorderY0(), alg.getBorderX1(), alg.getBorderY1()) == tr.borders(tw, th)
        alg.process(view(tpl, 2))
        _same(alg.getIntensity().array(), _want(W, H, tw, th, kind, score, False), "%s %s" % (kind, score))


def test_direct_c_abi_call(api):
    from boofcv_amd import _lib
    L, ctx = _lib.load(), api.Context.default()
    W, H, tw, th = 67, 21, 5, 8
    image, tpl, mask = np.array(_image(W, H, "f32")), np.array(_template(tw, th, "f32")), np.array(_mask(tw, th, "f32"))
    out = np.full((H, W), np.nan, np.float32)
    fp = lambda a: a.ctypes.data_as(_lib._fp)   # noqa: E731
    st = L.bhip_template_intensity_f32(ctx._h, _lib.BHIP_TEMPLATE_NCC, fp(image), 0, W, W, H, fp(tpl), 0, tw, tw, th, fp(mask), 0, tw, tw, th, fp(out), 0, W)
    assert st == _lib.BHIP_OK, L.bhip_last_error(ctx._h)
    _same(out, _want(W, H, tw, th, "f32", tr.NCC, True), "C ABI")
    # the selection: no candidates, no matches
    n = C.c_int(-1)
    xy, sc = np.zeros((4, 2), np.int16), np.zeros(4, np.float32)
    st = L.bhip_template_select_f32(ctx._h, fp(out), 0, W, W, H, xy.ctypes.data_as(_lib._i16p), 0, 3, 1, xy.ctypes.data_as(_lib._i16p), fp(sc), C.byref(n))
    assert st == _lib.BHIP_OK and n.value == 0
    bad = np.array([[W, 0]], np.int16)
    st = L.bhip_template_select_f32(ctx._h, fp(out), 0, W, W, H, bad.ctypes.data_as(_lib._i16p), 1, 3, 1, xy.ctypes.data_as(_lib._i16p), fp(sc), C.byref(n))
    assert st == _lib.BHIP_ERR_INVALID


# ---- matching ----
MATCH_IMAGE = (150, 60)
MATCH_TEMPLATE = (9, 12)


@functools.lru_cache(maxsize=None)
def _match_scene(kind, seed):
    """noise with three copies of the template planted, one of them degraded"""
    W, H = MATCH_IMAGE
    tw, th = MATCH_TEMPLATE
    img = np.array(_image(W, H, kind, 10 + seed))
    tpl = np.array(_template(tw, th, kind, 10 + seed))
    for i, (x, y) in enumerate(((10, 7), (70, 30), (120, 44))):
        img[y:y + th, x:x + tw] = tpl
        if i == 2:
            img[y, x] = 0
    return img, tpl


@functools.lru_cache(maxsize=None)
def _want_match(kind, seed, score, max_matches, radius):
    img, tpl = _match_scene(kind, seed)
    return tr.match(img, tpl, None, score, max_matches, radius)


@pytest.mark.parametrize("kind", DTYPES)
@pytest.mark.parametrize("score", [tr.SAD, tr.NCC], ids=["minimise", "maximise"])
@pytest.mark.parametrize("radius", [2, 6], ids=["r2", "template_radius"])
def test_device_match(dev, kind, score, radius):
    ops, torch = dev
    scenes = [_match_scene(kind, s) for s in range(2)]
    imgs = _t(dev, np.stack([s[0] for s in scenes]))
    tpls = _t(dev, np.stack([s[1] for s in scenes]))
    for max_matches in (1, 3, 5000):   # 5000 is more than there are candidates: N == n, the list is still permuted
        xy, sc, counts, ncand = ops.templateMatch(imgs, tpls, None, score, max_matches, radius)
        ops.ctx.synchronize()
        xy, sc, counts, ncand = xy.cpu().numpy(), sc.cpu().numpy(), counts.cpu().numpy(), ncand.cpu().numpy()
        assert xy.shape == (2, max_matches, 2) and sc.shape == (2, max_matches)
        for b in range(2):
            wxy, wsc, _, cand = _want_match(kind, b, score, max_matches, radius)
            assert ncand[b] == len(cand) and counts[b] == len(wxy) == min(max_matches, len(cand))
            assert np.array_equal(xy[b, :counts[b]], wxy), (b, max_matches)
            _same(sc[b, :counts[b]], wsc, "scores image %d maxMatches %d" % (b, max_matches))
            assert not xy[b, counts[b]:].any() and not sc[b, counts[b]:].any()
        if max_matches == 3:
            assert sorted(map(tuple, xy[0].tolist())) == [(10, 7), (70, 30), (120, 44)]


@pytest.mark.parametrize("kind", DTYPES)
@pytest.mark.parametrize("score", tr.SCORES)
def test_host_matcher(api, kind, score):
    cls = api.GrayU8 if kind == "u8" else api.GrayF32
    img, tpl = _match_scene(kind, 0)
    alg = api.FactoryTemplateMatching.createMatcher(score, cls)
    alg.setImage(cls.wrap(img))
    for max_matches, radius in ((1, 2), (3, 2), (5000, 2), (3, 6)):
        alg.setMinimumSeparation(radius)
        alg.setTemplate(cls.wrap(tpl), None, max_matches)
        alg.process()
        wxy, wsc, _, _ = _want_match(kind, 0, score, max_matches, radius)
        got = alg.getResults()
        assert [(m.x, m.y) for m in got] == [tuple(p) for p in wxy.tolist()]
        _same(np.array([m.score for m in got], np.float32), wsc, "scores")
    mask = np.ones(tpl.shape, tpl.dtype)
    alg.setTemplate(cls.wrap(tpl), cls.wrap(mask), 3)
    alg.process()
    assert sorted((m.x, m.y) for m in alg.getResults()) == [(10, 7), (70, 30), (120, 44)]


# ---- refusals: nothing is written ----
def test_refusals_leave_the_output_untouched(dev, api):
    ops, torch = dev
    W, H = 200, 30
    img = _t(dev, _image(W, H, "f32")).unsqueeze(0)
    parent, out = vl.make_view("pad4", 1, H, W, torch.float32, ops.device)
    before = vl.snapshot(parent)
    torch.cuda.synchronize()
    tpl = _t(dev, _template(5, 8, "f32"))
    with pytest.raises(RuntimeError, match="use the Java path") as e:
        ops.templateIntensity(img, tpl, None, tr.CORRELATION, out=out)
    assert not isinstance(e.value, api.IllegalArgumentException)
    with pytest.raises(RuntimeError, match="use the Java path") as e:   # wider than the limit
        ops.templateIntensity(img, _t(dev, _template(MAX_WIDTH + 1, 4, "f32")), None, tr.SAD, out=out)
    assert not isinstance(e.value, api.IllegalArgumentException)
    with pytest.raises(api.IllegalArgumentException):                   # larger than the image
        ops.templateIntensity(img, _t(dev, _template(5, H + 1, "f32")), None, tr.SAD, out=out)
    with pytest.raises(api.IllegalArgumentException):                   # a mask of another size
        ops.templateIntensity(img, tpl, _t(dev, _mask(5, 7, "f32")), tr.SSE, out=out)
    with pytest.raises(api.IllegalArgumentException):                   # types that differ
        ops.templateIntensity(img, _t(dev, _template(5, 8, "u8")), None, tr.SSE, out=out)
    with pytest.raises(api.IllegalArgumentException):
        ops.templateIntensity(img, tpl, None, "MUTUAL_INFORMATION", out=out)
    ops.ctx.synchronize()
    assert bool((vl.bits(parent) == before).all())
    # the host mirror: the same split
    alg = api.FactoryTemplateMatching.createIntensity(tr.SAD, api.GrayF32)
    alg.setInputImage(api.GrayF32(20, 10))
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayF32(21, 4))
    with pytest.raises(api.IllegalArgumentException):
        alg.process(api.GrayF32(5, 4), api.GrayF32(4, 4))
    alg.setInputImage(api.GrayF32(MAX_WIDTH + 40, 10))
    with pytest.raises(RuntimeError, match="use the Java path"):
        alg.process(api.GrayF32(MAX_WIDTH + 1, 4))
