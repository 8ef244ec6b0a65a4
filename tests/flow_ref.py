"""numpy float32 restatement of the reference's dense KLT optical flow (test reference, not product code; never imported by boofcv_amd/).

Written from the cited BoofCV sources (F: = main/boofcv-feature/src/main/java/boofcv/):
  FactoryDenseOpticalFlow.flowKlt          F:factory/flow/FactoryDenseOpticalFlow.java:61-82
  FlowKlt_to_DenseOpticalFlow.process      F:abst/flow/FlowKlt_to_DenseOpticalFlow.java:76-86
  DenseOpticalFlowKlt.process              F:alg/flow/DenseOpticalFlowKlt.java:62-131
  ImageFlow.D.markInvalid                  F:struct/flow/ImageFlow.java:126-139

track_all is klt_ref's KltTracker / PyramidKltTracker with the pixel as an array axis: arrays [N, (2r+1)^2], every sum the reference forms in a loop
one fp32 chain along the element axis (np.add.accumulate is sequential), iterations under a mask.  test_flow_reference.py checks it against
klt_ref.PyramidKltTracker run pixel by pixel.  The records it returns are what the library's `tracks` output holds: fault (KltTrackFault ordinal,
THROWS where the reference throws, NO_DESCRIPTION where setDescription returned false), and error / flow where the track succeeded, 0 elsewhere.

assign_sequential is checkNeighbors as written, in raster order; assign_reduce is the same result per slot without the order (the argument is in
its docstring); classify says which rule decided each slot.
"""
import numpy as np

import klt_ref as kr
import klt_u8_ref as ku

F = np.float32
SUCCESS, DRIFTED, OUT_OF_BOUNDS, FAILED, LARGE_ERROR, THROWS, NO_DESCRIPTION = range(7)
MAGIC_ADJUSTMENT = F(0.7)
FLOAT_MAX = kr.FLOAT_MAX
OWN, LATER, EARLIER, INVALID, TIE = range(5)
CLASS_NAMES = ("own flow kept", "from a later pixel", "from an earlier pixel", "invalid", "equal-score rule")


def _chain(values, ok=None):
    """total = 0; for v in row: if ok: total += v   (fp32, in order; a skipped element adds +0, which leaves a sum that started at +0 unchanged)"""
    if ok is not None:
        values = np.where(ok, values, F(0))
    a = np.zeros((values.shape[0], values.shape[1] + 1), np.float32)
    a[:, 1:] = values
    return np.add.accumulate(a, axis=1)[:, -1]


# ---------------------------------------------------------------------------------------------------------------- BilinearRectangle_F32.region
def _region(img, tlx, tly, w, h, JJ, II):
    """element (JJ, II) of region(tl_x, tl_y, output of w x h) for every row n: img [H, W] float32, tlx / tly [N] float32, w / h [N] int,
    JJ / II [N, len] int -> (values [N, len], thrown [N]).  Elements outside [0, w) x [0, h) are garbage (never out-of-range reads)."""
    H, W = img.shape
    thrown = (tlx < 0) | (tly < 0) | (tlx + w.astype(np.float32) > F(W)) | (tly + h.astype(np.float32) > F(H)) | (w <= 0) | (h <= 0)
    xt = np.where(thrown | np.isnan(tlx), 0, np.nan_to_num(tlx, nan=0.0, posinf=0.0, neginf=0.0)).astype(np.int64)
    yt = np.where(thrown | np.isnan(tly), 0, np.nan_to_num(tly, nan=0.0, posinf=0.0, neginf=0.0)).astype(np.int64)
    thrown = thrown | (xt + w > W) | (yt + h > H)
    ax, ay = tlx - xt.astype(np.float32), tly - yt.astype(np.float32)
    bx, by = F(1.0) - ax, F(1.0) - ay
    a0, a1, a2, a3 = (bx * by)[:, None], (ax * by)[:, None], (ax * ay)[:, None], (bx * ay)[:, None]
    bR, bB = xt + w == W, yt + h == H
    regW, regH = np.where(bR, w - 1, w)[:, None], np.where(bB, h - 1, h)[:, None]
    bR, bB, xt, yt = bR[:, None], bB[:, None], xt[:, None], yt[:, None]
    ax, ay, bx, by = ax[:, None], ay[:, None], bx[:, None], by[:, None]

    def px(y, x):
        return img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]

    y, x = yt + II, xt + JJ
    inner = a0 * px(y, x) + a1 * px(y, x + 1) + a2 * px(y + 1, x + 1) + a3 * px(y + 1, x)
    right = by * px(y, x) + ay * px(y + 1, x)              # handleBorder: the right border column (x == xt + regW)
    corner = px(y, x)                                      # right and bottom
    bottom = bx * px(y, x) + ax * px(y, x + 1)             # the bottom border row
    odd = by * px(y, x) + ay * px(regH + 0 * y, x + 1)     # bottom only, last column: orig.get(xt+regWidth, regHeight), the row is regHeight
    out = np.where((JJ < regW) & (II < regH), inner,
                   np.where(II < regH, right,
                            np.where(JJ == regW, corner,
                                     np.where(~bR & (JJ == regW - 1), odd, bottom))))
    return out.astype(np.float32), thrown


def _bounds(r, W, H):
    return dict(aL=F(r), aT=F(r), aR=F(W - r - 1), aB=F(H - r - 1), oL=F(-r), oT=F(-r), oR=F(W + r - 1), oB=F(H + r - 1))


def _inside(b, x, y):
    return ~((x < b["aL"]) | (x > b["aR"])) & ~((y < b["aT"]) | (y > b["aB"]))


def _outside(b, x, y):
    return (x < b["oL"]) | (x > b["oR"]) | (y < b["oT"]) | (y > b["oB"])


def _sub_bounds(cx, cy, r, W, H):
    """KltTracker.computeSubImageBounds :421-457 -> (dx0, dy0, dx1, dy1, sx0, sy0, thrown)"""
    w = 2 * r + 1
    n = len(cx)
    dx0, dy0 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    dx1, dy1 = np.full(n, w, np.int64), np.full(n, w, np.int64)
    sx0, sy0 = cx - F(r), cy - F(r)
    sx1, sy1 = sx0 + F(w), sy0 + F(w)

    def ints(v):
        return np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)

    m = sx0 < 0
    dx0 = np.where(m, ints(-np.floor(sx0)), dx0)
    sx0 = np.where(m, sx0 + dx0.astype(np.float32), sx0).astype(np.float32)
    m = sx1 > F(W)
    dx1 = np.where(m, dx1 - ints(np.ceil(sx1 - F(W))), dx1)
    dx1 = np.where(m & (sx0 + (dx1 - dx0).astype(np.float32) > F(W)), dx1 - 1, dx1)
    m = sy0 < 0
    dy0 = np.where(m, ints(-np.floor(sy0)), dy0)
    sy0 = np.where(m, sy0 + dy0.astype(np.float32), sy0).astype(np.float32)
    m = sy1 > F(H)
    dy1 = np.where(m, dy1 - ints(np.ceil(sy1 - F(H))), dy1)
    dy1 = np.where(m & (sy0 + (dy1 - dy0).astype(np.float32) > F(H)), dy1 - 1, dy1)
    thrown = (sx0 < 0) | (sy0 < 0) | (sx0 + (dx1 - dx0).astype(np.float32) > F(W)) | (sy0 + (dy1 - dy0).astype(np.float32) > F(H))
    return dx0, dy0, dx1, dy1, sx0, sy0, thrown


def _patch(imgs, x, y, r, full):
    """the (2r+1)^2 patch at (x, y) of every image of `imgs`, by the inside form (region at (x-r, y-r)) where `full`, by the border form
    (computeSubImageBounds, NaN outside the visible box) elsewhere -> ([values [N, len] per image], inbox [N, len], thrown [N])"""
    H, W = imgs[0].shape
    w = 2 * r + 1
    e = np.arange(w * w)
    J, I = (e % w)[None, :], (e // w)[None, :]
    dx0, dy0, dx1, dy1, sx0, sy0, thrown = _sub_bounds(x, y, r, W, H)
    dx0, dy0 = np.where(full, 0, dx0), np.where(full, 0, dy0)
    dx1, dy1 = np.where(full, w, dx1), np.where(full, w, dy1)
    tlx = np.where(full, x - F(r), sx0).astype(np.float32)
    tly = np.where(full, y - F(r), sy0).astype(np.float32)
    thrown = thrown & ~full
    inbox = (J >= dx0[:, None]) & (J < dx1[:, None]) & (I >= dy0[:, None]) & (I < dy1[:, None])
    out = []
    for img in imgs:
        v, t = _region(img, tlx, tly, dx1 - dx0, dy1 - dy0, J - dx0[:, None], I - dy0[:, None])
        out.append(v)
        thrown = thrown | t
    return out, inbox, thrown


# ---------------------------------------------------------------------------------------------------------------- KltTracker, one layer, N pixels
def describe_layer(img, dX, dY, x, y, r, cfg):
    """KltTracker.setDescription :147-240 -> (ok [N]: 1 / 0 the reference's boolean, -1 it throws; D, X, Y [N, len]; Gxx, Gyy, Gxy [N])"""
    H, W = img.shape
    b = _bounds(r, W, H)
    inside = _inside(b, x, y)
    outside = ~inside & _outside(b, x, y)
    (d, gx, gy), inbox, thrown = _patch((img, dX, dY), x, y, r, inside)
    D = np.where(inbox, d, kr.NAN).astype(np.float32)
    X = np.where(inbox, gx, F(0)).astype(np.float32)   # the reference leaves derivX / derivY stale there and never reads them
    Y = np.where(inbox, gy, F(0)).astype(np.float32)
    ok = inside[:, None] | ~np.isnan(D)                # internalSetDescription sums every element, the border form skips NaN
    Gxx, Gyy, Gxy = _chain(X * X, ok), _chain(Y * Y, ok), _chain(X * Y, ok)
    det = Gxx * Gyy - Gxy * Gxy
    res = (det >= cfg.minDeterminant * ok.sum(1).astype(np.float32)).astype(np.int64)
    res = np.where(thrown, -1, res)
    res = np.where(outside, 0, res)
    return res, D, X, Y, Gxx, Gyy, Gxy


def track_layer(img, x, y, D, X, Y, Gxx, Gyy, Gxy, r, cfg, run):
    """KltTracker.track :251-325 for the pixels of `run` -> (fault [N], x, y, error [N], iterations [N]); rows outside `run` come back as they were"""
    H, W = img.shape
    w = 2 * r + 1
    n = w * w
    b = _bounds(r, W, H)
    x, y = x.copy(), y.copy()
    N = len(x)
    fault = np.full(N, -1, np.int64)    # -1: still iterating
    fault[~run] = -2                    # not ours
    error = np.zeros(N, np.float32)
    iters = np.zeros(N, np.int64)
    fault[run & _outside(b, x, y)] = OUT_OF_BOUNDS
    complete = ~np.isnan(D).any(1)
    Gxx, Gyy, Gxy = Gxx.copy(), Gyy.copy(), Gxy.copy()
    det = np.where(complete, Gxx * Gyy - Gxy * Gxy, F(0)).astype(np.float32)
    fault[(fault == -1) & complete & (det < cfg.minDeterminant * F(n))] = FAILED
    origX, origY = x.copy(), y.copy()
    errS, errC = np.zeros(N, np.float32), np.ones(N, np.int64)
    done = np.zeros(N, bool)            # left the loop by break or by running out of iterations
    for _ in range(cfg.maxIterations):
        act = (fault == -1) & ~done
        if not act.any():
            break
        iters[act] += 1
        inside = complete & _inside(b, x, y)            # computeE, else computeGandE_border
        (c,), inbox, thrown = _patch((img,), x, y, r, inside)
        c = np.where(inbox, c, kr.NAN).astype(np.float32)
        fault[act & thrown] = THROWS
        act = act & ~thrown
        d = D - c
        valid = ~(np.isnan(D) | np.isnan(c))
        okE = inside[:, None] | valid
        Ex, Ey = _chain(d * X, okE), _chain(d * Y, okE)
        bxx, byy, bxy = _chain(X * X, valid), _chain(Y * Y, valid), _chain(X * Y, valid)
        upd = act & ~inside
        Gxx, Gyy, Gxy = np.where(upd, bxx, Gxx), np.where(upd, byy, Gyy), np.where(upd, bxy, Gxy)
        det = np.where(upd, Gxx * Gyy - Gxy * Gxy, det).astype(np.float32)
        failed = upd & (det <= cfg.minDeterminant * valid.sum(1).astype(np.float32))
        fault[failed] = FAILED
        act = act & ~failed
        errS = np.where(act, _chain(np.abs(d), valid), errS)   # computeError :346-359 on this iteration's currDesc
        errC = np.where(act, valid.sum(1), errC)
        dx = (Gyy * Ex - Gxy * Ey) / det
        dy = (Gxx * Ey - Gxy * Ex) / det
        x = np.where(act, x + dx, x).astype(np.float32)
        y = np.where(act, y + dy, y).astype(np.float32)
        oob = act & _outside(b, x, y)
        fault[oob] = OUT_OF_BOUNDS
        act = act & ~oob
        drift = act & ((np.abs(x - origX) > F(w)) | (np.abs(y - origY) > F(w)))
        fault[drift] = DRIFTED
        act = act & ~drift
        done |= act & (np.abs(dx) < cfg.minPositionDelta) & (np.abs(dy) < cfg.minPositionDelta)
    fin = fault == -1
    e = errS / errC.astype(np.float32)
    error = np.where(fin, e, error).astype(np.float32)
    fault[fin & (e > cfg.maxPerPixelError)] = LARGE_ERROR
    fault[fault == -1] = SUCCESS
    return fault, x, y, error, iters


# ---------------------------------------------------------------------------------------------------------------- PyramidKltTracker at every pixel
def track_all(layers0, dx0, dy0, layers1, scales, radius, cfg=None):
    """For every pixel (x, y) of layer 0, in raster order: feature.setPosition(x, y), PyramidKltTracker.setDescription on (layers0, dx0, dy0)
    (:58-71), track on layers1 (:113-151) -> dict(fault int32, error, dx, dy float32, iterations int64), each [H, W]; flow = (feature.x - x, feature.y - y)"""
    cfg = cfg or kr.KltConfig()
    f32 = lambda a: np.ascontiguousarray(a, np.float32)   # GrayU8 / GrayS16 taps converted to float: exact (klt_u8_ref)
    layers0, dx0, dy0, layers1 = [[f32(a) for a in v] for v in (layers0, dx0, dy0, layers1)]
    H, W = layers0[0].shape
    L = len(layers0)
    fx0 = np.tile(np.arange(W, dtype=np.float32), H)
    fy0 = np.repeat(np.arange(H, dtype=np.float32), W)
    N = H * W
    fault = np.zeros(N, np.int64)
    alive = np.ones(N, bool)
    desc = []
    with np.errstate(all="ignore"):
        for l in range(L):
            scale = F(float(scales[l]))
            ok, D, X, Y, Gxx, Gyy, Gxy = describe_layer(layers0[l], dx0[l], dy0[l], fx0 / scale, fy0 / scale, radius, cfg)
            desc.append((D, X, Y, Gxx, Gyy, Gxy))
            fault[alive & (ok == 0)] = NO_DESCRIPTION
            fault[alive & (ok < 0)] = THROWS
            alive &= ok == 1
        x, y = fx0.copy(), fy0.copy()
        error = np.zeros(N, np.float32)
        iters = np.zeros(N, np.int64)
        for l in range(L - 1, -1, -1):
            scale = F(float(scales[l]))
            x, y = x / scale, y / scale
            f, lx, ly, e, it = track_layer(layers1[l], x, y, *desc[l], radius, cfg, alive)
            iters += it
            fault[alive] = f[alive]
            error = np.where(alive & (f != SUCCESS) | ~alive, error, e).astype(np.float32)
            alive = alive & (f == SUCCESS)
            x, y = np.where(alive, lx * scale, x).astype(np.float32), np.where(alive, ly * scale, y).astype(np.float32)
    ok = fault == SUCCESS
    z = F(0)
    return dict(fault=fault.astype(np.int32).reshape(H, W), error=np.where(ok, error, z).astype(np.float32).reshape(H, W),
                dx=np.where(ok, x - fx0, z).astype(np.float32).reshape(H, W), dy=np.where(ok, y - fy0, z).astype(np.float32).reshape(H, W),
                iterations=iters.reshape(H, W))


# ---------------------------------------------------------------------------------------------------------------- checkNeighbors
def _new_flow(H, W, flow):
    """every flow markInvalid(): x = NaN, y as it was (0 in a new ImageFlow)"""
    out = np.zeros((H, W, 2), np.float32) if flow is None else np.array(flow, np.float32)
    out[:, :, 0] = kr.NAN
    return out


def assign_sequential(rec, radius, flow=None, trace=None):
    """DenseOpticalFlowKlt.process :68-98 and checkNeighbors :105-131 as written, on the per-pixel records.  flow: what the caller's ImageFlow
    held (its y survives in invalid pixels).  trace: a dict that receives holder [H, W] (raster index of the pixel whose flow the slot holds,
    -1 none) and tie [H, W] (the slot's last replacement went through the equal-score branch)."""
    fault, error, dx, dy = rec["fault"], rec["error"], rec["dx"], rec["dy"]
    H, W = fault.shape
    scores = np.full((H, W), FLOAT_MAX, np.float32)
    out = _new_flow(H, W, flow)
    holder = np.full((H, W), -1, np.int64)
    tie = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if fault[y, x] != SUCCESS:
                    continue
                score, fx, fy = error[y, x], dx[y, x], dy[y, x]
                scores[y, x] = score * MAGIC_ADJUSTMENT
                out[y, x] = (fx, fy)
                holder[y, x], tie[y, x] = y * W + x, False
                for i in range(max(0, y - radius), min(H, y + radius + 1)):
                    for j in range(max(0, x - radius), min(W, x + radius + 1)):
                        s = scores[i, j]
                        if s > score:
                            out[i, j] = (fx, fy)
                            scores[i, j] = score
                            holder[i, j], tie[i, j] = y * W + x, False
                        elif s == score:
                            m0 = out[i, j, 0] * out[i, j, 0] + out[i, j, 1] * out[i, j, 1]
                            m1 = fx * fx + fy * fy
                            if m1 < m0:
                                out[i, j] = (fx, fy)
                                scores[i, j] = score
                                holder[i, j], tie[i, j] = y * W + x, True
    if trace is not None:
        trace["holder"], trace["tie"] = holder, tie
    return out


def assign_reduce(rec, radius, flow=None):
    """The same result slot by slot, with no order between slots.  Call q a success when its own track succeeded.  Slot p is written by the
    checkNeighbors of the successes of its clipped window, in raster order, and by p's own unconditional write (score_p * 0.7f, flow_p) at
    time p, which wipes whatever earlier pixels left there.  So the slot is the reference's fold -- replace when the held score is greater,
    or equal with a strictly greater motion -- started from (Float.MAX_VALUE, invalid) over: the own entry first and then the successes
    after p, when p succeeded (p's own checkNeighbors visit changes nothing: score_p * 0.7f <= score_p and a tie has equal motion); all
    successes of the window, when p failed."""
    fault, error, dx, dy = rec["fault"], rec["error"], rec["dx"], rec["dy"]
    H, W = fault.shape
    out = _new_flow(H, W, flow)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                own = fault[y, x] == SUCCESS
                bs, bx, by = FLOAT_MAX, out[y, x, 0], out[y, x, 1]
                for i in range(max(0, y - radius), min(H, y + radius + 1)):
                    for j in range(max(0, x - radius), min(W, x + radius + 1)):
                        if fault[i, j] != SUCCESS:
                            continue
                        if i == y and j == x:
                            bs, bx, by = error[i, j] * MAGIC_ADJUSTMENT, dx[i, j], dy[i, j]
                            continue
                        if own and (i, j) < (y, x):
                            continue
                        score = error[i, j]
                        take = bs > score
                        if not take and bs == score:
                            take = dx[i, j] * dx[i, j] + dy[i, j] * dy[i, j] < bx * bx + by * by
                        if take:
                            bs, bx, by = score, dx[i, j], dy[i, j]
                out[y, x] = (bx, by)
    return out


def classify(rec, radius):
    """-> [H, W] of OWN (own flow kept), LATER (taken from a later pixel), EARLIER (from an earlier pixel: the centre failed), INVALID, TIE (the
    slot's value was installed by the equal-score rule)"""
    trace = {}
    assign_sequential(rec, radius, trace=trace)
    holder, tie = trace["holder"], trace["tie"]
    H, W = holder.shape
    idx = np.arange(H * W).reshape(H, W)
    cls = np.where(holder < 0, INVALID, np.where(holder == idx, OWN, np.where(holder > idx, LATER, EARLIER)))
    return np.where(tie, TIE, cls)


def same_bits(a, b):
    """bit patterns equal, every NaN counting as one value"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------------------- test scene
def scene(W, H, seed, shift=(0.6, -0.4), angle=0.02, flat=None, occluder=None):
    """-> (src, dst) float32 [H, W] in 0..255: a smooth random texture; dst is src moved by the sub-pixel `shift` and turned by `angle` about
    the centre (bilinear samples of one larger texture).  flat = (x0, y0, w, h): a patch without texture in both frames (setDescription
    fails there); occluder = (x0, y0, w, h): a bright patch that only the second frame has (tracks into it fail)."""
    rng = np.random.RandomState(seed)
    m = 8
    t = rng.rand(H + 2 * m, W + 2 * m)
    for _ in range(2):
        t = (t + np.roll(t, 1, 0) + np.roll(t, 1, 1) + np.roll(np.roll(t, 1, 0), 1, 1)) / 4
    t = (t - t.min()) / (t.max() - t.min()) * 255

    def sample(xs, ys):
        x0, y0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
        ax, ay = xs - x0, ys - y0
        x0, y0 = np.clip(x0, 0, t.shape[1] - 2), np.clip(y0, 0, t.shape[0] - 2)
        return (1 - ax) * (1 - ay) * t[y0, x0] + ax * (1 - ay) * t[y0, x0 + 1] + ax * ay * t[y0 + 1, x0 + 1] + (1 - ax) * ay * t[y0 + 1, x0]

    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    c, s_ = np.cos(angle), np.sin(angle)
    src = sample(xs + m, ys + m)
    dst = sample(c * (xs - cx) - s_ * (ys - cy) + cx - shift[0] + m, s_ * (xs - cx) + c * (ys - cy) + cy - shift[1] + m)
    if flat:
        x0, y0, w, h = flat
        src[y0:y0 + h, x0:x0 + w] = 40
        dst[y0:y0 + h, x0:x0 + w] = 40
    if occluder:
        x0, y0, w, h = occluder
        dst[y0:y0 + h, x0:x0 + w] = 250
    return src.astype(np.float32), dst.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- FlowKlt_to_DenseOpticalFlow
def pyramids(orc, src, dst, scales, u8=False):
    """the two pyramids and the source gradient of FlowKlt_to_DenseOpticalFlow.process :76-86"""
    if u8:
        l0, gx, gy = ku.pyramid_gradient_u8(np.ascontiguousarray(src, np.uint8), scales)
        l1 = ku.pyramid_u8(np.ascontiguousarray(dst, np.uint8), scales)
    else:
        l0, gx, gy = kr.pyramid_gradient(orc, np.ascontiguousarray(src, np.float32), scales)
        l1, _ = orc.pyramid(orc.gaussian1d_f32(-1, 2), -1, scales, orc.Gray.from_array(np.ascontiguousarray(dst, np.float32)))
    return l0, gx, gy, l1


def dense_flow_klt(orc, src, dst, scales, radius, cfg=None, u8=False, flow=None):
    """DenseOpticalFlow.process(src, dst, flow) of flowKlt -> (flow [H, W, 2] float32, the per-pixel records)"""
    l0, gx, gy, l1 = pyramids(orc, src, dst, scales, u8)
    rec = track_all(l0, gx, gy, l1, scales, radius, cfg)
    return assign_reduce(rec, radius, flow), rec
