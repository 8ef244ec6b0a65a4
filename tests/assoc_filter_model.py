"""CPU model (numpy only) of the fp16 filter of the greedy L2 association, boofcv_amd/csrc/assoc_mfma.hip.

The model restates k_assoc_norms, scaleExp, k_assoc_half and k_assoc_thresholds from the kernel's header and source, so that inputs
can be CONSTRUCTED at the filter's error bound.  It is not an oracle for results: tests compare the GPU with orc.associate_l2 only.

    raw norm     fl32(sum of squares in fp64) * fl32(1 + 4 * 2^-24)                    (k_assoc_norms: rounded up)
    q            (e + 1) >> 1 with frexp(max raw norm) = (m, e): max * 2^-2q in [1/4, 1)  (scaleExp)
    a^           fl16(fl32(2^-q a))                                                    (k_assoc_half)
    n = hi + lo  hi = fl16(n), lo = fl16(n - hi), n = raw norm * 2^-2q
    d~(i, j)     1 + (hi + lo)_i + (hi + lo)_j - 2 <a^_i, b^_j>    fp16 products are exact; the model sums in float64
    band         fl32 arithmetic of k_assoc_thresholds: 2 (C16 (n + max n) + ABS16)

The matrix cores accumulate the 80 terms in fp32 in an order the model does not know.  The header bounds that by
2^-16 (1 + n_a + n_b + 2 |a'| |b'|); uncertainty() returns this term: the model's d~ and the hardware's differ by no more.

The adversarial builder (quad) works on the fp16 grid just above a power of two, a0_k = s_k 2^-3 (1 + g_k 2^-10) with u = 2^-13 one fp16
ulp there.  Every power-of-two multiple of such a problem rounds the same way (until fp16 goes subnormal):
    "plus"  rows a0 + theta u s (theta = 0.49, 0.47) round to a0 and their norm is OVER-counted by about theta * 2u * sum |a0_k|,
    "minus" rows a0 - 0.49 u s + m u (m: a few whole ulps of alternating sign) round to a0 + m u, norm UNDER-counted by as much.
The kernel keeps ONE candidate list for both directions: the pair (i, j*) is listed when it is inside the band of row i OR inside the
band of column j*.  A row inversion alone can therefore not make a filter with a too small band lose (i, j*), the column rule lists it
as the minimum of its column.  So a quad plants both directions on the same pair:
    source i   = plus(0.49)     destination j* = plus(0.47)     exact d(i, j*) tiny, d~(i, j*) - 1 about +2E
    source i2  = minus(m2)      destination j' = minus(m1)      exact d(i, j'), d(i2, j*) larger, d~ - 1 about their exact value
Row i sees j' below j* and column j* sees i2 below i, both by 2E minus the exact gap: about 0.44 of the band.
"""
import numpy as np

C16 = np.float32(1.03e-3)
ABS16 = np.float32(2.0e-5)
ROUND_UP = np.float32(1.0) + np.float32(4.0) * np.float32(2.0 ** -24)
DOF = 64
U = 2.0 ** -13          # one fp16 ulp in [2^-3, 2^-2)


def norm_sums(D):
    """fp64 sum of squares in the kernel's order: 16 lanes with (x0^2 + x1^2) + (x2^2 + x3^2) each, then xor-butterfly 8, 4, 2, 1."""
    sq = np.ascontiguousarray(D, np.float64).reshape(-1, 16, 4) ** 2
    s = (sq[:, :, 0] + sq[:, :, 1]) + (sq[:, :, 2] + sq[:, :, 3])
    lanes = np.arange(16)
    for o in (8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def raw_norms(D):
    """k_assoc_norms: fp32 norms rounded up by (1 + 4 * 2^-24) -> float32[rows]"""
    with np.errstate(over="ignore"):
        return norm_sums(D).astype(np.float32) * ROUND_UP


def degenerate(*sets):
    """k_assoc_norms raises the 'use the exact path' flag: a sum of squares that is not below 1e30 (NaN and Inf included)"""
    return any(bool(np.any(~(norm_sums(D) < 1e30))) for D in sets)


def scale_exp(maxN):
    """scaleExp: q with maxN * 2^-2q in [1/4, 1); 0 when there is no positive norm"""
    maxN = np.float32(maxN)
    if not maxN > 0:
        return 0
    _, e = np.frexp(maxN)
    return (int(e) + 1) >> 1      # arithmetic shift: floor for negative e + 1, like the kernel's int shift


class Side:
    """One descriptor set after k_assoc_half: h = a^ (as float64), n = scaled fp32 norm, hl = hi + lo (float64)."""

    def __init__(self, D, raw, q):
        D = np.ascontiguousarray(D, np.float64).reshape(-1, DOF)
        self.h = np.ldexp(D, -q).astype(np.float32).astype(np.float16).astype(np.float64)
        self.n = np.ldexp(raw, -2 * q)
        assert self.n.dtype == np.float32
        hi = self.n.astype(np.float16)
        lo = (self.n - hi.astype(np.float32)).astype(np.float16)
        self.hl = hi.astype(np.float64) + lo.astype(np.float64)


class FilterModel:
    def __init__(self, src, dst, buffer=None):
        """buffer: every row the call's norm pass sees (a batched call takes q from the whole shared buffer)"""
        rawS, rawD = raw_norms(src), raw_norms(dst)
        self.maxRaw = np.float32(max(rawS.max(), rawD.max()) if buffer is None else raw_norms(buffer).max())
        self.q = scale_exp(self.maxRaw)
        self.maxN = np.ldexp(self.maxRaw, -2 * self.q)
        self.S, self.D = Side(src, rawS, self.q), Side(dst, rawD, self.q)
        self.src = np.ascontiguousarray(src, np.float64)
        self.dst = np.ascontiguousarray(dst, np.float64)

    def _band(self, n):
        band = np.float32(2.0) * (C16 * (n + self.maxN) + ABS16)
        assert band.dtype == np.float32
        return band

    def band_row(self, i):
        return float(self._band(self.S.n[i]))

    def band_col(self, j):
        return float(self._band(self.D.n[j]))

    def d_tilde(self, i, j):
        return 1.0 + self.S.hl[i] + self.D.hl[j] - 2.0 * float(np.dot(self.S.h[i], self.D.h[j]))

    def d_tilde_all(self):
        return 1.0 + self.S.hl[:, None] + self.D.hl[None, :] - 2.0 * (self.S.h @ self.D.h.T)

    def uncertainty(self, i, j):
        na, nb = float(self.S.n[i]), float(self.D.n[j])
        return 2.0 ** -16 * (1.0 + na + nb + 2.0 * np.sqrt(na * nb))

    def eps(self, i, j):
        """the header's bound on |d~ - 1 - d'|"""
        return float(C16) * (float(self.S.n[i]) + float(self.D.n[j])) + float(ABS16)

    def exact(self, i, j):
        return exact_l2(self.src[i], self.dst[j])

    def exact_scaled(self, i, j):
        return float(np.ldexp(self.exact(i, j), -2 * self.q))


def exact_l2(a, b):
    """DescriptorDistance.euclideanSq in the reference's loop order, plain Python floats"""
    total = 0.0
    for x, y in zip(a.tolist(), b.tolist()):
        d = x - y
        total += d * d
    return total


# ---------------------------------------------------------------------------------------------------------------- adversarial builder
M_ULPS = 2          # whole ulps of the minus rows
G_LO, G_HI = M_ULPS + 1, 8   # a0 - 0.49 u - M_ULPS u stays inside the binade [2^-3, 2^-2)


def quad(rng, active=DOF):
    """-> (src_i, src_i2, dst_jstar, dst_jprime) of one planted pair; components active.. are zero (lowers the norm below 1)."""
    s = rng.choice([-1.0, 1.0], DOF)
    g = rng.integers(G_LO, G_HI + 1, DOF)
    s[active:] = 0.0
    a0 = s * 2.0 ** -3 * (1.0 + g * 2.0 ** -10)
    m1, m2 = np.zeros(DOF), np.zeros(DOF)
    m1[0:8] = M_ULPS * (-1.0) ** np.arange(8)
    m2[8:16] = M_ULPS * (-1.0) ** np.arange(8)
    return (a0 + 0.49 * U * s, a0 - 0.49 * U * s + m2 * U, a0 + 0.47 * U * s, a0 - 0.49 * U * s + m1 * U)


def filler(rng, n):
    a = rng.normal(size=(n, DOF))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def build_problem(ns, nd, plants, seed, active=DOF):
    """Random rows of the quads' norm with one quad per entry (i, i2, jstar, jprime) of plants.  Random 64-vectors of norm 1 lie at a
    squared distance of about 2 from each other and from every planted row; the planted distances are below 1e-5."""
    rng = np.random.default_rng(seed)
    norm = np.sqrt(active / DOF)
    src, dst = norm * filler(rng, ns), norm * filler(rng, nd)
    rows = [r for p in plants for r in p[:2]]
    cols = [c for p in plants for c in p[2:]]
    assert len(set(rows)) == len(rows) and len(set(cols)) == len(cols), "planted rows / columns collide"
    assert 0 <= min(rows) and max(rows) < ns and 0 <= min(cols) and max(cols) < nd
    for i, i2, js, jp in plants:
        src[i], src[i2], dst[js], dst[jp] = quad(rng, active)
    return src, dst


def with_norm_leader(src, target):
    """Appends a source row c * e_63 whose raw (rounded-up fp32) norm is exactly `target`: the row q is taken from."""
    target = np.float32(target)
    row = np.zeros((1, DOF))
    # fl32(x^2) * (1 + 2^-22) == target: walk fl32(x^2) down from target until the rounded-up value matches
    n = target
    for _ in range(16):
        if n * ROUND_UP == target:
            break
        n = np.nextafter(n, np.float32(0))
    row[0, 63] = np.sqrt(float(n))
    out = np.concatenate([src, row])
    assert raw_norms(row)[0] == target, (raw_norms(row)[0], target)
    return out


def check_planted(model, i, i2, js, jp):
    """The conditions that make a planted pair a test of the band, row direction (i; j*, j') and column direction (j*; i, i2).
    Returns the two inversion-to-band ratios."""
    ratios = []
    for true, comp, band in (((i, js), (i, jp), model.band_row(i)), ((i, js), (i2, js), model.band_col(js))):
        # 1. exact fp64, reference loop order: the true match is strictly closer
        assert model.exact(*true) < model.exact(*comp)
        # 2. the filter sees it the other way round, by at least 0.35 of the band
        inv = model.d_tilde(*true) - model.d_tilde(*comp)
        assert inv >= 0.35 * band, (inv / band, true, comp)
        # 3. what the model does not know about the hardware's fp32 accumulation is small against that
        for pr in (true, comp):
            assert model.uncertainty(*pr) <= 0.05 * band
        # 4. the documented bound holds for both pairs: a correct filter must list the true match
        for pr in (true, comp):
            assert abs(model.d_tilde(*pr) - 1.0 - model.exact_scaled(*pr)) <= model.eps(*pr), pr
        ratios.append(inv / band)
    return ratios


# ---------------------------------------------------------------------------------------------------------------- the GPU file's problems
SRC_ROWS = (0, 31, 32, 63, 64, 255, 256)      # and ns - 1: wave-tile, half-tile and row-chunk edges
NS = 600                                      # a single problem walks its rows in chunks of 256: 256 + 256 + 88
DECOY_ROWS = (130, 200, 300, 390, 450, 500, 520, 580)   # the i2 of each quad, spread over other wave tiles and chunks

# (j*, j') per destination size.  Columns sit in tiles of 32, a step sweeps two tiles, a strip holds 384 columns.
COLUMNS = {
    # 384 + 33: a second strip of two tiles (32 + 1 columns)
    417: [(5, 9), (31, 32), (63, 64), (383, 384), (200, 416), (127, 128), (400, 390), (415, 10)],
    # 384 + 1: a strip of one column; its only step has no second tile
    385: [(5, 9), (31, 32), (63, 64), (383, 384), (200, 100), (127, 128), (300, 301), (0, 382)],
    # 384 + 65: a second strip of THREE tiles (32 + 32 + 1), the step after a full one has no second tile
    449: [(5, 9), (31, 32), (63, 64), (383, 384), (200, 448), (446, 447), (415, 416), (440, 10)],
}


def row_problem(nd, active=DOF):
    """Test (a): one quad per source row of SRC_ROWS + (ns - 1), each with another column geometry."""
    rows = SRC_ROWS + (NS - 1,)
    plants = [(i, i2, js, jp) for i, i2, (js, jp) in zip(rows, DECOY_ROWS, COLUMNS[nd])]
    return build_problem(NS, nd, plants, 1000 + nd, active), plants


# Test (b): the two source rows (i, i2) of column j* in different wave tiles of one chunk, then in different row chunks
COL_PLANTS = [(10, 70, 20, 300), (100, 191, 384, 2), (192, 5, 416, 100), (20, 300, 64, 65), (599, 255, 383, 200), (256, 31, 31, 400),
              (511, 512, 0, 1)]


def col_problem():
    return build_problem(NS, 417, COL_PLANTS, 2000), COL_PLANTS


SCALES = (-40, -7, -1, 0, 1, 8, 21, 40)
SCALE_FALLBACK = 50      # 2^100 > 1e30: the norms kernel sends the call to the exact path


def q_boundary_problem(below):
    """The row q is taken from has a raw norm of exactly 1 = 4^0 (q = 1, scaled maximum 1/4), or one fp32 ulp below it (q = 0, scaled
    maximum just under 1).  The quads use 63 components so that their norms (about 0.99) stay below the leader's."""
    (src, dst), plants = row_problem(417, active=63)
    target = np.nextafter(np.float32(1.0), np.float32(0)) if below else np.float32(1.0)
    return (with_norm_leader(src, target), dst), plants


def subnormal_problem(shift):
    """The quads and fillers of row_problem(417) at 2^-shift of the norm of one source and one destination row: after the common scaling
    their components (about 2^-4 * 2^-shift) are fp16 subnormals, multiples of 2^-24."""
    (src, dst), plants = row_problem(417)
    src, dst = np.ldexp(src, -shift), np.ldexp(dst, -shift)
    rng = np.random.default_rng(4000 + shift)
    src[400], dst[250] = filler(rng, 2)          # neither is a planted row
    return (src, dst), plants


# Test (f): 19 problems in one buffer.  nd of 1 (a strip of one column), 385 (one more column than a strip) and 800 (three strips); the
# block counts per problem differ, so the per-XCD queues (problem index mod 8) get padding entries
BATCH_NS = (300, 1, 64, 129, 257, 33, 5, 200, 65, 17, 256, 31, 100, 2, 90, 63, 128, 40, 77)
BATCH_ND = (417, 1, 385, 800, 50, 64, 7, 383, 33, 1, 96, 200, 384, 3, 65, 500, 32, 10, 129)
BATCH_GAP = 3                                    # rows between the segments that belong to no problem
BATCH_PLANTS = [(255, 256, 383, 384)]            # in problem 0


def batched_problem():
    """-> (rows of the shared buffer, srcOff, dstOff): segment order src 0, dst 0, src 1, ... with BATCH_GAP random rows in between"""
    rng = np.random.default_rng(3000)
    parts, src_off, dst_off, at = [], [], [], 0
    for p, (ns, nd) in enumerate(zip(BATCH_NS, BATCH_ND)):
        if p == 0:
            s, d = build_problem(ns, nd, BATCH_PLANTS, 3001)
        else:
            s, d = filler(rng, ns), filler(rng, nd)
            k = min(ns, nd) // 2
            d[:k] = s[:k] + rng.normal(scale=0.02, size=(k, DOF))
            d[:k] /= np.linalg.norm(d[:k], axis=1, keepdims=True)
        for seg, offs in ((s, src_off), (d, dst_off)):
            offs.append(at)
            parts += [seg, filler(rng, BATCH_GAP)]
            at += len(seg) + BATCH_GAP
    return np.concatenate(parts), np.array(src_off, np.int64), np.array(dst_off, np.int64)


def exact_matrix(src, dst):
    """every exact score, each summed over the components in the reference's order"""
    total = np.zeros((len(src), len(dst)))
    for k in range(DOF):
        d = src[:, k, None] - dst[None, :, k]
        total += d * d
    return total


def emulate_forward(model, band_scale=1.0):
    """Forward pairs (maxFitError unbounded) that the exact stages give from the MODEL's candidate list, the bands multiplied by
    band_scale: what a filter with another band factor would answer, up to the model's uncertainty."""
    dt = model.d_tilde_all()
    br = band_scale * model._band(model.S.n).astype(np.float64)
    bc = band_scale * model._band(model.D.n).astype(np.float64)
    listed = (dt <= dt.min(axis=1, keepdims=True) + br[:, None]) | (dt <= dt.min(axis=0, keepdims=True) + bc[None, :])
    score = np.where(listed, exact_matrix(model.src, model.dst), np.inf)
    best = score.min(axis=1, keepdims=True)
    nd = score.shape[1]
    return (nd - 1 - np.argmax((score == best)[:, ::-1], axis=1)).astype(np.int32)      # largest index among the exact ties
