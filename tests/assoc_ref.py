"""Plain NumPy model of the greedy association (no GPU, no oracle), and the tie-dense inputs of tests/test_gpu_assoc_hamming.py.

  hamming_scores   DescriptorDistance.hamming      F:alg/descriptor/DescriptorDistance.java:196-220   the whole [ns, nd] score matrix
  greedy           AssociateGreedy.associate       F:alg/feature/associate/AssociateGreedy.java:65-118 on any score matrix
  column_top2      the (min1, min2, argmin1) record per destination column that a rank of the sharded association contributes
  tie_dense        descriptors whose score matrix is full of equal row and column minima, far apart in index, next to unique best pairs
  tie_stats        how many of them there are (tests/test_assoc_reference.py asserts the shares, so the GPU tests cannot pass vacuously)

The reference keeps the score matrix and applies three rules to it: per row the LAST index among equal minima (`fit <= best`), an
inclusive threshold (`score <= maxFitError`), and with backwards validation a match (i -> m) is dropped as soon as any other row is
at or below it in column m.  The device code never stores the matrix, so these rules live in key encodings and merge steps there."""
import numpy as np

MAX_VALUE = 1.7976931348623157e308   # Double.MAX_VALUE


def hamming_scores(src, dst):
    """int32 [ns, nd]: popcount(src[i] xor dst[j]) over the int32 words taken as 32 raw bits each."""
    a = np.ascontiguousarray(src, dtype=np.int32).view(np.uint32)
    b = np.ascontiguousarray(dst, dtype=np.int32).view(np.uint32)
    ns, nd = len(a), len(b)
    W = np.zeros((ns, nd), dtype=np.int32)
    if ns == 0 or nd == 0:
        return W
    assert a.shape[1] == b.shape[1]
    for k in range(a.shape[1]):          # one word at a time: the temporary stays [ns, nd]
        W += np.bitwise_count(a[:, k, None] ^ b[None, :, k])
    return W


def greedy(W, maxErr=MAX_VALUE, backwards=True):
    """(pairs int32[ns], fit float64[ns]) of AssociateGreedy on the score matrix W [ns, nd]."""
    W = np.asarray(W)
    ns, nd = W.shape
    pairs = np.full(ns, -1, dtype=np.int32)
    fit = np.full(ns, float(maxErr), dtype=np.float64)
    if ns == 0 or nd == 0:
        return pairs, fit
    # forward: `fit <= bestScore` from bestScore = maxFitError -- the last index among the minima, kept iff minimum <= maxFitError
    last = nd - 1 - np.argmin(W[:, ::-1], axis=1)
    best = W[np.arange(ns), last].astype(np.float64)
    keep = best <= maxErr
    pairs[keep] = last[keep]
    fit[keep] = best[keep]
    if backwards:
        # (i -> m) is dropped iff some j != i has W[j, m] <= W[i, m]; the check reads the forward result of row i only
        for i in np.nonzero(keep)[0]:
            col = W[:, pairs[i]]
            if np.count_nonzero(col <= col[i]) > 1:      # row i itself counts once
                pairs[i] = -1
                fit[i] = MAX_VALUE
    return pairs, fit


def column_top2(W, src_begin=0):
    """(min1 float64[nd], min2 float64[nd], idx1 int32[nd]) over the rows of W, which are the global sources src_begin, src_begin + 1, ...
    min2 is the second smallest entry counted with multiplicity (== min1 when the minimum occurs twice), idx1 the smallest global source
    index that attains min1.  No rows: inf, inf, -1.  One row: min2 = inf."""
    W = np.asarray(W)
    c, nd = W.shape
    min1 = np.full(nd, np.inf); min2 = np.full(nd, np.inf); idx1 = np.full(nd, -1, dtype=np.int32)
    if c == 0 or nd == 0:
        return min1, min2, idx1
    first = np.argmin(W, axis=0)                         # the first occurrence
    min1[:] = W[first, np.arange(nd)]
    idx1[:] = src_begin + first
    if c >= 2:
        min2[:] = np.partition(W, 1, axis=0)[1]
    return min1, min2, idx1


CODEBOOK = 24    # distinct code words (fewer for small sets, see tie_dense)
FLIP_BITS = 6    # bit positions a row may differ from its code word in
FLIP_P = 0.25


def _random_words(rng, n, words):
    return rng.integers(-2**31, 2**31, size=(n, words), dtype=np.int64).astype(np.int32)


def tie_dense(rng, ns, nd, words=16):
    """(src int32[ns, words], dst int32[nd, words]).

    Every row is one of up to CODEBOOK random code words with each of FLIP_BITS fixed bit positions flipped with probability FLIP_P: two rows
    of the same code word are 0..FLIP_BITS bits apart, so a row's minimum takes a handful of values and is attained by many destinations
    spread over the whole index range, and the same holds down the columns.  Then min(ns, nd) // 3 randomly placed sources are replaced
    by full-entropy rows and as many randomly placed destinations by copies of them, half of the copies with one bit flipped: unique
    mutual-best pairs, which survive the backward check."""
    nbook = max(2, min(CODEBOOK, min(ns, nd) // 8))      # small sets keep about eight rows per code word, so they tie as well
    book = _random_words(rng, nbook, words)
    pos = rng.choice(32 * words, size=min(FLIP_BITS, 32 * words), replace=False)

    def rows(n):
        out = book[rng.integers(0, nbook, size=n)].view(np.uint32).copy()
        for p in pos:
            flip = rng.random(n) < FLIP_P
            out[flip, p // 32] ^= np.uint32(1 << (p % 32))
        return out.view(np.int32)

    src, dst = rows(ns), rows(nd)
    k = min(ns, nd) // 3
    if k:
        si = rng.choice(ns, size=k, replace=False)
        di = rng.choice(nd, size=k, replace=False)
        uniq = _random_words(rng, k, words)
        src[si] = uniq
        twin = uniq.view(np.uint32).copy()
        bit = rng.integers(0, 32 * words, size=k)
        half = np.arange(k) % 2 == 1
        twin[half, bit[half] // 32] ^= (np.uint32(1) << (bit[half] % 32).astype(np.uint32))
        dst[di] = twin.view(np.int32)
    return np.ascontiguousarray(src), np.ascontiguousarray(dst)


def tie_stats(W):
    """Shares of ties in the score matrix W [ns, nd] (both sizes > 0), maxFitError = Double.MAX_VALUE:
      tied_rows      rows whose minimum is attained more than once                        / ns
      tied_cols      columns whose minimum is attained more than once                     / nd
      median_span    median over the tied rows of (last - first index among the row's minima)
      survivors      matches left with backwards validation (a count)
      killed         forward matches the backward check removes (a count)"""
    W = np.asarray(W)
    ns, nd = W.shape
    at_row_min = W == W.min(axis=1, keepdims=True)
    at_col_min = W == W.min(axis=0, keepdims=True)
    tied_r = at_row_min.sum(axis=1) > 1
    tied_c = at_col_min.sum(axis=0) > 1
    first = np.argmax(at_row_min, axis=1)
    last = nd - 1 - np.argmax(at_row_min[:, ::-1], axis=1)
    span = (last - first)[tied_r]
    fwd, _ = greedy(W, MAX_VALUE, False)
    bwd, _ = greedy(W, MAX_VALUE, True)
    return dict(tied_rows=float(tied_r.mean()), tied_cols=float(tied_c.mean()),
                median_span=float(np.median(span)) if len(span) else 0.0,
                survivors=int((bwd >= 0).sum()), killed=int(((fwd >= 0) & (bwd < 0)).sum()))


# ---- the cases shared by tests/test_assoc_reference.py (CPU) and tests/test_gpu_assoc_hamming.py ----
# 16 words.  What each shape reaches in the tiling of the matrix-core kernel is listed in tests/test_gpu_assoc_hamming.py.
SHAPES_16 = [(1, 1), (1, 33), (33, 1), (31, 32), (32, 33), (129, 97), (4096, 1100), (1100, 4096)]
LARGE_16 = [(4096, 1100), (1100, 4096)]
SHAPES_OTHER = [(300, 200, 1), (300, 200, 5), (300, 200, 17), (65, 129, 1), (65, 129, 5), (65, 129, 17)]   # (ns, nd, words)
SHAPES_SHARDED = [(1100, 700), (5, 40)]

_cases = {}


def case(ns, nd, words=16):
    """(src, dst, W) of the tie-dense problem of this shape: fixed seed, computed once per process, read-only."""
    key = (ns, nd, words)
    if key not in _cases:
        src, dst = tie_dense(np.random.default_rng(1000003 * ns + 1009 * nd + words), ns, nd, words)
        W = hamming_scores(src, dst)
        for a in (src, dst, W):
            a.setflags(write=False)
        _cases[key] = (src, dst, W)
    return _cases[key]


def thresholds(W):
    """maxFitError values for a problem: no bound; the (lower) median row minimum m, which the inclusive bound admits; m - 0.5, which
    shuts the rows at m out; 0 (exact copies only); a negative bound (nothing); and m + 1, because on the large shapes m is 0 and a bound
    at a positive score, met by a second class of tied rows, would otherwise be missing."""
    m = float(np.sort(np.asarray(W).min(axis=1))[(W.shape[0] - 1) // 2])
    return [MAX_VALUE, m, m - 0.5, 0.0, -1.0, m + 1.0]
