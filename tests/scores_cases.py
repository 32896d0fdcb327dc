"""Inputs shared by tests/test_scores_cases_host.py and tests/test_gpu_scores_layout.py: rows with planted duplicates in
several memory layouts, the np.longdouble reference of mused_row_sq_norms / mused_pairwise_scores, the rounding bands, and a
NumPy emulation of the two summation orders a row norm can take.

What the device promises and these cases test:
  * a row's norm, and with it every score, is a function of the row's VALUES, d and the dtype: not of the pitch, not of the
    address.  Duplicate rows then have bit-identical norms and scores, and the selection breaks their tie by column.
  * norms within (d + 8) 2^-52 of the exact value (relative); squared-L2 scores within (d + 8) 2^-52 (|x|^2 + |y|^2), the
    one-evaluation bound of tests/test_dbscan_host.py; negated cosines within (d + 8) 2^-52 (absolute, the values lie in
    [-1, 1]): a dot product of d terms, two norms, two square roots, two reciprocals and two products.

N = 257 rows: two 128-row GEMM tiles and one row more.  Row ZERO_ROW is zero (the cosine normaliser).  PAIRS holds 8 pairs
(a, b), a < b, of identical rows.  b - a is odd for seven of them, so that with an odd pitch in doubles, or a pitch in floats
that is no multiple of four, the two rows of a pair start at different offsets inside a 16-byte line; the pairs (60, 189),
(100, 201) and (126, 255) lie in different GEMM tiles and straddle the rows in between.

The band decides no comparison but the planted ties (`ambiguity`): in exact arithmetic no row has two unrelated scores within
twice the band of its k-th smallest one.  Two degenerate rows are named and left out of that statement, not out of the device
test: every cosine at d = 1 is +-1, and every cosine of the zero row is 0."""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
N = 257
DS = (1, 3, 9, 33, 50, 130)
DTYPES = (np.float32, np.float64)
KS = (1, 7, 50)
METRICS = (0, 1)                      # METRIC_L2, METRIC_COSINE
ZERO_ROW = 5
PAIRS = ((10, 11), (20, 23), (33, 38), (40, 47), (60, 189), (100, 201), (126, 255), (130, 256))
LAYOUTS = ("tight", "pad3", "offset1", "aligned")
CASES = [(dt, d) for dt in DTYPES for d in DS]
IDS = [f"{np.dtype(dt).name}-d{d}" for dt, d in CASES]


def coefficient(d):
    return (d + 8) * EPS


@functools.lru_cache(maxsize=None)
def rows(dtype, d):
    """The N x d rows of a case (read-only)."""
    rng = np.random.default_rng([d, np.dtype(dtype).itemsize])
    X = rng.standard_normal((N, d)).astype(dtype)
    X[ZERO_ROW] = 0
    for a, b in PAIRS:
        X[b] = X[a]
    X.setflags(write=False)
    return X


def layout(X, name):
    """(flat buffer, element offset of row 0, pitch): the same values in another place.  Everything that is not a value is
    NaN.  With V = 16 / itemsize elements per 16-byte line:
      tight    ld = d
      pad3     ld = d + 3
      offset1  ld = the next multiple of V, row 0 one element into the buffer: no row starts on a line
      aligned  ld = the next multiple of V, row 0 at the buffer's start: every row starts on a line (the buffer itself is
               allocated on a line by the test)"""
    n, d = X.shape
    V = 16 // X.dtype.itemsize
    ldv = -(-d // V) * V
    off, ld = {"tight": (0, d), "pad3": (0, d + 3), "offset1": (1, ldv), "aligned": (0, ldv)}[name]
    buf = np.full(off + n * ld, np.nan, dtype=X.dtype)
    view = buf[off:off + n * ld].reshape(n, ld)
    view[:, :d] = X
    return buf, off, ld


def line_offsets(dtype, d, name):
    """Byte offset of every row's start inside its 16-byte line, for a buffer that starts on a line."""
    X = rows(dtype, d)
    _, off, ld = layout(X, name)
    return ((off + np.arange(N) * ld) * X.dtype.itemsize) % 16


# ---- the reference ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(dtype, d):
    """(norms[N], L2[N, N], cosine[N, N]) in longdouble from the rows converted to fp64: the device's expressions,
    max(0, |x|^2 - 2 x.y + |y|^2) and 0 - x.y / (|x| |y|) with zero norms replaced by 1."""
    X = np.asarray(rows(dtype, d), dtype=np.float64).astype(LD)
    nrm = (X * X).sum(axis=1)
    dot = X @ X.T
    l2 = np.maximum(nrm[:, None] - 2 * dot + nrm[None, :], LD(0))
    root = np.sqrt(nrm)
    inv = np.where(root == 0, LD(1), 1 / np.where(root == 0, LD(1), root))
    cos = LD(0) - dot * inv[:, None] * inv[None, :]
    for a in (nrm, l2, cos):
        a.setflags(write=False)
    return nrm, l2, cos


def bands(dtype, d):
    """(norm band[N], L2 band[N, N], cosine band): the largest |device - reference| the rounding analysis allows."""
    nrm = reference(dtype, d)[0]
    return coefficient(d) * nrm, coefficient(d) * (nrm[:, None] + nrm[None, :]), LD(coefficient(d))


def reference_scores(dtype, d, metric):
    return reference(dtype, d)[1 + metric]


def row_band(dtype, d, metric):
    """Per row the largest band of its scores."""
    if metric == 0:
        return bands(dtype, d)[1].max(axis=1)
    return np.full(N, bands(dtype, d)[2], dtype=LD)


def partner():
    p = np.arange(N)
    for a, b in PAIRS:
        p[a], p[b] = b, a
    return p


def degenerate(dtype, d, metric, i):
    """Rows whose scores tie by construction, in exact arithmetic: all of them under cosine at d = 1 (every score is +-1, or
    0 against the zero row), and the zero row under cosine (every score is 0)."""
    return metric == 1 and (d == 1 or i == ZERO_ROW)


def ambiguity(dtype, d, metric, k):
    """Rows (not degenerate) where a column that is neither the k-th smallest score's own nor its planted duplicate lies
    within twice the band of the k-th smallest score.  Empty: the band decides nothing but the planted ties."""
    S = reference_scores(dtype, d, metric)
    B = row_band(dtype, d, metric)
    p = partner()
    bad = []
    for i in range(N):
        if degenerate(dtype, d, metric, i):
            continue
        order = np.argsort(S[i], kind="stable")
        kth = order[k - 1]
        near = np.flatnonzero(np.abs(S[i] - S[i, kth]) <= 2 * B[i])
        if set(near.tolist()) - {int(kth), int(p[kth])}:
            bad.append(i)
    return bad


def check_topk(dtype, d, metric, k, idx):
    """idx (N x k, ascending columns) is a valid answer to "the k smallest scores of every row" for scores within the band
    of the reference: with t the k-th smallest reference score of a row and B the row's band, the k-th smallest device
    score lies within B of t (order statistics move by no more than the entries do), so every column below t - 2 B is
    selected and no column above t + 2 B is.  For a planted pair a < b equal scores go to the smaller column: b selected
    implies a selected, in every row."""
    S = reference_scores(dtype, d, metric)
    B = row_band(dtype, d, metric)
    idx = np.asarray(idx)
    assert idx.shape == (N, k) and idx.min() >= 0 and idx.max() < N
    assert k == 1 or (np.diff(idx, axis=1) > 0).all(), "columns not ascending / repeated"
    sel = np.zeros((N, N), dtype=bool)
    np.put_along_axis(sel, idx.astype(np.int64), True, axis=1)
    t = np.partition(S, k - 1, axis=1)[:, k - 1]
    must = S < (t - 2 * B)[:, None]
    may = S <= (t + 2 * B)[:, None]
    assert not (must & ~sel).any(), "a closer column was left out"
    assert not (sel & ~may).any(), "a farther column was taken"
    for a, b in PAIRS:
        assert not (sel[:, b] & ~sel[:, a]).any(), f"pair ({a}, {b}): the larger column was taken without the smaller"


# ---- the two summation orders of a row norm, emulated ------------------------------------------------------------------
def _wave_sum(lanes):
    """The butterfly of wave_sum (common.h): v += v[lane ^ o] for o = 32 .. 1; every lane ends with the same sum."""
    v = np.array(lanes, dtype=np.float64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ o]
    return v[0]


def norm_line_order(x):
    """Lane L sums the squares of columns L V .. L V + V - 1 (one 16-byte line, added up first) at stride 64 V, then the
    columns past the last whole line at stride 64: the order of the 16-byte loads.  fp64, no fused multiply-add."""
    x = np.asarray(x)
    V = 16 // x.dtype.itemsize
    x = x.astype(np.float64)
    d = len(x)
    s = np.zeros(64)
    for lane in range(64):
        c = lane * V
        while c + V <= d:
            t = x[c] * x[c]
            for e in range(1, V):
                t = t + x[c + e] * x[c + e]
            s[lane] = s[lane] + t
            c += 64 * V
        for t in range((d // V) * V + lane, d, 64):
            s[lane] = s[lane] + x[t] * x[t]
    return _wave_sum(s)


def norm_column_order(x):
    """Lane L sums the squares of columns L, L + 64, ...: the order of element-wise loads."""
    x = np.asarray(x).astype(np.float64)
    s = np.zeros(64)
    for lane in range(64):
        for t in range(lane, len(x), 64):
            s[lane] = s[lane] + x[t] * x[t]
    return _wave_sum(s)


def address_dependent_norms(dtype, d, name):
    """Norms of a device that takes the line order for rows that start on a 16-byte line and the column order for the
    others, in layout `name`: the defect the layout test exists to catch."""
    X = rows(dtype, d)
    off = line_offsets(dtype, d, name)
    return np.array([norm_line_order(X[i]) if off[i] == 0 else norm_column_order(X[i]) for i in range(N)])
