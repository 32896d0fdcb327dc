"""Shared inputs, scikit-learn references and error bounds of the silhouette / Davies-Bouldin / Calinski-Harabasz tests
(tests/test_silhouette_host.py, tests/test_gpu_silhouette.py, tests/test_gpu_internal_scores.py).

Inputs are small seeded Gaussian blobs: the smallest shapes at which the kernels of csrc/silhouette.hip can still go wrong
(n around the 128-row tile, an odd tile count, d around the 16-wide K step and beyond the 128 columns of a tile; clusters
aligned to a tile, straddling one, of one row each; labels of any int32 value, in shuffled row order; duplicated rows).

THE BOUND (never a constant: computed from each case's inputs).  u = 2^-52.

1. d2(i, j) = |x_i|^2 + |x_j|^2 - 2 x_i.x_j, evaluated in any order of its sums, and sum (x_i - x_j)^2 alike, lie within
   E_ij = (d + 8) u (|x_i|^2 + |x_j|^2) of the exact value (mused_amd/dbscan.py: tau_coefficient).
2. With D_ij the exact distance (np.longdouble, from sum (x - y)^2): where D_ij^2 >= 2 E_ij both evaluations are roots of
   numbers in [D^2 - E, D^2 + E], which differ by at most 2 E / (sqrt(D^2 + E) + sqrt(D^2 - E)) ~ 2 E / D; otherwise
   both are roots of numbers in [0, D^2 + E] clamped at 0, and sqrt(D^2 + E) - sqrt(max(0, D^2 - E)) <= sqrt(2 E)
   (its largest value, at D^2 = E).  delta_ij = 2 E_ij / D_ij or sqrt(2 E_ij).  The pair (i, i) is exactly 0 on both sides.
3. A cluster mean is a sum of m <= n such distances divided by m (or m - 1): the terms move it by at most max delta, the
   m - 1 additions in any order by at most m u max D.  Delta = max delta + n u max D.
4. s = (b - a) / max(a, b) with |da|, |db| <= Delta (b is a minimum of means: it moves by no more than they do): for a <= b,
   s = 1 - a / b and |ds| <= Delta / b + a Delta / b^2 <= 2 Delta / b, and likewise for a > b: 2 Delta / max(a, b) to first
   order.  The factor 4 covers the second-order terms and the oracle's own rounding: bound_i = 4 * 2 Delta / max(a_i, b_i).
   A row alone in its cluster is 0 on both sides.
5. The score's bound is the mean of the samples' bounds.

Davies-Bouldin.  A centroid coordinate is a sum of n_k values divided by n_k: whatever the order, the centroid is within
e_k = (n_k + 2) u r_k of the exact one, r_k = |(max_i |x_ij|)_j| over the cluster's rows.  A distance is 1-Lipschitz in
either end, so the mean distance s_k of a cluster's rows to its centroid moves by at most
ds_k = max_i delta(x_i, c_k) + e_k + n_k u max_i D(x_i, c_k) and a centroid distance M_kl by dM_kl = delta(c_k, c_l) + e_k + e_l
(delta as in 2., with E from the norms of the two ends; it covers the expansion scikit-learn evaluates and the differences the
kernel evaluates).  R_kl = (s_k + s_l) / M_kl moves by (ds_k + ds_l) / M_kl + R_kl dM_kl / M_kl to first order; the score is
the mean over k of the maximum over l, which moves by no more than its terms: bound = 4 mean_k max_l of that, the 4 as above.

Calinski-Harabasz = (B / (C - 1)) / (W / (n - C)), W = sum_i |x_i - c_k(i)|^2 (n d terms), B = sum_k n_k |c_k - m|^2 (C d
terms).  Each term (difference, square) carries 3 u, the additions in any order (terms) u: (n d + 4) u W and (C d + 4) u B.
The centroids' errors e_k and the mean's e = (n + 4) u r add sum_k (2 e_k sum_{i in k} |x_i - c_k| + n_k e_k^2) to W's bound
and sum_k n_k (2 |c_k - m| (e_k + e) + (e_k + e)^2) to B's.  The quotient's relative bound is the sum of the two relative
bounds, twice (two evaluations), plus 8 u for the final products and quotients.  W == 0 exactly (integer-valued rows whose
sums are exact in any order): 1.0 on both sides, bound 0.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -52
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


class Case:
    def __init__(self, name, X, labels, ld=None, dup=False):
        self.name = name
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.n, self.d = self.X.shape
        self.ld = int(ld) if ld is not None else self.d
        self.dup = dup    # holds duplicated rows: the sqrt(2 E) branch of the bound, which is not below 1e-8

    def __repr__(self):
        return self.name


def blobs(sizes, d, seed, values=None, shuffle=True, spread=6.0):
    """Gaussian blobs of the given sizes around centres drawn from N(0, spread^2); label values `values` (default 0, 1, ...)."""
    rng = np.random.default_rng(seed)
    C = len(sizes)
    centres = rng.normal(0.0, spread, size=(C, d))
    X = np.concatenate([centres[c] + rng.normal(size=(m, d)) for c, m in enumerate(sizes)])
    vals = np.arange(C) if values is None else np.asarray(values, dtype=np.int64)
    labels = np.concatenate([np.full(m, vals[c], dtype=np.int64) for c, m in enumerate(sizes)])
    if shuffle:
        p = rng.permutation(len(X))
        X, labels = X[p], labels[p]
    return X, labels.astype(np.int32)


def _cases():
    out = []

    def add(name, sizes, d, seed, **kw):
        extra = {k: kw.pop(k) for k in ("ld", "dup") if k in kw}
        X, lab = blobs(sizes, d, seed, **kw)
        out.append(Case(name, X, lab, **extra))
        return out[-1]

    add("n3_d2_pair_and_single", [2, 1], 2, 1)
    # d = 1: Gaussian draws of 127 numbers come within 1e-4 of each other, which the bound (2 E / D) does not take below 1e-8;
    # a jittered lattice per cluster keeps every gap above 0.025
    rng = np.random.default_rng(2)
    X = np.concatenate([c + 0.05 * (np.arange(m) + 0.5 * rng.uniform(size=m)) for c, m in ((-6.0, 60), (3.0, 67))])[:, None]
    p = rng.permutation(127)
    out.append(Case("n127_d1_two_clusters", X[p], np.repeat([0, 1], [60, 67])[p]))
    add("n128_d15", [50, 40, 38], 15, 3)
    add("n129_d16", [43, 43, 43], 16, 4)
    add("n257_d17_straddle", [100, 100, 57], 17, 5)            # clusters across both tile boundaries, 3 tiles
    add("n384_d50_aligned", [128, 128, 128], 50, 6)            # every cluster exactly one tile
    add("n1000_d129", [300, 250, 200, 150, 100], 129, 7)
    add("n1000_d2", [400, 350, 250], 2, 8)
    add("n200_d15_ld19", [90, 110], 15, 9, ld=19)              # ld > d (odd: no 16-byte loads from the caller's rows)
    add("singletons", [1, 1, 60, 1, 70], 8, 10)
    add("n130_129_labels", [2] + [1] * 128, 4, 11)             # every tile full of one- and two-row clusters
    add("any_int32_labels", [30, 20, 25, 27, 25], 16, 12, values=[-1, 0, 5, I32_MAX, I32_MIN])
    add("rows_already_sorted", [70, 80], 5, 13, shuffle=False)

    X, lab = blobs([75, 75], 8, 14)
    i0, i1 = np.flatnonzero(lab == 0)[:3], np.flatnonzero(lab == 1)[:1]
    X[i1[0]] = X[i0[0]]    # bit-equal rows in different clusters
    X[i0[2]] = X[i0[1]]    # bit-equal rows in the same cluster
    out.append(Case("duplicates_across_and_within", X, lab, dup=True))

    X, lab = blobs([40, 60], 6, 15)
    X[lab == 0] = X[np.flatnonzero(lab == 0)[0]]               # a cluster of identical rows beside a distinct one
    out.append(Case("identical_cluster", X, lab, dup=True))

    # integer-valued rows, two clusters of identical rows, sizes powers of two: every sum is exact in any order, so the
    # within-cluster dispersion is exactly 0 (Calinski-Harabasz 1.0) and every mean distance is 0 (Davies-Bouldin 0.0)
    rng = np.random.default_rng(16)
    rows = rng.integers(-3, 4, size=(2, 6)).astype(np.float64)
    rows[1, 0] = rows[0, 0] + 2.0
    lab = rng.permutation(np.repeat([0, 1], [32, 64])).astype(np.int32)
    out.append(Case("all_identical_integers", rows[lab], lab, dup=True))
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def error_cases():
    """(name, X, labels, scikit-learn's message)."""
    X, lab = blobs([10, 10], 3, 20)
    Xn, Xi = X.copy(), X.copy()
    Xn[7, 1] = np.nan
    Xi[3, 2] = np.inf
    return [
        ("one_label", X, np.zeros(20, dtype=np.int32), "Number of labels is 1. Valid values are 2 to n_samples - 1 (inclusive)"),
        ("n_labels", X, np.arange(20, dtype=np.int32), "Number of labels is 20. Valid values are 2 to n_samples - 1 (inclusive)"),
        ("nan_row", Xn, lab, "Input X contains NaN."),
        ("inf_row", Xi, lab, "Input X contains infinity or a value too large for dtype('float64')."),
    ]


def four_blobs():
    """The selector's input: 4 well-separated blobs, n = 400, d = 8."""
    X, lab = blobs([100, 100, 100, 100], 8, 30, spread=10.0)
    return X, lab


@functools.lru_cache(maxsize=None)
def reference(name):
    """scikit-learn's (silhouette_samples, davies_bouldin_score, calinski_harabasz_score) of a case, computed once."""
    from sklearn import metrics as skm

    c = next(c for c in CASES if c.name == name)
    s = skm.silhouette_samples(c.X, c.labels, metric="euclidean")
    s.setflags(write=False)
    return s, float(skm.davies_bouldin_score(c.X, c.labels)), float(skm.calinski_harabasz_score(c.X, c.labels))


def _exact_d2(A, B):
    """sum (a - b)^2 in np.longdouble, (len(A), len(B)), one coordinate at a time."""
    A, B = np.asarray(A, dtype=np.longdouble), np.asarray(B, dtype=np.longdouble)
    out = np.zeros((len(A), len(B)), dtype=np.longdouble)
    for k in range(A.shape[1]):
        df = A[:, k][:, None] - B[:, k][None, :]
        out += df * df
    return out


def _delta(D2, E):
    """Step 2 of the bound, elementwise (float64)."""
    D2, E = np.asarray(D2, dtype=np.float64), np.asarray(E, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(D2 >= 2.0 * E, 2.0 * E / np.sqrt(D2), np.sqrt(2.0 * E))


def sample_bounds(X, labels):
    """Steps 1-4: the bound of every silhouette sample, n float64."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    _, enc = np.unique(labels, return_inverse=True)
    C = int(enc.max()) + 1
    freq = np.bincount(enc, minlength=C).astype(np.float64)
    D2 = _exact_d2(X, X)
    D = np.sqrt(D2).astype(np.float64)
    sq = (X * X).sum(axis=1)
    delta = _delta(D2, (d + 8) * U * (sq[:, None] + sq[None, :]))
    np.fill_diagonal(delta, 0.0)
    Delta = float(delta.max()) + n * U * float(D.max())
    onehot = np.zeros((n, C))
    onehot[np.arange(n), enc] = 1.0
    sums = D @ onehot
    rows = np.arange(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = sums[rows, enc] / (freq[enc] - 1.0)
        sums[rows, enc] = np.inf
        b = (sums / freq).min(axis=1)
        bound = 4.0 * 2.0 * Delta / np.maximum(a, b)
    bound[freq[enc] == 1.0] = 0.0                      # alone in its cluster: 0 on both sides
    bound[~np.isfinite(bound)] = 2.0                   # a = b = 0: the quotient hangs on rounding alone; s lies in [-1, 1]
    return np.minimum(bound, 2.0)


def score_bound(X, labels):
    """Step 5."""
    return float(sample_bounds(X, labels).mean())


def _centroid_terms(X, labels):
    X = np.asarray(X, dtype=np.float64)
    _, enc = np.unique(labels, return_inverse=True)
    C = int(enc.max()) + 1
    freq = np.bincount(enc, minlength=C)
    Xl = X.astype(np.longdouble)
    cen = np.stack([Xl[enc == k].mean(axis=0) for k in range(C)])
    r = np.array([np.sqrt((np.abs(X[enc == k]).max(axis=0) ** 2).sum()) for k in range(C)])
    e = (freq + 2) * U * r
    return X, enc, C, freq, cen, e


def davies_bouldin_bound(X, labels):
    X, enc, C, freq, cen, e = _centroid_terms(X, labels)
    n, d = X.shape
    cen64 = cen.astype(np.float64)
    csq, xsq = (cen64 * cen64).sum(axis=1), (X * X).sum(axis=1)
    s, ds = np.zeros(C), np.zeros(C)
    for k in range(C):
        rows = enc == k
        D2 = _exact_d2(X[rows], cen[k : k + 1])[:, 0]
        Dk = np.sqrt(D2).astype(np.float64)
        s[k] = Dk.mean()
        ds[k] = float(_delta(D2, (d + 8) * U * (xsq[rows] + csq[k])).max()) + e[k] + freq[k] * U * float(Dk.max())
    M2 = _exact_d2(cen, cen)
    M = np.sqrt(M2).astype(np.float64)
    dM = _delta(M2, (d + 8) * U * (csq[:, None] + csq[None, :])) + e[:, None] + e[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        R = (s[:, None] + s[None, :]) / M
        dR = (ds[:, None] + ds[None, :]) / M + R * dM / M
    dR[~np.isfinite(dR)] = 0.0     # the diagonal, and exactly equal centroids (ratio 0 on both sides)
    return 4.0 * float(dR.max(axis=1).mean())


def calinski_harabasz_bound(X, labels):
    """RELATIVE bound."""
    X, enc, C, freq, cen, e = _centroid_terms(X, labels)
    n, d = X.shape
    Xl = X.astype(np.longdouble)
    mean = Xl.mean(axis=0)
    em = (n + 4) * U * float(np.sqrt((np.abs(X).max(axis=0) ** 2).sum()))
    dist = np.sqrt(((Xl - cen[enc]) ** 2).sum(axis=1)).astype(np.float64)
    W = float((dist ** 2).sum())
    cm = np.sqrt(((cen - mean) ** 2).sum(axis=1)).astype(np.float64)
    B = float((freq * cm ** 2).sum())
    if W == 0.0:
        return 0.0
    dW = (n * d + 4) * U * W + float((2.0 * e * np.bincount(enc, weights=dist, minlength=C) + freq * e ** 2).sum())
    dB = (C * d + 4) * U * B + float((freq * (2.0 * cm * (e + em) + (e + em) ** 2)).sum())
    return 2.0 * (dW / W + dB / B) + 8.0 * U


@functools.lru_cache(maxsize=None)
def bounds(name):
    """(per-sample bounds, score bound, Davies-Bouldin bound, relative Calinski-Harabasz bound) of a case, computed once."""
    c = next(c for c in CASES if c.name == name)
    sb = sample_bounds(c.X, c.labels)
    sb.setflags(write=False)
    return sb, float(sb.mean()), davies_bouldin_bound(c.X, c.labels), calinski_harabasz_bound(c.X, c.labels)


def min_pair_distance(X):
    D2 = _exact_d2(X, X)
    np.fill_diagonal(D2, np.inf)
    return float(np.sqrt(D2.min()))
