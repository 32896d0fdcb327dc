"""sklearn.cluster.DBSCAN(eps, min_samples, metric="euclidean").fit_predict written out as a closed-form rule: the
specification of csrc/dbscan.hip (plain NumPy, O(n^2) time, row blocks of O(n) memory).

scikit-learn's `dbscan_inner` visits the rows in index order and runs a depth-first search from every unlabelled core
row.  With N(i) = { j : d2(i, j) <= eps^2 } (i itself included) its result is

    core rows      i is core iff |N(i)| >= min_samples
    clusters       the connected components of the graph on the core rows with the edges d2 <= eps^2
    numbering      0, 1, ... by ascending smallest core index of the component
    non-core rows  the smallest label among the core neighbours, -1 (noise) without one

(a border row is labelled by the first search that reaches it: the one of the lowest-numbered cluster it touches).
Only the comparisons d2 <= eps^2 depend on rounding; `tau` bounds how far any two ways of evaluating one can disagree, and
a pair within tau of eps^2 is AMBIGUOUS: the device then leaves the call to scikit-learn.
"""
from __future__ import annotations

import numpy as np

FLAG_AMBIGUOUS, FLAG_NONFINITE = 1, 2
_BLOCK = 512   # rows per block of distances


def tau_coefficient(d: int) -> float:
    """c(d) of tau = c(d) 2^-52 (|x|^2 + |y|^2) + 4 ulp(eps^2), with u = 2^-53 and S = |x|^2 + |y|^2.  Every comparison
    scikit-learn or the device makes for a pair is covered:

    * |x|^2 + |y|^2 - 2 x.y (scikit-learn's brute path, d > 15, and the device).  A sum of d rounded products in ANY order
      is off by at most gamma_d sum |terms| (gamma_d = d u / (1 - d u)): gamma_d S for the two norms together,
      2 gamma_d sum |x_k y_k| <= gamma_d S for the doubled dot product (2 |ab| <= a^2 + b^2; doubling is exact).  The two
      additions that combine the three numbers round results of magnitude <= |x|^2 + |y|^2 + 2 |x.y| <= 2 S: 4 u S.
      Together (2 d + 4) u S = (d + 2) 2^-52 S to first order.
    * sum (x_k - y_k)^2 against r^2 (the leaves of scikit-learn's k-d tree, d <= 15): difference, square and up to d - 1
      additions give every term a relative error <= gamma_{d+2}, and the exact sum is d2 <= 2 S: (2 d + 4) u S again.
    * the k-d tree's node tests, which prune a node when the smallest distance from the query to its bounding box exceeds
      r and accept it whole when the largest does not (distances, compared with r itself).  Either bound is a sum over
      the coordinates of squared differences between x_k and a box edge, rounded like the leaf form (gamma_{d+2}), then
      a root by pow (<= 1 ulp: 2 u on the root, 4 u on its square): relative (d + 6) u to first order.  Each term of the
      lower bound is at most (x_k - y_k)^2 and each term of the upper bound at least that for every row y in the box, so
      a node test can decide a pair (x, y) differently from the exact d2 <= r^2 only if the exact bound, and with it
      d2(x, y) <= 2 S, lies within that relative error of r^2: (2 d + 12) u S = (d + 6) 2^-52 S.

    Every evaluation is therefore within (d + 6) 2^-52 S of a value on the exact d2's side of eps^2; 2 more units take the
    second-order terms (d u << 1) and the rounding of the bound itself: e(d) = (d + 8) 2^-52 S.  Two evaluations that
    land on different sides of eps^2 are each within e(d) of the exact d2, so c(d) = 2 (d + 8) separates them."""
    return 2.0 * (d + 8)


def eps_slack(eps: float) -> float:
    """4 ulp of eps^2, taken as 4 eps^2 2^-52 (an ulp is at most that): eps * eps, pow(eps, 2) and the exact square are
    within 1 ulp of one another; the rest covers the rounding of d2 - eps^2 near eps^2."""
    e2 = float(eps) * float(eps)
    return 4.0 * max(e2 * 2.0 ** -52, 5e-324)


def _check(X, eps, min_samples):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be (n, d) with n, d >= 1")
    if not (float(eps) > 0.0) or int(min_samples) < 1:
        raise ValueError("eps must be > 0 and min_samples >= 1")
    return X


class Scan:
    """One pass over the pairs: `a`, `b` (the pairs a < b with d2 <= eps^2 -- the only O(edges) memory of this module),
    `margin` (smallest |d2 - eps^2| over the pairs i != j), `tau` (the largest tau(i, j) of any pair) and `ambiguous` (some
    pair i != j lies within ITS tau of eps^2: false whenever tau < margin)."""

    def __init__(self, X, eps):
        X = _check(X, eps, 1)
        n, d = X.shape
        self.n = n
        e2 = float(eps) * float(eps)
        sq = np.einsum("ij,ij->i", X, X)
        c, te = tau_coefficient(d) * 2.0 ** -52, eps_slack(eps)
        aa, bb = [], []
        self.margin, self.tau, self.ambiguous = np.inf, c * 2.0 * float(sq.max()) + te, False
        for i0 in range(0, n, _BLOCK):
            i1 = min(n, i0 + _BLOCK)
            rows = np.arange(i0, i1)
            s = sq[i0:i1, None] + sq[None, :]
            d2 = s - 2.0 * (X[i0:i1] @ X.T)       # the device's form, with its own order of the sums
            d2[rows - i0, rows] = 0.0              # the pair (i, i) is in range by definition
            r, col = np.nonzero(d2 <= e2)
            keep = (r + i0) < col
            aa.append(r[keep] + i0)
            bb.append(col[keep])
            d2 -= e2
            np.abs(d2, out=d2)
            d2[rows - i0, rows] = np.inf
            lo = float(d2.min())
            self.margin = min(self.margin, lo)
            if lo <= self.tau:                     # (only then can a pair of this block be within its own tau)
                s *= c
                s += te
                self.ambiguous = self.ambiguous or bool((d2 <= s).any())
        self.a, self.b = np.concatenate(aa), np.concatenate(bb)


def margins(X, eps):
    """(smallest |d2 - eps^2| over the pairs i != j, the largest tau of any pair).  The labels are decided beyond rounding
    iff no pair lies within its own tau (`ambiguous`), in particular when the second number is below the first."""
    s = Scan(X, eps)
    return s.margin, s.tau


def ambiguous(X, eps) -> bool:
    """Some pair i != j lies within tau(i, j) of eps^2."""
    return Scan(X, eps).ambiguous


def dbscan_labels(X, eps=0.5, min_samples=5, scan=None):
    """The rule above: int64 labels like DBSCAN.fit_predict (equal to scikit-learn's wherever `ambiguous` is False).
    scan: a Scan(X, eps) made earlier."""
    X = _check(X, eps, min_samples)
    if not np.isfinite(X).all():
        raise ValueError("Input contains NaN or infinity.")
    n = X.shape[0]
    sc = scan if scan is not None else Scan(X, eps)
    a, b = sc.a, sc.b
    count = 1 + np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    core = count >= int(min_samples)
    # union-find over the core-core edges in rounds: every root that sees a smaller root across an edge is hooked under the
    # smallest such one, then all paths are shortened -- parent[x] <= x throughout, so a component's root is its smallest index
    cc = core[a] & core[b]
    ea, eb = a[cc], b[cc]
    parent = np.arange(n)
    while True:
        pa, pb = parent[ea], parent[eb]
        diff = pa != pb
        if not diff.any():
            break
        np.minimum.at(parent, np.maximum(pa, pb)[diff], np.minimum(pa, pb)[diff])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    roots = np.flatnonzero(core & (parent == np.arange(n)))
    rank = np.full(n, -1, dtype=np.int64)
    rank[roots] = np.arange(len(roots))
    big = np.iinfo(np.int64).max
    labels = np.where(core, rank[parent], big)
    for u, v in ((a, b), (b, a)):   # non-core u next to core v
        sel = ~core[u] & core[v]
        np.minimum.at(labels, u[sel], labels[v[sel]])
    labels[labels == big] = -1
    return labels
