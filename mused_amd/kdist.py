"""DBSCAN's eps from the data, as a closed-form rule: the specification of csrc/kdist.hip (plain NumPy, O(n^2) time, row
blocks of O(n) memory like mused_amd.dbscan.Scan).

The textbook recipe is the sorted k-distance plot: take every row's distance to its `min_samples`-th nearest row (the row
itself counted, scikit-learn's convention for `min_samples` and for `NearestNeighbors(n_neighbors=k).kneighbors(X)`), sort
the n values and cut at the knee of the curve.  Two things are fixed here so that the device can restate the rule bit for bit
and so that the device DBSCAN can use the result:

* the knee is the FIRST maximum of g_i = x_i - y_i over the curve normalised to the unit square (x_i = i / (n - 1),
  y_i = (v_i - v_0) / (v_{n-1} - v_0)): divisions and subtractions only, no fused multiply-add to disagree about;
* eps is NOT the curve's value at the knee.  A k-distance is by construction the exact distance of a pair, so with
  eps = v[knee] that pair lies on the threshold, mused_dbscan raises FLAG_AMBIGUOUS and the call falls back to the host
  -- on every input.  eps is the midpoint between v[knee] and the next LARGER value of the curve: strictly between two
  distinct k-distances, so no k-th neighbour pair sits on it.
"""
from __future__ import annotations

import numpy as np

from .dbscan import tau_coefficient

FLAG_NONFINITE, FLAG_FLAT = 2, 4   # csrc/kdist.hip (FLAG_NONFINITE as in mused_amd.dbscan)
MAX_K = 64                         # csrc/kdist.hip: the longest per-row list
MAX_ROWS = 1 << 19                 # what the tile grid of one launch holds (csrc/dbscan_common.h)
_BLOCK = 512                       # rows per block of distances

FLAT_TEXT = "the k-distance curve is flat"


def _check(X, k):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be (n, d) with n, d >= 1")
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= X.shape[0]:
        raise ValueError(f"k must be an integer in [1, n = {X.shape[0]}], got {k!r}")
    if not np.isfinite(X).all():
        raise ValueError("Input contains NaN or infinity.")
    return X, int(k)


def kth_sq_distances(X, k, rows=None):
    """kd2[i] = the k-th smallest of d2(i, j) over ALL j, the row itself included with d2(i, i) = 0 exactly;
    d2(i, j) = max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j), the device's form.  n float64; with `rows` (an index array) the values
    of those rows only, in that order."""
    X, k = _check(X, k)
    n = X.shape[0]
    sq = np.einsum("ij,ij->i", X, X)
    sel = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    out = np.empty(sel.size)
    for i0 in range(0, sel.size, _BLOCK):
        r = sel[i0:i0 + _BLOCK]
        d2 = sq[r, None] + sq[None, :]
        d2 -= 2.0 * (X[r] @ X.T)
        np.maximum(d2, 0.0, out=d2)
        d2[np.arange(r.size), r] = 0.0
        out[i0:i0 + r.size] = np.partition(d2, k - 1, axis=1)[:, k - 1]
    return out


def kd2_bound(X, kd2, rows=None):
    """How far two evaluations of kd2 may lie apart, per row (`rows`: kd2 holds the values of these rows only):
    c(d) 2^-52 (|x_i|^2 + max_j |x_j|^2) + 4 ulp(kd2[i]), with c(d) = mused_amd.dbscan.tau_coefficient(d) = 2 (d + 8).

    Every evaluation of a d2(i, j) -- this module's, the device's, scikit-learn's -- lies within
    e(d) = (d + 8) 2^-52 (|x_i|^2 + |x_j|^2) of the exact value (the derivation: dbscan.tau_coefficient), hence within
    E_i = (d + 8) 2^-52 (|x_i|^2 + max_j |x_j|^2) for every j of row i.  The k-th order statistic of n numbers is
    monotone in each of them, so moving every one by at most E_i moves it by at most E_i: each evaluation of kd2[i] is
    within E_i of the exact one and two of them within 2 E_i = c(d) 2^-52 (...) of each other.  scikit-learn returns the
    ROOT of its d2; squaring that costs a rounding of the root (relative 2^-53, doubled by the square) and one of the
    product: under 2 ulp of kd2[i], 4 are allowed."""
    X = np.asarray(X, dtype=np.float64)
    kd2 = np.asarray(kd2, dtype=np.float64)
    sq = np.einsum("ij,ij->i", X, X)
    own = sq if rows is None else sq[np.asarray(rows, dtype=np.int64).reshape(-1)]
    return tau_coefficient(X.shape[1]) * 2.0 ** -52 * (own + sq.max()) + 4.0 * np.spacing(kd2)


def knee(v):
    """(i*, nxt) of an ASCENDING curve v of n >= 2 values (the k-distance curve of n >= 3 rows is the intended use):
    i* = the first argmax of g_i = i / (n - 1) - (v_i - v_0) / (v_{n-1} - v_0), nxt = the first index > i* with
    v[nxt] > v[i*].  nxt exists: g_0 = 0, and g <= 0 wherever v equals its maximum (y = 1, x <= 1), so the first maximum
    is at a value below v_{n-1}.  A flat curve (v_{n-1} == v_0, always so for k = 1 and for n = 1) has no knee: ValueError."""
    v = np.asarray(v, dtype=np.float64)
    if v.ndim != 1 or v.size < 1:
        raise ValueError("v must be a non-empty 1-D array")
    n = v.size
    if not np.isfinite(v).all() or (v < 0).any():
        raise ValueError("Input contains NaN or infinity.")
    if (np.diff(v) < 0).any():
        raise ValueError("v must be ascending")
    span = v[-1] - v[0]
    if not span > 0.0:
        raise ValueError(FLAT_TEXT)
    x = np.arange(n, dtype=np.float64) / np.float64(n - 1)
    y = (v - v[0]) / span
    g = x - y
    i = int(np.argmax(g))               # (NumPy's argmax returns the first of equal maxima)
    nxt = i + 1 + int(np.argmax(v[i + 1:] > v[i]))
    return i, nxt


def eps_from_curve(v):
    """0.5 * (v[i*] + v[nxt]): strictly between two distinct values of the curve."""
    v = np.asarray(v, dtype=np.float64)
    i, nxt = knee(v)
    return 0.5 * (v[i] + v[nxt])


def select_eps(X, min_samples):
    """The whole rule: v = sort(sqrt(kth_sq_distances(X, min_samples))) -> (eps, i*, nxt, v[i*], v[nxt])."""
    v = np.sort(np.sqrt(kth_sq_distances(X, min_samples)))
    i, nxt = knee(v)
    return float(0.5 * (v[i] + v[nxt])), i, nxt, float(v[i]), float(v[nxt])
