"""Cluster quality without ground truth, written out as rules: the specification of csrc/silhouette.hip (plain NumPy, O(n^2)
time, row blocks of O(n) memory).  The three functions restate scikit-learn 1.7's

    sklearn.metrics.silhouette_samples(X, labels, metric="euclidean")
    sklearn.metrics.davies_bouldin_score(X, labels)
    sklearn.metrics.calinski_harabasz_score(X, labels)

and the tests pin them, and the kernels, to those.

Conventions (scikit-learn's):

* labels: any int32 value is a cluster id; -1 is a cluster like any other.  Callers that treat -1 as noise (DBSCAN, HDBSCAN)
  mask those rows themselves before they score.
* fewer than 2 or more than n - 1 distinct labels: `ValueError` with scikit-learn's text; a non-finite row: `ValueError`
  with scikit-learn's text (checked first, as `check_X_y` runs before the label count).
* distances: d2 = |x|^2 + |y|^2 - 2 x.y, clamped at 0, then the square root; the pair of a row with itself is exactly 0.
* silhouette: a(i) = (sum over the own cluster) / (size - 1), b(i) = the smallest cluster mean over the other clusters,
  s(i) = (b - a) / max(a, b); 0 for a row alone in its cluster and wherever the quotient is 0 / 0 (`nan_to_num`).
* Davies-Bouldin: distances of the rows to their centroid and between centroids; 0.0 when all mean distances or all centroid
  distances are within 1e-8 of 0 (`np.allclose`); a zero centroid distance is treated as infinite (ratio 0).
* Calinski-Harabasz: 1.0 when the within-cluster dispersion is exactly 0.
"""
from __future__ import annotations

import numpy as np

FLAG_NONFINITE, FLAG_LABELS = 2, 4
_BLOCK = 512   # rows per block of distances


def labels_error(n_labels: int) -> ValueError:
    """scikit-learn's `check_number_of_labels` error."""
    return ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % n_labels)


def nonfinite_error(has_nan: bool) -> ValueError:
    """scikit-learn's `_assert_all_finite` error for the argument X."""
    if has_nan:
        return ValueError("Input X contains NaN.")
    return ValueError("Input X contains infinity or a value too large for dtype('float64').")


def _check(X, labels):
    X = np.asarray(X, dtype=np.float64)
    labels = np.asarray(labels)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be (n, d) with n, d >= 1")
    if labels.shape != (X.shape[0],) or labels.dtype.kind not in "iu":
        raise ValueError("labels must be n integers")
    if not np.isfinite(X).all():
        raise nonfinite_error(bool(np.isnan(X).any()))
    _, enc = np.unique(labels, return_inverse=True)
    n_labels = int(enc.max()) + 1
    if not 1 < n_labels < X.shape[0]:
        raise labels_error(n_labels)
    return X, enc.astype(np.int64), n_labels


def silhouette_samples_numpy(X, labels):
    """silhouette_samples(X, labels, metric="euclidean"): n float64 values."""
    X, enc, C = _check(X, labels)
    n = X.shape[0]
    freq = np.bincount(enc, minlength=C).astype(np.float64)
    sq = np.einsum("ij,ij->i", X, X)
    onehot = np.zeros((n, C))
    onehot[np.arange(n), enc] = 1.0
    out = np.empty(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i0 in range(0, n, _BLOCK):
            i1 = min(n, i0 + _BLOCK)
            rows = np.arange(i0, i1)
            d2 = sq[i0:i1, None] + sq[None, :] - 2.0 * (X[i0:i1] @ X.T)
            np.maximum(d2, 0.0, out=d2)
            D = np.sqrt(d2)
            D[rows - i0, rows] = 0.0
            sums = D @ onehot                               # (block, C) sums per cluster
            own = enc[i0:i1]
            a = sums[rows - i0, own] / (freq[own] - 1.0)    # 0 / 0 for a row alone in its cluster
            sums[rows - i0, own] = np.inf
            b = (sums / freq).min(axis=1)
            out[i0:i1] = (b - a) / np.maximum(a, b)
    return np.nan_to_num(out)


def _centroids(X, enc, C):
    cen = np.zeros((C, X.shape[1]))
    np.add.at(cen, enc, X)
    return cen / np.bincount(enc, minlength=C)[:, None]


def davies_bouldin_numpy(X, labels) -> float:
    """davies_bouldin_score(X, labels)."""
    X, enc, C = _check(X, labels)
    cen = _centroids(X, enc, C)
    freq = np.bincount(enc, minlength=C)
    dist = np.sqrt(((X - cen[enc]) ** 2).sum(axis=1))
    intra = np.bincount(enc, weights=dist, minlength=C) / freq
    M = np.sqrt(((cen[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2))
    if np.allclose(intra, 0) or np.allclose(M, 0):
        return 0.0
    M[M == 0] = np.inf
    return float(np.mean(np.max((intra[:, None] + intra[None, :]) / M, axis=1)))


def calinski_harabasz_numpy(X, labels) -> float:
    """calinski_harabasz_score(X, labels)."""
    X, enc, C = _check(X, labels)
    n = X.shape[0]
    cen = _centroids(X, enc, C)
    freq = np.bincount(enc, minlength=C)
    extra = float((freq * ((cen - X.mean(axis=0)) ** 2).sum(axis=1)).sum())
    intra = float(((X - cen[enc]) ** 2).sum())
    return 1.0 if intra == 0.0 else extra * (n - C) / (intra * (C - 1.0))
