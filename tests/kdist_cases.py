"""Shared inputs and helpers of the k-distance / eps="auto" tests (tests/test_kdist_host.py, tests/test_gpu_kdist.py,
tests/test_gpu_eps_auto.py).  Everything is generated from seeds; no golden files.

BLOBS: the six blob-plus-noise inputs the feature was specified on -- Gaussian blobs (sklearn.datasets.make_blobs,
cluster_std 0.5, centres uniform in [-10, 10]^d) with a share of rows drawn uniformly from that same box, shuffled, seeds 0
to 5.  The last one (150 centres, no noise, k = 2) has no planted count that a single eps recovers.

The tolerance of every comparison of k-th squared distances is mused_amd.kdist.kd2_bound (derived there, never tuned).
"""
from __future__ import annotations

import functools

import numpy as np

# (n, d, centres, noise share, k)
BLOBS = [(2000, 50, 4, 0.2, 2), (2000, 50, 4, 0.2, 5), (1000, 8, 6, 0.5, 4), (3000, 16, 10, 0.1, 8), (300, 3, 3, 0.3, 3),
         (2000, 50, 150, 0.0, 2)]
BLOB_IDS = [f"n{n}_d{d}_c{c}_noise{noise}_k{k}" for n, d, c, noise, k in BLOBS]
PLANTED = [4, 4, 6, 10, 3]   # what DBSCAN(eps, k) must find on the first five


@functools.lru_cache(maxsize=None)
def blob_input(i):
    """Input i of BLOBS: (X, k), X read-only."""
    from sklearn.datasets import make_blobs

    n, d, centres, noise, k = BLOBS[i]
    m = int(round(n * noise))
    rng = np.random.default_rng(i)
    X, _ = make_blobs(n_samples=n - m, n_features=d, centers=centres, cluster_std=0.5, random_state=i)
    if m:
        X = np.concatenate([X, rng.uniform(-10.0, 10.0, size=(m, d))])
    X = np.ascontiguousarray(X[rng.permutation(n)], dtype=np.float64)
    X.setflags(write=False)
    return X, k


def sklearn_kd2(X, k):
    """scikit-learn's k-th neighbour distance (the row itself counted), squared."""
    from sklearn.neighbors import NearestNeighbors

    dist = NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)[0]
    return dist[:, k - 1] ** 2


@functools.lru_cache(maxsize=None)
def blob_reference(i):
    """(the NumPy rule's kd2, scikit-learn's kd2, the bound) of input i, computed once."""
    from mused_amd import kdist

    X, k = blob_input(i)
    kd2 = kdist.kth_sq_distances(X, k)
    return kd2, sklearn_kd2(X, k), kdist.kd2_bound(X, kd2)


def gaussian(n, d, seed, scale=1.0):
    return np.random.default_rng(seed).normal(size=(n, d)) * scale


def two_point_blobs(pairs=150, d=5, seed=11):
    """`pairs` distinct integer centres, each held by two rows; every second pair is an exact duplicate (kd2 = 0 for k = 2),
    the others differ in one coordinate by the same 2^-3 (ties between the k-distances).  Small integers and eighths: every
    product and sum of the expansion is exact in fp64 whatever its order, so the zeros and the 2^-6 are exact too."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-20, 21, size=(pairs, d)).astype(np.float64)
    c[:, 0] = 2.0 * np.arange(pairs) - pairs      # distinct centres, at least 2 apart
    X = np.repeat(c, 2, axis=0)
    X[2::4, 0] += 0.125
    return np.ascontiguousarray(X[rng.permutation(2 * pairs)])


def ramp(n=1000):
    """X[i] = -i in one dimension: for the last row tile every column tile brings smaller distances than all before."""
    return -np.arange(n, dtype=np.float64).reshape(n, 1)


def slices(n):
    """Column slices of mused_kth_distance: the rule of mused_silhouette_slices."""
    tiles = (n + 127) // 128
    return 1 if tiles >= 256 else min(tiles, 512 // tiles, 16)


def A(b):
    return (b + 255) & ~255


def ws_kth(n, k):
    """The workspace of mused_kth_distance, array by array (each on a multiple of 256 bytes)."""
    return A(16) + A(8 * n) + (A(8 * slices(n) * k * n) if slices(n) > 1 else 0)


def ws_knee(n):
    return 2 * A(8 * n) + 6 * A(4 * n) + A(4 * 256 * ((n + 1023) // 1024)) + A(16)


# ---- the device cases: the smallest shapes at which csrc/kdist.hip can go wrong ---------------------------------------------
# n: one tile, a ragged tile, an odd tile count, slice counts 1, 2, 3, 16, 12, and 256 tiles, where slicing switches off;
# d and pitch: the VEC instance (even pitch) and the plain one; k: both list lengths (<= 8, <= 64), their edges, k = n
class Case:
    def __init__(self, name, make, k, ld=None, check_rows=None):
        self.name, self._make, self.k, self._ld, self._rows = name, make, int(k), ld, check_rows

    @functools.cached_property
    def X(self):
        X = np.ascontiguousarray(self._make(), dtype=np.float64)
        X.setflags(write=False)
        return X

    @property
    def ld(self):
        return self._ld or self.X.shape[1]

    @functools.cached_property
    def rows(self):
        """The rows whose values are compared with the NumPy rule (None: all of them)."""
        return None if self._rows is None else np.asarray(self._rows(self.X.shape[0]), dtype=np.int64)

    @functools.cached_property
    def rule(self):
        from mused_amd import kdist

        return kdist.kth_sq_distances(self.X, self.k, rows=self.rows)

    @functools.cached_property
    def sklearn(self):
        return sklearn_kd2(self.X, self.k)

    @functools.cached_property
    def bound(self):
        from mused_amd import kdist

        return kdist.kd2_bound(self.X, self.sklearn)

    def __repr__(self):
        return self.name


def _edge_rows(n):
    """Of a large case: the first, a middle and the last row tile and 256 rows anywhere."""
    mid = (n // 256) * 128
    return np.unique(np.concatenate([np.arange(128), np.arange(mid, mid + 128), np.arange(n - 128, n),
                                     np.random.default_rng(1).integers(0, n, 256)]))


CASES = [
    Case("n1_d3_k1", lambda: gaussian(1, 3, 20), 1),
    Case("n2_d1_k2", lambda: gaussian(2, 1, 21), 2),
    Case("n64_d3_k64_pitch4", lambda: gaussian(64, 3, 22), 64, ld=4),
    Case("n127_d50_k5", lambda: gaussian(127, 50, 23), 5),
    Case("n128_d51_k8", lambda: gaussian(128, 51, 24), 8),
    Case("n128_d3_k1", lambda: gaussian(128, 3, 25), 1),
    Case("n129_d50_k9", lambda: gaussian(129, 50, 26), 9),
    Case("n257_d3_k2_pitch5", lambda: gaussian(257, 3, 27), 2, ld=5),
    Case("n300_d1_k64", lambda: gaussian(300, 1, 28), 64),
    Case("n2000_d50_k2_blobs", lambda: blob_input(0)[0], 2),
    Case("n2000_d51_k64", lambda: gaussian(2000, 51, 29), 64),
    Case("n3000_d16_k8_blobs", lambda: blob_input(3)[0], 8),
    Case("n5000_d3_k5_pitch8", lambda: gaussian(5000, 3, 30), 5, ld=8),
    Case("n5000_d50_k9", lambda: gaussian(5000, 50, 31), 9),
    Case("ramp_n1000_k64", ramp, 64),
    Case("ramp_n1000_k8", ramp, 8),
    Case("two_point_blobs_k2", two_point_blobs, 2),
    Case("n32768_d4_k5", lambda: gaussian(32768, 4, 32), 5, check_rows=_edge_rows),
]
CASE_IDS = [c.name for c in CASES]


def case(name):
    return next(c for c in CASES if c.name == name)
