"""Inputs shared by tests/test_hdbscan_host.py, tests/test_gpu_emst.py and tests/test_gpu_hdbscan.py: seeded generators only.
case(name) -> (X, min_cluster_size, ld) -- ld: the row pitch the device tests give the rows (0 = contiguous).  scikit-learn's
fit is computed once per case and kept read-only, and so is the specification's tree."""
import functools

import numpy as np


def _gauss(n, d, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d))


def _blobs(n, d, seed=0, centres=6):
    """80 % of the rows around `centres` centres, 20 % uniform over their box, permuted."""
    rng = np.random.default_rng(seed)
    m = n - n // 5
    cen = 4.0 * rng.standard_normal((centres, d))
    X = cen[rng.integers(0, centres, m)] + 0.4 * rng.standard_normal((m, d))
    noise = rng.uniform(X.min(axis=0), X.max(axis=0), (n - m, d))
    return np.concatenate([X, noise])[rng.permutation(n)]


def _chain(n=640, seed=0):
    """A jittered chain along the first axis whose gaps alternate at every scale: the gap in front of point i is
    1 + 0.05 * (trailing zero bits of i), so the components merge in pairs and the rounds reach ceil(log2 n)."""
    rng = np.random.default_rng(seed)
    i = np.arange(1, n)
    tz = np.log2(i & -i).astype(np.int64)
    x = np.concatenate([[0.0], np.cumsum(1.0 + 0.05 * tz + rng.uniform(-0.01, 0.01, n - 1))])
    return np.stack([x, rng.uniform(-0.01, 0.01, n)], axis=1)[rng.permutation(n)]


def _two_groups():
    """Two far groups of 256 rows each IN ROW ORDER: whole 128-row tiles hold one component after a few rounds."""
    X = _gauss(512, 8, seed=5)
    X[256:, 0] += 100.0
    return X


def _duplicates():
    X = _gauss(180, 8, seed=6)
    return np.concatenate([X, X[:20]])


def _lattice():
    g = np.arange(12.0)
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(144, 2)


def _nan_row():
    X = _gauss(150, 6, seed=7)
    X[77, 3] = np.nan
    return X


# name -> (generator, min_cluster_size, ld)
_TABLE = {
    "gauss_n2_d3": (lambda: _gauss(2, 3), 3, 0),
    "gauss_n3_d1": (lambda: _gauss(3, 1), 3, 0),
    "gauss_n127_d1": (lambda: _gauss(127, 1), 3, 0),
    "gauss_n128_d1": (lambda: _gauss(128, 1), 3, 0),
    "gauss_n129_d1": (lambda: _gauss(129, 1), 3, 0),
    "gauss_n127_d50": (lambda: _gauss(127, 50), 3, 0),
    "gauss_n128_d50": (lambda: _gauss(128, 50), 3, 0),
    "gauss_n129_d50": (lambda: _gauss(129, 50), 3, 0),
    "blobs_n300_d50": (lambda: _blobs(300, 50), 3, 0),
    "blobs_n512_d3": (lambda: _blobs(512, 3), 3, 0),
    "gauss_n1000_d50": (lambda: _gauss(1000, 50), 3, 0),
    "blobs_n1500_d10": (lambda: _blobs(1500, 10), 5, 0),
    "chain_n640_d2": (_chain, 3, 0),
    "blobs_n4097_d50": (lambda: _blobs(4097, 50, centres=12), 5, 0),
    "two_groups": (_two_groups, 3, 0),
    "pitch_n300_d8_ld11": (lambda: _gauss(300, 8, seed=3), 3, 11),
    "gauss_n200_d52": (lambda: _gauss(200, 52, seed=4), 3, 0),
}
_AMBIGUOUS = {"duplicates": (_duplicates, 3, 0), "lattice": (_lattice, 3, 0)}
_NAN = {"nan_row": (_nan_row, 3, 0)}

CASE_NAMES = list(_TABLE)               # decided far beyond rounding
AMBIGUOUS_NAMES = list(_AMBIGUOUS)      # exact ties on purpose
NAN_NAME = "nan_row"
# the shapes the prototype of the split ran with min_samples = 2; min_samples = 1 must give the same
MIN_SAMPLES_1_NAMES = ["gauss_n2_d3", "gauss_n129_d1", "blobs_n300_d50", "blobs_n512_d3", "gauss_n1000_d50",
                       "blobs_n1500_d10", "chain_n640_d2"]


@functools.lru_cache(maxsize=None)
def case(name):
    gen, mcs, ld = {**_TABLE, **_AMBIGUOUS, **_NAN}[name]
    X = np.ascontiguousarray(gen(), dtype=np.float64)
    X.setflags(write=False)
    return X, mcs, ld


@functools.lru_cache(maxsize=None)
def sklearn_fit(name, min_samples=2):
    """(labels_ as int64, the sorted weights _single_linkage_tree_["value"]) of
    HDBSCAN(min_cluster_size, min_samples, metric="euclidean").fit(X), computed once (read-only)."""
    from sklearn.cluster import HDBSCAN

    X, mcs, _ = case(name)
    m = HDBSCAN(min_cluster_size=mcs, min_samples=min_samples, metric="euclidean").fit(X)
    lab, val = np.asarray(m.labels_, dtype=np.int64).copy(), np.asarray(m._single_linkage_tree_["value"]).copy()
    lab.setflags(write=False)
    val.setflags(write=False)
    return lab, val


def sklearn_labels(name, min_samples=2):
    return sklearn_fit(name, min_samples)[0]


@functools.lru_cache(maxsize=None)
def spec_tree(name):
    """mused_amd.hdbscan.emst_boruvka of the case, computed once."""
    from mused_amd import hdbscan as spec

    return spec.emst_boruvka(case(name)[0])


def edge_set(a, b):
    """The edges as a set of unordered pairs."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    return set(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()))


def blobs(n, d, seed=0):
    """Blobs plus 20 % uniform noise at a size of the caller's choice (the invariant-only device test)."""
    return _blobs(n, d, seed=seed, centres=10)
