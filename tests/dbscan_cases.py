"""Inputs shared by tests/test_dbscan_host.py and tests/test_gpu_dbscan.py: (name, X, eps, min_samples, ld) -- ld: row pitch
the device tests give the rows (0 = contiguous).  scikit-learn's labels are computed once per case and kept."""
import functools

import numpy as np


def _normal(n, d):
    return np.random.default_rng(0).standard_normal((n, d))


def _chain(d):
    X = np.zeros((1000, d))
    X[:, 0] = 0.9 * np.arange(1000)
    return X[np.random.default_rng(0).permutation(1000)]


def _bridge(swap):
    a, b = np.arange(5) * 0.1, 2.0 + np.arange(5) * 0.1
    x = np.concatenate([b, a, [1.2]]) if swap else np.concatenate([a, b, [1.2]])
    return np.stack([x, np.zeros_like(x)], axis=1)


@functools.lru_cache(maxsize=None)
def _centres(c, d):
    rng = np.random.default_rng(1)
    n = 20000
    cen = 3 * rng.standard_normal((c, d))
    return cen[rng.integers(0, c, n)] + 0.1 * rng.standard_normal((n, d))


def _duplicates():
    X = _normal(300, 8)
    return np.concatenate([X, X[:50]])


def _pairs(n, h):
    """Row i and row i + h are 0.5 apart, every other pair at least 9.5: with h a multiple of 128 each neighbour pair lies in
    a pair of row tiles h / 128 apart -- antipodal at n = 512 (4 tiles), across the wrap-around at n = 640 (5 tiles)."""
    i = np.arange(n)
    return np.stack([10.0 * (i % h) + 0.5 * (i // h), np.zeros(n)], axis=1)


def small_cases():
    out = []
    for n in (1, 2, 127, 128, 129):
        out.append((f"small_n{n}", _normal(n, 8), 2.5, 3, 0))
        out.append((f"small_n{n}_ld11", _normal(n, 8), 2.5, 3, 11))
    for d in (15, 16):
        for ms in (2, 3):
            out.append((f"chain_d{d}_m{ms}", _chain(d), 1.0, ms, 0))
    out.append(("bridge_ab", _bridge(False), 0.85, 5, 0))
    out.append(("bridge_ba", _bridge(True), 0.85, 5, 0))
    out.append(("duplicates", _duplicates(), 2.0, 4, 0))
    out.append(("min_samples_1", _normal(300, 8), 1.0, 1, 0))
    # a tile pair served twice makes the m3 cases core (scikit-learn: all noise), one never served makes the m2 cases noise
    # (scikit-learn: label[i] == i % h)
    for n in (512, 640):
        for ms in (2, 3):
            out.append((f"pairs_n{n}_m{ms}", _pairs(n, n // 2), 1.0, ms, 0))
    return out


def centres_cases():
    return [("centres_A", _centres(400, 50), 1.0, 5, 0), ("centres_B", _centres(400, 50), 0.95, 40, 0),
            ("centres_C", _centres(2000, 16), 0.55, 6, 0)]


def all_cases():
    return small_cases() + centres_cases()


CASE_NAMES = [c[0] for c in small_cases()] + ["centres_A", "centres_B", "centres_C"]
_SK = {}


def case(name):
    for c in all_cases() if name.startswith("centres") else small_cases():
        if c[0] == name:
            return c
    raise KeyError(name)


def _fit(name):
    if name not in _SK:
        from sklearn.cluster import DBSCAN

        _, X, eps, ms, _ = case(name)
        m = DBSCAN(eps=eps, min_samples=ms, metric="euclidean").fit(X)
        lab, core = m.labels_.copy(), m.core_sample_indices_.copy()
        lab.setflags(write=False)
        core.setflags(write=False)
        _SK[name] = (lab, core)
    return _SK[name]


def sklearn_labels(name):
    """DBSCAN(eps, min_samples).fit(X).labels_ of the case, computed once (read-only)."""
    return _fit(name)[0]


def sklearn_core(name):
    """... and its core_sample_indices_."""
    return _fit(name)[1]
