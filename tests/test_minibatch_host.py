"""CPU checks of the device MiniBatchKMeans (mused_amd/cluster.py, approach "sSVDMC_mini", main.py:82-86).

The C ABI of csrc/minibatch.hip is declared and exported.  The host half of the class -- batch / init sizes, k-means++ on
the init subsample, the reassignment decision, the argsort trim, the RandomState draws, the count reset -- reproduces
scikit-learn's MiniBatchKMeans bit for bit when the device operations are replaced by a NumPy stand-in that does what the
kernels do: labels from sklearn's own E step (_labels_inertia), the centre update as a left-to-right sum per cluster."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mused_mbkm_ws_bytes", "mused_mbkm_step", "mused_mbkm_reassign", "mused_kmeans_assign")


def test_minibatch_symbols_declared_and_exported():
    from mused_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mused_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mused_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTED, name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name


class NumpyOps:
    """What csrc/minibatch.hip computes, in NumPy."""

    def __init__(self, k):
        self.k = k

    def prepare(self, X):
        X = np.asarray(X)
        assert X.dtype == np.float64 and X.ndim == 2
        return np.ascontiguousarray(X)

    @staticmethod
    def shape(X):
        return X.shape

    @staticmethod
    def to_host(X):
        return X.copy()

    def load(self, centers, counts):
        self.C, self.counts = centers.copy(), counts.copy()

    def _labels(self, X):
        from sklearn.cluster._kmeans import _labels_inertia

        return _labels_inertia(X, np.ones(len(X)), self.C, n_threads=1, return_inertia=False)

    def step(self, X):
        labels = self._labels(X)
        for c in range(self.k):
            rows = np.flatnonzero(labels == c)
            if len(rows) == 0:
                continue
            # c * counts, then the rows in sample order: np.cumsum adds left to right
            acc = np.cumsum(np.vstack([self.C[c] * self.counts[c], X[rows]]), axis=0)[-1]
            self.counts[c] += float(len(rows))
            self.C[c] = acc * (1 / self.counts[c])

    def read_counts(self):
        return self.counts.copy()

    def reassign(self, X, rows, dst, counts):
        self.C[dst] = X[rows]
        self.counts = counts.copy()

    def labels_and_counts(self, X, want_counts):
        return self._labels(X), (self.counts.copy() if want_counts else None)

    def centers(self):
        return self.C.copy()


def _host_class():
    from mused_amd.cluster import MiniBatchKMeans

    class HostMiniBatch(MiniBatchKMeans):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.decisions = []   # (reassign?, counts had a zero) per step

        def _make_ops(self):
            return NumpyOps(self.n_clusters)

        def _random_reassign(self):
            zeros = bool((self._counts == 0).any())
            r = super()._random_reassign()
            self.decisions.append((r, zeros))
            return r

    return HostMiniBatch


def _compare(batches, k, seed, **kw):
    from sklearn.cluster import MiniBatchKMeans as SkMiniBatch

    ours = _host_class()(n_clusters=k, random_state=seed, **kw)
    ref = SkMiniBatch(n_clusters=k, random_state=seed, **kw)
    for t, X in enumerate(batches):
        ours.partial_fit(X)
        ref.partial_fit(X)
        assert np.array_equal(ours.cluster_centers_, ref.cluster_centers_), f"step {t}: centres differ"
        assert np.array_equal(ours._counts, ref._counts), f"step {t}: counts differ"
        assert np.array_equal(ours.labels_, ref.labels_), f"step {t}: labels differ"
        assert np.array_equal(ours.predict(X), ref.predict(X)), f"step {t}: predict differs"
        assert ours.n_steps_ == ref.n_steps_ == t + 1
    assert ours._batch_size == ref._batch_size and ours._init_size == ref._init_size
    return ours, ref


def _blobs(steps, n, d, seed, centres=5):
    rng = np.random.default_rng(seed)
    mu = rng.normal(scale=4.0, size=(centres, d))
    return [mu[rng.integers(0, centres, n)] + rng.normal(size=(n, d)) for _ in range(steps)]


def test_host_logic_matches_sklearn_stream_like():
    """The reference's use: batch_size = n, k > true clusters; reassignment every 10 k / n steps."""
    ours, _ = _compare(_blobs(12, 500, 16, 0), 150, 0, batch_size=500)
    fired = [r for r, _ in ours.decisions]
    assert any(fired) and not all(fired)


def test_init_subsample_and_empty_cluster_reassignment():
    """batch_size 64 on 300 rows: init_size 192 < 300 draws the init subsample (randint); 10 k = 80 > 64, so the first
    step's reassignment is forced by the empty clusters alone."""
    ours, ref = _compare(_blobs(10, 300, 6, 1), 8, 3, batch_size=64)
    assert ref._init_size == 192 < 300
    assert ours.decisions[0] == (True, True)
    assert any(not r for r, _ in ours.decisions), "no step without a reassignment"


def test_argsort_trim_branch(monkeypatch):
    """More than 0.5 n centres below the threshold: the argsort trim of _mini_batch_step."""
    rng = np.random.default_rng(1)
    batches = [rng.normal(size=(64, 8)) for _ in range(12)]
    calls = []
    real = np.argsort

    def spy(a, *args, **kw):
        if sys._getframe(1).f_code.co_name == "_plan_reassign":
            calls.append(len(a))
        return real(a, *args, **kw)

    monkeypatch.setattr(np, "argsort", spy)
    _compare(batches, 48, 0, batch_size=64, reassignment_ratio=0.5)
    assert calls, "the > 0.5 n trim branch was not taken"


def test_random_init_and_seed_object():
    rs_a, rs_b = np.random.RandomState(5), np.random.RandomState(5)
    from sklearn.cluster import MiniBatchKMeans as SkMiniBatch

    ours = _host_class()(n_clusters=6, random_state=rs_a, batch_size=100, init="random")
    ref = SkMiniBatch(n_clusters=6, random_state=rs_b, batch_size=100, init="random")
    for X in _blobs(10, 100, 3, 2):
        ours.partial_fit(X)
        ref.partial_fit(X)
        assert np.array_equal(ours.cluster_centers_, ref.cluster_centers_)
        assert np.array_equal(ours._counts, ref._counts)


def test_unsupported_inputs_raise():
    from mused_amd.cluster import MiniBatchKMeans

    X = _blobs(1, 100, 4, 0)[0]
    cls = _host_class()
    with pytest.raises(ValueError):
        MiniBatchKMeans(4, init=X[:4])
    with pytest.raises(ValueError):
        MiniBatchKMeans(4, init=lambda X, k, random_state: X[:k])
    m = cls(n_clusters=4, random_state=0)
    with pytest.raises(ValueError):
        m.partial_fit(X, sample_weight=np.ones(len(X)))
    with pytest.raises(ValueError):
        m.partial_fit(X.astype(np.float32))
    with pytest.raises(ValueError):
        m.partial_fit(X[:3])
    import scipy.sparse as sp

    with pytest.raises(ValueError):
        m.partial_fit(sp.csr_matrix(X))
    with pytest.raises(ValueError):
        m.predict(X)  # not fitted
    m.partial_fit(X)
    with pytest.raises(ValueError):
        m.partial_fit(X[:, :3])


def test_pipeline_requires_n_clusters_total():
    from mused_amd.pipeline import StreamPipeline

    with pytest.raises(ValueError, match="n_clusters_total"):
        StreamPipeline(500, 16, 50, 0, "sSVDMC_mini")
