"""`MiniBatchKMeans` with its arithmetic on the device: the clusterer of the reference's "sSVDMC_mini" approach
(main.py:82-86: ONE `sklearn.cluster.MiniBatchKMeans(n_clusters=n_clusters_total, random_state=seed, batch_size=W)` for the
whole stream, `partial_fit(reduced).predict(reduced)` per window).

The split follows the device k-means of `matrix_operations.perform_clustering_on_device`: everything that draws from the
RandomState stays on the host and runs the very NumPy expressions of scikit-learn 1.7 (cluster/_kmeans.py) on a host copy of
the k counts -- `_check_params_vs_input` (batch / init size), `_init_centroids` (the init subsample and sklearn's own
`kmeans_plusplus`), `_random_reassign`, and the reassignment block of `_mini_batch_step` (threshold, argsort trim,
`random_state.choice`, count reset).  The E step and the ordered centre update run in libmused_hip (csrc/minibatch.hip), so
centres and counts equal scikit-learn's bit for bit wherever the labels agree.

Per `partial_fit` the host waits once, for the counts and the labels; a step that reassigns centres waits once more, for
the counts after the update, before it picks the rows.  Only the reference's use is supported (dense fp64 rows, no sample
weights, init "k-means++" or "random"); anything else raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib

MAX_CLUSTERS = 1024
MAX_FEATURES = 512


class MiniBatchKMeans:
    def __init__(self, n_clusters, random_state=None, batch_size=1024, init="k-means++", init_size=None,
                 reassignment_ratio=0.01, stream=None):
        if not isinstance(init, str) or init not in ("k-means++", "random"):
            raise ValueError(f"init={init!r}: only 'k-means++' and 'random' are supported on the device path")
        self.n_clusters = int(n_clusters)
        if not 1 <= self.n_clusters <= MAX_CLUSTERS:
            raise ValueError(f"n_clusters={n_clusters}: 1 .. {MAX_CLUSTERS} on the device path")
        if int(batch_size) < 1 or (init_size is not None and int(init_size) < 1):
            raise ValueError("batch_size and init_size must be >= 1")
        if reassignment_ratio < 0:
            raise ValueError(f"reassignment_ratio should be >= 0, got {reassignment_ratio} instead.")
        self.random_state = random_state
        self.batch_size = int(batch_size)
        self.init = init
        self.init_size = init_size
        self.reassignment_ratio = reassignment_ratio
        self.stream = stream
        self._ops = None

    # ---- the device half (replaced by a NumPy stand-in in tests/test_minibatch_host.py) ----------------------------------
    def _make_ops(self):
        return _DeviceOps(self.n_clusters, self.stream)

    # ---- scikit-learn's host logic ------------------------------------------------------------------------------------------
    def _check_input(self, X, sample_weight):
        if sample_weight is not None:
            raise ValueError("sample_weight is not supported on the device path")
        try:
            import scipy.sparse as sp

            if sp.issparse(X):
                raise ValueError("sparse input is not supported on the device path")
        except ImportError:  # pragma: no cover
            pass
        if type(X).__module__.startswith("torch"):
            ok = str(X.dtype) == "torch.float64" and X.dim() == 2
        else:
            X = np.asarray(X)
            ok = X.dtype == np.float64 and X.ndim == 2
        if not ok:
            raise ValueError(f"expected 2-D float64 rows, got {X.dtype} with shape {tuple(X.shape)}")
        if self._ops is None:
            self._ops = self._make_ops()
        Xo = self._ops.prepare(X)
        n, d = self._ops.shape(Xo)
        if n < self.n_clusters:
            raise ValueError(f"n_samples={n} should be >= n_clusters={self.n_clusters}.")
        if not 1 <= d <= MAX_FEATURES:
            raise ValueError(f"{d} features: 1 .. {MAX_FEATURES} on the device path")
        if hasattr(self, "_centers_shape") and d != self._centers_shape[1]:
            raise ValueError(f"X has {d} features, but MiniBatchKMeans is expecting {self._centers_shape[1]} features")
        return Xo, n, d

    def _check_params_vs_input(self, n):  # _kmeans.py MiniBatchKMeans._check_params_vs_input
        import warnings

        self._batch_size = min(self.batch_size, n)
        self._init_size = self.init_size
        if self._init_size is None:
            self._init_size = 3 * self._batch_size
            if self._init_size < self.n_clusters:
                self._init_size = 3 * self.n_clusters
        elif self._init_size < self.n_clusters:
            warnings.warn(f"init_size={self._init_size} should be larger than n_clusters={self.n_clusters}. Setting it to "
                          "min(3*n_clusters, n_samples)", RuntimeWarning, stacklevel=3)
            self._init_size = 3 * self.n_clusters
        self._init_size = min(self._init_size, n)

    def _init_centroids(self, X, random_state):  # _kmeans.py _BaseKMeans._init_centroids, sample_weight = ones
        from sklearn.cluster import kmeans_plusplus
        from sklearn.utils.extmath import row_norms

        x_squared_norms = row_norms(X, squared=True)
        sample_weight = np.ones(X.shape[0], dtype=X.dtype)
        n_samples = X.shape[0]
        if self._init_size is not None and self._init_size < n_samples:
            init_indices = random_state.randint(0, n_samples, self._init_size)
            X = X[init_indices]
            x_squared_norms = x_squared_norms[init_indices]
            n_samples = X.shape[0]
            sample_weight = sample_weight[init_indices]
        if self.init == "k-means++":
            centers, _ = kmeans_plusplus(X, self.n_clusters, x_squared_norms=x_squared_norms, random_state=random_state,
                                         sample_weight=sample_weight)
        else:
            seeds = random_state.choice(n_samples, size=self.n_clusters, replace=False, p=sample_weight / sample_weight.sum())
            centers = X[seeds]
        return np.ascontiguousarray(centers, dtype=np.float64)

    def _random_reassign(self):  # _kmeans.py MiniBatchKMeans._random_reassign
        self._n_since_last_reassign += self._batch_size
        if (self._counts == 0).any() or self._n_since_last_reassign >= (10 * self.n_clusters):
            self._n_since_last_reassign = 0
            return True
        return False

    def _plan_reassign(self, weight_sums, n):
        """The host half of the reassignment block of _kmeans.py _mini_batch_step, on the counts after the update.
        Returns (rows, centres, counts): rows of X to copy into those centres (both None if there are none), new counts."""
        to_reassign = weight_sums < self.reassignment_ratio * weight_sums.max()
        # pick at most .5 * batch_size samples as new centers
        if to_reassign.sum() > 0.5 * n:
            indices_dont_reassign = np.argsort(weight_sums)[int(0.5 * n):]
            to_reassign[indices_dont_reassign] = False
        n_reassigns = to_reassign.sum()
        rows = dst = None
        if n_reassigns:
            rows = self._random_state.choice(n, replace=False, size=n_reassigns)
            dst = np.where(to_reassign)[0]
        weight_sums[to_reassign] = np.min(weight_sums[~to_reassign])
        return rows, dst, weight_sums

    # ---- public interface ---------------------------------------------------------------------------------------------------
    def partial_fit(self, X, y=None, sample_weight=None):
        """Update the centres on the batch X ((n, d) fp64: CUDA tensor or NumPy array); returns self."""
        from sklearn.utils import check_random_state

        Xo, n, d = self._check_input(X, sample_weight)
        if not hasattr(self, "_random_state"):
            self._random_state = check_random_state(self.random_state)
        self.n_steps_ = getattr(self, "n_steps_", 0)
        ops = self._ops
        if not hasattr(self, "_centers_shape"):
            self._check_params_vs_input(n)
            centers = self._init_centroids(ops.to_host(Xo), self._random_state)
            self._counts = np.zeros(self.n_clusters, dtype=np.float64)
            self._n_since_last_reassign = 0
            ops.load(centers, self._counts)
            self._centers_shape = centers.shape
        random_reassign = self._random_reassign()   # decided on the counts BEFORE the step, as sklearn does
        ops.step(Xo)
        reassigned = False
        if random_reassign and self.reassignment_ratio > 0:
            counts = ops.read_counts()
            rows, dst, counts = self._plan_reassign(counts, n)
            if rows is not None:
                ops.reassign(Xo, rows, dst, counts)
            self._counts = counts
            reassigned = True
        labels, counts = ops.labels_and_counts(Xo, want_counts=not reassigned)
        if not reassigned:
            self._counts = counts
        self.labels_ = labels
        self.n_steps_ += 1
        return self

    def predict(self, X):
        """Index of the nearest centre for each row of X (int32 NumPy array)."""
        if not hasattr(self, "_centers_shape"):
            raise ValueError("this MiniBatchKMeans instance is not fitted yet")
        Xo, _, _ = self._check_input(X, None)
        return self._ops.labels_and_counts(Xo, want_counts=False)[0]

    @property
    def cluster_centers_(self):
        if self._ops is None or not hasattr(self, "_centers_shape"):
            raise AttributeError("cluster_centers_")
        return self._ops.centers()

    def close(self):
        self._ops = None


class _DeviceOps:
    """Centres, counts and the batch on the device; every call on one stream (the class's, else the current one at the
    first call).  Host reads go through pinned buffers behind an event."""

    def __init__(self, k, stream):
        import torch

        self.k = k
        self.st = stream if stream is not None else torch.cuda.current_stream()
        self.dev = self.st.device
        self.C = self.counts = self.ws = None
        self._lab = {}
        self._pin_counts = torch.empty(k, dtype=torch.float64, pin_memory=True)
        self._pin_lab = None
        self._ev = torch.cuda.Event()

    def prepare(self, X):
        import torch

        if isinstance(X, torch.Tensor):
            if not X.is_cuda:
                X = X.numpy()
            else:
                if X.dtype != torch.float64 or X.dim() != 2:
                    raise ValueError(f"expected a 2-D float64 tensor, got {X.dtype} with shape {tuple(X.shape)}")
                if X.stride(1) != 1 or X.stride(0) < max(X.shape[1], 1):
                    X = X.contiguous()
                # rows produced on the caller's stream: this stream waits for them
                self.st.wait_stream(torch.cuda.current_stream(X.device))
                return X
        a = np.asarray(X)
        if a.dtype != np.float64 or a.ndim != 2:
            raise ValueError(f"expected a 2-D float64 array, got {a.dtype} with shape {a.shape}")
        with torch.cuda.stream(self.st):
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    @staticmethod
    def shape(X):
        return int(X.shape[0]), int(X.shape[1])

    def to_host(self, X):
        with _stream(self.st):
            out = X.cpu().numpy()
        return np.ascontiguousarray(out)

    def load(self, centers, counts):
        import torch

        with _stream(self.st):
            self.C = torch.from_numpy(centers.copy()).to(self.dev)
            self.counts = torch.from_numpy(counts.copy()).to(self.dev)
            self.d = centers.shape[1]
            self.ws = torch.empty(int(_lib.lib().mused_mbkm_ws_bytes(1, self.d, self.k)), dtype=torch.uint8, device=self.dev)

    def _labels_buf(self, n, key):
        import torch

        buf = self._lab.get((key, n))
        if buf is None:
            # allocated on the stream that writes it: taken from the calling thread's current stream, the block can be one
            # that a tensor freed there (a window's sigma) still has a pending write to, which then lands on the labels
            with _stream(self.st):
                buf = self._lab[(key, n)] = torch.empty(n, dtype=torch.int32, device=self.dev)
        return buf

    def _args(self, X):
        from .engine import ptr

        return ptr(X), X.stride(0), int(X.shape[0]), int(X.shape[1]), self.k

    def step(self, X):
        import ctypes as C

        from .engine import ptr

        lab = self._labels_buf(int(X.shape[0]), "step")
        _lib.call("mused_mbkm_step", *self._args(X), ptr(self.C), ptr(self.counts), ptr(lab), ptr(self.ws), self.ws.numel(),
                  C.c_void_p(self.st.cuda_stream))

    def read_counts(self):
        with _stream(self.st):
            self._pin_counts.copy_(self.counts, non_blocking=True)
            self._ev.record(self.st)
        self._ev.synchronize()
        return self._pin_counts.numpy().copy()

    def reassign(self, X, rows, dst, counts):
        import ctypes as C

        import torch

        from .engine import ptr

        pairs = np.concatenate([np.asarray(rows), np.asarray(dst)]).astype(np.int32)
        m = len(rows)
        with _stream(self.st):
            pairs_d = torch.from_numpy(pairs).to(self.dev)
            counts_d = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.float64)).to(self.dev)
            _lib.call("mused_mbkm_reassign", *self._args(X), ptr(pairs_d), ptr(pairs_d[m:]), m, ptr(counts_d), ptr(self.C),
                      ptr(self.counts), C.c_void_p(self.st.cuda_stream))
            self._ev.record(self.st)
        self._ev.synchronize()  # the uploads' sources are host arrays of this frame

    def labels_and_counts(self, X, want_counts):
        """E step of X on the current centres -> host labels (and the host counts), one wait."""
        import ctypes as C

        import torch

        from .engine import ptr

        n = int(X.shape[0])
        lab = self._labels_buf(n, "out")
        _lib.call("mused_kmeans_assign", *self._args(X), ptr(self.C), ptr(lab), ptr(self.ws), self.ws.numel(),
                  C.c_void_p(self.st.cuda_stream))
        if self._pin_lab is None or self._pin_lab.numel() != n:
            self._pin_lab = torch.empty(n, dtype=torch.int32, pin_memory=True)
        with _stream(self.st):
            self._pin_lab.copy_(lab, non_blocking=True)
            if want_counts:
                self._pin_counts.copy_(self.counts, non_blocking=True)
            self._ev.record(self.st)
        self._ev.synchronize()
        return self._pin_lab.numpy().copy(), (self._pin_counts.numpy().copy() if want_counts else None)

    def centers(self):
        with _stream(self.st):
            out = self.C.cpu().numpy()
        return out


def _stream(st):
    import torch

    return torch.cuda.stream(st)
