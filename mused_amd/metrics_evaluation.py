"""Drop-in `metrics_evaluation` (the reference's module of that name): `get_initial_results()` and
`compute_all_metrics(...)` with the same signatures, the same appends to the same lists and the same printed log line.

The seven numbers come from ONE launch of csrc/score.hip (one upload when the labels are on the host, a read of
8 doubles + 8 ints).  Accuracy and MAE are scikit-learn's bits; F1, NMI, NMI_e, precision and recall agree with
scikit-learn within 1e-12 (the rounding of `log` and of the sums).  The host path makes the
reference's own scikit-learn calls.  It runs, and `score_fallbacks` counts it, when MUSED_SCORE=host, when the labels
are not integers, when the lengths differ or the input is empty (scikit-learn raises, and so does this), and when the
kernel raised a flag (a label outside [-1, 65534], more than 4096 distinct values on a side, a table above the cap).

Beside the reference's seven: `compute_partition_metrics` and `partition_windows`, nine scores that do not depend on how the
clusters are numbered (csrc/score_partitions.hip; the rule: mused_amd/partition_scores.py), and the three truth-free indices
of csrc/silhouette.hip.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

from .scores import KEYS

score_fallbacks = 0
_fallback_lock = threading.Lock()
_SCORE_WS = {}
SCORE_FLAG_RANGE, SCORE_FLAG_SIZE = 4, 8
RUN_CELLS_CAP = 1 << 22      # one segment: compute_all_metrics
WINDOW_CELLS_CAP = 1 << 16   # K segments: score_windows
_VARIABLES = ("subset_size", "noise_rate", "label_mode", "sorting", "reduced_dim", "k_basis", "window_size")
# the order in which the reference computes and logs the values
_LOGGED = (("nmi_score", "nmi"), ("nmi_e_score", "nmi_e"), ("f1_score", "f1"), ("precision", "precision"),
           ("recall", "recall"), ("accuracy", "accuracy"), ("mae", "mae"))


def get_initial_results(partition=False):
    """(results, independent_variables): empty lists for the seven metrics, the processing time and the seven
    independent variables of an experiment.  `partition=True` adds the nine lists of PARTITION_KEYS, which
    compute_all_metrics then fills as well."""
    results = {k: [] for k in KEYS + ("processing_time",) + _VARIABLES}
    if partition:
        results.update({k: [] for k in PARTITION_KEYS})
    return results, list(_VARIABLES)


def _count_fallback():
    global score_fallbacks
    with _fallback_lock:
        score_fallbacks += 1


def _to_host(x):
    try:
        import torch

        if isinstance(x, torch.Tensor):
            return x.detach().cpu().numpy()
    except ImportError:
        pass
    return x


def host_scores(true_labels, clusters, keys=KEYS):
    """The reference's scikit-learn calls (metrics_evaluation.py:47-92), for the values named in `keys`."""
    from sklearn import metrics as skm

    true_labels, clusters = _to_host(true_labels), _to_host(clusters)
    out = {}
    for key in keys:
        if key == "nmi_score":
            out[key] = skm.normalized_mutual_info_score(true_labels, clusters)
        elif key == "nmi_e_score":
            events = [i for i, label in enumerate(true_labels) if label > 0]
            te, ce = [true_labels[i] for i in events], [clusters[i] for i in events]
            out[key] = skm.normalized_mutual_info_score(te, ce) if len(set(te)) > 1 and len(set(ce)) > 1 else 0
        elif key == "f1_score":
            out[key] = skm.f1_score(true_labels, clusters, average="weighted", zero_division=0)
        elif key == "precision":
            out[key] = skm.precision_score(true_labels, clusters, average="weighted", zero_division=0)
        elif key == "recall":
            out[key] = skm.recall_score(true_labels, clusters, average="weighted", zero_division=0)
        elif key == "accuracy":
            out[key] = skm.accuracy_score(true_labels, clusters)
        elif key == "mae":
            out[key] = skm.mean_absolute_error(true_labels, clusters)
    return out


def _is_cuda(x):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(x, torch.Tensor) and x.is_cuda


def _device_labels(true_labels, clusters):
    """Both label arrays as int32 CUDA tensors of equal shape, or None when the device cannot take them.  A value outside
    [-2, 65535] is clamped to the nearest of the two, which the kernel flags as out of range all the same."""
    import torch

    sides = [true_labels, clusters]
    host = []
    for i, x in enumerate(sides):
        if isinstance(x, torch.Tensor):
            if x.dtype not in (torch.int32, torch.int64):
                return None
            if not x.is_cuda:
                sides[i] = x.numpy()
        if not isinstance(sides[i], torch.Tensor):
            a = np.asarray(sides[i])
            if a.dtype.kind not in "iu" or a.ndim == 0:
                return None
            sides[i] = a
            host.append(i)
    if tuple(sides[0].shape) != tuple(sides[1].shape) or len(sides[0]) == 0:
        return None
    dev = next((x.device for x in sides if isinstance(x, torch.Tensor)), torch.device("cuda", torch.cuda.current_device()))
    if host:   # one upload for whatever is on the host
        packed = np.stack([np.clip(sides[i], -2, 65535).astype(np.int32) for i in host])
        up = torch.from_numpy(packed).to(dev)
        for row, i in enumerate(host):
            sides[i] = up[row]
    for i, x in enumerate(sides):
        if x.dtype != torch.int32:
            sides[i] = x.clamp(-2, 65535).to(torch.int32)
        sides[i] = sides[i].contiguous()
    return sides[0], sides[1]


def score_labels_on_device(truth_dev, pred_dev, cells_cap, stream=None):
    """mused_score_labels on int32 CUDA tensors of shape (n,) or (K, W): (out (K, 8) float64, info (K, 8) int32) as NumPy
    arrays, after ONE read.  Synchronises the stream."""
    import torch

    from . import _lib
    from . import engine as _eng

    if truth_dev.shape != pred_dev.shape or truth_dev.dtype != torch.int32 or pred_dev.dtype != torch.int32:
        raise ValueError("score_labels_on_device: int32 tensors of equal shape")
    n_seg, seg_len = (1, truth_dev.shape[0]) if truth_dev.dim() == 1 else tuple(truth_dev.shape)
    dev = truth_dev.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    need = int(_lib.lib().mused_score_ws_bytes(n_seg, cells_cap))
    with torch.cuda.stream(st):
        key = (dev, st.cuda_stream)
        ws = _SCORE_WS.get(key)
        if ws is None or ws.numel() < need:
            if len(_SCORE_WS) > 16:
                _SCORE_WS.clear()
            ws = _SCORE_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        res = torch.empty(n_seg * 96, dtype=torch.uint8, device=dev)   # 8 doubles, then 8 ints per segment
        out, info = res[: n_seg * 64], res[n_seg * 64 :]
        truth_dev, pred_dev = truth_dev.contiguous(), pred_dev.contiguous()
        _lib.call("mused_score_labels", _eng.ptr(truth_dev), _eng.ptr(pred_dev), n_seg, seg_len, int(cells_cap),
                  _eng.ptr(out), _eng.ptr(info), _eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
        res_h = res.cpu().numpy()
    return (res_h[: n_seg * 64].view(np.float64).reshape(n_seg, 8).copy(),
            res_h[n_seg * 64 :].view(np.int32).reshape(n_seg, 8).copy())


def _want_host():
    return os.environ.get("MUSED_SCORE", "").lower() == "host"


def seven_scores(true_labels, clusters, keys=KEYS):
    """{key: value} for the metrics named in `keys`: the device path, or the host path (counted) in the cases the
    module's docstring lists."""
    if not _want_host():
        labels = _device_labels(true_labels, clusters)
        if labels is not None:
            out, info = score_labels_on_device(labels[0], labels[1], RUN_CELLS_CAP)
            if info[0, 5] == 0:
                return {k: float(out[0, i]) for i, k in enumerate(KEYS) if k in keys}
    _count_fallback()
    return host_scores(true_labels, clusters, keys)


def score_windows(true_kw, pred_kw):
    """K x W label arrays (lists, NumPy, int32 / int64 CUDA tensors) scored as K segments in ONE launch: a (K, 7) float64
    array in the order of scores.KEYS.  A flagged window is scored on the host (and counted)."""
    labels = None
    if not _want_host():
        t2, p2 = (x if _is_cuda(x) else np.asarray(_to_host(x)) for x in (true_kw, pred_kw))
        if t2.ndim != 2 or tuple(t2.shape) != tuple(p2.shape):
            raise ValueError("score_windows: two K x W label arrays of equal shape")
        labels = _device_labels(t2, p2)
    if labels is None:
        th, ph = np.asarray(_to_host(true_kw)), np.asarray(_to_host(pred_kw))
        res = np.empty((len(th), 7))
        for k in range(len(th)):
            _count_fallback()
            h = host_scores(th[k], ph[k])
            res[k] = [h[key] for key in KEYS]
        return res
    out, info = score_labels_on_device(labels[0], labels[1], WINDOW_CELLS_CAP)
    res = out[:, :7].copy()
    flagged = np.flatnonzero(info[:, 5])
    if len(flagged):
        th, ph = np.asarray(_to_host(true_kw)), np.asarray(_to_host(pred_kw))
        for k in flagged:
            _count_fallback()
            h = host_scores(th[k], ph[k])
            res[k] = [h[key] for key in KEYS]
    return res


def compute_all_metrics(results, subset_size, noise_rate, label_mode, sorting, reduced_dim, k_basis, window_size, clusters,
                        true_labels, end_time, start_time):
    """The reference's compute_all_metrics: appends the independent variables, then every metric whose list `results`
    holds, then the processing time (ns -> s); prints the reference's log line; returns `results`."""
    given = (subset_size, noise_rate, label_mode, sorting, reduced_dim, k_basis, window_size)
    for name, value in zip(_VARIABLES, given):
        results[name].append(value)
    wanted = tuple(k for k in KEYS if k in results)
    values = seven_scores(true_labels, clusters, wanted) if wanted else {}
    parts = []
    for key, short in _LOGGED:
        if key in results:
            results[key].append(values[key])
            parts.append(f"{short}={values[key]:.2f}, ")
    if any(k in results for k in PARTITION_KEYS):   # the nine partition scores, after the seven
        values = compute_partition_metrics(true_labels, clusters)
        for key, short in _PARTITION_LOGGED:
            if key in results:
                results[key].append(values[key])
                parts.append(f"{short}={values[key]:.2f}, ")
    if "processing_time" in results:
        processing_time = (end_time - start_time) / 1e9
        results["processing_time"].append(processing_time)
        print(f"processing_time={processing_time}")
        parts.append(f"processing_time={processing_time:.2f}")
    print("".join(parts))
    return results


# ---- scores without ground truth: silhouette, Davies-Bouldin, Calinski-Harabasz (csrc/silhouette.hip) -------------------
INTERNAL_KEYS = ("silhouette", "davies_bouldin", "calinski_harabasz")
INTERNAL_MAX_ROWS = 1 << 19   # csrc/silhouette.hip: what the tile grid of dbscan.hip holds, the limit of every tile kernel
_INTERNAL_WS = {}


def _internal_stream(X, stream, wait_current=True):
    """The stream the kernels and every conversion of their inputs run on: the caller's, behind whatever the current stream
    holds (tensor arguments) unless `wait_current` is off, or the current one."""
    import torch

    dev = X.device if isinstance(X, torch.Tensor) and X.is_cuda else torch.device("cuda", torch.cuda.current_device())
    cur = torch.cuda.current_stream(dev)
    if stream is None:
        return cur
    if wait_current:
        stream.wait_stream(cur)
    return stream


def _internal_inputs(X, labels):
    """(X as an (n, d) fp64 CUDA tensor with unit column stride, labels as n int32 CUDA) for the kernels; uploads and
    conversions run on the current stream (the caller has entered the kernels' stream)."""
    import torch

    if isinstance(X, torch.Tensor):
        Xd = X if X.is_cuda else X.cuda()
    else:
        a = np.asarray(X)
        if a.dtype.kind not in "fiub":
            raise ValueError("X must be numeric")
        Xd = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    if Xd.dim() != 2 or Xd.shape[0] < 1 or Xd.shape[1] < 1:
        raise ValueError("X must be (n, d) with n, d >= 1")
    if Xd.dtype != torch.float64:
        Xd = Xd.to(torch.float64)
    if Xd.stride(1) != 1 or Xd.stride(0) < Xd.shape[1]:
        Xd = Xd.contiguous()
    if isinstance(labels, torch.Tensor):
        if labels.dtype not in (torch.int32, torch.int64):
            raise ValueError("labels must be integers")
        ld = labels.to(Xd.device)
    else:
        a = np.asarray(labels)
        if a.dtype.kind not in "iu" or (a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31)):
            raise ValueError("labels must be int32 values")
        ld = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(Xd.device)
    if tuple(ld.shape) != (Xd.shape[0],):
        raise ValueError(f"labels must be {Xd.shape[0]} integers, got shape {tuple(ld.shape)}")
    if Xd.shape[0] > INTERNAL_MAX_ROWS or Xd.shape[1] >= 1 << 20:
        raise ValueError(f"{Xd.shape[0]} x {Xd.shape[1]} rows: the device indices take at most 2^19 rows "
                         "(MUSED_SCORE=host scores any size with scikit-learn)")
    return Xd, ld.to(torch.int32).contiguous()


def _internal_ws(kind, need, dev, st):
    import torch

    key = (kind, dev, st.cuda_stream)
    ws = _INTERNAL_WS.get(key)
    if ws is None or ws.numel() < need:
        if len(_INTERNAL_WS) > 16:
            _INTERNAL_WS.clear()
        ws = _INTERNAL_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws


def silhouette_launch(Xd, labels_d, st, samples=None, info=None):
    """mused_silhouette enqueued on stream `st` (entered by the caller): (samples n fp64 CUDA, info 16 bytes CUDA = {int32
    flags, int32 clusters, fp64 sum of the samples}).  Nothing is read."""
    import torch

    from . import _lib
    from . import engine as _eng

    n, d = Xd.shape
    ws = _internal_ws("sil", int(_lib.lib().mused_silhouette_ws_bytes(n, d)), Xd.device, st)
    if samples is None:
        samples = torch.empty(n, dtype=torch.float64, device=Xd.device)
    if info is None:
        info = torch.empty(16, dtype=torch.uint8, device=Xd.device)
    _lib.call("mused_silhouette", _eng.ptr(Xd), n, d, Xd.stride(0), _eng.ptr(labels_d), _eng.ptr(samples), _eng.ptr(info),
              _eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
    return samples, info


def _raise_flags(flags, clusters, Xd):
    """A flag of csrc/silhouette.hip as scikit-learn's ValueError (the non-finite check comes first there too)."""
    import torch

    from . import silhouette as _sil

    if flags & _sil.FLAG_NONFINITE:
        raise _sil.nonfinite_error(bool(torch.isnan(Xd).any().item()))
    if flags & _sil.FLAG_LABELS:
        raise _sil.labels_error(int(clusters))


def _host_internal(X, labels):
    from sklearn import metrics as skm

    X, labels = np.asarray(_to_host(X)), np.asarray(_to_host(labels))
    return {"silhouette": float(skm.silhouette_score(X, labels, metric="euclidean")),
            "davies_bouldin": float(skm.davies_bouldin_score(X, labels)),
            "calinski_harabasz": float(skm.calinski_harabasz_score(X, labels))}


def silhouette_samples_on_device(X, labels, stream=None):
    """sklearn.metrics.silhouette_samples(X, labels, metric="euclidean") as an n fp64 CUDA tensor (csrc/silhouette.hip; the
    rule: mused_amd/silhouette.py).  X: (n, d) NumPy array or tensor (taken as fp64), labels: n integers, NumPy or tensor;
    any int32 value is a cluster id and -1 is a cluster like any other -- mask noise rows yourself.  Raises scikit-learn's
    ValueError for a non-finite row and for fewer than 2 or more than n - 1 distinct labels (the call reads the flags, so
    it returns after the stream has finished).  MUSED_SCORE=host: scikit-learn on host copies, uploaded."""
    import torch

    if _want_host():
        from sklearn import metrics as skm

        s = skm.silhouette_samples(np.asarray(_to_host(X)), np.asarray(_to_host(labels)), metric="euclidean")
        return torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64)).cuda()
    st = _internal_stream(X, stream)
    with torch.cuda.stream(st):
        Xd, ld = _internal_inputs(X, labels)
        samples, info = silhouette_launch(Xd, ld, st)
        head = info.cpu().numpy()[:8].view(np.int32)
    _raise_flags(int(head[0]), int(head[1]), Xd)
    return samples


def internal_metrics_raw(X, labels, stream=None, indices=True, wait_current=True):
    """Both kernels of csrc/silhouette.hip and ONE read: (flags, clusters, silhouette score, Davies-Bouldin,
    Calinski-Harabasz, the device X).  With a flag the three numbers are NaN; `indices=False` runs the silhouette alone.
    `wait_current=False`: `stream` does not wait for the current stream -- for callers whose tensors are already complete
    for it (the pipeline's label workers, like perform_clustering_on_device)."""
    import torch

    from . import _lib
    from . import engine as _eng

    st = _internal_stream(X, stream, wait_current)
    with torch.cuda.stream(st):
        Xd, ld = _internal_inputs(X, labels)
        n, d = Xd.shape
        res = torch.zeros(48, dtype=torch.uint8, device=Xd.device)   # silhouette info | {DB, CH} | indices info
        silhouette_launch(Xd, ld, st, info=res[:16])
        if indices:
            ws = _internal_ws("idx", int(_lib.lib().mused_cluster_indices_ws_bytes(n, d)), Xd.device, st)
            _lib.call("mused_cluster_indices", _eng.ptr(Xd), n, d, Xd.stride(0), _eng.ptr(ld), _eng.ptr(res[16:32]),
                      _eng.ptr(res[32:]), _eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
        h = res.cpu().numpy()
    flags, clusters = (int(v) for v in h[:8].view(np.int32))
    if flags:
        return flags, clusters, float("nan"), float("nan"), float("nan"), Xd
    db, ch = (float(v) for v in h[16:32].view(np.float64)) if indices else (float("nan"), float("nan"))
    return flags, clusters, float(h[8:16].view(np.float64)[0]) / n, db, ch, Xd


def compute_internal_metrics(X, labels, stream=None):
    """{"silhouette", "davies_bouldin", "calinski_harabasz"} of a clustering as Python floats, without ground truth:
    scikit-learn's silhouette_score(metric="euclidean"), davies_bouldin_score and calinski_harabasz_score from
    csrc/silhouette.hip (the rules and conventions: mused_amd/silhouette.py; the error bound: DESIGN section 20).
    X: (n, d) NumPy array or tensor, n <= 2^19 on the device; labels: n integers.  Any int32 value is a cluster id, -1
    included: callers that treat -1 as noise mask those rows themselves.  A non-finite row and a label count outside
    [2, n - 1] raise scikit-learn's ValueError.  MUSED_SCORE=host: scikit-learn's three calls on host copies."""
    if _want_host():
        return _host_internal(X, labels)
    flags, clusters, s, db, ch, Xd = internal_metrics_raw(X, labels, stream)
    _raise_flags(flags, clusters, Xd)
    return {"silhouette": s, "davies_bouldin": db, "calinski_harabasz": ch}


# ---- scores against the truth that ignore how clusters are numbered (csrc/score_partitions.hip) ---------------------------
# ARI, AMI, homogeneity / completeness / V-measure, Fowlkes-Mallows, purity, inverse purity and the accuracy under the best
# one-to-one matching of clusters to classes.  The rule: mused_amd/partition_scores.py; the bounds: DESIGN section 21.
from . import partition_scores as _ps  # noqa: E402
from .partition_scores import KEYS as PARTITION_KEYS  # noqa: E402

partition_fallbacks = 0
PARTITION_FLAG_NO_EMI = 64           # the kernel left the EMI out (csrc/score_partitions.hip): only AMI goes to the host
PARTITION_MATCH_MAX_LEN = 1 << 20    # the wide solver's window length (matrix_operations.MATCH_WIDE_MAX_W)
_PARTITION_WS = {}
_PARTITION_LOGGED = (("ari_score", "ari"), ("ami_score", "ami"), ("homogeneity", "homogeneity"), ("completeness", "completeness"),
                     ("v_measure", "v_measure"), ("fowlkes_mallows", "fowlkes_mallows"), ("purity", "purity"),
                     ("inverse_purity", "inverse_purity"), ("matched_accuracy", "matched_accuracy"))


def _count_partition_fallback():
    global partition_fallbacks
    with _fallback_lock:
        partition_fallbacks += 1


def host_partition_scores(true_labels, clusters, keys=PARTITION_KEYS):
    """The nine values from scikit-learn's and SciPy's calls on host copies, for the values named in `keys`."""
    from scipy.optimize import linear_sum_assignment
    from sklearn import metrics as skm
    from sklearn.metrics.cluster import contingency_matrix

    true_labels, clusters = np.asarray(_to_host(true_labels)), np.asarray(_to_host(clusters))
    out = {}
    if "ari_score" in keys:
        out["ari_score"] = float(skm.adjusted_rand_score(true_labels, clusters))
    if "ami_score" in keys:
        out["ami_score"] = float(skm.adjusted_mutual_info_score(true_labels, clusters))
    if any(k in keys for k in ("homogeneity", "completeness", "v_measure")):
        h, c, v = skm.homogeneity_completeness_v_measure(true_labels, clusters)
        out.update({k: x for k, x in (("homogeneity", h), ("completeness", c), ("v_measure", v)) if k in keys})
    if "fowlkes_mallows" in keys:
        out["fowlkes_mallows"] = float(skm.fowlkes_mallows_score(true_labels, clusters))
    if any(k in keys for k in ("purity", "inverse_purity", "matched_accuracy")):
        table = contingency_matrix(true_labels, clusters).astype(np.int64)
        n = int(table.sum())
        if n == 0:
            raise ValueError("no samples")
        rows, cols = linear_sum_assignment(table, maximize=True)
        own = {"purity": int(table.max(axis=0).sum()) / n, "inverse_purity": int(table.max(axis=1).sum()) / n,
               "matched_accuracy": int(table[rows, cols].sum()) / n}
        out.update({k: x for k, x in own.items() if k in keys})
    return {k: out[k] for k in PARTITION_KEYS if k in out}


def partition_scores_on_device(truth_dev, pred_dev, cells_cap, want_emi=True, want_table=True, stream=None):
    """mused_score_partitions on int32 CUDA tensors of shape (n,) or (K, W): (out (K, 8) float64, ints (K, 8) int64, info
    (K, 8) int32 as NumPy arrays after ONE read, the tables as a (K, cells) int32 CUDA tensor or None).  `cells` is cells_cap,
    or seg_len^2 where that is smaller (no table is larger).  Synchronises the stream."""
    import torch

    from . import _lib
    from . import engine as _eng

    if truth_dev.shape != pred_dev.shape or truth_dev.dtype != torch.int32 or pred_dev.dtype != torch.int32:
        raise ValueError("partition_scores_on_device: int32 tensors of equal shape")
    n_seg, seg_len = (1, truth_dev.shape[0]) if truth_dev.dim() == 1 else tuple(truth_dev.shape)
    cells = int(min(cells_cap, seg_len * seg_len))
    dev = truth_dev.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    need = int(_lib.lib().mused_score_partitions_ws_bytes(n_seg, seg_len, cells))
    with torch.cuda.stream(st):
        key = (dev, st.cuda_stream)
        ws = _PARTITION_WS.get(key)
        if ws is None or ws.numel() < need:
            if len(_PARTITION_WS) > 16:
                _PARTITION_WS.clear()
            ws = _PARTITION_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        res = torch.empty(n_seg * 160, dtype=torch.uint8, device=dev)   # 8 doubles, 8 int64, 8 int32 per segment
        out, ints, info = res[: n_seg * 64], res[n_seg * 64 : n_seg * 128], res[n_seg * 128 :]
        tables = torch.empty((n_seg, cells), dtype=torch.int32, device=dev) if want_table else None
        truth_dev, pred_dev = truth_dev.contiguous(), pred_dev.contiguous()
        _lib.call("mused_score_partitions", _eng.ptr(truth_dev), _eng.ptr(pred_dev), n_seg, seg_len, cells, 1 if want_emi else 0,
                  _eng.ptr(out), _eng.ptr(ints), _eng.ptr(info), _eng.ptr(tables) if want_table else None, _eng.ptr(ws),
                  ws.numel(), C.c_void_p(st.cuda_stream))
        res_h = res.cpu().numpy()
    return (res_h[: n_seg * 64].view(np.float64).reshape(n_seg, 8).copy(),
            res_h[n_seg * 64 : n_seg * 128].view(np.int64).reshape(n_seg, 8).copy(),
            res_h[n_seg * 128 :].view(np.int32).reshape(n_seg, 8).copy(), tables)


def _matched_total(truth_seg, pred_seg, table_seg, T, P, stream):
    """The optimum of the assignment problem on one segment's T x P table (`table_seg`: its cells on the device): the wide
    Hungarian solver with the truth as the previous window and min_overlap 0 (every count is a finite cost), the table summed
    over the assigned cells.  A solve the solver flags, and a segment longer than its window limit, take SciPy on a host copy
    of the table (counted)."""
    import torch

    from . import matrix_operations as mo

    tab = table_seg[: T * P].view(T, P)
    if truth_seg.shape[0] <= PARTITION_MATCH_MAX_LEN:
        _, info_h, assign = mo.match_wide_launch(pred_seg.view(1, -1), truth_seg, 0, stream=stream, want_assign=True)
        if info_h[0, 4] == 0 and info_h[0, 3] == 1 and info_h[0, 0] == T and info_h[0, 1] == P:
            with torch.cuda.stream(stream):
                col = assign[0, :T].to(torch.int64)
                picked = tab.gather(1, col.clamp(min=0).unsqueeze(1)).squeeze(1).to(torch.int64)
                return int((picked * (col >= 0)).sum().item())
    _count_partition_fallback()
    return _ps.matched_total(tab.cpu().numpy())


def _finish_partition(out, ints, info):
    """The values of one unflagged segment but the matched accuracy, finished with the rule's own expressions: Python ints and
    np.int64 for the integer-derived ones (scikit-learn's bits), scikit-learn's order of operations for the rest.  `ami_score`
    is None where the kernel left the EMI out (flag 64)."""
    mi, ht, hp, e = (float(v) for v in out[:4])
    sq, sa, sb, cmax, rmax, _, n = (int(v) for v in ints[:7])
    T, P, flags = (int(v) for v in info[:3])
    h, c, v = _ps.hcv_from(mi, ht, hp)
    no_emi = bool(flags & PARTITION_FLAG_NO_EMI) and T > 1 and P > 1
    return {"ari_score": _ps.ari_from_sums(sq, sa, sb, n), "ami_score": None if no_emi else _ps.ami_from(mi, ht, hp, e, T, P),
            "homogeneity": h, "completeness": c, "v_measure": v, "fowlkes_mallows": _ps.fowlkes_mallows_from_sums(sq, sa, sb, n),
            "purity": cmax / n, "inverse_purity": rmax / n}


def _partition_segment(k, labels, out, ints, info, tables, stream, host_labels):
    """The nine values of segment k of a device result as a dict in the order of PARTITION_KEYS; `host_labels()` gives the
    (truth, clusters) of the segment on the host for what the device left out."""
    if info[k, 2] & (SCORE_FLAG_RANGE | SCORE_FLAG_SIZE):
        _count_partition_fallback()
        return host_partition_scores(*host_labels())
    vals = _finish_partition(out[k], ints[k], info[k])
    if vals["ami_score"] is None:
        _count_partition_fallback()
        vals["ami_score"] = host_partition_scores(*host_labels(), keys=("ami_score",))["ami_score"]
    t2, p2 = (x.view(len(info), -1) for x in labels)
    total = _matched_total(t2[k], p2[k], tables[k], int(info[k, 0]), int(info[k, 1]), stream)
    vals["matched_accuracy"] = total / int(ints[k, 6])
    return {key: vals[key] for key in PARTITION_KEYS}


def compute_partition_metrics(true_labels, clusters, stream=None):
    """{key: value} for the nine PARTITION_KEYS as Python floats: adjusted Rand index, adjusted mutual information
    (arithmetic mean), homogeneity, completeness, V-measure, Fowlkes-Mallows, purity, inverse purity and the accuracy under
    the best one-to-one matching of clusters to classes.  None depends on how either side numbers its groups.
    true_labels, clusters: lists, NumPy arrays or int32 / int64 CUDA tensors of equal length.  One launch group of
    csrc/score_partitions.hip and one read; the integer-derived values (ARI, Fowlkes-Mallows, the purities, the matched
    accuracy) are scikit-learn's and SciPy's bits, the others agree within the bounds of DESIGN section 21.  The matching is
    the wide Hungarian solver's (csrc/match_wide.hip).  The host path (scikit-learn and SciPy, counted in
    `partition_fallbacks`) runs when MUSED_SCORE=host, when the labels are not integers, when the lengths differ or the
    input is empty (scikit-learn raises, and so does this) and when the kernel raised flag 4 or 8; with flag 64 only
    `ami_score` comes from scikit-learn."""
    if not _want_host():
        import torch

        labels = None
        dev = next((x.device for x in (true_labels, clusters) if _is_cuda(x)), None)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            labels = _device_labels(true_labels, clusters)
        if labels is not None and labels[0].dim() == 1:
            out, ints, info, tables = partition_scores_on_device(labels[0], labels[1], RUN_CELLS_CAP, stream=st)
            return _partition_segment(0, labels, out, ints, info, tables, st, lambda: (true_labels, clusters))
    _count_partition_fallback()
    return host_partition_scores(true_labels, clusters)


def partition_windows(true_kw, pred_kw):
    """K x W label arrays (lists, NumPy, int32 / int64 CUDA tensors) scored as K segments of one launch group: a (K, 9) float64
    array in the order of PARTITION_KEYS.  The matched accuracy takes one solver call per window.  A flagged window is scored
    on the host (and counted)."""
    labels = None
    if not _want_host():
        t2, p2 = (x if _is_cuda(x) else np.asarray(_to_host(x)) for x in (true_kw, pred_kw))
        if t2.ndim != 2 or tuple(t2.shape) != tuple(p2.shape):
            raise ValueError("partition_windows: two K x W label arrays of equal shape")
        labels = _device_labels(t2, p2)
    th, ph = None, None

    def host_pair(k):
        nonlocal th, ph
        if th is None:
            th, ph = np.asarray(_to_host(true_kw)), np.asarray(_to_host(pred_kw))
        return th[k], ph[k]

    if labels is None:
        K = len(np.asarray(_to_host(true_kw)))
        res = np.empty((K, len(PARTITION_KEYS)))
        for k in range(K):
            _count_partition_fallback()
            h = host_partition_scores(*host_pair(k))
            res[k] = [h[key] for key in PARTITION_KEYS]
        return res
    import torch

    st = torch.cuda.current_stream(labels[0].device)
    out, ints, info, tables = partition_scores_on_device(labels[0], labels[1], WINDOW_CELLS_CAP, stream=st)
    res = np.empty((len(info), len(PARTITION_KEYS)))
    for k in range(len(info)):
        vals = _partition_segment(k, labels, out, ints, info, tables, st, lambda k=k: host_pair(k))
        res[k] = [vals[key] for key in PARTITION_KEYS]
    return res
