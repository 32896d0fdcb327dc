"""Drop-in `metrics_evaluation` (the reference's module of that name): `get_initial_results()` and
`compute_all_metrics(...)` with the same signatures, the same appends to the same lists and the same printed log line.

The seven numbers come from ONE launch of csrc/score.hip (one upload when the labels are on the host, a read of
8 doubles + 8 ints).  Accuracy and MAE are scikit-learn's bits; F1, NMI, NMI_e, precision and recall agree with
scikit-learn within 1e-12 (the rounding of `log` and of the sums).  The host path makes the
reference's own scikit-learn calls.  It runs, and `score_fallbacks` counts it, when MUSED_SCORE=host, when the labels
are not integers, when the lengths differ or the input is empty (scikit-learn raises, and so does this), and when the
kernel raised a flag (a label outside [-1, 65534], more than 4096 distinct values on a side, a table above the cap).
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


def get_initial_results():
    """(results, independent_variables): empty lists for the seven metrics, the processing time and the seven
    independent variables of an experiment."""
    results = {k: [] for k in KEYS + ("processing_time",) + _VARIABLES}
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
    if "processing_time" in results:
        processing_time = (end_time - start_time) / 1e9
        results["processing_time"].append(processing_time)
        print(f"processing_time={processing_time}")
        parts.append(f"processing_time={processing_time:.2f}")
    print("".join(parts))
    return results
