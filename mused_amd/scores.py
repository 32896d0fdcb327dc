"""The seven numbers of the reference's `metrics_evaluation.compute_all_metrics` (metrics_evaluation.py:47-92) as
functions of ONE integer table, the true-class x predicted-cluster contingency counts.  NumPy only.

PARITY PINNED: scikit-learn is installed, so tests/test_scores_host.py compares every value with the scikit-learn calls the
reference makes.  scikit-learn stays the authority (the host path of mused_amd/metrics_evaluation.py keeps calling it);
this module is the statement of the arithmetic the device kernel (csrc/score.hip) follows.  Line numbers are
scikit-learn 1.7.2's:

  nmi        metrics/cluster/_supervised.py:1147-1174 (normalized_mutual_info_score), :903-924 (mutual_info_score),
             :1303-1314 (entropy), :70-82 (_generalized_average, "arithmetic": np.mean([U, V]))
  f1 / precision / recall
             metrics/_classification.py:2007-2009 (tp_sum, pred_sum, true_sum over unique_labels(y_true, y_pred)),
             :2043-2054 (f = 2 tp / (true_sum + pred_sum)), :1697-1733 (_prf_divide: a zero denominator gives
             zero_division = 0), :2058-2067 (weights = true_sum; _nanaverage = np.average: sum(x * w) / sum(w))
  accuracy   metrics/_classification.py:296 ff. (the mean of y_true == y_pred)
  mae        metrics/_regression.py:289 (the mean of |y_pred - y_true|, int64)
"""
from __future__ import annotations

from math import log

import numpy as np

KEYS = ("f1_score", "nmi_score", "nmi_e_score", "precision", "recall", "accuracy", "mae")
_EPS = float(np.finfo(np.float64).eps)   # 2^-52


def contingency(true, pred):
    """(tv, pv, table): the sorted distinct values of each side as np.unique gives them and the T x P int64 table of
    row counts, table[i, j] = rows with true == tv[i] and pred == pv[j]."""
    t, p = np.asarray(true).ravel(), np.asarray(pred).ravel()
    if t.shape != p.shape:
        raise ValueError(f"inconsistent numbers of samples: {t.shape[0]}, {p.shape[0]}")
    tv, ti = np.unique(t, return_inverse=True)
    pv, pi = np.unique(p, return_inverse=True)
    T, P = len(tv), len(pv)
    table = np.bincount(ti.ravel().astype(np.int64) * P + pi.ravel(), minlength=T * P).reshape(T, P).astype(np.int64)
    return tv, pv, table


def _entropy(counts):
    c = counts[counts > 0].astype(np.float64)
    if c.size == 1:   # a single class
        return 0.0
    s = c.sum()
    return float(-np.sum((c / s) * (np.log(c) - log(s))))


def mutual_info(table):
    """mutual_info_score of a table: the non-zero cells in row-major order."""
    nzx, nzy = np.nonzero(table)
    nz = table[nzx, nzy].astype(np.float64)
    total = nz.sum()
    a, b = table.sum(axis=1), table.sum(axis=0)
    p = nz / total
    outer = a[nzx].astype(np.int64) * b[nzy].astype(np.int64)
    log_outer = -np.log(outer) + log(float(a.sum())) + log(float(b.sum()))
    mi = p * (np.log(nz) - log(total)) + p * log_outer
    mi = np.where(np.abs(mi) < _EPS, 0.0, mi)
    return float(np.clip(mi.sum(), 0.0, None))


def nmi(table):
    """normalized_mutual_info_score (arithmetic mean) of a table without empty rows or columns."""
    T, P = table.shape
    if T == P == 1 or T == P == 0:
        return 1.0
    mi = mutual_info(table)
    if mi == 0:
        return 0.0
    h_true, h_pred = _entropy(table.sum(axis=1)), _entropy(table.sum(axis=0))
    return float(mi / ((h_true + h_pred) / 2.0))


def event_table(tv, table):
    """The rows whose true value is > 0 and the predicted columns those rows reach (metrics_evaluation.py:54-58)."""
    sub = table[np.asarray(tv) > 0]
    return sub[:, sub.sum(axis=0) > 0]


def _union_sums(tv, pv, table):
    """labels (the sorted union), tp, true_sum, pred_sum per label, as int64."""
    tv, pv = np.asarray(tv), np.asarray(pv)
    labels = np.union1d(tv, pv)
    tp, ts, ps = (np.zeros(len(labels), dtype=np.int64) for _ in range(3))
    it, ip = np.searchsorted(labels, tv), np.searchsorted(labels, pv)
    ts[it] = table.sum(axis=1)
    ps[ip] = table.sum(axis=0)
    common, ct, cp = np.intersect1d(tv, pv, return_indices=True)
    tp[np.searchsorted(labels, common)] = table[ct, cp]
    return labels, tp, ts, ps


def _divide(num, den):
    out = np.zeros(len(num), dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)   # zero_division = 0
    return out


def table_info(tv, pv, table):
    """(T, P, size of the union, event rows, agreeing rows): the integers csrc/score.hip reports beside the values."""
    labels, tp, _, _ = _union_sums(tv, pv, table)
    return (len(tv), len(pv), len(labels), int(table[np.asarray(tv) > 0].sum()), int(tp.sum()))


def scores_from_table(tv, pv, table):
    """The seven values in the order of KEYS, as Python floats."""
    tv, pv, table = np.asarray(tv), np.asarray(pv), np.asarray(table, dtype=np.int64)
    n = int(table.sum())
    if n == 0:
        raise ValueError("no samples")
    nmi_all = nmi(table)
    ev = event_table(tv, table)
    nmi_e = nmi(ev) if ev.shape[0] > 1 and ev.shape[1] > 1 else 0.0
    _, tp, ts, ps = _union_sums(tv, pv, table)
    tpf, w = tp.astype(np.float64), ts.astype(np.float64)
    precision, recall, f1 = _divide(tpf, ps.astype(np.float64)), _divide(tpf, w), _divide(2.0 * tpf, w + ps)
    avg = [float(np.multiply(x, w).sum() / w.sum()) for x in (f1, precision, recall)]
    accuracy = float(tp.sum()) / n
    dist = np.abs(tv.astype(np.int64)[:, None] - pv.astype(np.int64)[None, :])
    mae = float((table * dist).sum()) / n
    return (avg[0], nmi_all, nmi_e, avg[1], avg[2], accuracy, mae)


def scores(true, pred):
    return scores_from_table(*contingency(true, pred))
