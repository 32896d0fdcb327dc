"""Nine scores of a clustering against the truth that do not depend on how the clusters are numbered, as functions of ONE
integer table, the true-class x predicted-cluster contingency counts of `scores.contingency`.  NumPy, SciPy and the
standard library only.

PARITY PINNED: scikit-learn and SciPy are installed, so tests/test_partition_scores_host.py compares every value with their
calls.  They stay the authority (the host path of mused_amd/metrics_evaluation.py keeps calling them); this module is the
statement of the arithmetic that csrc/score_partitions.hip and the host finish of `compute_partition_metrics` follow.  Line
numbers are scikit-learn 1.7.2's metrics/cluster/_supervised.py unless another file is named:

  ari_score        :443-451 (adjusted_rand_score), :244-259 (pair_confusion_matrix): Python integers
  ami_score        :1030-1062 (adjusted_mutual_info_score), _expected_mutual_info_fast.pyx:12-69
  homogeneity, completeness, v_measure
                   :528-552 (homogeneity_completeness_v_measure, beta = 1), :903-924 (mutual_info_score), :1303-1314 (entropy)
  fowlkes_mallows  :1264-1272: np.int64 values, sqrt(tk / pk) * sqrt(tk / qk)
  purity, inverse_purity
                   the sum of the column (row) maxima over n: no scikit-learn call; one division of exact integers
  matched_accuracy the optimum of scipy.optimize.linear_sum_assignment(table, maximize=True) over n; the optimum VALUE is
                   unique where the assignment is not, so no tie rule enters
"""
from __future__ import annotations

from math import lgamma, log

import numpy as np

from .scores import _entropy, mutual_info

KEYS = ("ari_score", "ami_score", "homogeneity", "completeness", "v_measure", "fowlkes_mallows", "purity", "inverse_purity",
        "matched_accuracy")
_EPS = float(np.finfo(np.float64).eps)   # 2^-52


# ---- values from exact integers ---------------------------------------------------------------------------------------------
def pair_sums(table):
    """(sum n_ij^2, sum a_i^2, sum b_j^2) as Python ints."""
    rows = [[int(v) for v in r] for r in np.asarray(table).tolist()]
    a = [sum(r) for r in rows]
    b = [sum(c) for c in zip(*rows)]
    return sum(v * v for r in rows for v in r), sum(v * v for v in a), sum(v * v for v in b)


def ari_from_sums(sq, sa, sb, n):
    """adjusted_rand_score from the three sums of pair_sums and n (:244-259, :445-451)."""
    sq, sa, sb, n = int(sq), int(sa), int(sb), int(n)
    tp = sq - n
    fp = sb - sq   # contingency.dot(n_k).sum() = sum b_j^2
    fn = sa - sq
    tn = n * n - fp - fn - sq
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def ari(table):
    return ari_from_sums(*pair_sums(table), int(np.asarray(table).sum()))


def fowlkes_mallows_from_sums(sq, sa, sb, n):
    """fowlkes_mallows_score (:1269-1272) from the three sums: np.int64 arithmetic, as there."""
    n = np.int64(n)
    tk, pk, qk = np.int64(sq) - n, np.int64(sb) - n, np.int64(sa) - n
    return float(np.sqrt(tk / pk) * np.sqrt(tk / qk)) if tk != 0.0 else 0.0


def fowlkes_mallows(table):
    return fowlkes_mallows_from_sums(*pair_sums(table), int(np.asarray(table).sum()))


def purity(table):
    table = np.asarray(table, dtype=np.int64)
    return int(table.max(axis=0).sum()) / int(table.sum())


def inverse_purity(table):
    table = np.asarray(table, dtype=np.int64)
    return int(table.max(axis=1).sum()) / int(table.sum())


def matched_total(table):
    """The largest sum of counts a one-to-one matching of classes to clusters reaches (a Python int)."""
    from scipy.optimize import linear_sum_assignment

    table = np.asarray(table, dtype=np.int64)
    rows, cols = linear_sum_assignment(table, maximize=True)
    return int(table[rows, cols].sum())


def matched_accuracy(table):
    return matched_total(table) / int(np.asarray(table).sum())


# ---- values from logarithms -------------------------------------------------------------------------------------------------
def hcv_from(mi, h_true, h_pred):
    """(homogeneity, completeness, v_measure) from MI and the two entropies (:539-552, beta = 1)."""
    homogeneity = mi / h_true if h_true else 1.0
    completeness = mi / h_pred if h_pred else 1.0
    if homogeneity + completeness == 0.0:
        v = 0.0
    else:
        v = (1 + 1.0) * homogeneity * completeness / (1.0 * homogeneity + completeness)
    return float(homogeneity), float(completeness), float(v)


def homogeneity_completeness_v_measure(table):
    table = np.asarray(table, dtype=np.int64)
    return hcv_from(mutual_info(table), _entropy(table.sum(axis=1)), _entropy(table.sum(axis=0)))


def emi(table):
    """(EMI, S_abs, G): expected_mutual_information (_expected_mutual_info_fast.pyx:12-69) term for term and in its order,
    with S_abs = the sum of the absolute values of the terms and G = gammaln(N + 1), which the tests' error bound needs.
    lgamma(m + 1) comes from one table of the C library's values, m = 0 .. N."""
    table = np.asarray(table, dtype=np.int64)
    N = int(table.sum())
    a, b = table.sum(axis=1), table.sum(axis=0)
    LG = np.array([lgamma(m + 1.0) for m in range(N + 1)])
    G = float(LG[N])
    if a.size == 1 or b.size == 1:   # :32
        return 0.0, 0.0, G
    nijs = np.arange(0, max(a.max(), b.max()) + 1, dtype=np.float64)
    nijs[0] = 1
    term1 = nijs / N
    log_a, log_b = np.log(a), np.log(b)
    log_Nnij = log(N) + np.log(nijs)                      # the sum, not log(N * nij)
    gln_a, gln_b, gln_Na, gln_Nb = LG[a], LG[b], LG[N - a], LG[N - b]
    gln_Nnij = LG[: len(nijs)] + LG[N]                    # gammaln(nijs + 1) + gammaln(N + 1); entry 0 is never used
    total, s_abs = 0.0, 0.0
    for i in range(len(a)):
        ai = int(a[i])
        for j in range(len(b)):
            bj = int(b[j])
            start, end = max(1, ai - N + bj), min(ai, bj) + 1
            if end <= start:
                continue
            nij = np.arange(start, end)
            term2 = log_Nnij[nij] - log_a[i] - log_b[j]
            gln = (gln_a[i] + gln_b[j] + gln_Na[i] + gln_Nb[j] - gln_Nnij[nij] - LG[ai - nij] - LG[bj - nij]
                   - LG[N - ai - bj + nij])
            terms = term1[nij] * term2 * np.exp(gln)
            total = float(np.cumsum(np.concatenate(([total], terms)))[-1])   # emi += term, one after the other
            s_abs += float(np.abs(terms).sum())
    return total, s_abs, G


def ami_from(mi, h_true, h_pred, emi_value, T, P):
    """adjusted_mutual_info_score (:1030-1062, arithmetic mean) from its four numbers; T, P: distinct values a side."""
    if T == P == 1 or T == P == 0:
        return 1.0
    if T == 1 or P == 1:
        return 0.0
    normalizer = float(np.mean([h_true, h_pred]))   # :70-82 "arithmetic"
    denominator = normalizer - emi_value
    if denominator < 0:
        denominator = min(denominator, -_EPS)
    else:
        denominator = max(denominator, _EPS)
    numerator = mi - emi_value
    if numerator < 0:
        numerator = min(numerator, -_EPS)
    else:
        numerator = max(numerator, _EPS)
    return float(numerator / denominator)


def ami_parts(table):
    """(mi, h_true, h_pred, emi, S_abs, G, numerator, denominator) of the AMI before the two clamps: the tests' bound."""
    table = np.asarray(table, dtype=np.int64)
    mi, ht, hp = mutual_info(table), _entropy(table.sum(axis=1)), _entropy(table.sum(axis=0))
    e, s_abs, G = emi(table)
    return mi, ht, hp, e, s_abs, G, mi - e, float(np.mean([ht, hp])) - e


def ami(table):
    table = np.asarray(table, dtype=np.int64)
    T, P = table.shape
    if T == 1 or P == 1 or T == 0 or P == 0:
        return ami_from(0.0, 0.0, 0.0, 0.0, T, P)
    mi, ht, hp, e = ami_parts(table)[:4]
    return ami_from(mi, ht, hp, e, T, P)


def scores_from_table(tv, pv, table):
    """The nine values in the order of KEYS, as Python floats."""
    table = np.asarray(table, dtype=np.int64)
    if int(table.sum()) == 0:
        raise ValueError("no samples")
    h, c, v = homogeneity_completeness_v_measure(table)
    return (ari(table), ami(table), h, c, v, fowlkes_mallows(table), purity(table), inverse_purity(table),
            matched_accuracy(table))


def scores(true, pred):
    from .scores import contingency

    return scores_from_table(*contingency(true, pred))
