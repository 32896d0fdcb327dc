"""Inputs, references and bounds shared by the partition-score tests (host and GPU).

Reference: scikit-learn 1.7.2 and SciPy on host copies.  Contract:
  equal bits      ari_score, fowlkes_mallows, purity, inverse_purity, matched_accuracy (exact integers, finished on the host)
  1e-12 absolute  homogeneity, completeness, v_measure: the project's bound for NMI, the same MI and entropy arithmetic
  EMI             |x - sklearn| <= 16 * 2^-52 * (G * S_abs + log N), G = gammaln(N + 1), S_abs = sum of |terms| (the rule's)
  ami_score       (tol_MI + tol_EMI) / |den| + |num| * (tol_H + tol_EMI) / den^2 with tol_MI = tol_H = 1e-12 and den, num
                  from the rule; the inputs of this bound have den >= 1e-3; the degenerate inputs are asserted on 1.0 and 0.0
"""
import functools
from math import log

import numpy as np

KEYS = ("ari_score", "ami_score", "homogeneity", "completeness", "v_measure", "fowlkes_mallows", "purity", "inverse_purity",
        "matched_accuracy")
EXACT = ("ari_score", "fowlkes_mallows", "purity", "inverse_purity", "matched_accuracy")
TOL = 1e-12
EPS = 2.0 ** -52
EMI_FACTOR = 16.0


def _random(n, T, P, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, T, n), rng.integers(0, P, n)


def _skewed(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(n) >= 0.95).astype(np.int64), rng.integers(0, 2, n)


def _identical(n, T, seed):
    t = np.random.default_rng(seed).integers(0, T, n)
    return t, t.copy()


def _edge_values(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice([-1, 0, 7, 65534], n), rng.choice([-1, 3, 65534], n)


def _high_overlap():
    # a 2 x 2 table with a_0 + b_0 > N: rows (9, 1), columns (8, 2) at N = 10, so nij of cell (0, 0) starts at 7
    t = np.array([0] * 9 + [1])
    p = np.array([0] * 8 + [1] * 2)
    return t, p


# name -> (builder, degenerate AMI value or None)
CASES = {
    "rand_300_3x5": (lambda: _random(300, 3, 5, 1), None),
    "rand_2000_4x4": (lambda: _random(2000, 4, 4, 2), None),
    "rand_2000_40x37": (lambda: _random(2000, 40, 37, 3), None),
    "rand_5000_150x150": (lambda: _random(5000, 150, 150, 4), None),
    "skew_4096_2x2": (lambda: _skewed(4096, 5), None),
    "identical_1000_6": (lambda: _identical(1000, 6, 6), None),
    "identical_257_40": (lambda: _identical(257, 40, 7), None),
    "one_class_7_clusters": (lambda: (np.zeros(700, dtype=np.int64), _random(700, 1, 7, 8)[1]), 0.0),
    "7_classes_one_cluster": (lambda: (_random(700, 7, 1, 9)[0], np.full(700, 3)), 0.0),
    "both_single": (lambda: (np.full(50, 2), np.full(50, 9)), 1.0),
    "n2_all_distinct": (lambda: (np.array([0, 1]), np.array([5, 4])), None),
    "edge_values": (lambda: _edge_values(1500, 10), None),
    "high_overlap_2x2": (_high_overlap, None),
    "rand_400_5x9": (lambda: _random(400, 5, 9, 11), None),
    "rand_400_9x5": (lambda: _random(400, 9, 5, 12), None),
    "rand_1000_2x60": (lambda: _random(1000, 2, 60, 13), None),
    "blocks_3000_12x10": (lambda: (np.arange(3000) // 250, np.arange(3000) // 300), None),
    "noisy_copy_2000_8": (lambda: (lambda t, r: (t, np.where(r.random(2000) < 0.2, r.integers(0, 8, 2000), (t + 3) % 8)))(
        _random(2000, 8, 8, 14)[0], np.random.default_rng(15)), None),
    "rand_1_1x1": (lambda: (np.array([4]), np.array([0])), 1.0),
    "rand_3_2x3": (lambda: (np.array([0, 1, 1]), np.array([2, 1, 0])), None),
    "rand_257_3x4": (lambda: _random(257, 3, 4, 16), None),
    "rand_3000_150x150": (lambda: _random(3000, 150, 150, 17), None),   # 22,500 cells: the largest table kept in LDS is 24,576
    "rand_3000_160x160": (lambda: _random(3000, 160, 160, 18), None),   # 25,600 cells: the table lives in the workspace
    "rand_5_2x2": (lambda: (np.array([0, 1, 1, 0, 1]), np.array([1, 1, 0, 0, 1])), None),
}
CASE_NAMES = list(CASES)
# n = 2 with all labels distinct: MI = H = EMI = log 2 analytically, so num = den = 0 and scikit-learn's value is the quotient of
# its two +-eps clamps, +1 or -1 by the sign of a rounding error.  The AMI bound needs |den| >= 1e-3, which every other
# non-degenerate input satisfies (asserted); here the AMI is only required to be finite, and its four doubles keep their bounds.
DEN_ZERO = ("n2_all_distinct",)


@functools.lru_cache(maxsize=None)
def case(name):
    t, p = CASES[name][0]()
    t, p = np.asarray(t, dtype=np.int64), np.asarray(p, dtype=np.int64)
    t.setflags(write=False)
    p.setflags(write=False)
    return t, p


def sklearn_values(true, pred):
    """The nine values in the order of KEYS from scikit-learn and SciPy, and scikit-learn's EMI."""
    from scipy.optimize import linear_sum_assignment
    from sklearn import metrics as skm
    from sklearn.metrics.cluster import contingency_matrix, expected_mutual_information

    table = contingency_matrix(true, pred).astype(np.int64)
    n = int(table.sum())
    h, c, v = skm.homogeneity_completeness_v_measure(true, pred)
    rows, cols = linear_sum_assignment(table, maximize=True)
    vals = (float(skm.adjusted_rand_score(true, pred)), float(skm.adjusted_mutual_info_score(true, pred)), h, c, v,
            float(skm.fowlkes_mallows_score(true, pred)), int(table.max(axis=0).sum()) / n, int(table.max(axis=1).sum()) / n,
            int(table[rows, cols].sum()) / n)
    return vals, float(expected_mutual_information(contingency_matrix(true, pred, sparse=True), n))


@functools.lru_cache(maxsize=None)
def reference(name):
    return sklearn_values(*case(name))


@functools.lru_cache(maxsize=None)
def rule_parts(name):
    """(mi, h_true, h_pred, emi, S_abs, G, num, den) of the rule for the case."""
    from mused_amd import partition_scores as ps
    from mused_amd import scores

    return ps.ami_parts(scores.contingency(*case(name))[2])


def emi_tolerance(s_abs, G, n):
    return EMI_FACTOR * EPS * (G * s_abs + log(n))


def ami_tolerance(parts, n):
    _, _, _, _, s_abs, G, num, den = parts
    tol_emi = emi_tolerance(s_abs, G, n)
    return (TOL + tol_emi) / abs(den) + abs(num) * (TOL + tol_emi) / den ** 2


def check_nine(got, name, what):
    """`got`: the nine values in the order of KEYS, against scikit-learn under the contract."""
    want, _ = reference(name)
    got = [float(x) for x in got]
    n = len(case(name)[0])
    for i, key in enumerate(KEYS):
        print(f"{what} {name} {key}: got {got[i]!r} want {want[i]!r} diff {abs(got[i] - want[i]):.3e}")
    for i, key in enumerate(KEYS):
        if key in EXACT:
            assert got[i] == want[i], (name, key, got[i], want[i])
        elif key == "ami_score":
            special = CASES[name][1]
            T, P = (len(np.unique(x)) for x in case(name))
            if special is not None:
                assert got[i] == special == want[i], (name, key, got[i], want[i])
            elif T < 2 or P < 2:
                assert got[i] == want[i], (name, key, got[i], want[i])
            else:
                parts = rule_parts(name)
                if name in DEN_ZERO:
                    assert abs(parts[7]) < 1e-3 and np.isfinite(got[i]), (name, key, got[i], parts[7])
                    continue
                assert abs(parts[7]) >= 1e-3, (name, "den", parts[7])
                tol = ami_tolerance(parts, n)
                print(f"{what} {name} ami tolerance {tol:.3e}")
                assert abs(got[i] - want[i]) <= tol, (name, key, got[i], want[i], tol)
        else:
            assert abs(got[i] - want[i]) <= TOL, (name, key, got[i], want[i])
