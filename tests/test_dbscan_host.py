"""mused_amd/dbscan.py -- the closed-form rule csrc/dbscan.hip implements -- against sklearn.cluster.DBSCAN, and the
ambiguity margin tau against the margins the inputs really have (no GPU)."""
import numpy as np
import pytest

import dbscan_cases as dc
from mused_amd import dbscan as spec


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.slow) if n.startswith("centres") else n
                                  for n in dc.CASE_NAMES])
def test_rule_equals_sklearn(name):
    _, X, eps, ms, _ = dc.case(name)
    want = dc.sklearn_labels(name)
    scan = spec.Scan(X, eps)   # one pass over the pairs for the labels and the margins
    got = spec.dbscan_labels(X, eps, ms, scan=scan)
    assert got.dtype == np.int64
    assert np.array_equal(got, want)
    # tau stays below the smallest |d2 - eps^2| of the input: nothing here is decided by rounding
    print(f"{name}: margin {scan.margin:.3e} tau {scan.tau:.3e}")
    assert scan.tau < scan.margin
    assert not scan.ambiguous


def test_bridge_row_takes_the_lower_label_in_both_orders():
    for name in ("bridge_ab", "bridge_ba"):
        lab = dc.sklearn_labels(name)
        assert lab[10] == 0 and set(lab[:10]) == {0, 1}, name


def test_centres_b_summary():
    """What makes centres_B a test of the border pass: thousands of non-core rows that take a label."""
    lab = dc.sklearn_labels("centres_B")
    core = np.zeros(len(lab), bool)
    core[dc.sklearn_core("centres_B")] = True
    assert lab.max() + 1 == 182 and int((lab < 0).sum()) == 11021 and int((~core & (lab >= 0)).sum()) == 8477


def test_tau_coefficient_and_slack():
    # c(d) = 2 (d + 8): two evaluations, each within (d + 8) 2^-52 (|x|^2 + |y|^2) of the exact value
    assert spec.tau_coefficient(50) == 116.0 and spec.tau_coefficient(1) == 18.0
    e2 = 1.5 * 1.5
    assert 4 * np.spacing(e2) <= spec.eps_slack(1.5) <= 8 * np.spacing(e2)


def test_tau_covers_the_forms_of_d2():
    """The three ways of evaluating d2 (norms and dot product, difference form, either in a permuted column order) stay
    within half of tau of one another, the spread the bound must cover, on rows with heavy cancellation."""
    rng = np.random.default_rng(5)
    for d in (2, 15, 16, 50, 300):
        X = 100.0 + rng.standard_normal((64, d))   # large norms, small distances
        perm = rng.permutation(d)
        sq = np.einsum("ij,ij->i", X, X)
        s = sq[:, None] + sq[None, :]
        forms = [s - 2.0 * (X @ X.T), ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1),
                 s - 2.0 * (X[:, perm] @ X[:, perm].T), ((X[:, None, perm] - X[None, :, perm]) ** 2).sum(-1)]
        exact = ((X[:, None, :].astype(np.longdouble) - X[None, :, :].astype(np.longdouble)) ** 2).sum(-1)
        half = 0.5 * spec.tau_coefficient(d) * 2.0 ** -52 * s
        for f in forms:
            assert (np.abs(f - exact) <= half).all(), d


def test_exact_eps_is_ambiguous():
    X = np.random.default_rng(2).standard_normal((40, 4))
    X[1] = X[0]
    X[1, 2] += 0.75
    assert spec.ambiguous(X, 0.75)
    assert not spec.ambiguous(X, 0.7501)


def test_rejects_what_sklearn_rejects():
    X = np.zeros((4, 2))
    X[2, 1] = np.nan
    with pytest.raises(ValueError):
        spec.dbscan_labels(X, 1.0, 2)
    with pytest.raises(ValueError):
        spec.dbscan_labels(np.zeros((4, 2)), 0.0, 2)
