"""mused_amd/hdbscan.py -- the specification of csrc/emst.hip and the host stage behind it -- against
sklearn.cluster.HDBSCAN, without a GPU: equal labels (numbering included) and bitwise equal weights on inputs that are
decided far beyond rounding, a flag on the two that are not, and three named wrong variants that must each break a case."""
import math

import numpy as np
import pytest

import hdbscan_cases as hc
from mused_amd import hdbscan as spec


@pytest.mark.parametrize("name", hc.CASE_NAMES)
def test_specification_equals_sklearn(name):
    X, mcs, _ = hc.case(name)
    n = len(X)
    t = hc.spec_tree(name)
    want, values = hc.sklearn_fit(name)
    print(f"{name}: rounds {t.rounds}, margin {t.margin:.3g} tau, ambiguous {t.ambiguous}")
    assert not t.ambiguous and t.margin >= 100.0          # a condition on the INPUT: regenerate a case that misses it
    assert len(t.a) == n - 1 and len(hc.edge_set(t.a, t.b)) == n - 1
    assert 1 <= t.rounds <= max(1, math.ceil(math.log2(n)))
    labels, w = spec.labels_from_edges(X, t.a, t.b, mcs)
    assert labels is not None, "two tree edges of equal weight"
    assert np.array_equal(np.sort(w), values)             # bitwise: the weights of scikit-learn's single-linkage tree
    assert labels.dtype == np.int64 and np.array_equal(labels, want)
    full, _, _ = spec.hdbscan_labels(X, mcs)
    assert np.array_equal(full, want)


@pytest.mark.parametrize("name", hc.MIN_SAMPLES_1_NAMES)
def test_min_samples_1_is_the_same_tree(name):
    X, mcs, _ = hc.case(name)
    t = hc.spec_tree(name)
    labels, _ = spec.labels_from_edges(X, t.a, t.b, mcs)
    assert np.array_equal(labels, hc.sklearn_labels(name, 1))


@pytest.mark.parametrize("name", hc.AMBIGUOUS_NAMES)
def test_exact_ties_are_flagged(name):
    t = hc.spec_tree(name)
    assert t.ambiguous and t.margin <= 1.0
    labels, _, _ = spec.hdbscan_labels(hc.case(name)[0], hc.case(name)[1])
    assert labels is None


def test_tie_guard_on_equal_weights():
    assert spec.weights_tie([0.5, 1.0, 0.5]) and not spec.weights_tie([0.5, 1.0, 0.25]) and not spec.weights_tie([1.0])
    X = np.array([[0.0], [1.0], [3.0], [4.0]])            # edges 0-1 and 2-3 weigh the same
    labels, w = spec.labels_from_edges(X, [0, 1, 2], [1, 2, 3], 2)
    assert labels is None and list(w) == [1.0, 2.0, 1.0]


def test_prim_order_orients_from_row_0():
    mst = spec.prim_order(4, [3, 1, 2], [2, 0, 1], [0.5, 3.0, 2.0])    # the path 0 - 1 - 2 - 3, given backwards
    assert mst["current_node"].tolist() == [0, 1, 2] and mst["next_node"].tolist() == [1, 2, 3]
    assert mst["distance"].tolist() == [3.0, 2.0, 0.5]
    with pytest.raises(ValueError):
        spec.prim_order(4, [0, 0, 1], [1, 1, 0], [1.0, 2.0, 3.0])      # does not span
    with pytest.raises(ValueError):
        spec.prim_order(4, [0], [1], [1.0])


def test_nan_rows_are_rejected_by_the_specification():
    with pytest.raises(ValueError):
        spec.emst_boruvka(hc.case(hc.NAN_NAME)[0])


# ---- named wrong variants: each must break at least one case -----------------------------------------------------------

def test_wrong_variant_pairwise_sum_changes_weight_bits():
    broken = []
    for name in hc.CASE_NAMES:
        X, _, _ = hc.case(name)
        t = hc.spec_tree(name)
        w = np.sqrt(((X[t.a] - X[t.b]) ** 2).sum(axis=1))
        if not np.array_equal(np.sort(w), hc.sklearn_fit(name)[1]):
            broken.append(name)
    assert broken, "sum(axis=1) gave scikit-learn's bits everywhere: the cases no longer tell the two apart"


def test_wrong_variant_unordered_edges_renumber_the_clusters():
    broken = []
    for name in hc.CASE_NAMES:
        X, mcs, _ = hc.case(name)
        t = hc.spec_tree(name)
        mst = np.empty(len(t.a), dtype=spec.sklearn_internals()[0])
        mst["current_node"], mst["next_node"], mst["distance"] = t.a, t.b, spec.edge_weights(X, t.a, t.b)
        if not np.array_equal(spec.labels_from_mst(mst, mcs), hc.sklearn_labels(name)):
            broken.append(name)
    assert broken, "edges in arbitrary order and orientation gave scikit-learn's numbering everywhere"


def test_wrong_variant_pick_without_the_index_tie_break_on_the_lattice():
    X, _, _ = hc.case("lattice")
    n = len(X)
    good = hc.spec_tree("lattice")                         # flagged, but under the total order still a spanning tree
    assert len(hc.edge_set(good.a, good.b)) == n - 1 and _acyclic(n, good.a, good.b)
    bad = spec.emst_boruvka(X, tie_rng=np.random.default_rng(0))
    assert len(bad.a) != n - 1 or not _acyclic(n, bad.a, bad.b)


def _acyclic(n, a, b):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in zip(a.tolist(), b.tolist()):
        ru, rv = find(u), find(v)
        if ru == rv:
            return False
        parent[ru] = rv
    return True
