"""mused_amd/dbscan_incr.py (the specification of csrc/dbscan_incr.hip) against scikit-learn: after EVERY insert the labels of
all rows seen so far must equal DBSCAN(eps, min_samples).fit_predict(prefix), numbering included.  Every comparison first
asserts that no pair of the prefix lies within the rounding margin of eps (mused_amd.dbscan.ambiguous), the condition
under which the rule is pinned."""
import numpy as np
import pytest

import dbscan_cases as dc
import dbscan_incr_cases as ic


def _run(batches, eps, ms):
    """Inserts the batches; returns the spec after comparing every prefix with scikit-learn's refit."""
    from mused_amd import dbscan as batch_spec
    from mused_amd.dbscan_incr import IncrementalSpec

    spec = IncrementalSpec(eps, ms)
    seen = None
    for b in batches:
        seen = b if seen is None else np.concatenate([seen, b])
        assert not batch_spec.ambiguous(seen, eps)
        got = spec.insert(b)
        want, n_core = ic.refit(seen, eps, ms)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert spec.clusters == want.max() + 1 and int(spec.core.sum()) == n_core
        assert spec.flags == 0
    return spec


@pytest.mark.parametrize("name", [c[0] for c in dc.small_cases()])
def test_small_cases_split_at_1_half_and_n_minus_1(name):
    _, X, eps, ms, _ = dc.case(name)
    n = len(X)
    for cut in sorted({c for c in (1, n // 2, n - 1) if 0 < c < n}) or [None]:
        _run([X] if cut is None else [X[:cut], X[cut:]], eps, ms)
    _run(ic.split_case(X, (1, n // 2, n - 1)), eps, ms)


@pytest.mark.parametrize("case", ic.hand_cases() + ic.random_streams(), ids=lambda c: c[0])
def test_streams(case):
    _, batches, eps, ms = case
    _run(batches, eps, ms)


def _labels_before_after(name):
    _, batches, eps, ms = next(c for c in ic.hand_cases() if c[0] == name)
    spec = _run(batches, eps, ms)
    before = ic.refit(batches[0], eps, ms)[0]
    after = ic.refit(np.concatenate(batches[:2]), eps, ms)[0]
    return spec, before, after


def test_case_a_is_the_merge_through_an_old_row():
    spec, before, after = _labels_before_after("a_old_row_turns_core_and_joins")
    assert before.max() == 1 and after.max() == 0
    assert spec.dirty[1][0] == 1 and after[9] == 0        # dirtyA is row 8 alone; the new row is its border row
    assert spec.core[8] and not spec.core[9]


def test_case_b_moves_a_border_row_that_gained_no_neighbour():
    spec, before, after = _labels_before_after("b_border_row_follows_a_merge")
    assert before.max() == 2 and before[13] == 1 and before[5] == 1 and before[9] == 2
    assert after.max() == 1 and after[13] == 0 and after[9] == 0 and after[5] == 1
    assert spec.count[13] == 3                             # itself and the two centres, as before the insert


def test_case_c_shifts_every_number():
    _, before, after = _labels_before_after("c_old_row_founds_the_first_cluster")
    assert before[0] == -1 and before[3] == 0 and before[7] == 1
    assert after[0] == 0 and after[3] == 1 and after[7] == 2


def test_case_d_chains_three_clusters():
    _, before, after = _labels_before_after("d_three_clusters_chained")
    assert before.max() == 2 and after.max() == 0 and (after >= 0).all()


def test_spread_keeps_the_labels_of_the_rows_it_moves():
    """`spread` (the device tests move interacting rows into different tiles with it) puts noise rows behind every row and
    changes nothing else."""
    _, batches, eps, ms = ic.hand_cases()[1]
    gap = 3
    from mused_amd.dbscan_incr import IncrementalSpec

    wide, narrow = IncrementalSpec(eps, ms), IncrementalSpec(eps, ms)
    for b, bw in zip(batches, ic.spread(batches, gap)):
        assert len(bw) == (gap + 1) * len(b)
        lw, ln = wide.insert(bw), narrow.insert(b)
    real = np.arange(0, len(lw), gap + 1)
    assert np.array_equal(lw[real], ln) and (np.delete(lw, real) == -1).all()


def test_rejected_input():
    from mused_amd.dbscan_incr import IncrementalSpec

    with pytest.raises(ValueError):
        IncrementalSpec(0.0, 3)
    with pytest.raises(ValueError):
        IncrementalSpec(1.0, 0)
    s = IncrementalSpec(1.0, 2)
    s.insert(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        s.insert(np.zeros((2, 4)))
    with pytest.raises(ValueError, match="Input contains NaN or infinity."):
        s.insert(np.array([[0.0, np.nan, 0.0]]))
