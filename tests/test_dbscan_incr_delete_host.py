"""mused_amd.dbscan_incr.IncrementalSpec under deletions of the oldest rows (the rule the kernels of mused_dbscan_incr_delete
implement) against scikit-learn: after EVERY operation the labels of the rows held equal DBSCAN(eps, min_samples).fit_predict on
those rows in their order and count[] equals the neighbour counts by direct differences.  Every stream is checked to hold no
pair within the rounding margin of eps (mused_amd.dbscan.ambiguous) and the spec must never raise its flag."""
import numpy as np
import pytest

import dbscan_incr_cases as ic
import dbscan_incr_delete_cases as dc
from mused_amd import dbscan as spec
from mused_amd.dbscan_incr import NONE, IncrementalSpec


def run(ops, eps, ms, max_rows=None):
    """Replays ops on the spec, checking everything after every operation; -> (the spec, [last_delete per delete])."""
    s = IncrementalSpec(eps, ms, max_rows=max_rows)
    infos = []
    for (kind, arg), held in zip(ops, dc.replay(ops)):
        labels = s.insert(arg) if kind == "ins" else s.delete_oldest(arg)
        if kind == "del":
            infos.append(s.last_delete)
        assert s.flags == 0 and s.n == len(held)
        if not len(held):
            assert len(labels) == 0 and s.X is None
            continue
        assert not spec.ambiguous(held, eps)
        want, n_core = ic.refit(held, eps, ms)
        assert np.array_equal(labels, want), (kind, np.flatnonzero(labels != want))
        assert np.array_equal(s.count, dc.counts(held, eps))
        assert np.array_equal(s.X, held)
        # what an insert relies on
        idx = np.arange(s.n)
        core = s.count >= ms
        assert (s.parent <= idx).all() and (s.parent[~core] == idx[~core]).all()
        root = s.parent[core]
        assert (s.parent[root] == root).all() and core[root].all()
        has = ~core & (s.best != NONE)
        assert core[s.best[has]].all() and (s.parent[s.best[has]] == s.best[has]).all()
        if kind == "del":
            assert s.last_delete[:3] == (0, want.max() + 1, n_core)
    return s, infos


@pytest.mark.parametrize("d", [1, 2, 5])
def test_hand_built_streams(d):
    by_name = {}
    for name, ops, eps, ms in dc.hand_cases(d):
        by_name[name] = (run(ops, eps, ms), ops)
    # the scenarios are what their names say
    (s, infos), _ = by_name["chain_ms3"]
    assert all(i[3] == 1 for i in infos[:-1])                       # the new end row loses core status every time
    (s, infos), _ = by_name["bridge"]
    assert infos[0][1] == 2 and infos[0][4] == 12                    # two clusters; both blobs were rebuilt
    (s, infos), ops = by_name["border_smaller_cluster_deleted"]
    assert infos[0][5] == 1 and s.clusters == 2                      # the border row alone was taken again
    (s, infos), _ = by_name["border_smaller_cluster_affected"]
    assert infos[0][3] == 2 and infos[0][4] == 1 and infos[0][5] == 3 and infos[0][2] == 11   # |R| = 1 < 11 core rows
    (s, infos), _ = by_name["untouched_far_cluster"]
    assert 0 < infos[0][4] < infos[0][2]
    (s, infos), _ = by_name["lost_core_status_ms5"]
    assert infos[0][3] == 1 and infos[0][4] == 0 and infos[0][5] == 4          # the centre and the three rows it labelled


@pytest.mark.parametrize("ms", [1, 2, 5])
@pytest.mark.parametrize("d", [1, 3])
def test_interleaved_under_max_rows(d, ms):
    """Windows of 96 rows under max_rows = 200: the class deletes the surplus itself, and does what the written-out operations
    do."""
    X = dc.blobs(960, d, 11 + d)
    ops = dc.interleaved(X, 96, 200)
    s, infos = run(ops, 0.8, ms)
    assert len(infos) == 8 and any(i[3] > 0 for i in infos) == (ms > 1)
    auto = IncrementalSpec(0.8, ms, max_rows=200)
    for lo in range(0, 960, 96):
        labels = auto.insert(X[lo:lo + 96])
    assert auto.n == 200 and np.array_equal(auto.X, s.X) and np.array_equal(labels, ic.refit(s.X, 0.8, ms)[0])
    assert np.array_equal(auto.count, s.count) and np.array_equal(auto.parent, s.parent) and np.array_equal(auto.best, s.best)
    with pytest.raises(ValueError):
        auto.insert(X[:201])


@pytest.mark.parametrize("seed", range(6))
def test_random_inserts_and_deletes(seed):
    rng = np.random.default_rng(seed)
    d, ms = 1 + seed % 4, 1 + seed % 6
    X = dc.blobs(400, d, 30 + seed)
    ops, lo, held = [], 0, 0
    while lo < 400:
        w = min(int(rng.integers(1, 70)), 400 - lo)
        ops.append(("ins", X[lo:lo + w]))
        lo, held = lo + w, held + w
        if rng.random() < 0.7:
            m = int(rng.integers(1, min(60, held) + 1))
            ops.append(("del", m))
            held -= m
    run(ops, 0.8, ms)


def test_arguments():
    s = IncrementalSpec(1.0, 3)
    with pytest.raises(ValueError):
        s.delete_oldest(1)
    s.insert(np.zeros((4, 2)) + np.arange(4)[:, None] * 3.0)
    for m in (0, 5, -1):
        with pytest.raises(ValueError):
            s.delete_oldest(m)
    assert s.n == 4
    with pytest.raises(ValueError):
        IncrementalSpec(1.0, 3, max_rows=0)
