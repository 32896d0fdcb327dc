"""mused_amd.dbscan_incr.IncrementalSpec.delete_rows (the rule the kernels of mused_dbscan_incr_delete_rows implement) against
scikit-learn: after EVERY operation the labels of the rows held equal DBSCAN(eps, min_samples).fit_predict on those rows in
their order, count[] equals the neighbour counts by direct differences and the invariants an insert relies on hold.  A stream
that holds a pair within the rounding margin of eps (mused_amd.dbscan.ambiguous) is skipped and counted; for the seeds here
that count must be 0."""
import numpy as np
import pytest

import dbscan_incr_cases as ic
import dbscan_incr_delete_cases as dc
import dbscan_incr_delete_rows_cases as rc
from mused_amd import dbscan as spec
from mused_amd.dbscan_incr import NONE, IncrementalSpec


def check(s, held, eps, ms):
    assert s.flags == 0 and s.n == len(held)
    if not len(held):
        assert s.X is None and len(s.count) == len(s.parent) == len(s.best) == len(s.nrm) == 0
        return None
    want, n_core = ic.refit(held, eps, ms)
    assert np.array_equal(s.X, held) and np.array_equal(s.nrm, np.einsum("ij,ij->i", held, held))
    assert np.array_equal(s.count, dc.counts(held, eps))
    idx = np.arange(s.n)
    core = s.count >= ms
    assert (s.parent <= idx).all() and (s.parent[~core] == idx[~core]).all()
    root = s.parent[core]
    assert (s.parent[root] == root).all() and core[root].all()
    has = ~core & (s.best != NONE)
    assert core[s.best[has]].all() and (s.parent[s.best[has]] == s.best[has]).all()
    return want, n_core


def run(ops, eps, ms):
    """Replays ops on the spec, checking everything after every operation; -> (the spec, [last_delete per delete]), or None
    for a stream that holds an ambiguous pair."""
    helds = rc.replay(ops)
    if any(len(h) and spec.ambiguous(h, eps) for h in helds):
        return None
    s = IncrementalSpec(eps, ms)
    infos = []
    for (kind, arg), held in zip(ops, helds):
        labels = rc.apply(s, kind, arg)
        ref = check(s, held, eps, ms)
        if kind != "ins":
            infos.append(s.last_delete)
        if ref is None:
            assert len(labels) == 0 and (kind == "ins" or s.last_delete == (0,) * 6)
            continue
        want, n_core = ref
        assert np.array_equal(labels, want), (kind, np.flatnonzero(labels != want))
        if kind != "ins":
            assert s.last_delete[:3] == (0, want.max() + 1, n_core)
            assert (s.best[s.count >= ms] == NONE).all()             # a delete resets the best of a core row
    return s, infos


@pytest.mark.parametrize("d", [1, 2, 5])
def test_hand_built_streams_from_the_middle(d):
    """dc.hand_cases behind 7 far noise rows that stay: every delete takes its rows from the middle of the rows held, and its
    info word is the one of the delete of the oldest rows."""
    for name, ops, eps, ms in dc.hand_cases(d):
        s0 = IncrementalSpec(eps, ms)
        want = []
        for kind, arg in ops:
            rc.apply(s0, kind, arg)
            if kind == "del":
                want.append(s0.last_delete)
        s, infos = run(rc.from_the_middle(ops, 7), eps, ms)
        assert infos == want, name
        assert s.n == s0.n + 7


@pytest.mark.parametrize("d", [1, 2, 8])
def test_bridge_row(d):
    ops, eps, ms = rc.bridge_case(d)
    s, infos = run(ops, eps, ms)
    assert infos[0] == (0, 2, 12, 0, 12, 0)                  # two clusters; both blobs rebuilt; the far rows have no best


@pytest.mark.parametrize("d", [1, 3])
def test_whole_cluster_all_noise_every_other_row(d):
    X, labels = rc.clusters_case(d)
    assert labels.max() >= 1 and (labels == -1).sum() >= 3
    eps, ms = 0.8, 5
    # every core row of cluster 0 (its border rows stay, and turn noise or move), then the whole of what was cluster 1
    core0 = np.flatnonzero((labels == 0) & (dc.counts(X, eps) >= ms))
    s, infos = run([("ins", X), ("rows", core0)], eps, ms)
    s, infos = run([("ins", X[:200]), ("ins", X[200:]), ("rows", np.flatnonzero(labels == 1))], eps, ms)
    assert infos[0][3] == 0 or infos[0][5] > 0
    # all noise: no count of a core row changes unless a noise row was a border-less neighbour; nothing is rebuilt
    s, infos = run([("ins", X), ("rows", np.flatnonzero(labels == -1))], eps, ms)
    assert infos[0][1] == labels.max() + 1
    for ms2 in (1, 2, 3, 5):
        s, infos = run([("ins", X), ("rows", np.arange(0, len(X), 2)), ("rows", np.arange(1, len(X) // 2, 2))], eps, ms2)
        assert s.n == len(X) // 2 - len(range(1, len(X) // 2, 2))


@pytest.mark.parametrize("ms", [1, 2, 3, 5])
def test_everything_then_an_insert_and_duplicates(ms):
    X = dc.blobs(150, 2, 17)
    rng = np.random.default_rng(3)
    s, infos = run([("ins", X[:100]), ("rows", rng.permutation(100)), ("ins", X[50:]), ("rows", [0])], 0.8, ms)
    assert infos[0] == (0,) * 6 and s.n == 99
    # every row three times; one occurrence of each of the first 40 goes, from the first, second or third copy
    Y = np.concatenate([X[:60]] * 3)
    which = rng.integers(0, 3, 40) * 60 + np.arange(40)
    s, infos = run([("ins", Y[:70]), ("ins", Y[70:]), ("rows", which)], 0.8, ms)
    assert s.n == 140


@pytest.mark.parametrize("block", range(6))
def test_random_interleavings(block):
    """48 streams of 8 operations (rc.random_stream): every d in {1, 2, 3, 8} with every min_samples in {1, 2, 3, 5}."""
    skipped = 0
    for seed in range(8 * block, 8 * block + 8):
        ops, eps, ms = rc.random_stream(seed)
        assert len(ops) == 8
        skipped += run(ops, eps, ms) is None
    assert skipped == 0


@pytest.mark.parametrize("ms", [1, 2, 3, 5])
@pytest.mark.parametrize("d", [1, 3])
def test_prefix_equivalence(d, ms):
    """delete_rows(range(m)) leaves exactly the state and last_delete of delete_oldest(m).  On the spec both now build a mask
    for one method, so this compares one path with itself; the real comparison is the device one
    (test_gpu_dbscan_incr_delete_rows.py::test_prefix_equals_the_delete_of_the_oldest_rows)."""
    X = dc.blobs(300, d, 50 + d)
    a, b = IncrementalSpec(0.8, ms), IncrementalSpec(0.8, ms)
    a.insert(X[:180]), b.insert(X[:180])
    a.insert(X[180:]), b.insert(X[180:])
    for m in (1, 77, 128, 94):
        la, lb = a.delete_oldest(m), b.delete_rows(np.arange(m)[::-1] if m == 77 else range(m))
        assert np.array_equal(la, lb) and a.last_delete == b.last_delete and a.n == b.n
        for name in ("X", "nrm", "count", "parent", "best"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.n == 0 and a.X is None and b.X is None


def test_arguments():
    s = IncrementalSpec(1.0, 3)
    with pytest.raises(ValueError):
        s.delete_rows([0])
    s.insert(np.zeros((4, 2)) + np.arange(4)[:, None] * 3.0)
    for bad in ([], [4], [-1], [1, 1], [0, 1, 2, 3, 0]):
        with pytest.raises(ValueError):
            s.delete_rows(bad)
    assert s.n == 4 and np.array_equal(s.count, np.ones(4))
