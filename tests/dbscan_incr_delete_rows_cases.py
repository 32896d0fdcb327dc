"""Streams with deletes of ANY rows, shared by tests/test_dbscan_incr_delete_rows_host.py and
tests/test_gpu_dbscan_incr_delete_rows.py: the operations of tests/dbscan_incr_delete_cases.py, ("ins", rows) and ("del", m),
and ("rows", positions): the rows at these distinct positions among the rows held go.  The oracle is the same: scikit-learn's
refit of the rows held, and the neighbour counts by direct differences."""
import numpy as np

import dbscan_incr_cases as ic
import dbscan_incr_delete_cases as dc


def replay(ops):
    """-> per operation the rows held after it."""
    held, out = None, []
    for kind, arg in ops:
        if kind == "ins":
            held = arg if held is None or not len(held) else np.concatenate([held, arg])
        elif kind == "del":
            held = held[arg:]
        else:
            keep = np.ones(len(held), dtype=bool)
            keep[np.asarray(arg)] = False
            held = held[keep]
        out.append(held)
    return out


def apply(s, kind, arg):
    """One operation on an IncrementalSpec -> its labels."""
    return s.insert(arg) if kind == "ins" else s.delete_oldest(arg) if kind == "del" else s.delete_rows(arg)


def from_the_middle(ops, pad):
    """The same stream behind `pad` far noise rows (x >= 5000, 3 apart: they see nothing and are never deleted), every delete
    of the m oldest rows turned into a delete of positions pad .. pad + m - 1: the same rows go, from the middle of the rows
    held, and the info word of every delete stays what it was."""
    d = ops[0][1].shape[1]
    noise = np.zeros((pad, d))
    noise[:, 0] = 5000.0 + 3.0 * np.arange(pad)
    out = [("ins", noise)]
    for kind, arg in ops:
        out.append((kind, arg) if kind == "ins" else ("rows", np.arange(pad, pad + arg)))
    return out


def bridge_case(d):
    """Blob A around -0.9, blob B around +0.9, the bridge row at 0 inserted LAST of the first batch and between two far noise
    rows; min_samples = 3.  The bridge goes: the cluster splits, both blobs are rebuilt."""
    rng = np.random.default_rng(21 + d)
    a, b = dc.line(-0.9 + 0.02 * np.arange(6), d, rng), dc.line(0.9 + 0.02 * np.arange(6), d, rng)
    far = dc.line([3000.0, 3003.0], d, rng)
    X = np.concatenate([a, far[:1], b, dc.line([0.0], d, rng), far[1:]])
    return [("ins", X[:9]), ("ins", X[9:]), ("rows", [13])], dc.EPS, 3


def clusters_case(d, n=330):
    """Three blobs and noise (dc.blobs; seeds at which eps = 0.8 separates at least two clusters of 80 rows or more) ->
    (X, scikit-learn's labels at min_samples = 5)."""
    X = dc.blobs(n, d, {1: 56, 2: 43}.get(d, 48))
    return X, ic.refit(X, 0.8, 5)[0]


def random_stream(seed):
    """8 operations on blobs of sigma 0.35 (+ noise), d in {1, 2, 3, 8}, min_samples in {1, 2, 3, 5}, eps in [0.3, 0.8]:
    inserts (some repeat rows held) and deletes of a random subset, of a contiguous range in the middle, or of every row of one
    cluster or of the noise.  -> (ops, eps, min_samples)"""
    rng = np.random.default_rng(1000 + seed)
    d, ms = (1, 2, 3, 8)[seed % 4], (1, 2, 3, 5)[(seed // 4) % 4]
    eps = float(rng.uniform(0.3, 0.8))
    cen = 2.5 * rng.standard_normal((4, d))

    def batch(w):
        X = cen[rng.integers(0, 4, w)] + 0.35 * rng.standard_normal((w, d))
        far = rng.random(w) < 0.15
        X[far] = 5.0 * rng.standard_normal((int(far.sum()), d))
        return X

    ops = [("ins", batch(int(rng.integers(40, 90))))]
    held = ops[0][1]
    while len(ops) < 8:
        n = len(held)
        kind = rng.integers(0, 6) if n else 0
        if kind <= 1:
            X = batch(int(rng.integers(1, 60)))
            if kind == 1 and n:                                   # duplicates of rows held
                X[:len(X) // 2] = held[rng.integers(0, n, len(X) // 2)]
            ops.append(("ins", X))
        else:
            if kind == 2:
                idx = rng.choice(n, int(rng.integers(1, max(2, n // 3))), replace=False)
            elif kind == 3:
                lo = int(rng.integers(0, n))
                idx = np.arange(lo, min(n, lo + int(rng.integers(1, 40))))
            else:
                labels = ic.refit(held, eps, ms)[0]
                idx = np.flatnonzero(labels == (rng.choice(np.unique(labels)) if kind == 4 else -1))
                if not len(idx):
                    idx = np.array([n // 2])
            ops.append(("rows", idx))
        held = replay(ops)[-1]
    return ops, eps, ms
