"""Streams of inserts and deletes shared by tests/test_dbscan_incr_delete_host.py and tests/test_gpu_dbscan_incr_delete.py:
(name, [("ins", rows) | ("del", m), ...], eps, min_samples), and the oracle of both: scikit-learn's refit of the rows held and
the neighbour counts by direct differences.

The hand-built streams live on a line (axis 0 of d dimensions) in units of eps = 1, on a grid of 0.3 (or 0.9 for the chain) with
a jitter of 1e-3 in every coordinate: every distance is at least 0.09 away from eps, far beyond rounding, and the coordinates
are continuous.  FAR rows (x >= 1000, 3 apart) are noise that sees nothing."""
import numpy as np

import dbscan_incr_cases as ic

EPS = 1.0


def line(xs, d, rng):
    """Rows at x = xs on axis 0 of d dimensions, jittered by 1e-3 in every coordinate."""
    X = np.zeros((len(xs), d))
    X[:, 0] = xs
    return X + 1e-3 * rng.uniform(-1.0, 1.0, X.shape)


def hand_cases(d=2):
    rng = np.random.default_rng(7 + d)
    out = []
    # chain: 40 rows 0.9 eps apart, inserted in order, deleted from the old end 3 at a time: the root goes every time, and with
    # min_samples = 3 the new end row loses core status and stays a border row
    xs = 0.9 * np.arange(40)
    for ms in (2, 3):
        ops = [("ins", line(xs[i:i + 8], d, rng)) for i in range(0, 40, 8)] + [("del", 3)] * 12
        out.append((f"chain_ms{ms}", ops, EPS, ms))
    # bridge: row 0 at the origin, blob A around -0.9, blob B around +0.9 (A and B are 1.8 apart): one cluster through row 0
    # alone; deleting it splits the cluster
    a = line(-0.9 + 0.02 * np.arange(6), d, rng)
    b = line(0.9 + 0.02 * np.arange(6), d, rng)
    out.append(("bridge", [("ins", np.concatenate([line([0.0], d, rng), a])), ("ins", b), ("del", 1), ("del", 3)], EPS, 3))
    # border row between two clusters, min_samples = 4.  P = rows at -1.2 .. 0 (step 0.3, every one core, root = the row at
    # -1.2), Q = rows at 1.8 .. 3.0, the border row at 0.9 sees P's row at 0 and Q's row at 1.8 and itself: best = P's root.
    # F: a far cluster of 5 rows that no delete touches
    p, q = line(-1.2 + 0.3 * np.arange(5), d, rng), line(1.8 + 0.3 * np.arange(5), d, rng)
    brow, f = line([0.9], d, rng), line(50.0 + 0.3 * np.arange(5), d, rng)
    # (1) P is deleted outright: the border row moves to Q, which becomes cluster 0
    out.append(("border_smaller_cluster_deleted", [("ins", p), ("ins", np.concatenate([brow, q, f])), ("del", 5)], EPS, 4))
    # (2) P is only affected: its two oldest rows go, the row at -0.6 and the row at -0.3 lose core status, the row at 0 is the
    # new root and the border row must follow it; F is untouched: |R| = 1 + ... < core rows
    out.append(("border_smaller_cluster_affected", [("ins", np.concatenate([p, q])), ("ins", np.concatenate([brow, f])), ("del", 2),
                                                    ("del", 1)], EPS, 4))
    # untouched far cluster first in the numbering of the survivors: noise, F, then P whose oldest row goes
    out.append(("untouched_far_cluster", [("ins", np.concatenate([p[:1], f, p[1:], q])), ("del", 1)], EPS, 4))
    # lost core status, min_samples = 5: a centre at 0 with rows at +-0.45 and +-0.9 is the only core row of its cluster (exactly
    # 5 within eps); beside it a chain at 1.8 .. 3.3 (step 0.3) whose first row sees the row at 0.9: that row has 4 within eps
    # and is a border row of both, labelled with the centre's cluster.  The oldest row (-0.9) goes: the centre loses core
    # status, the rows at +-0.45 turn noise with it, the row at 0.9 becomes a border row of the chain
    cell = line([-0.9, -0.45, 0.0, 0.45, 0.9], d, rng)
    clump = line(1.8 + 0.3 * np.arange(6), d, rng)
    out.append(("lost_core_status_ms5", [("ins", cell), ("ins", clump), ("del", 1), ("del", 2)], EPS, 5))
    # m == n, then an insert
    out.append(("delete_all_then_insert", [("ins", p), ("ins", q), ("del", 10), ("ins", np.concatenate([q, brow])), ("del", 6),
                                           ("ins", p)], EPS, 4))
    return out


def blobs(n, d, seed, noise=0.2):
    """n rows: three blobs and noise in random order, scaled so that eps = 0.8 cuts through the blobs' fringes in any d."""
    rng = np.random.default_rng(seed)
    cen = 3.0 * rng.standard_normal((3, d)) / np.sqrt(d)
    X = cen[rng.integers(0, 3, n)] + (0.55 / np.sqrt(d)) * rng.standard_normal((n, d))
    far = rng.random(n) < noise
    X[far] = 3.0 * rng.standard_normal((int(far.sum()), d)) / np.sqrt(d)
    return X


def interleaved(X, window, max_rows):
    """The operations of a stream of windows under max_rows, written out: the surplus oldest rows go before each insert."""
    ops, held = [], 0
    for lo in range(0, len(X) - window + 1, window):
        if held + window > max_rows:
            ops.append(("del", held + window - max_rows))
            held = max_rows - window
        ops.append(("ins", X[lo:lo + window]))
        held += window
    return ops


def spread_ops(ops, gap):
    """The same stream with `gap` far noise rows behind every row (ic.spread): rows that interact lie in different 128-row
    tiles, and a delete of m rows becomes one of m (gap + 1)."""
    batches = ic.spread([o[1] for o in ops if o[0] == "ins"], gap)
    out, k = [], 0
    for kind, arg in ops:
        if kind == "ins":
            out.append(("ins", batches[k]))
            k += 1
        else:
            out.append(("del", arg * (gap + 1)))
    return out


def counts(X, eps):
    """|N(i)| by direct differences (the row itself included)."""
    out = np.empty(len(X), dtype=np.int64)
    for lo in range(0, len(X), 64):
        diff = X[lo:lo + 64, None, :] - X[None, :, :]
        out[lo:lo + 64] = (np.einsum("ijk,ijk->ij", diff, diff) <= eps * eps).sum(axis=1)
    return out


def replay(ops):
    """-> per operation the rows held after it."""
    held, out = None, []
    for kind, arg in ops:
        if kind == "ins":
            held = arg if held is None or not len(held) else np.concatenate([held, arg])
        else:
            held = held[arg:]
        out.append(held)
    return out
