"""Rows looked up by value, written out as a rule: the specification of csrc/rows_find.hip (mused_rows_find), which the tests
pin the kernels to.

Two rows are equal when all their d fp64 values have the same bits: -0.0 is not +0.0, a difference in the last bit is a
difference, and a NaN row finds a row with the same NaN bits (`row.tobytes()` is the key).  A value held at positions
h1 < h2 < ... and asked for at query positions q1 < q2 < ...: query q_k gets h_k, and -1 beyond the last held occurrence --
so asking for the rows held, duplicates included, returns every position once."""
from __future__ import annotations

import numpy as np


def rows_find(X, Q):
    """X: (n, d) held rows, Q: (q, d) query rows (taken as fp64) -> int64 (q,): the position of each query row, or -1."""
    X, Q = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, Q))
    if X.ndim != 2 or Q.ndim != 2 or X.shape[1] != Q.shape[1]:
        raise ValueError("rows_find: X must be (n, d) and Q (q, d)")
    held = {}
    for i, row in enumerate(X):
        held.setdefault(row.tobytes(), []).append(i)
    taken = {}
    out = np.full(len(Q), -1, dtype=np.int64)
    for k, row in enumerate(Q):
        key = row.tobytes()
        t = taken.get(key, 0)
        taken[key] = t + 1
        positions = held.get(key, ())
        if t < len(positions):
            out[k] = positions[t]
    return out
