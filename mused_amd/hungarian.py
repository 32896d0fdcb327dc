"""The assignment solver behind `scipy.optimize.linear_sum_assignment(cost)` (matrix_operations.py:170, every Hungarian
approach), written out.  NumPy only.

PARITY PINNED: SciPy is installed, so tests/test_match_hung_host.py compares `lsap` with it pair for pair, ties included.
SciPy stays the authority and `match_clusters(method="hungarian")` keeps calling it; this module is the statement of the
algorithm the device kernel (csrc/match_hung.hip) follows step by step: the shortest-augmenting-path method of SciPy 1.15's
rectangular_lsap, with its scan order over the remaining columns and its tie rule.
"""
from __future__ import annotations

import numpy as np


def lsap(cost):
    """(rows, cols, steps) with (rows, cols) what linear_sum_assignment(cost) returns; `steps` is the number of passes of
    the inner `while` loop over all rows (one Dijkstra step each; a diagnostic).  Raises ValueError("cost matrix is
    infeasible") when no complete assignment exists."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2:
        raise ValueError("expected a matrix (2-D array)")
    transposed = cost.shape[0] > cost.shape[1]
    if transposed:
        cost = cost.T
    nr, nc = cost.shape
    inf = float("inf")
    cost = cost.tolist()   # plain lists of Python floats: the same doubles, without NumPy's per-element overhead
    u, v = [0.0] * nr, [0.0] * nc
    col4row, row4col, path = [-1] * nr, [-1] * nc, [-1] * nc
    steps = 0
    for cur in range(nr):
        min_val, i = 0.0, cur
        remaining = [nc - 1 - it for it in range(nc)]   # reversed on purpose: SciPy's order
        nrem = nc
        SR, SC = [False] * nr, [False] * nc
        sp = [inf] * nc
        sink = -1
        while sink == -1:
            steps += 1
            index, lowest = -1, inf
            SR[i] = True
            row = cost[i]
            for it in range(nrem):
                j = remaining[it]
                r = min_val + row[j] - u[i] - v[j]
                if r < sp[j]:
                    path[j] = i
                    sp[j] = r
                # among equal lowest values the LAST position holding an unassigned column wins, else the FIRST position
                if sp[j] < lowest or (sp[j] == lowest and row4col[j] == -1):
                    lowest = sp[j]
                    index = it
            min_val = lowest
            if min_val == inf:
                raise ValueError("cost matrix is infeasible")
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            nrem -= 1
            remaining[index] = remaining[nrem]
        u[cur] += min_val
        for i in range(nr):
            if SR[i] and i != cur:
                u[i] += min_val - sp[col4row[i]]
        for j in range(nc):
            if SC[j]:
                v[j] -= min_val - sp[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    col4row = np.array(col4row, dtype=np.int64)
    if transposed:
        order = np.argsort(col4row)
        return col4row[order], order, steps
    return np.arange(nr, dtype=np.int64), col4row, steps


def overlap_counts(prev, new):
    """(up, un, inverse of new, counts): the sorted distinct values of both sides (np.unique: -1 comes first) and the P x N
    positional overlap counts in ONE contingency pass over the rows."""
    up, ip = np.unique(np.asarray(prev), return_inverse=True)
    un, iq = np.unique(np.asarray(new), return_inverse=True)
    P, N = len(up), len(un)
    cnt = np.bincount(ip.ravel().astype(np.int64) * N + iq.ravel(), minlength=P * N).reshape(P, N)
    return up, un, iq.ravel(), cnt


def costs_of(cnt, min_overlap):
    """The cost matrix match_clusters builds: -count where the count reaches min_overlap, inf elsewhere."""
    return np.where(cnt >= min_overlap, -cnt.astype(np.float64), np.inf)


def is_feasible(cost) -> bool:
    """match_clusters' own test (matrix_operations.py:176-178): every row and every column keeps a finite entry."""
    fin = np.isfinite(cost)
    return bool(fin.size and fin.any(axis=1).all() and fin.any(axis=0).all())


def match_labels(prev, new, min_overlap):
    """`match_clusters(prev, new, "hungarian", min_overlap)` restated without its P x N passes over the rows: (labels, P, N,
    steps, feasible).  `labels` is `new` itself without a previous window or when the costs are infeasible (P, N are still
    reported, steps = 0), the relabelled int64 array otherwise; raises lsap's ValueError where SciPy raises.  This is what
    the wide device chain (csrc/match_wide.hip) computes, and the yardstick at sizes where the host loop takes seconds."""
    if prev is None or len(prev) == 0:
        return new, 0, 0, 0, False
    up, un, iq, cnt = overlap_counts(prev, new)
    cost = costs_of(cnt, min_overlap)
    if not is_feasible(cost):
        return new, len(up), len(un), 0, False
    rows, cols, steps = lsap(cost)
    table = un.astype(np.int64)
    table[cols] = up[rows]   # a matched new label takes the previous value of its row, any other keeps its own
    return table[iq], len(up), len(un), steps, True
