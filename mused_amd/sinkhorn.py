"""The Sinkhorn-Knopp iteration behind the reference's `ot.sinkhorn(a, b, M, reg=0.1)` call
(matrix_operations.py:198, approach "sSVDMC_pot"), written out.  NumPy only.

PARITY UNPINNED: the POT package is not available to this project, so nothing here is compared with it.  This module IS
the specification the device kernel (csrc/match.hip) and the tests are held to: POT's `sinkhorn_knopp` with every
argument but `reg` at its default (numItermax=1000, stopThr=1e-9, no warm start, no log), restated operation by operation.
"""
from __future__ import annotations

import numpy as np

POT_REG = 0.1          # matrix_operations.py:198
SELECT_FRACTION = 0.5  # matrix_operations.py:201


def sinkhorn_knopp(a, b, M, reg, numItermax=1000, stopThr=1e-9):
    """(plan, iterations run).  a: (P,) and b: (N,) marginals, M: (P, N) cost.  The dtype of M carries through (float64, or
    np.longdouble for the tests' precision yardstick)."""
    M = np.asarray(M)
    dt = M.dtype if M.dtype.kind == "f" else np.float64
    a, b, M = np.asarray(a, dtype=dt), np.asarray(b, dtype=dt), M.astype(dt, copy=False)
    P, N = M.shape
    u = np.ones(P, dtype=dt) / P
    v = np.ones(N, dtype=dt) / N
    K = np.exp(M / (-dt.type(reg)))
    Kp = (1 / a)[:, None] * K
    it = 0
    for ii in range(numItermax):
        it = ii + 1
        uprev, vprev = u, v
        KtU = K.T @ u
        v = b / KtU
        u = 1.0 / (Kp @ v)
        if np.any(KtU == 0) or np.any(np.isnan(u)) or np.any(np.isnan(v)) or np.any(np.isinf(u)) or np.any(np.isinf(v)):
            u, v = uprev, vprev  # numerical error: keep the last finite scalings (cannot fire for costs in [0, 1], reg 0.1)
            break
        if ii % 10 == 0:
            err = np.linalg.norm(np.einsum("i,ij,j->j", u, K, v) - b)
            if err < stopThr:
                break
    return u[:, None] * K * v[None, :], it


def pot_cost(cost):
    """matrix_operations.py:188-192: inf -> 1e9, abs (a larger overlap IS a larger cost: reproduced, not repaired), / max."""
    cost = np.abs(np.where(np.isinf(cost), 1e9, cost))
    return cost / cost.max()


def pot_plan(cost, dtype=np.float64):
    """Transport plan of the reference's pot_matching for an overlap cost matrix (-overlap, inf where infeasible)."""
    M = pot_cost(cost).astype(dtype)
    P, N = M.shape
    return sinkhorn_knopp(np.ones(P, dtype=dtype) / P, np.ones(N, dtype=dtype) / N, M, POT_REG)


def select(plan):
    """matrix_operations.py:201-204: {column: row} over np.where's row-major order, so the LARGEST selected row of a column
    wins."""
    rows, cols = np.where(plan > plan.max() * SELECT_FRACTION)
    return {int(c): int(r) for r, c in zip(rows, cols)}
