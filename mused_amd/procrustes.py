"""Orthogonal Procrustes as a closed-form rule: the specification of csrc/procrustes.hip (plain NumPy, no torch, no GPU).

Two consecutive hopping windows share W - step stream rows, but each window's embedding is expressed in that window's own
singular vectors: between the two the same row moves by an arbitrary orthogonal map.  The map R that best carries the new
coordinates A (m x r) of the shared rows onto their previous coordinates B (m x r), min |A R - B|_F over orthogonal R, is the
orthogonal polar factor of M = A^T B (`scipy.linalg.orthogonal_procrustes`): R = U V^T for M = U S V^T.  Right-multiplying
the whole window by R is an isometry, so nothing inside the window changes; only its frame becomes the previous window's.

The rule, step by step (the device restates each of them):

* M = A^T B.
* One-sided (Hestenes) Jacobi on the COLUMNS of M: sweeps over all column pairs in the fixed round-robin order of
  `schedule`, a pair (p, q) rotated when (w_p.w_q)^2 > 2^-100 (w_p.w_p)(w_q.w_q); stop after the first sweep that rotated
  nothing, at most MAX_SWEEPS sweeps.  The result is W = M V with orthogonal columns w_j = sigma_j u_j.
* R0 = U (U^T M / sigma), U = W / sigma column-wise and row j of U^T M divided by sigma_j: U V^T without V ever being
  formed (V^T = S^-1 U^T M).  Its error grows with kappa = sigma_max / sigma_min -- as does the conditioning of the polar
  factor itself (first order: |dR| <= |dM| / sigma_min).
* One Newton-Schulz step R = 1/2 R0 (3 I - R0^T R0): orthogonality back to rounding, R moved by a second-order amount only.
* scale = sum_j sigma_j, SciPy's second return value.

Reflections are allowed, as in SciPy: det R may be -1.
"""
from __future__ import annotations

import numpy as np

from .dbscan import FLAG_NONFINITE   # 2: a non-finite entry in A or B (SciPy raises ValueError there)

FLAG_ILLCOND = 4    # sigma_max == 0 or sigma_min <= ILLCOND_RATIO sigma_max: the data do not determine R (m < r, zero columns, ...)
FLAG_NOCONV = 8     # the sweep cap was hit
MAX_SWEEPS = 30
MAX_R = 128         # csrc/procrustes.hip: an r x r fp64 matrix with a padded pitch in one CU's LDS
ROT_THRESHOLD = 2.0 ** -100
# The polar factor moves by |dM| / sigma_min for a perturbation dM of M, and M itself is known to about
# 2^-52 (r + sqrt(m)) | |A|^T |B| |_F (see `unit`).  With sigma_min > 2^-14 sigma_max, r <= 128 and the windows in use
# (m <= 10^4, | |A|^T |B| |_F <= r sigma_max) that keeps 4 units below 4 * 2^-52 * 228 * 128 * 2^14 = 4e-7 in the worst case and
# below 1e-8 wherever kappa <= 400 -- the level the eigenstep's parity tests assert.  Past the ratio the answer is SciPy's.
ILLCOND_RATIO = 2.0 ** -14

NONFINITE_TEXT = "array must not contain infs or NaNs"   # (SciPy's check_finite text)


def schedule(r):
    """The round-robin order of one sweep over r columns: a list of steps, each a pair of index arrays (P, Q) with P < Q
    elementwise, the pairs of one step disjoint.  Circle method on n2 = r rounded up to even: step s pairs s with n2 - 1
    and (s + k) mod (n2 - 1) with (s - k) mod (n2 - 1) for k = 1 .. n2 / 2 - 1; with r odd the pair that holds column r (which
    does not exist) is that step's bye."""
    n2 = r + (r & 1)
    nm = n2 - 1
    steps = []
    for s in range(nm):
        k = np.arange(n2 // 2)
        x = np.where(k == 0, s, (s + k) % max(nm, 1))
        y = np.where(k == 0, nm, (s - k + nm) % max(nm, 1))
        p, q = np.minimum(x, y), np.maximum(x, y)
        keep = q < r
        steps.append((p[keep], q[keep]))
    return steps


def jacobi_columns(M):
    """Hestenes sweeps on a copy of M (r x r) -> (W, sweeps, converged)."""
    W = np.array(M, dtype=np.float64)
    steps = schedule(W.shape[1])
    sweeps, rotated = 0, True
    while rotated and sweeps < MAX_SWEEPS:
        rotated = False
        sweeps += 1
        for P, Q in steps:
            if P.size == 0:
                continue
            wp, wq = W[:, P], W[:, Q]
            a, b, c = (wp * wp).sum(0), (wq * wq).sum(0), (wp * wq).sum(0)
            rot = c * c > ROT_THRESHOLD * a * b
            if not rot.any():
                continue
            rotated = True
            cc = np.where(rot, c, 1.0)
            zeta = (b - a) / (2.0 * cc)
            t = np.where(zeta < 0.0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            cs = 1.0 / np.sqrt(1.0 + t * t)
            sn = cs * t
            cs, sn = np.where(rot, cs, 1.0), np.where(rot, sn, 0.0)
            W[:, P], W[:, Q] = cs * wp - sn * wq, sn * wp + cs * wq
    return W, sweeps, not rotated


def orthogonal_procrustes_rule(A, B):
    """(R, scale, flags, sweeps) for A, B of shape (m, r), fp64: R (r x r) orthogonal minimising |A R - B|_F, scale = the sum of
    the singular values of A^T B.  flags: FLAG_NONFINITE (R is NaN, nothing was computed), FLAG_ILLCOND, FLAG_NOCONV; with
    either of the last two R is what the steps gave and is not to be relied on."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or A.shape != B.shape:
        raise ValueError(f"the shapes of A and B differ ({A.shape} vs {B.shape})")
    r = A.shape[1]
    if r < 1:
        raise ValueError("A and B need at least one column")
    with np.errstate(all="ignore"):   # (flagged inputs overflow and divide by zero on their way to the flag)
        return _rule(A, B, r)


def _rule(A, B, r):
    M = A.T @ B
    if not np.isfinite(M).all() or not (np.isfinite(A).all() and np.isfinite(B).all()):
        return np.full((r, r), np.nan), float("nan"), FLAG_NONFINITE, 0
    W, sweeps, converged = jacobi_columns(M)
    flags = 0 if converged else FLAG_NOCONV
    sig = np.sqrt((W * W).sum(0))
    smax, smin = sig.max(), sig.min()
    if smax == 0.0 or smin <= ILLCOND_RATIO * smax:
        flags |= FLAG_ILLCOND
    safe = np.where(sig > 0.0, sig, 1.0)
    U = W / safe
    R0 = U @ ((U.T @ M) / safe[:, None])
    R = 0.5 * (R0 @ (3.0 * np.eye(r) - R0.T @ R0))
    return R, float(sig.sum()), flags, sweeps


def align_rule(E_new, E_ref, shift):
    """(E_new @ R, R, residual, unaligned): R carries the rows the two windows share, A = E_new[:W - shift], onto
    B = E_ref[shift:]; residual = |A R - B|_F / |B|_F, unaligned = |A - B|_F / |B|_F.  Raises ValueError for a non-finite
    entry; a flagged rule (FLAG_ILLCOND, FLAG_NOCONV) is answered by SciPy."""
    E_new = np.asarray(E_new, dtype=np.float64)
    E_ref = np.asarray(E_ref, dtype=np.float64)
    W = E_new.shape[0]
    if E_new.ndim != 2 or E_new.shape != E_ref.shape or not 0 < int(shift) < W:
        raise ValueError(f"need two (W, r) windows and 0 < shift < W, got {E_new.shape}, {E_ref.shape}, shift {shift!r}")
    A, B = E_new[:W - int(shift)], E_ref[int(shift):]
    R, _, flags, _ = orthogonal_procrustes_rule(A, B)
    if flags & FLAG_NONFINITE:
        raise ValueError(NONFINITE_TEXT)
    if flags:
        from scipy.linalg import orthogonal_procrustes

        R = orthogonal_procrustes(A, B)[0]
    nb = np.linalg.norm(B)
    return E_new @ R, R, float(np.linalg.norm(A @ R - B) / nb), float(np.linalg.norm(A - B) / nb)


def unit(A, B):
    """u(A, B) = 2^-52 (r + sqrt(m)) | |A|^T |B| |_F / sigma_r(A^T B): what one rounding-level perturbation of M = A^T B (the
    rounding of length-m dot products, |dM| <= about 2^-52 sqrt(m) .. m times |A|^T |B| entrywise, and of the r-term sums
    behind it) moves the polar factor by, from |dR| <= |dM| / sigma_r.  sigma_r from NumPy's SVD.  Two correct evaluations
    are allowed 4 u apart."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    m, r = A.shape
    s = np.linalg.svd(A.T @ B, compute_uv=False)
    return 2.0 ** -52 * (r + np.sqrt(m)) * np.linalg.norm(np.abs(A).T @ np.abs(B)) / s[-1]
