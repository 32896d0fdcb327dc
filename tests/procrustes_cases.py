"""Inputs shared by the Procrustes tests: B = A Q + noise with a chosen conditioning of A^T B, reflections, and the degenerate
sets the flags are for.  Plain NumPy."""
import numpy as np


def orthogonal(r, rng, det=None):
    """A Haar-ish r x r orthogonal matrix (QR of a Gaussian, signs fixed); det = +1 / -1 on request."""
    Q, T = np.linalg.qr(rng.standard_normal((r, r)))
    Q = Q * np.where(np.diag(T) < 0, -1.0, 1.0)
    if det is not None and np.sign(np.linalg.det(Q)) != det:
        Q[:, 0] = -Q[:, 0]
    return Q


def conditioned(m, r, rng, cond=16.0, mean=0.0):
    """A (m x r, m >= r) = P diag(s) Z^T with orthonormal P, orthogonal Z and singular values from 1 down to cond^-1/2, so that
    A^T A -- and A^T B for B close to A Q -- has sigma_1 / sigma_r = cond: far above the 2^14 of FLAG_ILLCOND.  `mean` is added
    to every entry (nonzero column means, as embeddings have in their leading column)."""
    P = np.linalg.qr(rng.standard_normal((m, r)))[0]
    s = np.geomspace(1.0, cond ** -0.5, r) if r > 1 else np.ones(1)
    return (P * s) @ orthogonal(r, rng).T + mean


def pair(m, r, seed, cond=16.0, noise=1e-3, det=None, mean=0.0):
    """(A, B, Q): B = A Q + noise * Gaussian / sqrt(m)."""
    rng = np.random.default_rng(seed)
    A = conditioned(m, r, rng, cond, mean)
    Q = orthogonal(r, rng, det)
    B = A @ Q + noise * rng.standard_normal((m, r)) / np.sqrt(m)
    return A, B, Q


# (m, r, cond, noise, det of Q, mean): the table of the host test -- small, every r parity, a reflection, scaled columns,
# nonzero means, m = r, and one case at the kernel's ceiling
HOST_CASES = [
    (5, 1, 1.0, 1e-3, None, 0.0),
    (9, 2, 4.0, 1e-3, None, 0.0),
    (40, 3, 16.0, 1e-2, -1, 0.0),
    (7, 7, 16.0, 1e-3, None, 0.0),
    (300, 8, 8e3, 1e-4, None, 0.0),     # sigma_r / sigma_1 = 1.25e-4: twice the flag's 2^-14
    (257, 16, 64.0, 1e-3, 1, 0.05),
    (700, 50, 100.0, 1e-3, -1, 0.02),
    (200, 65, 16.0, 1e-3, None, 0.0),
    (400, 128, 16.0, 1e-3, None, 0.0),
]


def degenerate():
    """name -> (A, B): inputs that FLAG_ILLCOND is for."""
    rng = np.random.default_rng(7)
    A1, B1 = rng.standard_normal((3, 5)), rng.standard_normal((3, 5))          # m < r: A^T B has rank 3
    A2, B2, _ = pair(60, 6, 8)
    A2 = A2.copy()
    A2[:, 2] = 0.0                                                               # a zero column: a zero row of A^T B
    return {"m_below_r": (A1, B1), "zero_column": (A2, B2)}


def nonfinite():
    A, B, _ = pair(30, 4, 9)
    A, B = A.copy(), B.copy()
    A[3, 1] = np.nan
    B2 = B.copy()
    B2[5, 0] = np.inf
    return {"nan_in_A": (A, B), "inf_in_B": (pair(30, 4, 9)[0], B2)}
