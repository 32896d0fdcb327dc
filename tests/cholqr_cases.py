"""Inputs shared by tests/test_cholqr_host.py and tests/test_gpu_cholqr.py: the case table of the eigenstep's Cholesky-QR
(csrc/rsvd.hip: gram_reduce_kernel, chol_kernel, trsm_rows_kernel, panel_sub_kernel and the two-block path), a plain fp64
restatement of every step with named wrong variants, and the bounds both tests assert, evaluated in np.longdouble.

One pass on an n x r panel Y (pitch r):
  r <= 143    G = Y^T Y,  delta = 16 r eps max diag G,  L L^T = G + delta I,  Q = Y L^-T
  r <= 286    the columns in two halves r1 = r // 2, r2 = r - r1:  Q1 = pass(Y1),  P = Q1^T Y2,  Y2' = Y2 - Q1 P,  Q2 = pass(Y2')

Every bound is a rounding-error theorem for ANY summation order, with eps = 2^-52 (twice the unit roundoff, which pays
for the second-order terms), elementwise; `ratio` below is max |error| / bound, so a bound holds when its ratio is <= 1.
  gram     |G - Y^T Y|               <= (n + 2) eps |Y|^T |Y|          n products and n - 1 additions per entry, in any tree
  factor   |L L^T - (G + delta I)|   <= 2 (r + 2) eps |L| |L|^T        gamma_{r+1} of a Cholesky (Higham, Accuracy and
           Stability, thm 10.3), doubled: the device takes 1 / sqrt(pivot) from v_rsq_f64 and two Newton steps and
           multiplies by it, which is not correctly rounded.  delta is recomputed from the device's G: (16 r eps) is exact
           and its product with max diag G has one rounding, in the kernel and in NumPy alike.
  solve    |Q L^T - Y|               <= 2 (r + 2) eps |Q| |L|^T        gamma_r of a substitution (Higham thm 8.5), doubled
  two-block, with Q1, Q2, L2 of the device and W = |Q2| |L2|^T, Pa = |Q1|^T |Y2|:
    project  |Y2 - Q1 (Q1^T Y2) - Q2 L2^T| <= eps ((n + 2) + (r1 + 2)) |Q1| Pa + eps (|Y2| + |Q1| Pa) + 2 (r2 + 2) eps W
             a split-K product of length n (error (n + 2) eps Pa, carried through |Q1|), a product of length r1 with the
             computed P (|P| <= Pa to first order), one subtraction of numbers below |Y2| + |Q1| Pa, one solve of order r2
    gram2    |G2 - Z^T Z| <= (n + 2 + 4 (r2 + 2) + 1) eps W^T W  for Z = Q2 L2^T: the panel the Gram was taken of is
             Z - E with |E| <= 2 (r2 + 2) eps W, |Z| <= W, so Z^T Z moves by at most 2 * 2 (r2 + 2) eps W^T W (+ E^T E)
  two passes (the final basis)   max |Q^T Q - I| <= 6 (n r + r (r + 1)) eps   (Yamamoto, Nakatsukasa, Yanagisawa, Fukaya 2015)
             and <= 4 x what the fp64 restatement leaves on the same case (another summation order, nothing more).

Weak-pivot word: chol_kernel raises it when a raw pivot is not above 1e-11 max diag G.  PIVOT_HIGH / PIVOT_LOW keep every case
away from that line: the smallest pivot of the UNSHIFTED longdouble Cholesky of the block's exact Gram, over max diag G,
lies above 1e-9 or below 1e-13.  The shift moves a pivot by about delta <= 16 * 143 eps = 5.1e-13 of max diag G and fp64
rounding by less, so neither can carry a case across 1e-11.  A case that misses gets another seed; it is not exempted."""
import dataclasses
import functools

import numpy as np
import scipy.linalg

LD = np.longdouble
EPS = 2.0 ** -52
MAX_R = 143            # CHOLQR_MAX_R: the largest single block
CH_NB = 9              # chol_kernel keeps 16 x CH_NB rows in registers
WEAK_REL = 1e-11
PIVOT_HIGH, PIVOT_LOW = 1e-9, 1e-13
VARIANTS = ("no_delta", "tail_unsolved", "last_rows_zeroed", "l_entry_off")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    n: int
    r: int
    data: str      # gauss | orth (cond 1) | graded (cond 1e3) | adj (0/1 adjacency times a Gaussian panel)
    #                zero_col | dup_col | low_rank (rank r - 1, small integers: exact)  -- these raise the weak-pivot word
    seed: int = 0

    @property
    def weak(self):
        return self.data in ("zero_col", "dup_col", "low_rank")

    @property
    def blocks(self):
        return (self.r,) if self.r <= MAX_R else (self.r // 2, self.r - self.r // 2)


def _case(n, r, data, seed=0):
    return Case(f"{data}_n{n}_r{r}", n, r, data, seed)


# the smallest shapes that reach every branch (tests/test_cholqr_host.py asserts which)
TABLE = [
    _case(1, 1, "gauss"), _case(65, 1, "gauss"),
    _case(63, 2, "gauss"),
    _case(3, 3, "gauss"), _case(64, 3, "graded"),
    _case(65, 4, "gauss"), _case(64, 4, "orth"),
    _case(127, 5, "graded"),
    _case(15, 15, "gauss"), _case(129, 15, "adj"),
    _case(64, 16, "gauss"),
    _case(17, 17, "gauss"), _case(65, 17, "graded"),
    _case(60, 60, "gauss"), _case(127, 60, "graded"), _case(333, 60, "adj"),
    _case(333, 138, "gauss"), _case(1000, 138, "adj"),
    _case(143, 143, "gauss"), _case(333, 143, "graded"), _case(333, 143, "orth"),
    _case(144, 144, "gauss"), _case(333, 144, "graded"),
    _case(333, 145, "gauss"),
    _case(333, 266, "adj"),
    _case(286, 286, "gauss"), _case(1000, 286, "gauss"),
    # exactly rank deficient
    _case(65, 5, "zero_col"), _case(127, 17, "dup_col"), _case(129, 60, "low_rank"),
    _case(333, 145, "dup_col"), _case(333, 266, "zero_col"),
]
IDS = [c.name for c in TABLE]
SINGLE = [c for c in TABLE if len(c.blocks) == 1]
TWO_BLOCK = [c for c in TABLE if len(c.blocks) == 2]


def yamamoto(n, r):
    return 6.0 * (n * r + r * (r + 1)) * EPS


# Two passes make an orthonormal basis of these.  The second pass's own shift leaves delta / pivot = 16 r_block eps on the
# diagonal of Q^T Q - I, which Yamamoto's bound (no shift in their algorithm) does not budget for: it is asserted where it
# leaves that shift as much room again for rounding, which excludes the 1 x 1 panel alone (18 eps against 16 eps).
SOUND = [c for c in TABLE if not c.weak and yamamoto(c.n, c.r) >= 32 * max(c.blocks) * EPS]


@functools.lru_cache(maxsize=None)
def panel(c):
    """Y of a case (n x r, fp64, read-only)."""
    n, r = c.n, c.r
    rng = np.random.default_rng([n, r, c.seed, sum(map(ord, c.data))])
    if c.data == "gauss":
        Y = rng.standard_normal((n, r))
    elif c.data in ("orth", "graded"):
        Qo = np.linalg.qr(rng.standard_normal((n, r)))[0]
        s = np.full(r, 3.0) if c.data == "orth" else np.logspace(0.0, -3.0, r)
        Y = Qo * s
    elif c.data == "adj":
        A = (rng.random((n, n)) < 0.1).astype(np.float64)
        Y = A @ rng.standard_normal((n, r))
    elif c.data == "zero_col":
        Y = rng.standard_normal((n, r))
        Y[:, (2 * r) // 3] = 0.0
    elif c.data == "dup_col":
        Y = rng.standard_normal((n, r))
        Y[:, r - 2] = Y[:, 1]          # (two-block cases: column 1 is in the first half, r - 2 in the second)
    elif c.data == "low_rank":
        Y = (rng.integers(-3, 4, (n, r - 1)) @ rng.integers(-2, 3, (r - 1, r))).astype(np.float64)
    else:
        raise KeyError(c.data)
    Y = np.ascontiguousarray(Y)
    Y.setflags(write=False)
    return Y


# ---- the fp64 restatement ------------------------------------------------------------------------------------------
def unpack(Lp, r):
    """packed rows of a lower triangle (entry (i, k) at i (i + 1) / 2 + k) -> r x r"""
    L = np.zeros((r, r), dtype=np.asarray(Lp).dtype)
    L[np.tril_indices(r)] = Lp
    return L


def shift_of(G, r):
    return 16.0 * r * EPS * float(np.max(np.diag(G)))


def chol_shifted(G, delta, dtype=np.float64):
    """Right-looking Cholesky of G + delta I as chol_kernel runs it: the shift joins the pivot, a pivot that is not above
    the shift is replaced by it.  Returns L and the raw pivots."""
    A = np.array(G, dtype=dtype)
    r = len(A)
    L = np.zeros_like(A)
    piv = np.zeros(r, dtype=dtype)
    delta = dtype(delta)
    for j in range(r):
        piv[j] = A[j, j]
        pc = A[j, j] + delta
        if not pc > delta:
            pc = delta
        d = np.sqrt(pc)
        L[j, j] = d
        L[j + 1:, j] = A[j + 1:, j] / d
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L, piv


def restate_block(Y, variant=None):
    """One single-block pass in fp64: (Q, G, L, weak)."""
    n, r = Y.shape
    G = Y.T @ Y
    G = np.triu(G) + np.triu(G, 1).T
    delta = shift_of(G, r)
    L, piv = chol_shifted(G, 0.0 if variant == "no_delta" else delta)
    weak = int(not np.all(piv > WEAK_REL * np.max(np.diag(G))))
    if variant == "l_entry_off":
        i, k = np.unravel_index(np.argmax(np.abs(L)), L.shape)
        L[i, k] *= 1.0 + 1e-10
    Q = scipy.linalg.solve_triangular(L, Y.T, lower=True).T
    if variant == "tail_unsolved" and r % 4:
        Q[:, r - r % 4:] = Y[:, r - r % 4:]
    if variant == "last_rows_zeroed" and n % 64:
        Q[n - n % 64:] = 0.0
    return np.ascontiguousarray(Q), G, L, weak


def restate(Y, variant=None):
    """One pass in fp64 on either path: (Q, G, L, weak) with G, L of the last block factorised."""
    n, r = Y.shape
    if r <= MAX_R:
        return restate_block(Y, variant)
    r1 = r // 2
    Q1, _, _, w1 = restate_block(Y[:, :r1], variant)
    P = Q1.T @ Y[:, r1:]
    Q2, G2, L2, w2 = restate_block(Y[:, r1:] - Q1 @ P, variant)
    return np.ascontiguousarray(np.hstack([Q1, Q2])), G2, L2, w1 | w2


@functools.lru_cache(maxsize=None)
def restated_orthogonality(c):
    """max |Q^T Q - I| after two fp64 passes on the case."""
    return orthogonality(restate(restate(panel(c))[0])[0])


# ---- the bounds, in longdouble ---------------------------------------------------------------------------------------
def ratio(err, bound):
    err, bound = np.abs(np.asarray(err, dtype=LD)), np.asarray(bound, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(np.max(q))


def gram_ratio(Y, G):
    n = Y.shape[0]
    Yl = np.asarray(Y, dtype=LD)
    return ratio(np.asarray(G, dtype=LD) - Yl.T @ Yl, (n + 2) * EPS * (np.abs(Yl).T @ np.abs(Yl)))


def factor_ratio(G, L):
    r = len(L)
    Ll, Gl = np.asarray(L, dtype=LD), np.asarray(G, dtype=LD)
    target = Gl + LD(shift_of(G, r)) * np.eye(r, dtype=LD)
    return ratio(Ll @ Ll.T - target, 2 * (r + 2) * EPS * (np.abs(Ll) @ np.abs(Ll).T))


def solve_ratio(Y, Q, L):
    r = len(L)
    Ql, Ll = np.asarray(Q, dtype=LD), np.asarray(L, dtype=LD)
    return ratio(Ql @ Ll.T - np.asarray(Y, dtype=LD), 2 * (r + 2) * EPS * (np.abs(Ql) @ np.abs(Ll).T))


def single_block_ratios(Y, Q, G, L):
    return {"gram": gram_ratio(Y, G), "factor": factor_ratio(G, L), "solve": solve_ratio(Y, Q, L)}


def two_block_ratios(Y, Q, G2, L2):
    """The second block of a two-block pass from what the pass returns (see the module docstring)."""
    n, r = Y.shape
    r1 = r // 2
    r2 = r - r1
    Yl, Ql, Ll = np.asarray(Y, dtype=LD), np.asarray(Q, dtype=LD), np.asarray(L2, dtype=LD)
    Y2, Q1, Q2 = Yl[:, r1:], Ql[:, :r1], Ql[:, r1:]
    Z = Q2 @ Ll.T
    W = np.abs(Q2) @ np.abs(Ll).T
    Pa = np.abs(Q1).T @ np.abs(Y2)
    QPa = np.abs(Q1) @ Pa
    project = Y2 - Q1 @ (Q1.T @ Y2) - Z
    bound = EPS * ((n + 2) + (r1 + 2)) * QPa + EPS * (np.abs(Y2) + QPa) + 2 * (r2 + 2) * EPS * W
    return {"project": ratio(project, bound),
            "gram2": ratio(np.asarray(G2, dtype=LD) - Z.T @ Z, (n + 2 + 4 * (r2 + 2) + 1) * EPS * (W.T @ W)),
            "factor": factor_ratio(G2, L2)}


def pass_ratios(Y, Q, G, L):
    return single_block_ratios(Y, Q, G, L) if Y.shape[1] <= MAX_R else two_block_ratios(Y, Q, G, L)


def orthogonality(Q):
    Ql = np.asarray(Q, dtype=LD)
    return float(np.max(np.abs(Ql.T @ Ql - np.eye(Ql.shape[1], dtype=LD))))


# ---- the weak-pivot margin -------------------------------------------------------------------------------------------
def _unshifted_pivot(Yl):
    """smallest pivot of the longdouble Cholesky of Yl^T Yl over its largest diagonal entry (stops at a pivot <= 0)"""
    A = Yl.T @ Yl
    gmax = np.max(np.diag(A))
    if gmax == 0:
        return 0.0
    low = LD(np.inf)
    for j in range(len(A)):
        p = A[j, j]
        low = min(low, p)
        if not p > 0:
            break
        col = A[j + 1:, j] / np.sqrt(p)
        A[j + 1:, j + 1:] -= np.outer(col, col)
    return float(low / gmax)


@functools.lru_cache(maxsize=None)
def smallest_pivot(c):
    """min over the blocks a pass factorises (the second block: of Y2 - Q1 (Q1^T Y2) with the shifted Q1, in longdouble)"""
    Yl = np.asarray(panel(c), dtype=LD)
    if len(c.blocks) == 1:
        return _unshifted_pivot(Yl)
    r1 = c.blocks[0]
    Y1, Y2 = Yl[:, :r1], Yl[:, r1:]
    G1 = Y1.T @ Y1
    L1, _ = chol_shifted(G1, LD(16 * r1 * EPS) * np.max(np.diag(G1)), dtype=LD)
    # Q1 = Y1 L1^-T by substitution in longdouble (scipy has no longdouble solver)
    Q1 = np.zeros_like(Y1)
    for k in range(r1):
        Q1[:, k] = (Y1[:, k] - Q1[:, :k] @ L1[k, :k]) / L1[k, k]
    return min(_unshifted_pivot(Y1), _unshifted_pivot(Y2 - Q1 @ (Q1.T @ Y2)))
