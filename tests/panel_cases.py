"""Inputs shared by tests/test_panel_cases_host.py and tests/test_gpu_panel.py: the case tables of the LU and Householder panel
kernels (csrc/panel.hip: lu_permute_l in its three variants, qr_economic), plain fp64 restatements of both with named wrong
variants, and the bounds both tests assert, evaluated in np.longdouble with eps = 2^-52; `ratio` is max |error| / bound.

LU (P L of partial pivoting, rows never swapped; k = min(n, r) columns; pivstep[row] = step + 1, 0 = never a pivot)
  rule       largest |a| among unpivoted rows, ties to the smallest ORIGINAL row; l = a * (1 / piv), l = a when piv == 0
  structure  exact: the nonzero pivstep are 1 .. k once each; pivot row s of PL is (l.., 1, 0..); |PL| <= 1 + 2 eps
             (|a| <= |piv|; the reciprocal and the product round once each)
  backward   p = the pivot rows in step order, L1 = PL[p] (unit lower triangular), U' = L1^-1 Y[p] by longdouble substitution,
             R = Y - PL U':   |R| <= 2 (k + 2) eps (|PL| |U'| + |PL| |L1^-1| |L1| |U'|),  R == 0 where the bound is 0.
             First term: Higham, Accuracy and Stability, thm 9.3 (gamma_k |L| |U|), doubled for the reciprocal multiply.  Second
             term: U itself is not returned; U' is recomputed from the pivot rows of Y, whose own residual (first term, rows p)
             goes through L1^-1 into U' and through PL into every row.
  order      pivstep equals the restatement's where the order is DETERMINED: either the case is exact (below), or in the
             longdouble elimination runner-up / winner <= 1 - GAP at every step (gap()), rows that are bit-for-bit copies of the
             winner's row of Y aside -- those tie with it in any arithmetic and the tie rule decides.  A case that misses the
             condition gets another seed.  `order=False` marks the one kind for which no seed can help: adj_dup with r above
             its number of distinct rows, where every step past the rank picks among rounding residues (the kernels may fuse
             the multiply-add, the restatement does not).  Its structure, backward error and the variants' bit-identity are
             asserted all the same.
  exact      hadamard, zeros, zero_col: the fp64 elimination has no rounding (exact_lu() repeats it in fractions.Fraction), so
             the device equals the restatement bit for bit, and every step is a tie among many rows.
  scale      Y 2^200 and Y 2^-200 give the bits of Y (LU and QR): nothing but exponents changes.

QR (economic Q of Householder reflections, dlarfg convention: beta = -sign(alpha) hypot(alpha, |x|), tau = (beta - alpha) /
beta, v = x / (alpha - beta), tau = 0 when x == 0; Q = H_0 .. H_{r-1} I[:, :r])
  orth       max |Q^T Q - I|                      <= n r eps
  span       |Y - Q (Q^T Y)|          column-wise <= n r eps ||y_j||_2
  tri        strict lower part of Q^T Y            <= n r eps ||y_j||_2
             all three: Higham thm 19.4 (gamma~_{n r} with constant 1, first order)
  sign       diag(Q^T Y)_j = -sign(alpha_j) |.| where tau_j != 0, = alpha_j where tau_j = 0, with alpha_j, tau_j of the
             restatement: asserted as a sign where |beta_j| > SIGN_REL ||y_j|| (a relative 1e-6 is 10^9 roundings away for these
             kinds: gauss, orth, graded (cond 1e3), zero_col, zero_sub, zeros), and as a value within the tri bound on the
             columns zero_sub builds so that alpha is exact
  scipy      against scipy.linalg.qr at atol 1e-11 on gauss and orth"""
import dataclasses
import fractions
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
GAP = 1e-9
SIGN_REL = 1e-6
LU_NB = 4                # columns per blocked panel
PANEL3_MAX, PANEL10_MAX = 3072, 10240   # rows of lu_panel_kernel<3>, <10>; above: the column-at-a-time kernels
QR_CHUNK = 512           # rows per workgroup of qr_dot_kernel
LU_VARIANTS = ("tie_last", "tie_position", "skip_last_update", "panel_tail")
QR_VARIANTS = ("sign", "chunk_dropped", "tau0_not_skipped")
DISTINCT = 20            # distinct rows of adj_dup
EXACT_KINDS = ("hadamard", "zeros", "zero_col")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    n: int
    r: int
    data: str
    seed: int = 0
    order: bool = True     # LU: the pivot order is asserted (see the module docstring)

    @property
    def k(self):
        return min(self.n, self.r)

    @property
    def exact(self):
        return self.data in EXACT_KINDS


def _lu(n, r, data, seed=0, order=True):
    return Case(f"lu_{data}_n{n}_r{r}", n, r, data, seed, order)


def _qr(n, r, data, seed=0):
    return Case(f"qr_{data}_n{n}_r{r}", n, r, data, seed)


_LU_NS = (1, 3, 15, 16, 17, 33, 1023, 1024, 1025, 2049, 3072, 3073, 10240, 10241)
_LU_RS = (1, 2, 3, 4, 5, 7, 8, 9)
LU_TABLE = [_lu(n, _LU_RS[i % len(_LU_RS)], "gauss") for i, n in enumerate(_LU_NS)] + [
    # every tail nbe of a 4-panel in lu_panel_kernel<10> as well (the cycle gives it nbe = 4 and 1), its largest panel
    _lu(3073, 7, "gauss"), _lu(10240, 2, "gauss"), _lu(10240, 9, "gauss"),
    _lu(300, 139, "gauss"),
    # r > n; the last takes the `+= 1024` loops over the columns into a second trip
    _lu(3, 7, "gauss"), _lu(8, 12, "gauss"), _lu(40, 1030, "gauss"),
    _lu(300, 139, "adj"), _lu(1025, 9, "adj"),
    _lu(300, 17, "adj_dup"), _lu(2049, 5, "adj_dup"), _lu(300, 139, "adj_dup", order=False),
    _lu(33, 7, "hadamard"), _lu(1025, 9, "hadamard"), _lu(2049, 5, "hadamard"), _lu(3200, 8, "hadamard"),
    _lu(10241, 4, "hadamard"), _lu(8, 12, "hadamard"),
    _lu(17, 5, "zeros"), _lu(3073, 3, "zeros"), _lu(3, 7, "zeros"),
    _lu(33, 7, "zero_col"), _lu(1025, 9, "zero_col"), _lu(3073, 8, "zero_col"), _lu(10241, 5, "zero_col"),
]
QR_TABLE = [
    _qr(1, 1, "gauss"), _qr(2, 1, "gauss"), _qr(2, 2, "gauss"), _qr(16, 15, "gauss"), _qr(16, 16, "gauss"),
    _qr(17, 16, "gauss"), _qr(17, 17, "gauss"), _qr(511, 2, "gauss"), _qr(511, 63, "gauss"), _qr(512, 64, "gauss"),
    _qr(513, 16, "gauss"), _qr(513, 65, "gauss"), _qr(1024, 1, "gauss"), _qr(1024, 64, "gauss"), _qr(1025, 2, "gauss"),
    _qr(1025, 65, "gauss"), _qr(1030, 15, "gauss"), _qr(1030, 17, "gauss"), _qr(1030, 63, "gauss"),
    _qr(40, 40, "gauss"), _qr(1030, 138, "gauss"), _qr(520, 515, "gauss"),
    _qr(513, 65, "orth"), _qr(17, 17, "orth"), _qr(511, 63, "graded"),
    _qr(1030, 138, "adj"), _qr(513, 63, "adj_dup"), _qr(1025, 16, "adj_dup"),
    _qr(17, 16, "zeros"), _qr(513, 2, "zeros"), _qr(1, 1, "zeros"),
    _qr(513, 17, "zero_col"), _qr(40, 40, "zero_col"), _qr(1030, 64, "zero_col"),
    _qr(17, 15, "zero_sub"), _qr(1025, 16, "zero_sub"), _qr(2, 2, "zero_sub"),
]
LU_IDS = [c.name for c in LU_TABLE]
QR_IDS = [c.name for c in QR_TABLE]
# scale invariance: one case per route and data kind that is not all zeros
LU_SCALED = [c for c in LU_TABLE if c.name in (
    "lu_gauss_n33_r7", "lu_gauss_n1024_r9", "lu_gauss_n3073_r4", "lu_gauss_n10241_r7", "lu_gauss_n40_r1030",
    "lu_adj_dup_n300_r139", "lu_zero_col_n1025_r9")]
QR_SCALED = [c for c in QR_TABLE if c.name in (
    "qr_gauss_n17_r17", "qr_gauss_n513_r65", "qr_gauss_n1030_r17", "qr_zero_col_n513_r17", "qr_adj_dup_n513_r63",
    "qr_zero_sub_n1025_r16")]
SCALES = (2.0 ** 200, 2.0 ** -200)
QR_WELL = ("gauss", "orth")                                            # compared with scipy.linalg.qr
QR_SIGNED = ("gauss", "orth", "graded", "zero_col", "zero_sub", "zeros")  # the sign of diag(Q^T Y) is asserted


def lu_route(c):
    """what csrc/panel.hip runs by default: 'panel3' / 'panel10' (blocked, lu_panel_kernel<3> / <10>) or 'column'"""
    return "panel3" if c.n <= PANEL3_MAX else "panel10" if c.n <= PANEL10_MAX else "column"


def lu_tails(c):
    """nbe of every blocked panel of the case"""
    return [min(LU_NB, c.k - j0) for j0 in range(0, c.k, LU_NB)]


# ---- data ------------------------------------------------------------------------------------------------------------
def hadamard(order):
    H = np.ones((1, 1))
    while len(H) < order:
        H = np.block([[H, H], [H, -H]])
    return H


def _hadamard_rows(n, r, rng, far=False):
    """which row of the order-64 Sylvester-Hadamard matrix each of the n rows repeats: every row in turn, then a fixed
    permutation.  far (r a power of two, so that the r distinct rows H[:, :r] has are independent): the rows that repeat the
    last of them are moved behind row PANEL3_MAX, so that the last pivot and the rows it ties with lie there."""
    t = rng.permutation(np.arange(n) % 64)
    if far:
        assert r & (r - 1) == 0 and n > PANEL3_MAX + 2
        low = t[:PANEL3_MAX]
        low[low % r == r - 1] -= 1      # (the first r columns of row t are those of row t % r)
        t[PANEL3_MAX:] = np.where(np.arange(n - PANEL3_MAX) % 3 == 0, t[PANEL3_MAX:] // r * r + r - 1, t[PANEL3_MAX:])
    return t


def _adj_panel(n, r, rng, dup):
    A = (rng.random((n, n)) < min(0.1, 30.0 / n)).astype(np.float64)
    Y = A @ rng.standard_normal((n, r))
    if dup:   # DISTINCT rows at random places, every other row a bit-for-bit copy of one of them
        keep = np.sort(rng.permutation(n)[:DISTINCT])
        src = keep[rng.integers(0, DISTINCT, n)]
        src[keep] = keep
        Y = Y[src]
    return Y


@functools.lru_cache(maxsize=None)
def panel(c):
    """Y of a case (n x r, fp64, read-only)."""
    n, r = c.n, c.r
    rng = np.random.default_rng([n, r, c.seed, sum(map(ord, c.data))])
    if c.data == "gauss":
        Y = rng.standard_normal((n, r))
    elif c.data in ("orth", "graded"):
        Qo = np.linalg.qr(rng.standard_normal((n, r)))[0]
        Y = Qo * (np.full(r, 3.0) if c.data == "orth" else np.logspace(0.0, -3.0, r))
    elif c.data in ("adj", "adj_dup"):
        Y = _adj_panel(n, r, rng, c.data == "adj_dup")
    elif c.data == "zeros":
        Y = np.zeros((n, r))
    elif c.data == "hadamard":
        Y = hadamard(64)[_hadamard_rows(n, min(r, 64), rng, far=PANEL3_MAX < n <= PANEL10_MAX)][:, :r]
    elif c.data == "zero_col" and c.name.startswith("lu_"):
        # small integers whose elimination is exact: Hadamard rows times 1, 2 or 4 (pivots stay powers of two, and a step
        # is a tie among the rows of the largest factor only); one column zero
        Y = hadamard(64)[_hadamard_rows(n, r, rng)][:, :r] * rng.choice([1.0, 2.0, 4.0], size=(n, 1))
        Y[:, (2 * r) // 3] = 0.0
    elif c.data == "zero_col":
        Y = rng.standard_normal((n, r))
        Y[:, (2 * r) // 3] = 0.0
    elif c.data == "zero_sub":
        # columns 0 and 1 are zero below their diagonal entries, -2.5 and +1.5: tau_0 = tau_1 = 0, H_0 = H_1 = I exactly
        Y = rng.standard_normal((n, r))
        Y[:, 0] = 0.0
        Y[0, 0] = -2.5
        if r > 1:
            Y[:, 1] = 0.0
            Y[0, 1], Y[1, 1] = 0.75, 1.5
    else:
        raise KeyError(c.data)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    Y.setflags(write=False)
    return Y


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- LU: the restatement -------------------------------------------------------------------------------------------------
def lu_restate(Y, variant=None, dtype=np.float64, trace=None):
    """(PL[:, :k], pivstep) column by column in `dtype`.  trace (a list): per step (winner, |column| with -1 at pivoted rows)."""
    A = np.array(Y, dtype=dtype)
    n, r = A.shape
    k = min(n, r)
    one = dtype(1.0)
    pivstep = np.zeros(n, dtype=np.int32)
    free = np.ones(n, dtype=bool)
    cur = np.arange(n)                       # tie_position: LAPACK's row order after its swaps
    for j in range(k):
        col = np.where(free, np.abs(A[:, j]), -one)
        if trace is not None:
            trace.append(col.copy())
        tied = np.flatnonzero(col == col.max())
        win = int(tied[0])
        if variant == "tie_last":
            win = int(tied[-1])
        elif variant == "tie_position":
            at = j + int(np.argmax(col[cur[j:]]))      # first maximum by current position
            win = int(cur[at])
            cur[j], cur[at] = cur[at], cur[j]
        pivstep[win] = j + 1
        free[win] = False
        piv = A[win, j]
        scaled = piv != 0 and not (variant == "panel_tail" and j >= k - k % LU_NB)
        l = A[free, j] * (one / piv) if scaled else A[free, j].copy()
        hi = r - 1 if variant == "skip_last_update" else r
        if hi > j + 1:
            A[free, j + 1:hi] -= l[:, None] * A[win, j + 1:hi][None, :]
        A[free, j] = l
    for row in np.flatnonzero(pivstep):
        s = pivstep[row] - 1
        A[row, s] = 1.0
        A[row, s + 1:k] = 0.0
    return np.ascontiguousarray(A[:, :k]), pivstep


def pivot_rows(pivstep, k):
    """rows in step order, or None when the nonzero entries are not 1 .. k once each"""
    pivstep = np.asarray(pivstep)
    rows = np.flatnonzero(pivstep)
    if len(rows) != k or sorted(pivstep[rows]) != list(range(1, k + 1)):
        return None
    return rows[np.argsort(pivstep[rows])]


def exact_lu(Y):
    """the elimination in rational arithmetic with the same pivot rule: (PL[:, :k] as Fractions, pivstep)"""
    n, r = Y.shape
    k = min(n, r)
    A = np.array([[fractions.Fraction(float(x)) for x in row] for row in Y], dtype=object).reshape(n, r)
    pivstep = np.zeros(n, dtype=np.int32)
    free = np.ones(n, dtype=bool)
    for j in range(k):
        col = np.where(free, np.abs(A[:, j]), -1)
        win = int(np.flatnonzero(col == col.max())[0])
        pivstep[win] = j + 1
        free[win] = False
        piv = A[win, j]
        l = A[free, j] / piv if piv != 0 else A[free, j].copy()
        if r > j + 1:
            A[free, j + 1:] -= l[:, None] * A[win, j + 1:][None, :]
        A[free, j] = l
    for row in np.flatnonzero(pivstep):
        s = pivstep[row] - 1
        A[row, s] = fractions.Fraction(1)
        A[row, s + 1:k] = fractions.Fraction(0)
    return A[:, :k], pivstep


def step_ties(Y):
    """per step of the fp64 restatement: (winner, the other unpivoted rows with the winner's |a|)"""
    tr = []
    lu_restate(Y, trace=tr)
    out = []
    for col in tr:
        tied = np.flatnonzero(col == col.max())
        out.append((int(tied[0]), tied[1:]))
    return out


def gap(Y):
    """max over the steps of the longdouble elimination of runner-up / winner, copies of the winner's row of Y aside; a step
    whose winner is 0 counts as 1 (nothing decides it but the tie rule)"""
    tr = []
    _, pivstep = lu_restate(Y, dtype=LD, trace=tr)
    order = pivot_rows(pivstep, min(Y.shape))
    worst = 0.0
    for win, col in zip(order, tr):
        others = col.copy()
        others[win] = -1
        others[np.all(Y == Y[win], axis=1)] = -1
        ru = others.max()
        if ru < 0:
            continue
        worst = max(worst, 1.0 if col[win] == 0 else float(ru / col[win]))
    return worst


# ---- LU: the bounds --------------------------------------------------------------------------------------------------------
def ratio(err, bound):
    err, bound = np.abs(np.asarray(err, dtype=LD)), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(np.max(q))


def _unit_lower_solve(L1, B):
    """L1^-1 B in longdouble by forward substitution"""
    X = np.array(B, dtype=LD)
    for i in range(1, len(L1)):
        X[i] -= L1[i, :i] @ X[:i]
    return X


def lu_structure(PL, pivstep, k):
    """the exact properties, as a list of the ones that fail"""
    bad = []
    p = pivot_rows(pivstep, k)
    if not np.isfinite(PL).all():
        bad.append("finite")
    if p is None:
        return bad + ["permutation"]
    L1 = PL[p]
    if not (np.all(np.diag(L1) == 1.0) and np.all(np.triu(L1, 1) == 0.0)):
        bad.append("pivot_rows")
    if not np.all(np.abs(PL) <= 1.0 + 2 * EPS):
        bad.append("magnitude")
    return bad


def lu_backward_ratio(Y, PL, pivstep):
    n, r = Y.shape
    k = min(n, r)
    p = pivot_rows(pivstep, k)
    Yl, Pl = np.asarray(Y, dtype=LD), np.asarray(PL, dtype=LD)
    L1 = Pl[p]
    U = _unit_lower_solve(L1, Yl[p])
    Linv = _unit_lower_solve(L1, np.eye(k, dtype=LD))
    aP, aU = np.abs(Pl), np.abs(U)
    bound = 2 * (k + 2) * EPS * (aP @ aU + aP @ (np.abs(Linv) @ (np.abs(L1) @ aU)))
    return ratio(Yl - Pl @ U, bound)


def lu_verdict(c, PL, pivstep, want=None):
    """Every assertion on one LU result: ({name: ratio}, [names that fail]).  want: the restatement's (PL, pivstep)."""
    Y = panel(c)
    if want is None:
        want = lu_restated(c)
    bad = lu_structure(PL, pivstep, c.k)
    ratios = {}
    if "permutation" not in bad and "finite" not in bad:
        ratios["backward"] = lu_backward_ratio(Y, PL, pivstep)
        if not ratios["backward"] <= 1.0:
            bad.append("backward")
    if c.order and not np.array_equal(pivstep, want[1]):
        bad.append("order")
    if c.exact and not np.array_equal(bits(PL), bits(want[0])):
        bad.append("bits")
    return ratios, bad


@functools.lru_cache(maxsize=None)
def lu_restated(c):
    PL, ps = lu_restate(panel(c))
    PL.setflags(write=False)
    ps.setflags(write=False)
    return PL, ps


# ---- QR: the restatement -------------------------------------------------------------------------------------------------
def qr_restate(Y, variant=None):
    """(Q, tau, alpha, beta): alpha_j the diagonal entry step j meets, beta_j what it leaves there (alpha_j where tau_j = 0)"""
    A = np.array(Y, dtype=np.float64)
    n, r = A.shape
    tau, alpha, beta = np.zeros(r), np.zeros(r), np.zeros(r)
    V = np.zeros((n, r))
    for j in range(r):
        x = A[j + 1:, j]
        a = A[j, j]
        xn2 = float(x @ x)
        alpha[j] = a
        V[j, j] = 1.0
        if xn2 == 0.0 and variant != "tau0_not_skipped":
            beta[j] = a
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            b = np.sqrt(a * a + xn2)
            if variant != "sign":
                b = -np.copysign(b, a)
            tau[j] = (b - a) / b
            V[j + 1:, j] = x * (1.0 / (a - b))
            beta[j] = b
            if j + 1 < r:
                w = V[j:, j] @ A[j:, j + 1:]
                A[j:, j + 1:] -= tau[j] * np.outer(V[j:, j], w)
    Q = np.eye(n, r)
    for j in range(r - 1, -1, -1):
        if tau[j] == 0.0:
            continue
        v = V[j:, j]
        if variant == "chunk_dropped" and j == 0:
            keep = np.ones(n, dtype=bool)
            keep[QR_CHUNK:2 * QR_CHUNK] = False
            w = v[keep] @ Q[keep, j:]
        else:
            w = v @ Q[j:, j:]
        Q[j:, j:] -= tau[j] * np.outer(v, w)
    return Q, tau, alpha, beta


@functools.lru_cache(maxsize=None)
def qr_restated(c):
    out = qr_restate(panel(c))
    for a in out:
        a.setflags(write=False)
    return out


def qr_ratios(Y, Q):
    """orth, span and tri over their bounds, and diag(Q^T Y) in fp64"""
    n, r = Y.shape
    Yl, Ql = np.asarray(Y, dtype=LD), np.asarray(Q, dtype=LD)
    b = n * r * EPS
    norms = np.sqrt(np.sum(Yl * Yl, axis=0))
    R = Ql.T @ Yl
    colb = np.broadcast_to(b * norms, (r, r))
    out = {"orth": ratio(Ql.T @ Ql - np.eye(r, dtype=LD), np.full((r, r), b)),
           "span": ratio(Yl - Ql @ R, np.broadcast_to(b * norms, (n, r))),
           "tri": ratio(np.tril(R, -1), colb)}
    return out, np.asarray(np.diag(R), dtype=np.float64)


def qr_verdict(c, Q):
    """Every assertion on one QR result: ({name: ratio}, [names that fail])."""
    Y = panel(c)
    bad = []
    if not np.isfinite(Q).all():
        return {}, ["finite"]
    ratios, d = qr_ratios(Y, Q)
    bad += [k for k, v in ratios.items() if not v <= 1.0]
    _, tau, alpha, beta = qr_restated(c)
    norms = np.linalg.norm(Y, axis=0)
    if c.data in QR_SIGNED:
        clear = np.abs(beta) > SIGN_REL * norms
        if not np.array_equal(np.sign(d[clear]), np.sign(beta[clear])):
            bad.append("sign")
    if c.data == "zero_sub":   # alpha exact: the steps before are the identity
        m = min(2, c.r)
        if not np.all(np.abs(d[:m] - alpha[:m]) <= c.n * c.r * EPS * norms[:m]):
            bad.append("alpha")
    if c.data in QR_WELL:
        import scipy.linalg

        ref = scipy.linalg.qr(Y, mode="economic")[0]
        ratios["scipy"] = float(np.max(np.abs(Q - ref))) / 1e-11
        if not ratios["scipy"] <= 1.0:
            bad.append("scipy")
    return ratios, bad
