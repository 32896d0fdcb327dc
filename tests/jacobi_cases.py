"""Inputs shared by tests/test_jacobi_cases_host.py and tests/test_gpu_jacobi.py: seeded symmetric PSD matrices, their fp64
reference spectra, the checker both tests use, the project's tolerances and the table of plans that reaches every kernel
instance of the one-sided block Jacobi (csrc/eig.hip) through the plan's shape alone.

Matrices (all symmetrised as 0.5 (M + M^T); scale = max |G|)
  separated    Q diag(lam) Q^T, lam geometric from 1 down to 1e-3: neighbouring eigenvalues >= 1e-3 / n apart relatively,
               the regime in which Jacobi converges quadratically
  gram         B B^T, B n x (n + 20) with its first n / 4 rows zero (a half-filled FD buffer): exact zero eigenvalues.
               Reference: the squared singular values of B, accurate relatively and not only absolutely
  clustered    two exactly multiple eigenvalues (7 and 2, n / 4 each) plus a ramp 1 .. 0.5
  zero, diagonal, rank_one     the degenerate three
  scaled       separated times 2^+-100 (exact: only exponents change)
  heavy        a 100-fold eigenvalue above the cut of a TOP_HALF plan: more than the 5 eigenvalues the direct solvers'
               certificate lets lie within 1e-7 lam_0 (trd_common.h), so the blocked direct solver hands it to the Jacobi

Checker: check_solution(G, evals, V, tol, ref) measures, in this order,
  eig_top   sorted eigenvalues against the reference, upper half, / scale
  eig_all   the same over all of them
  resid     max |G V - V diag(evals)| / scale over the live columns (evals > 1e-9 scale)
  orth      max |V^T V - I| over the live columns
and raises AssertionError beyond `tol`; columns that are not live must carry |eigenvalue| <= 1e-9 scale and finite
entries (the solver returns them as zero vectors or as directions inside the numerical null space: documented).

Tolerances: the project's own (tests/test_gpu_primitives.py: test_syevj for separated / gram, test_syevj_special_matrices for
clustered / degenerate), the same for every kernel family."""
import collections

import numpy as np

EPS = 2.0 ** -52
SWEEP_CAP = 30
LIVE = 1e-9

Tol = collections.namedtuple("Tol", "eig_top eig_all resid orth")
TOL_SEPARATED = Tol(2e-12, 2e-10, 2e-10, 1e-11)   # separated / gram
TOL_CLUSTERED = Tol(1e-10, 1e-10, 1e-7, 1e-7)     # clustered / degenerate
TOLERANCES = {"separated": TOL_SEPARATED, "clustered": TOL_CLUSTERED}

Matrix = collections.namedtuple("Matrix", "name G ref tol")
Measured = collections.namedtuple("Measured", "eig_top eig_all resid orth")


def _sym(M):
    return 0.5 * (M + M.T)


def _orthogonal(rng, n):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def _ref(G):
    return np.maximum(np.linalg.eigvalsh(G), 0.0)


def separated(n, seed=0):
    rng = np.random.default_rng(1000 + 7 * n + seed)
    lam = np.geomspace(1.0, 1e-3, n)
    Q = _orthogonal(rng, n)
    G = _sym((Q * lam) @ Q.T)
    return Matrix("separated", G, _ref(G), TOL_SEPARATED)


def gram(n, seed=0):
    rng = np.random.default_rng(2000 + 7 * n + seed)
    B = rng.standard_normal((n, n + 20))
    B[: n // 4] = 0.0
    G = _sym(B @ B.T)
    ref = np.zeros(n)  # the zero rows are exact zero eigenvalues; the others the squared singular values of the rest
    ref[n // 4:] = np.sort(np.linalg.svd(B[n // 4:], compute_uv=False) ** 2)
    return Matrix("gram", G, ref, TOL_SEPARATED)


def clustered(n, seed=0):
    rng = np.random.default_rng(3000 + 7 * n + seed)
    q = n // 4
    lam = np.concatenate([np.full(q, 7.0), np.full(q, 2.0), np.linspace(1.0, 0.5, n - 2 * q)])
    Q = _orthogonal(rng, n)
    G = _sym((Q * lam) @ Q.T)
    return Matrix("clustered", G, _ref(G), TOL_CLUSTERED)


def zero(n, seed=0):
    return Matrix("zero", np.zeros((n, n)), np.zeros(n), TOL_CLUSTERED)


def diagonal(n, seed=0):
    d = np.linspace(5.0, 0.0, n)
    return Matrix("diagonal", np.diag(d), np.sort(d), TOL_CLUSTERED)


def rank_one(n, seed=0):
    rng = np.random.default_rng(4000 + 7 * n + seed)
    u = rng.standard_normal(n)
    G = _sym(np.outer(u, u))
    ref = np.zeros(n)
    ref[-1] = u @ u
    return Matrix("rank_one", G, ref, TOL_CLUSTERED)


def scaled(n, exponent, seed=0):
    m = separated(n, seed)
    s = 2.0 ** exponent
    return Matrix(f"scaled{exponent:+d}", m.G * s, m.ref * s, TOL_SEPARATED)


def heavy(n, seed=0, fold=100):
    rng = np.random.default_rng(5000 + 7 * n + seed)
    s = np.r_[np.full(fold, 5.0), np.linspace(4.0, 0.5, n - fold)]
    Q = _orthogonal(rng, n)
    G = _sym((Q * s ** 2) @ Q.T)
    return Matrix("heavy", G, _ref(G), TOL_CLUSTERED)


BUILDERS = {"separated": separated, "gram": gram, "clustered": clustered, "zero": zero, "diagonal": diagonal,
            "rank_one": rank_one}
DEGENERATE = ("zero", "diagonal", "rank_one")


def measure(G, evals, V, ref):
    """(Measured, problem with the columns that are not live or None)."""
    G, evals, V = np.asarray(G), np.asarray(evals), np.asarray(V)
    n = G.shape[0]
    scale = max(np.abs(G).max(), 1e-300)
    if not (np.isfinite(evals).all() and np.isfinite(V).all()):
        return Measured(np.inf, np.inf, np.inf, np.inf), "not finite"
    d = np.abs(np.sort(evals) - np.sort(ref)) / scale
    live = evals > LIVE * scale
    Vl = V[:, live]
    resid = np.abs(G @ Vl - Vl * evals[live][None, :]).max(initial=0.0) / scale
    orth = np.abs(Vl.T @ Vl - np.eye(int(live.sum()))).max(initial=0.0)
    dead = None
    if (np.abs(evals[~live]) > LIVE * scale).any():
        dead = f"a column that is not live carries eigenvalue {evals[~live].min():.3e} (scale {scale:.3e})"
    return Measured(d[n // 2:].max(), d.max(), resid, orth), dead


def check_solution(G, evals, V, tol, ref=None, what=""):
    """The four measured quantities; AssertionError naming the first one beyond `tol`."""
    m, dead = measure(G, evals, V, _ref(np.asarray(G)) if ref is None else ref)
    for name in Measured._fields:
        got, bound = getattr(m, name), getattr(tol, name)
        assert got <= bound, f"{what}: {name} = {got:.3e} > {bound:.1e} ({m})"
    assert dead is None, f"{what}: {dead}"
    return m


# ------------------------------------------------------------------ plans ---------------------------------------------------
# jacobi: 0 persistent work queue, 1 wave-private sweep graph, 2 row-per-thread sweep graph (mused_debug_eig_choice)
QUEUE, WAVE, ROW = 0, 1, 2
Case = collections.namedtuple("Case", "n batch sweeps flags need direct jacobi ldn")


def _case(n, batch, jacobi, ldn):
    return Case(n, batch, SWEEP_CAP, 0, 0, 0, jacobi, ldn)


CASES = (
    # Queue: osjq_kernel<1 .. 4>
    _case(64, 3, QUEUE, 64), _case(62, 2, QUEUE, 64), _case(2, 2, QUEUE, 64), _case(128, 3, QUEUE, 128),
    _case(130, 2, QUEUE, 192), _case(192, 2, QUEUE, 192), _case(256, 2, QUEUE, 256),
    # WaveGraph, orders <= 256: osjw_launch_sweep<1 .. 4>, one matrix past the queue's 224-unit bound
    # (224 / (nb / 2) + 1 matrices.  At order 192 that is 75: 57 -- the bound of order 256 -- is still the queue's, 57 x 3 =
    # 171 units, and is kept as a queue row)
    _case(64, 225, WAVE, 64), _case(128, 113, WAVE, 128), _case(192, 75, WAVE, 192), _case(256, 57, WAVE, 256),
    _case(192, 57, QUEUE, 192),
    # WaveGraph, orders 320 .. 512: osj_round_kernel<16, NT, 2> + osjw_kernel<RP, 4, false>
    _case(258, 2, WAVE, 320), _case(320, 2, WAVE, 320), _case(384, 2, WAVE, 384), _case(448, 2, WAVE, 448),
    _case(512, 2, WAVE, 512),
    # RowGraph: osj_round_kernel<16, NT, 2> + <32, NT, 1>
    _case(514, 2, ROW, 640), _case(640, 2, ROW, 640), _case(768, 2, ROW, 768), _case(896, 2, ROW, 896),
    _case(900, 2, ROW, 1024), _case(1024, 2, ROW, 1024),
)
# every (family, padded order) instance eig_choose() can pick for a flags = 0 plan
INSTANCES = frozenset([(QUEUE, o) for o in (64, 128, 192, 256)] + [(WAVE, o) for o in (64, 128, 192, 256, 320, 384, 448, 512)]
                      + [(ROW, o) for o in (640, 768, 896, 1024)])
# orders at which the degenerate three (and a clustered matrix) are solved as well, one per kernel family and more
DEGENERATE_ORDERS = (64, 256, 320, 640)
# the pre-rotation plan: FIXED_SWEEPS | NO_SORT, 5 sweeps; batch 12 is the queue's, 240 the sweep graph's
FIXED_SWEEPS, NO_SORT, TOP_HALF = 1, 2, 4
FIXED_CASES = (
    Case(64, 12, 5, 3, 0, 0, QUEUE, 64), Case(64, 240, 5, 3, 0, 0, WAVE, 64), Case(256, 12, 5, 3, 0, 0, QUEUE, 256),
    Case(256, 240, 5, 3, 0, 0, WAVE, 256),
    # padded inside the class: zero rows and columns next to live ones
    Case(62, 12, 5, 3, 0, 0, QUEUE, 64), Case(250, 240, 5, 3, 0, 0, WAVE, 256),
)
MIXED_CASE = Case(320, 4, SWEEP_CAP, TOP_HALF, 0, 2, WAVE, 320)


def case_id(c):
    return f"{('queue', 'wave', 'row')[c.jacobi]}{c.ldn}-n{c.n}-b{c.batch}"


def batch_matrices(c):
    """The distinct matrices of a table row: separated and gram, clustered too where the batch has room for three."""
    kinds = ("separated", "gram", "clustered") if c.batch >= 3 else ("separated", "gram")
    return [BUILDERS[k](c.n) for k in kinds]


def extra_matrices(n):
    """The degenerate three and a clustered matrix (a batch of four)."""
    return [BUILDERS[k](n) for k in DEGENERATE + ("clustered",)]


def fill(mats, batch):
    """batch x n x n: the distinct matrices repeated in turn."""
    return np.stack([mats[b % len(mats)].G for b in range(batch)])
