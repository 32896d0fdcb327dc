"""Inputs shared by tests/test_lloyd_host.py and tests/test_gpu_lloyd.py: a high-precision restatement of scikit-learn's
`_kmeans_single_lloyd` (what csrc/kmeans.hip runs on the device) and the table of cases both tests walk.

A case is a `Case`: rows X (n x d), their column means, k seed centres of the centred rows, the absolute tolerance and
`max_iter`, with the kernel the library picks for (d, k) (`rows`: 64 / 32 / 16 rows per LDS sub-tile, 0 = the
row-per-thread kernel) and the row pitch the device test gives X.  The reference result of a case is computed once and
kept read-only.

Every table case and every max_iter / forced-tolerance case must keep two margins (tests/test_lloyd_host.py asserts them),
so that an fp64 run that is right cannot differ from the reference in a label, a count or a stop:
  e_margin >= 1e-9   no row of any E step has its two best centres closer than that, relative to |x|^2 + max |c|^2
                     (fp64 `csq - 2 dot` is within about 2 (d + 8) 2^-52 of that scale: 2.3e-13 at d = 512)
  s_margin >= 1e-6   no tolerance test is decided by less than that, relative to tol (a fixed-order fp64 sum of k d
                     squares is good to about k d 2^-52)
A case that misses a bound gets another seed; it is not exempted."""
import dataclasses
import functools

import numpy as np

LD = np.longdouble
E_MARGIN_MIN = 1e-9
S_MARGIN_MIN = 1e-6


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    n: int
    d: int
    k: int
    seed: int
    rows: int             # sub-tile rows of the E/M-step kernel the library picks for (d, k); 0 = row per thread
    ld: int = 0           # row pitch on the device (0 = contiguous)
    max_iter: int = 300
    tol_between: tuple = ()   # (i, i + 1): tol = geometric mean of the centre shifts of iterations i and i + 1 (1-based)
    data: str = "gauss"   # "gauss", "far" (gauss with the last seed moved to 1e3 everywhere), "three" (3 distinct points)


@dataclasses.dataclass(frozen=True)
class Result:
    labels: np.ndarray    # n int32
    centers: np.ndarray   # k x d longdouble, centres of the centred rows
    iters: int
    code: int             # 1 strict convergence, 2 shift <= tol, 0 max_iter
    empty: int            # some M step met a cluster without rows
    e_margin: float
    s_margin: float
    shifts: tuple         # total squared centre shift of every iteration
    history: tuple        # labels of every E step, the final one included


def lloyd_reference(X, mean, C0, tol, max_iter):
    """`_kmeans_single_lloyd` (sklearn cluster/_kmeans.py) in np.longdouble on the rows X - mean from the centres C0.
    E step: argmin_j |c_j|^2 - 2 x.c_j, first minimum on ties.  M step: sum of a cluster's rows times the reciprocal of
    their count; a cluster without rows keeps its centre and raises `empty` (scikit-learn relocates it: the device
    reports the flag and the caller leaves the device path, so nothing after that point is compared).  Stop: strict
    convergence if the labels repeat (never in the first iteration), else shift <= tol.  One more E step unless the stop
    was strict."""
    Xc = np.asarray(X, dtype=LD) - np.asarray(mean, dtype=LD)
    C = np.array(C0, dtype=LD)
    n, _ = Xc.shape
    k = len(C)
    xsq = (Xc * Xc).sum(1)
    margins = []

    def e_step():
        csq = (C * C).sum(1)
        D = csq[None, :] - 2 * (Xc @ C.T)
        lab = D.argmin(1)
        if k > 1:
            two = np.partition(D, 1, axis=1)[:, :2]
            margins.append(float(((two[:, 1] - two[:, 0]) / (xsq + csq.max())).min()))
        return lab.astype(np.int32)

    old = np.full(n, -1, dtype=np.int32)
    iters, code, empty, s_margin = 0, 0, 0, np.inf
    shifts, history = [], []
    for it in range(max_iter):
        lab = e_step()
        history.append(lab)
        cnt = np.bincount(lab, minlength=k)
        S = np.zeros_like(C)
        np.add.at(S, lab, Xc)
        new = C.copy()
        hit = cnt > 0
        new[hit] = S[hit] * (LD(1) / cnt[hit].astype(LD))[:, None]
        empty |= int(not hit.all())
        shift = ((new - C) ** 2).sum()
        shifts.append(float(shift))
        C = new
        iters = it + 1
        if np.array_equal(lab, old):
            code = 1
            break
        if tol > 0:
            s_margin = min(s_margin, float(abs(shift - LD(tol)) / LD(tol)))
        if shift <= tol:
            code = 2
            break
        old = lab
    if code != 1:
        lab = e_step()
        history.append(lab)
    return Result(lab, C, iters, code, empty, min(margins, default=np.inf), s_margin, tuple(shifts), tuple(history))


# ---- inputs -------------------------------------------------------------------------------------------------------
def _gauss(c):
    """Gaussian centres (0.6 per coordinate: neighbouring clusters overlap, so the iterations go on for a while) with unit
    noise, off the origin (the means matter); the seeds are k of the centred rows."""
    rng = np.random.default_rng([c.n, c.d, c.k, c.seed])
    mu = 0.6 * rng.standard_normal((c.k, c.d))
    X = mu[rng.integers(0, c.k, c.n)] + rng.standard_normal((c.n, c.d)) + rng.uniform(-5.0, 5.0, size=c.d)
    pick = rng.permutation(c.n)[: c.k]
    return np.ascontiguousarray(X), pick


def three_points(seed=0):
    """60 rows that are copies of 3 distinct points (d = 4): with k = 5 at least two clusters run empty."""
    rng = np.random.default_rng(100 + seed)
    return np.ascontiguousarray(rng.standard_normal((3, 4))[rng.integers(0, 3, 60)] + 2.0)


def sklearn_tolerance(X, rel=1e-4):
    """KMeans._check_params_vs_input -> _tolerance: from the raw rows, before centring."""
    return float(np.mean(np.var(X, axis=0)) * rel)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(X, mean, C0, tol) of a case, read-only."""
    if c.data == "three":
        from sklearn.cluster import kmeans_plusplus
        from sklearn.utils.extmath import row_norms

        X = three_points(c.seed)
        mean = X.mean(axis=0)
        Xc = X - mean
        C0, _ = kmeans_plusplus(Xc, c.k, x_squared_norms=row_norms(Xc, squared=True),
                                random_state=np.random.RandomState(c.seed))
        C0 = np.ascontiguousarray(C0)
    else:
        X, pick = _gauss(c)
        mean = X.mean(axis=0)
        C0 = np.ascontiguousarray((X - mean)[pick])
        if c.data == "far":
            C0[-1] = 1e3
    tol = sklearn_tolerance(X)
    if c.tol_between:
        i, j = c.tol_between
        free = reference(dataclasses.replace(c, tol_between=(), name=c.name + "_free"))
        assert j == i + 1 and free.shifts[j - 1] < free.shifts[i - 1], "the shifts do not fall between these iterations"
        tol = sklearn_tolerance(X, float(np.sqrt(free.shifts[i - 1] * free.shifts[j - 1])) / float(np.mean(np.var(X, axis=0))))
    for a in (X, mean, C0):
        a.setflags(write=False)
    return X, mean, C0, tol


def relative_tolerance(c):
    """The `tol` argument with which scikit-learn's KMeans arrives at the case's absolute tolerance."""
    X, _, _, tol = inputs(c)
    return tol / float(np.mean(np.var(X, axis=0))) if c.tol_between else 1e-4


@functools.lru_cache(maxsize=None)
def reference(c):
    """lloyd_reference of a case, computed once (read-only)."""
    X, mean, C0, tol = inputs(c)
    r = lloyd_reference(X, mean, C0, tol, c.max_iter)
    for a in (r.labels, r.centers) + r.history:
        a.setflags(write=False)
    return r


# ---- the table ----------------------------------------------------------------------------------------------------
# the smallest shapes that reach each path; KM_CHUNK = 256 rows per block
_SHAPES = [
    # name      n     d    k     rows  seeds
    ("tiled64", 300, 8, 5, 64, (0, 1, 2)),       # two chunks, the last of 44 rows (a short last sub-tile)
    ("tiled32", 513, 200, 20, 32, (0, 1, 2)),    # the third chunk holds one row
    ("tiled16", 257, 200, 40, 16, (0, 1)),       # the second chunk holds one row
    ("plain_a", 300, 256, 32, 0, (0, 1)),        # row per thread, k d = 8192
    ("plain_b", 260, 512, 16, 0, (0, 1)),        # row per thread at the d limit of the seeding path
    ("many_k", 1100, 8, 1024, 64, (0, 1)),       # k = 1024 > the 256 threads of a chunk and = the update kernel's block
    ("k_is_1", 64, 3, 1, 64, (0, 1)),            # one cluster; n < every sub-tile count
    ("k_is_n", 40, 16, 40, 64, (0, 1)),          # every row its own centre: tolerance stop in iteration 1, shift 0
    ("one_col", 1025, 1, 7, 64, (0, 1, 2)),      # d = 1, five chunks, many iterations
]
PITCHED = "tiled32_s1"   # this case sits in rows of pitch d + 3


def _table():
    out = []
    for name, n, d, k, rows, seeds in _SHAPES:
        for s in seeds:
            cid = f"{name}_s{s}"
            out.append(Case(cid, n, d, k, s, rows, ld=d + 3 if cid == PITCHED else 0))
    return out


TABLE = _table()
TILED = [c for c in TABLE if c.rows]

# derived from one tiled32 seed whose free run converges strictly in 8 iterations, its shifts falling up to the 5th
_BASE = next(c for c in TABLE if c.name == "tiled32_s0")
MAX_ITER = [dataclasses.replace(_BASE, name=f"tiled32_max{m}", max_iter=m) for m in (1, 2, 3, 4, 5, 7, 9)]
FORCED_TOL_ITER = 4      # tol between the shifts of iterations 3 and 4: the run stops on it in iteration 4
FORCED_TOL = dataclasses.replace(_BASE, name="tiled32_tol", tol_between=(FORCED_TOL_ITER - 1, FORCED_TOL_ITER))
DERIVED = MAX_ITER + [FORCED_TOL]

EMPTY = ([dataclasses.replace(c, name=c.name.replace("tiled64", "far_seed"), data="far") for c in TABLE
          if c.name == "tiled64_s0"]
         + [Case(f"three_points_s{s}", 60, 4, 5, s, 64, data="three") for s in (0, 1, 2)])

EXACT = TABLE + DERIVED    # the cases on which labels, info and centres are compared


def by_name(name):
    for c in EXACT + EMPTY:
        if c.name == name:
            return c
    raise KeyError(name)
