"""Inputs shared by tests/test_lloyd_wide_host.py and tests/test_gpu_lloyd_wide.py: the cases of mused_kmeans_lloyd_wide
(csrc/kmeans.hip), the Lloyd iterations for k * d > 8192, on the `gauss` data and against the high-precision reference of
tests/lloyd_cases.py.  The same two margins hold for every case here (tests/test_lloyd_wide_host.py asserts them)."""
import dataclasses

import lloyd_cases as lc

K_MAX, D_MAX = 1024, 512      # the limits of mused_kmeans_lloyd_wide (those of mused_kmeans_seed and mused_kmeans_assign)
LDS_MAX = 156 * 1024          # the ceiling csrc/kmeans.hip keeps every workgroup under

_SHAPES = [
    # name        n     d    k     seeds
    ("wide_min", 300, 482, 17, (0, 1)),        # k d = 8194, the first shape past the old limit; last chunk of 44 rows
    ("wide_kd1", 257, 512, 17, (0, 1)),        # d at its limit; the second chunk holds one row
    ("wide_ref", 600, 100, 150, (0, 1, 2)),    # the reference's 150 clusters at reduced_dim 100
    ("wide_c3", 513, 256, 40, (0, 1)),         # BASELINE config 3's reduced_dim; the third chunk holds one row
    ("wide_k1024", 1100, 16, 1024, (0, 1)),    # k at its limit, beyond any centre tile
    ("wide_max", 1030, 512, 1024, (0,)),       # both limits at once (k d = 524288)
]
PITCHED = "wide_ref_s1"   # this case sits in rows of pitch d + 3


def _table():
    out = []
    for name, n, d, k, seeds in _SHAPES:
        for s in seeds:
            cid = f"{name}_s{s}"
            out.append(lc.Case(cid, n, d, k, s, 0, ld=d + 3 if cid == PITCHED else 0))
    return out


TABLE = _table()

# derived from wide_c3_s1, whose free run converges strictly in 10 iterations
_BASE = next(c for c in TABLE if c.name == "wide_c3_s1")
FREE_ITERS = 10
MAX_ITER = [dataclasses.replace(_BASE, name=f"wide_c3_max{m}", max_iter=m) for m in (1, 4, 5)]
FORCED_TOL_ITER = 4      # tol between the shifts of iterations 3 and 4: the run stops on it in iteration 4
FORCED_TOL = dataclasses.replace(_BASE, name="wide_c3_tol", tol_between=(FORCED_TOL_ITER - 1, FORCED_TOL_ITER))
DERIVED = MAX_ITER + [FORCED_TOL]

# wide_min_s0 with the last seed moved to 1e3 everywhere: that cluster never gets a row
EMPTY = dataclasses.replace(TABLE[0], name="wide_far_seed_s0", data="far")

EXACT = TABLE + DERIVED
