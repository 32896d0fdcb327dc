"""Cases, references and a schedule model for the fused kNN kernels (mused_amd/csrc/knn_fused.hip): shared by
tests/test_knn_fused_cases_host.py (CPU) and tests/test_gpu_knn_fused.py (MI355X).  NumPy only.

References
  * l2, EXACT: rows are integer valued (in float32 and in float64), so every product, every squared norm and
    nrm_i - 2 v + nrm_j is an integer far below 2^53: fp64 gives it exactly in any summation order, and the expected
    neighbours follow from int64 arithmetic with no tolerance -- the k smallest by (squared distance, column), the own
    column ranked like any other and cleared in the mask.  "wide" rows (|x| <= 512, d = 8) rarely tie; "narrow" rows
    (|x| <= 20, d = 5 and |x| <= 12, d = 6) tie across the k-th boundary in dozens of rows per case, which makes the
    exact reference decide the tie rule (smaller column) without pushing a candidate list near its capacity.
  * cosine: -(x.y) / (|x| |y|) in np.longdouble on Gaussian rows without engineered ties.  The host test asserts a gap of
    at least COS_GAP between the k-th and the (k+1)-th reference score of every row (fp64 error: ~1e-15), so the neighbour
    SET of the device has to equal the reference's, no row skipped.
  * "dup" rows (duplicated rows, a zero row) are compared with the classic path (mused_knn_topk) only.

schedule() restates the host-side phase schedule of knn_fused_t.  It is a restatement of code under test and decides
nothing about correctness: its only use is to assert on the CPU that every case reaches the path it is named for."""
import functools
from collections import namedtuple

import numpy as np

from mused_amd import synth

TILE = 128          # GEMM_BM = GEMM_BN: rows per tile
LD = np.longdouble
COS_GAP = 1e-9
MIN_BOUNDARY_TIES = 20
MAX_EQUAL_RUN = 32

Schedule = namedtuple("Schedule", "tiles a direct kthr phases tripled pl first_select_early")


def schedule(n, k, cap, ring=False):
    """What knn_fused_t does for (n, k, cap): tile count, a, whether the first phase is DIRECT, kthr, the band launches
    as (d_lo, d_hi), how often the tripling branch was taken, the select template size, and whether the first select returns
    early for every row (its fixed slots do not exceed k)."""
    tiles = -(-n // TILE)
    hmax = tiles // 2
    kthr = max(k, min(2 * k, cap // 4)) if ring else k
    a = 2
    while a > 0 and ((2 * a + 1) * TILE > cap or kthr > 2 * a * TILE):
        a -= 1
    direct = tiles >= 2 * a + 2 and (2 * a + 1) * TILE <= cap and a <= hmax
    d_hi = a if direct else min(hmax, 1)
    d_lo, phases, tripled = 0, [], 0
    while True:
        d_hi = min(d_hi, hmax)
        phases.append((d_lo, d_hi))
        if d_hi >= hmax:
            break
        d_lo = d_hi + 1
        seen = (2 * d_hi + 1) * TILE
        left = n - seen
        est = (kthr * left + seen - 1) // seen if left > 0 else 0
        if kthr + (3 if ring else 2) * est <= cap:
            d_hi = hmax
        else:
            d_hi, tripled = 3 * d_hi + 2, tripled + 1
    pl = -(-cap // 64)
    early = direct and len(phases) > 1 and (2 * a + 1) * TILE <= kthr
    return Schedule(tiles, a, direct, kthr, tuple(phases), tripled, 4 if pl <= 4 else 8 if pl <= 8 else 16, early)


# ---- the tumbling cases -------------------------------------------------------------------------------------------------
# reaches: what the schedule model must say of (n, k, cap)
Case = namedtuple("Case", "name n k cap reaches")
CASES = [
    Case("sel4_a0", 1000, 10, 256, dict(pl=4, a=0, direct=True, phases=((0, 0), (1, 4)))),
    Case("sel8_a1_odd", 1100, 30, 512, dict(pl=8, a=1, direct=True, tiles=9, phases=((0, 1), (2, 4)))),
    Case("tripled", 2000, 55, 512, dict(pl=8, a=1, direct=True, tripled=1, phases=((0, 1), (2, 5), (6, 8)))),
    Case("five_tiles", 513, 20, 704, dict(pl=16, a=2, direct=False, tiles=5, phases=((0, 1), (2, 2)))),
    Case("four_tiles", 512, 20, 704, dict(pl=16, a=2, direct=False, tiles=4, phases=((0, 1), (2, 2)))),
    Case("first_direct_a2", 641, 20, 704, dict(pl=16, a=2, direct=True, tiles=6, phases=((0, 2), (3, 3)))),
    Case("ten_tiles_ragged", 1153, 25, 704, dict(pl=16, a=2, direct=True, tiles=10, phases=((0, 2), (3, 5)))),
    Case("k_above_512", 700, 600, 1024, dict(pl=16, a=0, direct=True, first_select_early=True, tripled=1,
                                            phases=((0, 0), (1, 2), (3, 3)))),
    Case("largest_engine_k", 1792, 224, 1024, dict(pl=16, a=2, direct=True, tiles=14, phases=((0, 2), (3, 7)))),
    Case("k1_two_tiles", 129, 1, 384, dict(pl=8, a=1, direct=False, tiles=2, phases=((0, 1),))),
    Case("n_k_cap_equal", 64, 64, 64, dict(pl=4, a=0, direct=False, tiles=1, phases=((0, 0),))),
]
NAMES = [c.name for c in CASES]
# the cases of the padded-rows, NULL-output, guard and argument tests
PADDED = "first_direct_a2"


def case(name):
    return CASES[NAMES.index(name)]


# (variant, metric, dtype, kind of rows): every case runs all of them
VARIANTS = [
    ("l2_f32_narrow", 0, np.float32, "narrow"),
    ("l2_f64_wide", 0, np.float64, "wide"),
    ("l2_f32_wide", 0, np.float32, "wide"),
    ("cos_f64_gauss", 1, np.float64, "gauss"),
    ("cos_f32_gauss", 1, np.float32, "gauss"),
    ("l2_f64_dup", 0, np.float64, "dup"),
    ("cos_f32_dup", 1, np.float32, "dup"),
]
VARIANT_NAMES = [v[0] for v in VARIANTS]


def variant(vname):
    return VARIANTS[VARIANT_NAMES.index(vname)]


def _seed(c, kind):
    return 7919 * c.n + 31 * c.k + {"narrow": 1, "wide": 2, "gauss": 3, "dup": 4}[kind]


@functools.lru_cache(maxsize=None)
def rows(name, kind):
    """The rows of a case as float64 (every kind is exactly representable in float32 after .astype(np.float32) for the
    integer kinds; the Gaussian kinds are DEFINED as what the cast gives: references are computed from the cast rows)."""
    c = case(name)
    rng = np.random.default_rng(_seed(c, kind))
    if kind == "wide":
        X = rng.integers(-512, 513, size=(c.n, 8)).astype(np.float64)
    elif kind == "narrow":
        # the two narrow ranges alternate over the table
        X = (rng.integers(-20, 21, size=(c.n, 5)) if NAMES.index(name) % 2 == 0 else rng.integers(-12, 13, size=(c.n, 6)))
        X = X.astype(np.float64)
    elif kind == "gauss":
        X = rng.standard_normal((c.n, 12))
    elif kind == "dup":
        X = rng.standard_normal((c.n, 9))
        X[c.n // 3] = X[c.n // 5]        # duplicate rows: exact score ties across tiles
        X[c.n - 1] = X[0]
        X[c.n // 2] = 0.0                # a zero row (dropped again for cosine: see rows_as)
    else:
        raise KeyError(kind)
    X.setflags(write=False)
    return X


def rows_as(name, vname):
    _, metric, dtype, kind = variant(vname)
    X = rows(name, kind).astype(dtype)
    if kind == "dup" and metric == 1:
        # a zero row under cosine scores 0 against every column: a run of n equal scores, which is what overflows the lists
        # by design (test_engine_cosine_zero_rows_fall_back); here the lists must not overflow
        X[case(name).n // 2] = X[1]
    return X


def l2_int_scores(X):
    Xi = np.asarray(X).astype(np.int64)
    assert np.array_equal(Xi, np.asarray(X)), "rows are not integer valued"
    G = Xi @ Xi.T
    nrm = np.diag(G)
    return nrm[:, None] - 2 * G + nrm[None, :]


def cosine_scores(X):
    Xl = np.asarray(X).astype(LD)
    G = Xl @ Xl.T
    nr = np.sqrt(np.diag(G))
    return -(G / (nr[:, None] * nr[None, :]))


def topk(S, k):
    """Columns of the k smallest by (score, column) per row, ascending columns (what out_idx holds)."""
    order = np.argsort(S, axis=1, kind="stable")[:, :k]
    return np.sort(order, axis=1).astype(np.int32)


def mask_of(lists, n, words):
    """uint64 bit rows of the lists, own column cleared."""
    bits = np.zeros((n, words * 64), dtype=np.uint8)
    np.put_along_axis(bits, lists.astype(np.int64), 1, axis=1)
    bits[np.arange(n), np.arange(n)] = 0
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64)


def words_for(n):
    return (n + 63) // 64


@functools.lru_cache(maxsize=None)
def scores(name, vname):
    _, metric, _, kind = variant(vname)
    assert kind != "dup", "the dup rows have no reference of their own"
    X = rows_as(name, vname)
    return l2_int_scores(X) if metric == 0 else cosine_scores(X)


@functools.lru_cache(maxsize=None)
def reference_lists(name, vname):
    L = topk(scores(name, vname), case(name).k)
    L.setflags(write=False)
    return L


def has_reference(vname):
    return variant(vname)[3] != "dup"


def boundary_ties(S, k):
    """Rows whose k-th and (k+1)-th smallest scores are equal, and the longest run of equal scores in any row."""
    srt = np.sort(S, axis=1)
    n = S.shape[1]
    tied = int((srt[:, k - 1] == srt[:, k]).sum()) if k < n else 0
    run = longest = np.ones(S.shape[0], dtype=np.int64)
    for j in range(1, n):
        run = np.where(srt[:, j] == srt[:, j - 1], run + 1, 1)
        longest = np.maximum(longest, run)
    return tied, int(longest.max())


def smallest_gap(S, k):
    """min over the rows of (k+1)-th minus k-th smallest score (inf for k = n)."""
    if k >= S.shape[1]:
        return np.inf
    part = np.partition(S, (k - 1, k), axis=1)
    return float((part[:, k] - part[:, k - 1]).min())


# ---- padded rows ------------------------------------------------------------------------------------------------------------
# (dtype, extra elements per row, the GEMM load variant the pitch selects: 16-byte vector loads need 16-byte aligned rows)
PITCHES = [(np.float32, 3, "scalar"), (np.float32, 4, "vector"), (np.float64, 2, "vector")]


def loads_vector(dtype, ld):
    return ld % (16 // np.dtype(dtype).itemsize) == 0


# ---- hop streams ----------------------------------------------------------------------------------------------------------
HopSeq = namedtuple("HopSeq", "name W hop k cap metric windows")
FRIENDLY = [HopSeq(f"friendly_hop{h}_{'cos' if m else 'l2'}_cap{cap}", 768, h, 20, cap, m, 8)
            for cap in (1024, 512) for h in (96, 100) for m in (0, 1)]
GROWTH = HopSeq("growth", 640, 8, 20, 1024, 0, 60)
POSITION_LIMIT = 1 << 30
# "bit 1 must come up": SHIFT_NEAR rows near the origin, then rows shifted by +50 in every coordinate.  The window has five
# tiles, so that a select between two phases gives every row a threshold of the order of its (2 k)-th squared distance.
# (lo, n_new): from scratch; reuse inside the near block; 10 near rows stay and 590 far rows enter (flag & 2); reuse on a
# flagged state (sticky); from scratch (cleared); reuse again (clean)
SHIFT_W, SHIFT_K, SHIFT_NEAR = 600, 20, 1000
SHIFT_CALLS = [(0, 0), (400, 400), (990, 590), (1100, 110), (1200, 0), (1300, 100)]
SHIFT_FLAGGED_AT = 2
# The same idea at W = 300 does NOT raise the flag, and must not: a window of at most three tiles is served by one band launch
# and the final select, no threshold is ever lowered (tau stays +inf), every list holds every window column, and a reuse call is
# exact whatever enters.
SINGLE_W, SINGLE_NEAR = 300, 500
SINGLE_CALLS = [(0, 0), (200, 200), (490, 290), (600, 110), (700, 0), (800, 100)]


@functools.lru_cache(maxsize=None)
def friendly_stream(hop):
    X = synth.blob_stream(768 + 8 * hop, 16, 3, n_centres=5)[0]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def growth_stream():
    X = synth.blob_stream(GROWTH.W + GROWTH.hop * GROWTH.windows, 16, 11, n_centres=5)[0]
    X.setflags(write=False)
    return X


def _shifted(n, near, seed):
    X = np.random.default_rng(seed).standard_normal((n, 10))
    X[near:] += 50.0
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def shift_stream():
    """SHIFT_NEAR rows near the origin, then rows shifted by +50 in every coordinate (d = 10)."""
    return _shifted(SHIFT_CALLS[-1][0] + SHIFT_W, SHIFT_NEAR, 4)


@functools.lru_cache(maxsize=None)
def single_phase_stream():
    return _shifted(SINGLE_CALLS[-1][0] + SINGLE_W, SINGLE_NEAR, 5)
