"""Inputs shared by tests/test_primitives_cases_host.py and tests/test_gpu_primitives_shared.py: the cases of the primitives
the kernel files share (csrc/scan.h, block_scan.h, radix_sort.h, radix_select.h, union_find.h, wave_ops.h) and a plain
NumPy / Python statement of what each must return.  The statements are exact: integers and bit patterns (fp64 sums are the
same IEEE additions, compared by their bits).  No torch, no device, everything seeded.

The device side is csrc/primitives_debug.hip: entries that call each primitive as its consumers do.  The host test proves on
the CPU that every case reaches the edge it is named for; select_trace restates the control flow of radix_select.h for that."""
import functools

import numpy as np

SENTINEL = -7                        # what output buffers hold before a launch
POISON = 0x7F7F7F7F                  # input padding nothing may read
M64 = (1 << 64) - 1
U64 = np.uint64


def _rng(name):
    return np.random.default_rng([ord(c) for c in name])


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- wave operations (wave_ops.h, wave_incl_scan of scan.h) ---------------------------------------------------------------------
WAVE_THREADS = 256
WAVE_OPS = ("QUAD_XOR1", "QUAD_XOR2", "ROW_HALF_MIRROR", "ROW_MIRROR", "ROW_ROR8", "xchg16", "xchg32", "swap16_add",
            "swap32_add", "wave_allsum")          # the rows of mused_debug_wave_ops' output
MOVE_SOURCE = {                                    # lane l receives the value of lane ...
    "QUAD_XOR1": lambda l: l ^ 1,
    "QUAD_XOR2": lambda l: l ^ 2,
    "ROW_HALF_MIRROR": lambda l: (l & ~7) + 7 - (l & 7),
    "ROW_MIRROR": lambda l: (l & ~15) + 15 - (l & 15),
    "ROW_ROR8": lambda l: l ^ 8,
    "xchg16": lambda l: l ^ 16,
    "xchg32": lambda l: l ^ 32,
}
# the specials and the thread that holds each: the three with a zero low word in three different waves
MOVE_SPECIALS = {5: 0x8000000000000000,            # -0.0
                 40: 0x00000ABC00000000,           # a subnormal (its low word is drawn)
                 64 + 9: 0x7FF0000000000000,       # +inf
                 128 + 17: 0xFFF0000000000000,     # -inf
                 192 + 33: 0x7FF812349ABCDEF0}     # a NaN with a payload


@functools.lru_cache(maxsize=None)
def wave_move_input():
    """512 doubles as uint64 bits: a = [0, 256), b = [256, 512).  All 32-bit halves of `a` are distinct but for the zero low
    words that -0.0, +inf and -inf force, and those three sit in three different waves: inside a wave all 128 halves differ,
    so a value assembled from two lanes' halves cannot equal the expected one."""
    rng = _rng("wave_move_input")
    halves = rng.permutation(np.arange(1, 1 << 20, dtype=np.uint64))[:1024] * U64(4093) + U64(17)
    hi, lo = halves[:512].copy(), halves[512:].copy()
    hi = hi & U64(0xFFFFFFFF)
    lo = lo & U64(0xFFFFFFFF)
    expo = (hi >> U64(20)) & U64(0x7FF)
    hi = np.where(expo == U64(0x7FF), hi ^ U64(1 << 30), hi)          # no NaN or inf but the planted ones
    bits = (hi << U64(32)) | lo
    for t, v in MOVE_SPECIALS.items():
        bits[t] = U64(v) | (lo[t] if t == 40 else U64(0))
    return _frozen(bits)


@functools.lru_cache(maxsize=None)
def wave_add_input():
    """512 finite doubles, a and b: mixed signs, magnitudes from 1e-300 to 1e300 in one half of the lanes and of order one in
    the other (where the rounding of a sum matters); every sum of 64 of them stays finite."""
    rng = _rng("wave_add_input")
    wide = 10.0 ** rng.uniform(-300, 300, 512)
    near = rng.uniform(1.0, 2.0, 512)
    v = np.where(rng.random(512) < 0.5, wide, near) * rng.choice([-1.0, 1.0], 512)
    return _frozen(v)


@functools.lru_cache(maxsize=None)
def wave_near_input():
    """512 doubles of order one and mixed sign: no value absorbs the others, so every level of wave_allsum rounds."""
    rng = _rng("wave_near_input")
    return _frozen(rng.uniform(1.0, 2.0, 512) * rng.choice([-1.0, 1.0], 512))


@functools.lru_cache(maxsize=None)
def wave_scan_input():
    """(int32, uint64) x 256 for wave_incl_scan: the uint64 values are below 2^40 with random low words, so their sums carry
    out of bit 31 many times in every wave."""
    rng = _rng("wave_scan_input")
    i = rng.integers(-1000, 1000, WAVE_THREADS).astype(np.int32)
    u = rng.integers(0, 1 << 40, WAVE_THREADS).astype(np.uint64)
    return _frozen(i), _frozen(u)


def ref_move(op, a):
    """a: 256 values; what every thread holds after the move `op`."""
    t = np.arange(WAVE_THREADS)
    src = (t & ~63) + np.array([MOVE_SOURCE[op](l) for l in range(64)])[t & 63]
    return a[src]


def ref_swap_add(a, b, bit):
    """swap16_add (bit 16) / swap32_add (bit 32): a(l) + a(l ^ bit) where the lane's bit is clear, b(l) + b(l ^ bit) where it
    is set.  One IEEE addition."""
    t = np.arange(WAVE_THREADS)
    return np.where(t & bit, b + b[t ^ bit], a + a[t ^ bit])


def ref_wave_scan(x):
    return np.cumsum(x.reshape(-1, 64), axis=1, dtype=x.dtype).reshape(-1)


ALLSUM_BOUND = 7 * 2.0 ** -53        # six levels of pairwise addition, one rounding each, and the second-order terms


# ---- block_excl_scan (scan.h) -----------------------------------------------------------------------------------------------------
SCAN_THREADS = tuple(range(64, 1025, 64))
SCAN_CALLS = 3
SCAN_DTYPES = {0: np.int32, 1: np.uint64}
# the launches of one workgroup size: three calls back to back, neighbours with different totals
SCAN_LAUNCHES = {0: (("zeros", "ones", "last_one"), ("first_one", "random", "random_b")),
                 1: (("zeros", "ones", "last_one"), ("first_one", "random", "packed"))}


def scan_values(pattern, threads, dtype):
    rng = _rng(f"scan_{pattern}_{threads}_{dtype}")
    T = SCAN_DTYPES[dtype]
    v = np.zeros(threads, dtype=T)
    if pattern == "ones":
        v[:] = 1
    elif pattern == "last_one":
        v[-1] = 1
    elif pattern == "first_one":
        v[0] = 1
    elif pattern in ("random", "random_b"):
        v = rng.integers(0, 1000, threads).astype(T)
    elif pattern == "packed":          # csrc/tfidf.hip: (d << 32) | flag
        assert dtype == 1
        d = rng.integers(1 << 28, 1 << 29, threads).astype(np.uint64)
        v = (d << U64(32)) | rng.integers(0, 2, threads).astype(np.uint64)
    else:
        assert pattern == "zeros", pattern
    return v


def scan_launch(threads, dtype, which):
    """The input of one launch: SCAN_CALLS x threads."""
    return np.stack([scan_values(p, threads, dtype) for p in SCAN_LAUNCHES[dtype][which]])


def ref_excl_scan(rows):
    """(exclusive sums, totals) of every row, in the rows' own integer type (sums wrap as the device's do)."""
    inc = np.cumsum(rows, axis=1, dtype=rows.dtype)
    return inc - rows, inc[:, -1]


# ---- blockscan_kernel (block_scan.h) ---------------------------------------------------------------------------------------------
BLOCKSCAN_M = (0, 1, 1023, 1024, 1025, 2048, 2049, 5000)
BLOCKSCAN_TOTAL = ("null", "separate", "alias")              # alias: total = a + m (csrc/tokenise.hip)
BLOCKSCAN_VALUES = ("zeros", "ones", "random")


def blockscan_values(pattern, m):
    if pattern == "random":
        return _rng(f"blockscan_{m}").integers(0, 1000, m).astype(np.int32)
    return np.full(m, 1 if pattern == "ones" else 0, dtype=np.int32)


# ---- lower_bound (scan.h) -----------------------------------------------------------------------------------------------------------
LB_LEN = 1000


@functools.lru_cache(maxsize=None)
def lower_bound_case():
    """(a, lo, hi, v): a ascending with runs of duplicates and gaps; one query per row of (lo, hi, v)."""
    rng = _rng("lower_bound")
    a = (10 + np.cumsum(rng.choice([0, 0, 0, 1, 3, 7], LB_LEN))).astype(np.int32)
    q = []
    vals = np.unique(a)
    gaps = np.setdiff1d(np.arange(a[0], a[-1] + 1), vals)
    for v in [a[0] - 1, a[0] - 1000, a[-1] + 1, a[-1] + 1000, *vals, *gaps]:
        q.append((0, LB_LEN, v))
    ranges = [(1, LB_LEN), (137, LB_LEN), (0, LB_LEN - 1), (0, 412), (250, 750), (499, 501), (999, 1000), (0, 1),
              (0, 0), (500, 500), (LB_LEN, LB_LEN)]
    for lo, hi in ranges:
        near = set()
        for p in (lo - 1, lo, lo + 1, (lo + hi) // 2, hi - 2, hi - 1, hi):
            if 0 <= p < LB_LEN:
                near |= {int(a[p]) - 1, int(a[p]), int(a[p]) + 1}
        for v in sorted(near | {int(a[0]) - 1, int(a[-1]) + 1}):
            q.append((lo, hi, v))
    q = np.array(q, dtype=np.int64)
    return _frozen(a), _frozen(q[:, 0].astype(np.int32)), _frozen(q[:, 1].astype(np.int32)), _frozen(q[:, 2].astype(np.int32))


def ref_lower_bound(a, lo, hi, v):
    return np.array([l + np.searchsorted(a[l:h], x, "left") for l, h, x in zip(lo, hi, v)], dtype=np.int32)


# ---- radix sort (radix_sort.h) -------------------------------------------------------------------------------------------------------
RADIX_TILE = 1024
SORT_N = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
SORT_PASSES = (1, 2, 4)
SORT_PATTERNS = ("all_equal", "two_values", "descending", "three_values", "chunk_one_digit", "digit_once_per_chunk",
                 "uniform", "low_byte_constant")
SORT_CAP_EXTRA = 1500
ONCE_DIGIT = 200                     # digit_once_per_chunk: the digit every chunk of 64 holds exactly once
CONSTANT_BYTE = 0x5A                 # low_byte_constant


def sort_top(passes):
    """The largest key: non-negative ints below 2^(8 passes)."""
    return min((1 << (8 * passes)) - 1, (1 << 31) - 1)


def chunk_digit(c):
    return (37 * c + 11) % 256       # 37 is odd: distinct for the first 256 chunks


@functools.lru_cache(maxsize=None)
def sort_keys(pattern, n, passes):
    rng = _rng(f"sort_{pattern}_{n}_{passes}")
    top = sort_top(passes)
    i = np.arange(n, dtype=np.int64)
    if pattern == "all_equal":
        k = np.full(n, top // 3, dtype=np.int64)
    elif pattern == "two_values":
        k = rng.integers(0, 2, n) * top
    elif pattern == "descending":
        k = (n - 1 - i) * top // max(n - 1, 1)
    elif pattern == "three_values":
        k = np.array([top // 7, top // 2 + 1, top])[rng.integers(0, 3, n)]
    elif pattern == "chunk_one_digit":                                 # the chunk's digit in every byte the passes reach
        d = np.array([chunk_digit(c) for c in range((n + 63) // 64)], dtype=np.int64)[i // 64]
        k = (d | (d << 8) | (d << 16) | ((d >> 1) << 24)) & top
    elif pattern == "digit_once_per_chunk":
        low = rng.integers(0, 255, n)
        low = np.where(low >= ONCE_DIGIT, low + 1, low)                # any digit but ONCE_DIGIT
        for c in range((n + 63) // 64):
            size = min(64, n - 64 * c)
            low[64 * c + (7 * c) % size] = ONCE_DIGIT
        k = ((rng.integers(0, top + 1, n) & ~np.int64(255)) | low) & top
    elif pattern == "uniform":
        k = rng.integers(0, top + 1, n)
    elif pattern == "low_byte_constant":
        k = ((rng.integers(0, top + 1, n) & ~np.int64(255)) | CONSTANT_BYTE) & top
    else:
        raise ValueError(pattern)
    k = np.asarray(k, dtype=np.int64)
    assert k.min() >= 0 and k.max() <= top
    return _frozen(k.astype(np.int32))


@functools.lru_cache(maxsize=None)
def sort_gather_src(n):
    return _frozen(_rng(f"gather_{n}").integers(-(1 << 30), 1 << 30, n).astype(np.int32))


def ref_sort(key):
    """The permutation of a stable sort: val_out; key_out = key[val_out], gather_out = gather_src[val_out]."""
    return np.argsort(key, kind="stable").astype(np.int32)


# ---- radix select (radix_select.h) ----------------------------------------------------------------------------------------------------
def f64_key(x):
    """f64_key of csrc/common.h: the uint64 whose unsigned order is the order of the doubles, with -0.0 below +0.0."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> U64(63), ~u, u | U64(1 << 63))


def _u64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def _with_top_byte(rng, byte, n):
    return (_u64(rng, n) >> U64(8)) | (U64(byte) << U64(56))


def _around_bin(rng, in_bin, below=372, above=372, byte=0x40):
    """`below` keys with a smaller top byte, `in_bin` keys with top byte `byte`, `above` with a larger one, shuffled: the
    m // 2-th smallest lies in the bin of `byte`."""
    lo = _with_top_byte(rng, 0, below) | (rng.integers(0, byte, below).astype(np.uint64) << U64(56))
    hi = _with_top_byte(rng, 0, above) | (rng.integers(byte + 1, 256, above).astype(np.uint64) << U64(56))
    return rng.permutation(np.concatenate([lo, _with_top_byte(rng, byte, in_bin), hi]))


def _copies(rng, copies):
    """`copies` of one key among 783 distinct others, 39 of which share its top byte."""
    k = _around_bin(rng, 40)
    thr = k[(k >> U64(56)) == U64(0x40)][0]
    return rng.permutation(np.concatenate([k, np.full(copies - 1, thr, dtype=np.uint64)]))


def _scores(rng):
    """fp64 scores for the f64_key mode: both zeros, negatives, both infinities, subnormals, and values held at many
    positions.  No NaN: the comment on f64_key gives it no place."""
    pool = np.array([-0.0, 0.0, -np.inf, np.inf, 5e-324, -5e-324, 2.0 ** -1060, -(2.0 ** -1060), 1.5, -1.5, 1e300, -1e300])
    rep = pool[rng.integers(0, len(pool), 700)]
    return rng.permutation(np.concatenate([rep, rng.standard_normal(500)]))


# name -> (mode, builder): mode 0 builds uint64 keys, mode 1 fp64 scores
SELECT_TABLE = {
    "m1": (0, lambda r: _u64(r, 1)),
    "uniform_2": (0, lambda r: _u64(r, 2)),
    "uniform_1023": (0, lambda r: _u64(r, 1023)),
    "uniform_1024": (0, lambda r: _u64(r, 1024)),
    "uniform_1025": (0, lambda r: _u64(r, 1025)),
    "uniform_5000": (0, lambda r: _u64(r, 5000)),
    "all_equal": (0, lambda r: np.full(700, 0x0123456789ABCDEF, dtype=np.uint64)),
    # keys that differ only in bit 63: top == 64, maskbits = 0.  100 keys: the first bin is ranked; 600: it never shrinks
    "bit63_small": (0, lambda r: U64(0x0123456789ABCDEF) | (r.integers(0, 2, 100).astype(np.uint64) << U64(63))),
    "bit63_big": (0, lambda r: U64(0x0123456789ABCDEF) | (r.permutation(np.arange(600) % 2).astype(np.uint64) << U64(63))),
    # keys that differ only in bit 0: one digit, one bit wide, at lo == 0
    "bit0": (0, lambda r: U64(0xFEDCBA9876543210) | r.permutation(np.arange(600) % 2).astype(np.uint64)),
    # the top 56 bits shared: the first and only pass has lo == 0, so not even a bin of <= 256 keys is ranked
    "share_top56": (0, lambda r: U64(0x7766554433221100) | r.permutation(np.arange(200) % 256).astype(np.uint64)),
    "bin_256": (0, lambda r: _around_bin(r, 256)),
    "bin_257": (0, lambda r: _around_bin(r, 257)),
    "copies_300": (0, lambda r: _copies(r, 300)),
    "copies_256": (0, lambda r: _copies(r, 256)),
    "five_values_small": (0, lambda r: _u64(r, 5)[r.integers(0, 5, 500)]),
    "five_values_big": (0, lambda r: _u64(r, 5)[r.integers(0, 5, 1700)]),
    "f64_scores": (1, _scores),
}
SELECT_NAMES = tuple(SELECT_TABLE)


@functools.lru_cache(maxsize=None)
def select_case(name):
    """(mode, what the device reads, the uint64 keys)."""
    mode, build = SELECT_TABLE[name]
    data = np.ascontiguousarray(build(_rng("select_" + name)))
    keys = f64_key(data) if mode else data.astype(np.uint64)
    return mode, _frozen(data), _frozen(np.ascontiguousarray(keys))


def select_kks(m):
    return sorted({kk for kk in (1, 2, m // 2, m - 1, m) if 1 <= kk <= m})


def ref_select(keys, kk):
    """(thr, need_eq, equal) from a sort of the (key, position) pairs: the kk-th smallest key, how many of the keys equal to
    it are among the kk smallest pairs, how many keys equal it."""
    order = np.lexsort((np.arange(len(keys)), keys))
    thr = keys[order[kk - 1]]
    return int(thr), kk - int((keys < thr).sum()), int((keys == thr).sum())


def select_trace(keys, kk):
    """block_select_threshold restated: bits above the highest one in which the smallest and the largest key differ are
    skipped; passes over digits of at most 8 bits from the top; a pass that leaves the kk-th key in a bin of <= 256 keys
    with lo > 0 ends the passes, and the bin is ranked by (key, position).
    -> passes, end ("all_equal", "ranked", "out_of_bits"), top, ranked_bin, thr, need_eq, eq_count (as the device returns)."""
    keys = [int(k) for k in np.asarray(keys, dtype=np.uint64)]
    assert 1 <= kk <= len(keys)
    mn, mx = min(keys), max(keys)
    diff = mn ^ mx
    if diff == 0:
        return dict(passes=0, end="all_equal", top=-1, ranked_bin=0, thr=mn, need_eq=kk, eq_count=-1)
    top0 = top = diff.bit_length()
    maskbits = 0 if top >= 64 else (M64 << top) & M64
    prefix, rem, passes, done = mn & maskbits, kk, 0, False
    while top > 0 and not done:
        lo = max(top - 8, 0)
        width = top - lo
        hist = [0] * (1 << width)
        for k in keys:
            if k & maskbits == prefix:
                hist[(k >> lo) & ((1 << width) - 1)] += 1
        cum = dsel = 0
        for b in range(1 << width):
            if cum + hist[b] >= rem:
                dsel = b
                break
            cum += hist[b]
        rem -= cum
        prefix |= dsel << lo
        maskbits |= ((1 << width) - 1) << lo
        top, passes = lo, passes + 1
        done = hist[dsel] <= 256 and lo > 0
    if not done:
        return dict(passes=passes, end="out_of_bits", top=top0, ranked_bin=0, thr=prefix, need_eq=rem, eq_count=-1)
    cand = sorted(k for k in keys if k & maskbits == prefix)
    thr = cand[rem - 1]
    return dict(passes=passes, end="ranked", top=top0, ranked_bin=len(cand), thr=thr,
                need_eq=rem - sum(k < thr for k in cand), eq_count=sum(k == thr for k in cand))


# ---- union-find (union_find.h) -----------------------------------------------------------------------------------------------------------
def _shuffled(rng, a, b):
    """The edges in random order, every second one turned round."""
    a, b = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32)
    p = rng.permutation(len(a))
    a, b = a[p], b[p]
    flip = rng.random(len(a)) < 0.5
    return np.where(flip, b, a).astype(np.int32), np.where(flip, a, b).astype(np.int32)


def _uf_two_trees(rng, n=4096, m=50000):
    """Rows 0 and 1 hammered: nearly every edge joins row 0 to an even row or row 1 to an odd one, so the two trees grow under
    contention on their roots; one edge in a hundred links the trees."""
    x = rng.integers(0, n, m)
    a = np.where(x % 2 == 0, 0, 1)
    link = rng.random(m) < 0.01
    a = np.where(link, x ^ 1, a)
    return n, a.astype(np.int32), x.astype(np.int32)


def _uf_forest(rng, n=20000, m=15000):
    """m rows get one edge each to a row before them: no cycle; then the rows are renumbered at random."""
    child = np.sort(rng.permutation(np.arange(1, n))[:m])
    par = (rng.random(m) * child).astype(np.int64)
    name = rng.permutation(n)
    return (n,) + _shuffled(rng, name[child], name[par])


UF_TABLE = {
    "single_self_loop": lambda r: (1, np.zeros(1, np.int32), np.zeros(1, np.int32)),
    "self_loops": lambda r: (100, *(2 * (r.integers(0, 100, 500).astype(np.int32),))),
    "same_pair": lambda r: (50, *_shuffled(r, np.full(10000, 7), np.full(10000, 31))),
    "path": lambda r: (4096, *_shuffled(r, np.arange(4095), np.arange(1, 4096))),
    "star_last": lambda r: (4096, *_shuffled(r, np.arange(4095), np.full(4095, 4095))),
    "star_first": lambda r: (4096, *_shuffled(r, np.arange(1, 4096), np.zeros(4095))),
    "two_trees": _uf_two_trees,
    "random_graph": lambda r: (4096, r.integers(0, 4096, 100000).astype(np.int32), r.integers(0, 4096, 100000).astype(np.int32)),
    "random_forest": _uf_forest,
}
UF_NAMES = tuple(UF_TABLE)


@functools.lru_cache(maxsize=None)
def uf_case(name):
    n, a, b = UF_TABLE[name](_rng("uf_" + name))
    return n, _frozen(np.ascontiguousarray(a, dtype=np.int32)), _frozen(np.ascontiguousarray(b, dtype=np.int32))


class HostUnionFind:
    """The smaller root stays a root: a tree's root is its smallest member."""

    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def unite(self, a, b):
        """True when the two were different trees."""
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.parent[max(a, b)] = min(a, b)
        return True

    def roots(self):
        return np.array([self.find(x) for x in range(len(self.parent))], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def ref_roots(name):
    """Per row the smallest member of its component."""
    n, a, b = uf_case(name)
    uf = HostUnionFind(n)
    for x, y in zip(a.tolist(), b.tolist()):
        uf.unite(x, y)
    return _frozen(uf.roots())


def spanning_forest_defect(n, a, b, joined, roots):
    """None when the edges flagged `joined` are a spanning forest of the components `roots`: as many as n - components, no
    cycle among them, and the same components.  Otherwise what is wrong."""
    comps = len(np.unique(roots))
    flagged = np.flatnonzero(joined)
    if len(flagged) != n - comps:
        return f"{len(flagged)} joined flags, n - components = {n - comps}"
    uf = HostUnionFind(n)
    for e in flagged.tolist():
        if not uf.unite(int(a[e]), int(b[e])):
            return f"edge {e} ({a[e]}, {b[e]}) closes a cycle among the joined edges"
    if not np.array_equal(uf.roots(), roots):
        return "the joined edges span other components"
    return None
