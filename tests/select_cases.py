"""Inputs shared by tests/test_select_cases_host.py and tests/test_gpu_select_meta.py: the case table of the metadata and
sparse-text neighbour selection (chunk_select_kernel of csrc/meta_stream.hip, select_k_kernel<SRC_HAVERSINE | SRC_TIME |
SRC_JACCARD> of csrc/knn.hip), a NumPy reference of every score source, the k smallest (score, column) pairs per row by a
stable lexsort, NumPy restatements of the running-list merge and of the radix select's control flow, and emulations of
plausibly wrong devices.  No torch, no device, everything seeded.

What the device promises and these cases test: per row the k smallest (score, column) pairs, ascending columns, ties to the
smaller column, for any chunk size; the scores restated operation by operation from csrc/meta_scores.h and
csrc/meta_stream.hip:
  time      |b0 - a0| + |b1 - a1| in fp64.  Every case uses whole numbers or multiples of one power of two, so that every
            operation is exact and the reference equals the device bit for bit.
  tags      0 - |A & B| / |A | B| with one fp64 division, 0 when either set is empty, +1.0 in a row's own column: exact.
  text      0 - sum_t x_it x_jt over row i's entries in STORED order from +0.0, each product rounded, then each addition;
            terms row j lacks add nothing.  The same roundings in the same order: exact.
  location  haversine km in np.longdouble.  The device differs in the last bits of sin, cos and asin, so the inputs make
            the answer unique: (a) no two distinct geotags closer than MIN_SEPARATION_DEG, which bounds the effect of
            rounding the coordinates to radians at about 4e-12 relative; (b) for every tested (row, k) no column but exact
            duplicates of the k-th one within REL_GAP = 1e-9 of the k-th score: more than two orders above (a)'s bound.

No score is -0.0 (the host test asserts it): |x| + |y|, 2 asin(sqrt(a)) 6371 and 0.0 - x are never -0.0, so the order of the
values is the order of the device's keys and a NumPy sort, which takes -0.0 and +0.0 for equal, decides as the device does.

Sizes: n = 257 (four 64-column chunks and one column more; a prime, so only the chunks 1 and n divide it), 600 for the big
tie, 100 and 1025 for the mask pitches around first_free = ceil(n / 1024) * 16, 1025 and 1100 for k = 1024 = CS_MAX_K, 1."""
import functools
from fractions import Fraction

import numpy as np

LD = np.longdouble
N = 257
CS_MAX_K = 1024                      # csrc/meta_stream.hip
CS_MAX_CHUNK = 16384
CS_LDS_DYN = 152 * 1024
MIN_SEPARATION_DEG = 0.01
REL_GAP = 1e-9
SCORE_RTOL = 1e-10                   # mused_record_scores against the longdouble haversine, nonzero entries
RECORDS = ("location", "time")
ENTRY = 5                            # the query row of text_order_probe ...
PROBE_P, PROBE_Q = 40, 200           # ... and its two tied columns
FMA_A, FMA_A_TWO, FMA_A_ONE = 5, 40, 200     # text_fma_probe: query row, its two-term column, its one-term column ...
FMA_B, FMA_B_ONE, FMA_B_TWO = 7, 30, 220     # ... and the mirrored probe, the one-term column first
TIE_ROWS = 400                       # time_big_tie: rows that share one record


def words_for(n):
    return (n + 63) // 64


def _rng(name):
    return np.random.default_rng([ord(c) for c in name])


class Case:
    """source "location" / "time": rec (n x 2 fp64).  "tags" / "text": rowptr, cols (tag / term ids in stored order), n_cols,
    postptr, postrow (and vals, postval for "text")."""

    def __init__(self, name, source, reaches, extra_ks, **data):
        self.name, self.source, self.reaches, self.extra_ks = name, source, reaches, extra_ks
        self.__dict__.update(data)
        if source in RECORDS:
            self.n = len(self.rec)
        else:
            self.n = len(self.rowptr) - 1
            self.postptr, self.postrow, self.postval = postings(self.rowptr, self.cols, self.n_cols, data.get("vals"))
        for a in self.__dict__.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


def postings(rowptr, cols, n_cols, vals=None):
    """Posting lists of a CSR, rows ascending inside a list, as WindowEngine._postings builds them."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rowptr))
    order = np.argsort(cols, kind="stable")
    postptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=max(n_cols, 1)))]).astype(np.int32)
    return postptr, rows[order], (None if vals is None else np.ascontiguousarray(vals[order], dtype=np.float64))


def _csr(sets, vals=None):
    rowptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    cols = np.concatenate([np.asarray(s, dtype=np.int32) for s in sets] + [np.zeros(0, np.int32)]).astype(np.int32)
    if vals is None:
        return rowptr, cols
    return rowptr, cols, np.concatenate([np.asarray(v, dtype=np.float64) for v in vals] + [np.zeros(0)])


# ---- builders ---------------------------------------------------------------------------------------------------------------
def loc_pairs(n):
    """(a, b), a < b, of exactly duplicated geotags: odd distances, and more than 128 rows apart."""
    pairs = [(10, 11), (20, 23), (60, 189), (100, 201), (126, 255)]
    if n > 1000:
        pairs += [(3, n - 1), (500, 901)]
    return [p for p in pairs if p[1] < n]


def _location(name, n):
    rng = _rng(name)
    rec = np.column_stack([rng.uniform(-60, 60, n), rng.uniform(-180, 180, n)])
    for a, b in loc_pairs(n):
        rec[b] = rec[a]
    return dict(rec=rec)


def _time_random(name, n):
    return dict(rec=_rng(name).integers(0, 10 ** 6, (n, 2)).astype(np.float64))


def _all_equal(name, n, value):
    return dict(rec=np.tile(np.asarray(value, dtype=np.float64), (n, 1)))


def _time_low_bits(name, n):
    rec = np.zeros((n, 2))
    rec[1:, 0] = 1.0 + np.arange(1, n) * 2.0 ** -52
    return dict(rec=rec)


def _time_tiny_steps(name, n):
    """Subnormal records floor(j / 2) 2^-1074: every score is a whole number of 2^-1074 below 2^7, its own column's 0
    included, so the keys of a row differ only below bit 8."""
    rec = np.zeros((n, 2))
    rec[:, 0] = (np.arange(n) // 2) * 2.0 ** -1074
    return dict(rec=rec)


def _time_big_tie(name, n):
    rng = _rng(name)
    rec = rng.integers(0, 1000, (n, 2)).astype(np.float64)
    shared = np.flatnonzero(np.arange(n) % 3 != 0)
    assert len(shared) == TIE_ROWS
    rec[shared] = (500.0, 500.0)
    return dict(rec=rec)


def _time_small_tie(name, n):
    """Groups of 2 to 40 identical records, their members scattered over the rows."""
    rng = _rng(name)
    sizes, total = [], 0
    while total < n:
        s = min((2, 3, 5, 8, 13, 21, 40)[len(sizes) % 7], n - total)
        sizes.append(s)
        total += s
    value = rng.permutation(10 * len(sizes))[:len(sizes)] * 1000.0
    group = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    return dict(rec=np.column_stack([value[group], np.zeros(n)]))


def _time_whole_hours(name, n):
    return dict(rec=_rng(name).integers(0, 24, (n, 2)).astype(np.float64))


def _tags_random(name, n, n_tags=20):
    rng = _rng(name)
    sets = [np.sort(rng.choice(n_tags, rng.integers(0, 5), replace=False)) for _ in range(n)]
    for a, b in loc_pairs(n):
        sets[b] = sets[a]
    rowptr, cols = _csr(sets)
    return dict(rowptr=rowptr, cols=cols, n_cols=n_tags)


def _tags_all_empty(name, n):
    return dict(rowptr=np.zeros(n + 1, np.int32), cols=np.zeros(0, np.int32), n_cols=0)


def _tags_block(name, n):
    """Tag t in rows [64 t, 64 t + 64), tag B + t in rows [64 t + 1, 64 t + 65), both cut at n."""
    B = (n + 63) // 64
    sets = [[] for _ in range(n)]
    for t in range(B):
        for r in range(64 * t, min(64 * t + 64, n)):
            sets[r].append(t)
        for r in range(64 * t + 1, min(64 * t + 65, n)):
            sets[r].append(B + t)
    rowptr, cols = _csr(sets)
    return dict(rowptr=rowptr, cols=cols, n_cols=2 * B)


def _tags_unused_ids(name, n):
    rng = _rng(name)
    sets = [np.sort(2 * rng.choice(10, rng.integers(0, 5), replace=False)) for _ in range(n)]   # even ids below 20 only
    rowptr, cols = _csr(sets)
    return dict(rowptr=rowptr, cols=cols, n_cols=40)


def _text_random(name, n, n_terms=24):
    rng = _rng(name)
    sets, vals = [], []
    for _ in range(n):
        nt = 0 if rng.random() < 0.1 else int(rng.integers(1, 9))
        sets.append(rng.permutation(n_terms)[:nt])                   # stored order: shuffled
        v = rng.uniform(0.1, 1.0, nt)
        vals.append(v / np.sqrt((v * v).sum()) if nt else v)
    for a, b in loc_pairs(n):
        sets[b], vals[b] = sets[a], vals[a]
    rowptr, cols, v = _csr(sets, vals)
    return dict(rowptr=rowptr, cols=cols, vals=v, n_cols=n_terms)


def _text_order_probe(name, n):
    """Row ENTRY stores the terms 2, 3, 1, 0 with value 1.  Column PROBE_P holds the terms 0, 1, 2 with 0.3, 0.2, 0.1: in
    stored order the products add up as (0.1 + 0.2) + 0.3 = 0.6000000000000001, in ascending-term order as (0.3 + 0.2) + 0.1 =
    0.6.  Column PROBE_Q holds term 3 alone with the stored-order sum.  No other row holds a term below 4."""
    rng = _rng(name)
    sets, vals = [], []
    for _ in range(n):
        nt = int(rng.integers(1, 5))
        sets.append(4 + rng.permutation(16)[:nt])
        vals.append(rng.uniform(0.1, 1.0, nt))
    sets[ENTRY], vals[ENTRY] = [2, 3, 1, 0], [1.0, 1.0, 1.0, 1.0]
    sets[PROBE_P], vals[PROBE_P] = [0, 1, 2], [0.3, 0.2, 0.1]
    sets[PROBE_Q], vals[PROBE_Q] = [3], [(0.1 + 0.2) + 0.3]
    rowptr, cols, v = _csr(sets, vals)
    return dict(rowptr=rowptr, cols=cols, vals=v, n_cols=20)


def fma(a, b, c):
    """a * b + c with one rounding."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _two_products(rng, fused_is_smaller):
    """(x1, x2), (y1, y2) in [0.1, 1): x1 y1 + x2 y2 with every operation rounded differs from the sum whose second product
    is not rounded before the addition, in the direction asked for."""
    while True:
        x1, x2, y1, y2 = rng.uniform(0.1, 1.0, 4)
        first = x1 * y1
        each, fused = first + x2 * y2, fma(x2, y2, first)
        if (fused < each) if fused_is_smaller else (fused > each):
            return (x1, x2), (y1, y2), each


def _text_fma_probe(name, n):
    """Row FMA_A stores the terms 0, 1, 2 with x1, x2, 1.  Column FMA_A_TWO holds the terms 0, 1 with y1, y2, column FMA_A_ONE
    behind it holds term 2 alone with fl(fl(x1 y1) + fl(x2 y2)): the two tie and the smaller column wins; with a fused
    multiply-add the two-term sum is smaller, so the one-term column wins.  Row FMA_B (terms 10, 11, 12) is the mirror: the
    one-term column FMA_B_ONE comes first and wins the tie, the fused sum of FMA_B_TWO is larger and would beat it.  So an
    error of either sign in the last bit of a sum changes a list.  No other row holds a term below 16."""
    rng = _rng(name)
    sets, vals = [], []
    for _ in range(n):
        nt = int(rng.integers(1, 5))
        sets.append(16 + rng.permutation(16)[:nt])
        vals.append(rng.uniform(0.1, 1.0, nt))
    x, y, each = _two_products(rng, True)
    sets[FMA_A], vals[FMA_A] = [0, 1, 2], [x[0], x[1], 1.0]
    sets[FMA_A_TWO], vals[FMA_A_TWO] = [0, 1], list(y)
    sets[FMA_A_ONE], vals[FMA_A_ONE] = [2], [each]
    x, y, each = _two_products(rng, False)
    sets[FMA_B], vals[FMA_B] = [10, 11, 12], [x[0], x[1], 1.0]
    sets[FMA_B_TWO], vals[FMA_B_TWO] = [10, 11], list(y)
    sets[FMA_B_ONE], vals[FMA_B_ONE] = [12], [each]
    rowptr, cols, v = _csr(sets, vals)
    return dict(rowptr=rowptr, cols=cols, vals=v, n_cols=32)


def _text_signed(name, n, n_terms=16):
    rng = _rng(name)
    sets, vals = [], []
    for _ in range(n):
        nt = int(rng.integers(1, 7))
        sets.append(rng.permutation(n_terms)[:nt])
        mag = rng.choice([1.0, 0.5, 1e-3, 1e-160, 1e-200], nt) * rng.uniform(1.0, 2.0, nt)
        vals.append(mag * rng.choice([-1.0, 1.0], nt))
    for a, b in loc_pairs(n):
        sets[b], vals[b] = sets[a], vals[a]
    rowptr, cols, v = _csr(sets, vals)
    return dict(rowptr=rowptr, cols=cols, vals=v, n_cols=n_terms)


# ---- the table: name, source, n, builder, extra k, what the case reaches (tests/test_select_cases_host.py checks each
# word against the keys; the words are explained at CLAIMS there) --------------------------------------------------------------
TABLE = (
    # the general path: wide first digit, candidate ranking, duplicates decided by column
    ("loc_random", "location", N, _location, (), ("cand_rank", "ballot_fast_path", "duplicate_ties")),
    # every key of every row equal: diff == 0, no radix pass, all k taken in column order by the general emit path
    ("loc_all_equal", "location", N, lambda s, n: _all_equal(s, n, (48.2, 16.37)), (), ("diff0",)),
    # k = 1024 = CS_MAX_K below n, two scan blocks of 1024 columns, a 17th mask word
    ("loc_1025", "location", 1025, _location, (), ("k_max", "ballot_fast_path", "duplicate_ties")),
    ("loc_n1", "location", 1, _location, (), ("single_row",)),
    ("time_random", "time", N, _time_random, (), ("cand_rank", "ballot_fast_path")),
    ("time_all_equal", "time", N, lambda s, n: _all_equal(s, n, (7.0, 9.0)), (), ("diff0",)),
    # row 0: its own column scores 0, the 256 others 1 + j 2^-52: the keys first differ at bit 61 and the bin of the k-th key
    # (k >= 2) holds exactly 256 keys, the most the candidate ranking takes.  (Its own column keeps row 0 from a narrow first
    # digit; time_tiny_steps has one.)
    ("time_low_bits", "time", N, _time_low_bits, (), ("cand_full",)),
    # keys that differ only below bit 8: the first digit is narrower than 8 bits and the only one, so the radix ends at bit 0
    # without a candidate ranking and ties of 2 to 4 columns are cut by an emit that does not know their size
    ("time_tiny_steps", "time", N, _time_tiny_steps, (), ("narrow_first_digit", "tie_cut_count_unknown")),
    # 400 of 600 columns tie at the threshold: the radix runs to bit 0, no candidate ranking, the count of equal keys is
    # unknown to the emit; at chunk 64 the tie spans every chunk boundary and k cuts it across them
    ("time_big_tie", "time", 600, _time_big_tie, (300, TIE_ROWS, TIE_ROWS + 1),
     ("radix_to_bit0", "tie_straddles_boundary")),
    # ties of 2 to 40 columns cut by k: finished by ranking the candidates
    ("time_small_tie", "time", N, _time_small_tie, (), ("cand_rank_tie_cut", "ballot_fast_path", "tie_straddles_boundary")),
    ("time_whole_hours", "time", N, _time_whole_hours, (), ("cand_rank_tie_cut", "tie_straddles_boundary")),
    ("time_100", "time", 100, _time_random, (), ("cand_rank", "ballot_fast_path")),        # mask pitches below first_free = 16
    ("time_1100", "time", 1100, _time_random, (), ("k_max", "ballot_fast_path")),          # k = 1024 with 76 columns left out
    ("time_n1", "time", 1, _time_random, (), ("single_row",)),
    # negative scores next to 0 and +1: keys that differ in the sign bit (top == 64); empty and duplicated sets
    ("tags_random", "tags", N, _tags_random, (), ("sign_bit", "empty_rows", "duplicate_ties", "cand_rank_tie_cut")),
    # every score 0 but a row's own +1: one key above 256 equal ones (the keys first differ at bit 61, not in the sign bit),
    # every k < n lands in the tie of 256 and is finished by ranking exactly 256 candidates
    ("tags_all_empty", "tags", N, _tags_all_empty, (), ("empty_rows", "cand_full", "empty_postings")),
    # posting lists that start and end on the boundaries of chunk 64, and one row behind them
    ("tags_block", "tags", N, _tags_block, (), ("postings_on_boundary", "postings_behind_boundary", "sign_bit",
                                                 "tie_straddles_boundary")),
    # n_tags above every id in use, odd ids unused: empty posting lists between and behind the used ones
    ("tags_unused_ids", "tags", N, _tags_unused_ids, (), ("empty_postings", "empty_rows", "sign_bit")),
    ("tags_100", "tags", 100, _tags_random, (), ("sign_bit",)),                            # mask pitches below first_free = 16
    ("tags_1025", "tags", 1025, _tags_random, (), ("sign_bit", "radix_to_bit0")),          # a 17th mask word, and a 33rd
    # unit rows of 0 to 8 terms in shuffled order, duplicated rows; a tenth of the rows empty: all their scores are 0 (diff == 0)
    ("text_random", "text", N, _text_random, (), ("sign_bit", "empty_rows", "diff0", "duplicate_ties", "stored_order_matters")),
    # one tie that only the stored summation order makes: PROBE_P wins it by column, ascending-term order gives PROBE_Q
    ("text_order_probe", "text", N, _text_order_probe, (), ("order_probe", "tie_straddles_boundary")),
    # two ties that only a rounded product makes: a fused multiply-add in the accumulation gives the other column, whichever
    # way it moves the last bit
    ("text_fma_probe", "text", N, _text_fma_probe, (), ("fma_probe",)),
    # both signs, products that underflow to a subnormal or to (-)0.  The accumulator starts at +0.0, +0.0 + -0.0 = +0.0 and
    # 0.0 - acc is never -0.0, so the order of the values is the order of the keys.
    ("text_signed", "text", N, _text_signed, (), ("sign_bit", "underflow", "duplicate_ties")),
)
NAMES = tuple(t[0] for t in TABLE)
NAMES_OF = {src: tuple(t[0] for t in TABLE if t[1] == src) for src in ("location", "time", "tags", "text")}
LDS_ROW_NAMES = NAMES_OF["location"] + NAMES_OF["time"] + NAMES_OF["tags"]     # mused_record_knn / mused_jaccard_knn


@functools.lru_cache(maxsize=None)
def case(name):
    _, source, n, builder, extra, reaches = TABLE[NAMES.index(name)]
    return Case(name, source, reaches, extra, **builder(name, n))


# ---- parameters -----------------------------------------------------------------------------------------------------------
def ks(name, chunked):
    """k of a case.  The chunked entries stop at CS_MAX_K; the LDS-row entries take any k <= n."""
    c = case(name)
    out = {1, 2, 50, 51, 151, c.n - 1, c.n} | set(c.extra_ks)
    if c.source in RECORDS and c.n in (1025, 1100):
        out.add(1024)
    return sorted(k for k in out if 1 <= k <= c.n and (not chunked or k <= CS_MAX_K))


def chunks(n):
    out = {1, 7, 64, 256, n - 1, n, n + 1, 0}
    if n >= 1025:
        out.discard(1)
    return sorted(out)


MASK_CHUNK = 64          # the chunk of the chunked runs that also build a mask


def mask_words(n, lds_row):
    out = [words_for(n), words_for(n) + 3]
    if lds_row and n == 100:
        out += [16, 17, 20]          # around first_free = 16: the kernel zeroes words from there on
    if lds_row and n == 1025:
        out += [33]                  # first_free = 32
    return out


def effective_chunk(k, chunk):
    """chunk_for of csrc/meta_stream.hip."""
    c = min((CS_LDS_DYN - 12 * k) // 8, CS_MAX_CHUNK)
    return chunk if 0 < chunk < c else c


# ---- scores -----------------------------------------------------------------------------------------------------------------
def haversine_km(rec, T):
    """haversine_km of csrc/meta_scores.h in type T, the row as location1 and the column as location2."""
    x = np.asarray(rec, dtype=np.float64).astype(T)
    pi = 4 * np.arctan(T(1)) if T is LD else T(np.pi)
    lat, lon = x[:, 0] * (pi / T(180)), x[:, 1] * (pi / T(180))
    sdlat = np.sin((lat[None, :] - lat[:, None]) * T(0.5))
    sdlon = np.sin((lon[None, :] - lon[:, None]) * T(0.5))
    a = sdlat * sdlat + (np.cos(lat)[:, None] * np.cos(lat)[None, :]) * (sdlon * sdlon)
    return T(2) * np.arcsin(np.sqrt(a)) * T(6371)


def time_l1(rec):
    a = np.asarray(rec, dtype=np.float64)
    return np.abs(a[None, :, 0] - a[:, None, 0]) + np.abs(a[None, :, 1] - a[:, None, 1])


def jaccard(c, drop=None, self_one=True):
    """drop: columns whose intersection counts a defective posting-list cut loses."""
    B = np.zeros((c.n, max(c.n_cols, 1)), dtype=np.int64)
    B[np.repeat(np.arange(c.n), np.diff(c.rowptr)), c.cols] = 1
    size = B.sum(axis=1)
    inter = B @ B.T
    if drop is not None:
        inter[:, drop] = 0
    both = (size[:, None] > 0) & (size[None, :] > 0)
    union = np.where(both, size[:, None] + size[None, :] - inter, 1)
    S = np.where(both, 0.0 - inter / union, 0.0)
    if self_one:
        np.fill_diagonal(S, 1.0)
    return S


def sparse_cosine(c, ascending=False, drop=None, fused=False):
    """Row i's entries in stored order (ascending: by term id, what the device must NOT do), each product rounded, then
    each addition, from +0.0 (fused: acc = fma(x_it, x_jt, acc), one rounding, what the device must NOT do either)."""
    S = np.zeros((c.n, c.n))
    for i in range(c.n):
        acc = np.zeros(c.n)
        entries = range(c.rowptr[i], c.rowptr[i + 1])
        if ascending:
            entries = sorted(entries, key=lambda t: c.cols[t])
        for t in entries:
            lo, hi = c.postptr[c.cols[t]], c.postptr[c.cols[t] + 1]
            rows = c.postrow[lo:hi]
            if fused:
                acc[rows] = [fma(c.vals[t], pv, a) for pv, a in zip(c.postval[lo:hi], acc[rows])]
            else:
                acc[rows] = acc[rows] + c.vals[t] * c.postval[lo:hi]
        if drop is not None:
            acc[drop] = 0.0
        S[i] = 0.0 - acc
    return S


@functools.lru_cache(maxsize=None)
def scores(name):
    """The reference score matrix (read-only): longdouble for "location", fp64 and exact for the others."""
    c = case(name)
    S = {"location": lambda: haversine_km(c.rec, LD), "time": lambda: time_l1(c.rec), "tags": lambda: jaccard(c),
         "text": lambda: sparse_cosine(c)}[c.source]()
    S.setflags(write=False)
    return S


def f64_key(S):
    """f64_key of csrc/common.h: unsigned keys in the order of the doubles."""
    u = np.ascontiguousarray(S, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


# ---- the reference selection ----------------------------------------------------------------------------------------------------
def full_order(S, larger_column_first=False):
    """Per row every column by (score, column): a stable lexsort."""
    cols = np.arange(S.shape[1])
    tie = -cols if larger_column_first else cols
    return np.stack([np.lexsort((tie, row)) for row in S])


def topk(S, k):
    """Per row the columns of the k smallest (score, column) pairs, ascending columns."""
    return np.sort(full_order(S)[:, :k], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _order(name):
    return full_order(scores(name))


@functools.lru_cache(maxsize=None)
def reference_lists(name, k):
    out = np.sort(_order(name)[:, :k], axis=1).astype(np.int32)
    out.setflags(write=False)
    return out


def mask_of(idx, n, words):
    """The bitmask of lists: the row's list bits, its own bit cleared, zero in every padding word."""
    sel = np.zeros((n, 64 * words), dtype=bool)
    np.put_along_axis(sel, np.asarray(idx, dtype=np.int64), True, axis=1)
    sel[np.arange(n), np.arange(n)] = False
    bits = sel.reshape(n, words, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(bits, axis=2)


# ---- the running-list merge, chunk by chunk -----------------------------------------------------------------------------------
def merge_select(K, k, chunk, chunk_first=False, skip_single_last=False):
    """chunk_select_kernel restated on keys K (rows x n, uint64): the running list (the k smallest pairs of the columns seen
    so far, ascending columns) is followed by the keys of the next chunk; the min(k, m) smallest by (key, position) stay, in
    position order.  Returns the lists, -1 where none came.
    chunk_first (defect E2): the chunk stands before the running list, so equal keys go to the chunk's columns.
    skip_single_last (defect E6): a last chunk of exactly one column is never read."""
    R, n = K.shape
    c = effective_chunk(k, chunk)
    run_key, run_col = np.zeros((R, 0), np.uint64), np.zeros((R, 0), np.int64)
    for c0 in range(0, n, c):
        c1 = min(n, c0 + c)
        if skip_single_last and c1 == n and c1 - c0 == 1 and c0 > 0:
            break
        parts = [(run_key, run_col), (K[:, c0:c1], np.broadcast_to(np.arange(c0, c1), (R, c1 - c0)))]
        if chunk_first:
            parts.reverse()
        key = np.concatenate([p[0] for p in parts], axis=1)
        col = np.concatenate([p[1] for p in parts], axis=1)
        keep = np.sort(np.argsort(key, axis=1, kind="stable")[:, :min(k, key.shape[1])], axis=1)
        run_key, run_col = np.take_along_axis(key, keep, axis=1), np.take_along_axis(col, keep, axis=1)
        if chunk_first:                                              # back to ascending columns, as the list is stored
            back = np.argsort(run_col, axis=1)
            run_key, run_col = np.take_along_axis(run_key, back, axis=1), np.take_along_axis(run_col, back, axis=1)
    out = np.full((R, k), -1, dtype=np.int32)
    out[:, :run_col.shape[1]] = run_col
    return out


# ---- the radix select's control flow ------------------------------------------------------------------------------------------
def radix_trace(keys, k):
    """What select_k_kernel / chunk_select_kernel do on one row of keys for the k-th smallest: top (bits [top, 64) are common
    to the min and max keys; -1 when all keys are equal), first_width (bits of the first digit), passes, done (finished by
    ranking the candidates), ncand, equal (keys equal to the threshold), need_eq (how many of them are taken), eq_known (the
    emit knows `equal`: only after a candidate ranking)."""
    keys = np.asarray(keys, dtype=np.uint64)
    thr = np.sort(keys)[k - 1]
    equal = int((keys == thr).sum())
    need_eq = k - int((keys < thr).sum())
    diff = int(keys.min()) ^ int(keys.max())
    t = dict(top=-1, first_width=0, passes=0, done=False, ncand=0, equal=equal, need_eq=need_eq, eq_known=False)
    if diff == 0:
        return t
    top = diff.bit_length()
    t["top"], t["first_width"] = top, top - max(top - 8, 0)
    alive, rem = keys, k
    while top > 0:
        lo = max(top - 8, 0)
        digit = (alive >> np.uint64(lo)) & np.uint64((1 << (top - lo)) - 1)
        hist = np.bincount(digit.astype(np.int64), minlength=1 << (top - lo))
        cum = np.cumsum(hist)
        dsel = int(np.searchsorted(cum, rem))
        rem -= int(cum[dsel] - hist[dsel])
        alive = alive[digit == np.uint64(dsel)]
        top = lo
        t["passes"] += 1
        if hist[dsel] <= 256 and lo > 0:
            t["done"], t["ncand"], t["eq_known"] = True, int(hist[dsel]), True
            break
    assert (alive == thr).sum() == equal and (t["done"] or len(alive) == equal)
    return t


# ---- defect emulations: the lists a plausibly wrong device would give -------------------------------------------------------
DEFECTS = ("E1", "E2", "E3a", "E3b", "E4", "E5", "E6", "E7")


def _scores_with(name, **kw):
    c = case(name)
    return jaccard(c, **kw) if c.source == "tags" else sparse_cosine(c, **kw)


def emulate(defect, name, k, chunk):
    """E1  ties go to the larger column
    E2  at a merge the chunk's columns rank before the running list's on equal keys
    E3a the posting-list cut drops row c1 - 1 of every chunk [c0, c1); E3b: row c0   (tags, text)
    E4  sparse cosine summed in ascending-term order                                   (text)
    E5  Jaccard self score not forced to +1                                            (tags)
    E6  the last chunk is skipped when it holds exactly one column
    E7  sparse cosine accumulated by fused multiply-adds: the products are not rounded    (text)"""
    c = case(name)
    S = scores(name)
    if defect == "E1":
        return np.sort(full_order(S, larger_column_first=True)[:, :k], axis=1).astype(np.int32)
    if defect == "E2":
        return merge_select(f64_key(S), k, chunk, chunk_first=True)
    if defect in ("E3a", "E3b"):
        ce = effective_chunk(k, chunk)
        starts = np.arange(0, c.n, ce)
        drop = starts if defect == "E3b" else np.minimum(starts + ce, c.n) - 1
        return topk(_scores_with(name, drop=drop), k)
    if defect == "E4":
        return topk(sparse_cosine(c, ascending=True), k)
    if defect == "E5":
        return topk(jaccard(c, self_one=False), k)
    if defect == "E7":
        return topk(sparse_cosine(c, fused=True), k)
    if defect == "E6":
        return merge_select(f64_key(S), k, chunk, skip_single_last=True)
    raise ValueError(defect)
