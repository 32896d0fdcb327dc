"""tests/primitives_cases.py on the CPU: every case reaches the edge it is named for, so tests/test_gpu_primitives_shared.py
tests what it says it tests.  For the radix select that is shown with select_trace, a restatement of the control flow of
csrc/radix_select.h: per case and kk the number of passes, the branch that ends them and the size of the ranked bin; for the
radix sort, the tile and chunk properties; for the rest, the properties of the inputs and of the reference statements (no
GPU)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import primitives_cases as pc

U64 = np.uint64


# ---- wave operations ------------------------------------------------------------------------------------------------------------------
def test_wave_move_input_has_distinct_halves_and_the_specials():
    bits = pc.wave_move_input()
    assert bits.dtype == np.uint64 and bits.shape == (512,)
    a = bits[:256]
    x = a.view(np.float64)
    assert np.signbit(x[5]) and x[5] == 0 and x[73] == np.inf and x[145] == -np.inf
    assert np.isnan(x[225]) and int(a[225]) & ((1 << 51) - 1) != 0                       # a payload
    assert x[40] != 0 and abs(x[40]) < np.finfo(np.float64).tiny                         # a subnormal
    assert np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2
    halves = np.concatenate([a & U64(0xFFFFFFFF), a >> U64(32)])
    forced = [5, 73, 145]                                                                # zero low words: -0.0, +inf, -inf
    assert all(halves[t] == 0 for t in forced) and len({t // 64 for t in forced}) == 3
    assert len(np.unique(np.delete(halves, forced))) == 512 - 3 and 0 not in np.delete(halves, forced)
    for w in range(4):                                                                   # inside a wave: all 128 differ
        assert len(np.unique(np.concatenate([halves[64 * w:64 * w + 64], halves[256 + 64 * w:256 + 64 * w + 64]]))) == 128


def test_wave_move_sources_are_involutions_inside_their_group():
    groups = {"QUAD_XOR1": 4, "QUAD_XOR2": 4, "ROW_HALF_MIRROR": 8, "ROW_MIRROR": 16, "ROW_ROR8": 16, "xchg16": 32, "xchg32": 64}
    assert set(groups) == set(pc.MOVE_SOURCE) and set(pc.WAVE_OPS[:7]) == set(groups)
    a = pc.wave_move_input()[:256]
    seen = set()
    for op, g in groups.items():
        src = np.array([pc.MOVE_SOURCE[op](l) for l in range(64)])
        assert (src != np.arange(64)).all() and np.array_equal(src[src], np.arange(64))   # every lane moves, and back
        assert np.array_equal(src // g, np.arange(64) // g)                              # inside the group of the control
        seen.add(tuple(src))
        r = pc.ref_move(op, a)
        assert np.array_equal(r[64:128], a[64:128][src])                                 # a wave reads its own lanes
    assert len(seen) == 7                                                                # seven different maps


def test_wave_add_input_and_the_swap_statement():
    v = pc.wave_add_input()
    a, b = v[:256], v[256:]
    assert np.isfinite(v).all() and (v > 0).any() and (v < 0).any()
    assert np.abs(v).min() < 1e-250 and np.abs(v).max() > 1e250 and np.abs(v).max() <= 1e300
    for bit in (16, 32):
        r = pc.ref_swap_add(a, b, bit)
        assert np.isfinite(r).all()
        t = np.arange(256)
        clear = (t & bit) == 0
        assert np.array_equal(r[clear], (a + a[t ^ bit])[clear]) and np.array_equal(r[~clear], (b + b[t ^ bit])[~clear])
        assert np.array_equal(r, r[t ^ bit]) is False                                   # the two partners hold different sums
        # the statement tells a from b, the partner l ^ bit from l ^ (48 - bit), and a sum from a move
        assert not np.array_equal(r, pc.ref_swap_add(b, a, bit)) and not np.array_equal(r, pc.ref_swap_add(a, b, 48 - bit))
        # (a huge value absorbs a tiny partner; where both are of order one the sum is neither operand)
        assert ((r != a) & (r != b) & (r != a[t ^ bit]) & (r != b[t ^ bit])).sum() >= 32
    for w in range(4):
        x = a[64 * w:64 * w + 64]
        assert math.isfinite(math.fsum(x)) and math.isfinite(float(np.abs(x).sum()))


def test_wave_near_input_makes_every_level_of_the_sum_round():
    v = pc.wave_near_input()
    assert ((np.abs(v) >= 1) & (np.abs(v) < 2)).all() and (v > 0).sum() > 200 and (v < 0).sum() > 200
    a = v[:256]
    inexact = [Fraction(float(x)) + Fraction(float(y)) != Fraction(float(x + y)) for x, y in zip(a[0::2], a[1::2])]
    # two of equal sign round when their last bits differ, one pair in four: already the first level of the sum rounds
    assert len(inexact) == 128 and sum(inexact) >= 16


def test_wave_scan_input_carries_out_of_bit_31():
    i, u = pc.wave_scan_input()
    assert i.dtype == np.int32 and u.dtype == np.uint64 and (i < 0).any() and (i > 0).any()
    ref = pc.ref_wave_scan(u).reshape(4, 64)
    low = np.cumsum((u & U64(0xFFFFFFFF)).reshape(4, 64).astype(object), axis=1)
    assert all(int(low[w, -1]) >> 32 >= 8 for w in range(4))                            # many carries in every wave
    assert all(int(ref[w, -1]) == sum(int(x) for x in u[64 * w:64 * w + 64]) for w in range(4))
    assert np.array_equal(pc.ref_wave_scan(i).reshape(4, 64)[:, -1], i.reshape(4, 64).sum(axis=1))
    assert pc.ref_wave_scan(i)[64] == i[64]                                              # a wave starts anew


# ---- block_excl_scan, blockscan_kernel, lower_bound -----------------------------------------------------------------------------------------
def test_block_scan_launches_cover_sizes_patterns_and_types():
    assert pc.SCAN_THREADS == tuple(64 * k for k in range(1, 17)) and pc.SCAN_CALLS == 3
    assert {p for l in pc.SCAN_LAUNCHES[0] for p in l} >= {"zeros", "ones", "last_one", "first_one", "random"}
    assert {p for l in pc.SCAN_LAUNCHES[1] for p in l} >= {"zeros", "ones", "last_one", "first_one", "random", "packed"}
    for dtype, T in pc.SCAN_DTYPES.items():
        for threads in pc.SCAN_THREADS:
            for which in (0, 1):
                rows = pc.scan_launch(threads, dtype, which)
                assert rows.shape == (3, threads) and rows.dtype == T
                excl, tot = pc.ref_excl_scan(rows)
                assert (excl[:, 0] == 0).all()
                # a total taken from the call before or behind would be wrong: neighbours differ
                assert tot[0] != tot[1] and tot[1] != tot[2]
                for c in range(3):
                    assert int(tot[c]) == sum(int(x) for x in rows[c]) % (1 << (32 if dtype == 0 else 64))
            v = pc.scan_values("last_one", threads, dtype)
            assert v[-1] == 1 and v.sum() == 1 and pc.scan_values("first_one", threads, dtype)[0] == 1
            r = pc.scan_values("random", threads, dtype)
            assert r.min() >= 0 and r.max() < 1000 and not np.array_equal(r, pc.scan_values("random_b", threads, dtype))
    for threads in pc.SCAN_THREADS:                                                      # tfidf's packing: high halves past 2^32
        p = pc.scan_values("packed", threads, 1)
        assert ((p & U64(0xFFFFFFFF)) <= 1).all() and len(np.unique(p & U64(1))) == 2
        assert sum(int(x) >> 32 for x in p) >= 1 << 32             # so the total wraps modulo 2^64, here as on the device


def test_blockscan_sizes_sit_on_the_chunk_edges():
    assert pc.BLOCKSCAN_M == (0, 1, 1023, 1024, 1025, 2048, 2049, 5000)
    chunks = [-(-m // 1024) for m in pc.BLOCKSCAN_M]
    assert chunks == [0, 1, 1, 1, 2, 2, 3, 5]
    assert pc.BLOCKSCAN_TOTAL == ("null", "separate", "alias") and pc.BLOCKSCAN_VALUES == ("zeros", "ones", "random")
    for m in pc.BLOCKSCAN_M:
        r = pc.blockscan_values("random", m)
        assert r.dtype == np.int32 and len(r) == m and (m < 2 or 0 <= r.min() <= r.max() < 1000)
        assert pc.blockscan_values("ones", m).sum() == m and not pc.blockscan_values("zeros", m).any()


def test_lower_bound_queries_reach_every_listed_kind():
    a, lo, hi, v = pc.lower_bound_case()
    assert len(a) == 1000 and (np.diff(a) >= 0).all()
    vals, counts = np.unique(a, return_counts=True)
    assert (counts > 1).sum() >= 50 and (np.diff(vals) > 1).sum() >= 50                  # runs of duplicates, and gaps
    full = (lo == 0) & (hi == 1000)
    assert (v[full] < a[0]).any() and (v[full] > a[-1]).any()
    assert set(vals[counts > 1]) <= set(v[full])                                         # every duplicated value
    assert (~np.isin(v[full], a) & (v[full] > a[0]) & (v[full] < a[-1])).sum() >= 50     # values in gaps
    assert ((lo > 0) & (hi == 1000)).any() and ((lo == 0) & (hi < 1000) & (hi > 0)).any() and ((lo > 0) & (hi < 1000) & (lo < hi)).any()
    assert {0, 500, 1000} <= set(lo[lo == hi])                                           # empty ranges
    assert (lo <= hi).all() and lo.min() >= 0 and hi.max() <= 1000
    ref = pc.ref_lower_bound(a, lo, hi, v)
    assert ((ref >= lo) & (ref <= hi)).all() and (ref[lo == hi] == lo[lo == hi]).all()
    sub = ~full & (lo < hi)
    assert (ref[sub] == lo[sub]).any() and (ref[sub] == hi[sub]).any() and ((ref[sub] > lo[sub]) & (ref[sub] < hi[sub])).any()
    # a search that ignored lo or hi would answer differently
    whole = pc.ref_lower_bound(a, np.zeros_like(lo), np.full_like(hi, 1000), v)
    assert (whole[sub] < lo[sub]).any() and (whole[sub] > hi[sub]).any()
    for p, (l, h, x) in zip(ref, zip(lo, hi, v)):                                        # the definition itself
        assert (a[l:p] < x).all() and (a[p:h] >= x).all()


# ---- radix sort -------------------------------------------------------------------------------------------------------------------------------
def _digits(key, p):
    return (key.astype(np.int64) >> (8 * p)) & 255


def test_sort_sizes_give_the_tiles_and_chunks_they_are_there_for():
    assert pc.SORT_N == (1, 63, 64, 65, 1023, 1024, 1025, 4097) and pc.SORT_PASSES == (1, 2, 4)
    tiles = {n: -(-n // pc.RADIX_TILE) for n in pc.SORT_N}
    assert [tiles[n] for n in pc.SORT_N] == [1, 1, 1, 1, 1, 1, 2, 5]
    assert 256 * tiles[4097] == 1280 > 1024                      # the histogram table crosses a chunk of blockscan_kernel
    capped = {n: -(-(n + pc.SORT_CAP_EXTRA) // pc.RADIX_TILE) for n in pc.SORT_N}
    assert all(capped[n] > tiles[n] for n in pc.SORT_N)          # cap > n: at least one tile with no live entry ...
    assert all((n + pc.SORT_CAP_EXTRA) // pc.RADIX_TILE * pc.RADIX_TILE >= n for n in pc.SORT_N[:-1])
    assert {n % 64 for n in pc.SORT_N} == {0, 1, 63}             # ... and last chunks that are full, one entry, one short


@pytest.mark.parametrize("passes", pc.SORT_PASSES)
@pytest.mark.parametrize("pattern", pc.SORT_PATTERNS)
def test_sort_pattern_is_what_its_name_says(pattern, passes):
    top = pc.sort_top(passes)
    assert top == (255, 65535, None, 2 ** 31 - 1)[passes - 1]
    for n in pc.SORT_N:
        key = pc.sort_keys(pattern, n, passes)
        assert key.dtype == np.int32 and len(key) == n and key.min() >= 0 and key.max() <= top
        order = pc.ref_sort(key)
        assert np.array_equal(np.sort(order), np.arange(n)) and (np.diff(key[order].astype(np.int64)) >= 0).all()
        same = np.diff(key[order]) == 0
        assert (np.diff(order)[same] > 0).all()                  # stable: equal keys in input order
        low = _digits(key, 0)
        chunks = [low[c:c + 64] for c in range(0, n, 64)]
        if pattern == "all_equal":
            assert len(np.unique(key)) == 1 and np.array_equal(order, np.arange(n))
        elif pattern == "two_values":
            assert set(key) <= {0, top} and (n < 63 or set(key) == {0, top})
        elif pattern == "descending":
            assert (np.diff(key.astype(np.int64)) <= 0).all() and key[0] == (top if n > 1 else 0) and key[-1] == 0
            assert n == 1 or order[0] > order[-1]
        elif pattern == "three_values":
            assert len(np.unique(key)) <= 3 and (n < 63 or len(np.unique(key)) == 3)
        elif pattern == "chunk_one_digit":                       # a whole chunk of 64 lanes one digit, another per chunk
            assert all(len(np.unique(ch)) == 1 for ch in chunks)
            assert len({int(ch[0]) for ch in chunks}) == len(chunks)
            for p in range(passes):                              # and a constant digit per chunk at every pass's byte
                assert all(len(np.unique(_digits(key[c:c + 64], p))) == 1 for c in range(0, n, 64))
        elif pattern == "digit_once_per_chunk":
            assert all((ch == pc.ONCE_DIGIT).sum() == 1 for ch in chunks)
            lanes = {int(np.flatnonzero(ch == pc.ONCE_DIGIT)[0]) for ch in chunks}
            assert len(chunks) < 3 or len(lanes) >= 3            # the lane that holds it moves from chunk to chunk
        elif pattern == "uniform":
            assert n < 1023 or all(len(np.unique(_digits(key, p))) > 100 for p in range(passes - (passes == 4)))
        elif pattern == "low_byte_constant":                     # the first pass moves nothing
            assert (low == pc.CONSTANT_BYTE).all()
            assert np.array_equal(np.argsort(low, kind="stable"), np.arange(n))
        if n >= 1023 and (passes == 1 or pattern in ("two_values", "three_values", "chunk_one_digit")):
            assert same.any()                                    # duplicates: stability is tested, not assumed
        print(f"{pattern} passes={passes} n={n}: tiles={-(-n // 1024)} chunks={len(chunks)} distinct keys={len(np.unique(key))} "
              f"distinct low digits={len(np.unique(low))}")


def test_sort_gather_source_tells_positions_apart():
    for n in pc.SORT_N:
        g = pc.sort_gather_src(n)
        assert g.dtype == np.int32 and len(np.unique(g)) == n and pc.SENTINEL not in g and pc.POISON not in g


# ---- radix select -------------------------------------------------------------------------------------------------------------------------------
# per case: {kk or "all": (passes, end, ranked_bin)}; "half" is kk = m // 2, the kk the planted bins are built around
SELECT_CLAIMS = {
    "m1": {"all": (0, "all_equal", 0)},
    "all_equal": {"all": (0, "all_equal", 0)},
    "bit63_small": {"all": (1, "ranked", None)},
    "bit63_big": {"all": (8, "out_of_bits", 0)},
    "bit0": {"all": (1, "out_of_bits", 0)},
    "share_top56": {"all": (1, "out_of_bits", 0)},
    "bin_256": {"half": (1, "ranked", 256)},
    "bin_257": {"half": (2, "ranked", None)},
    "copies_300": {"half": (8, "out_of_bits", 0)},
    "copies_256": {"half": (2, "ranked", 256)},      # 40 other keys share its first digit, none its second
    "five_values_big": {"all": (8, "out_of_bits", 0)},
}


@pytest.mark.parametrize("name", pc.SELECT_NAMES)
def test_select_case_takes_the_branch_it_is_named_for(name):
    mode, data, keys = pc.select_case(name)
    m = len(keys)
    kks = pc.select_kks(m)
    assert kks and all(1 <= kk <= m for kk in kks) and {1, m} <= set(kks) and (m < 4 or {2, m // 2, m - 1} <= set(kks))
    traces = {kk: pc.select_trace(keys, kk) for kk in kks}
    for kk, t in traces.items():
        thr, need_eq, equal = pc.ref_select(keys, kk)
        # the restatement finds what the sort finds
        assert (t["thr"], t["need_eq"]) == (thr, need_eq), kk
        assert t["eq_count"] == (equal if t["end"] == "ranked" else -1), kk
        assert 1 <= need_eq <= equal and (t["end"] != "ranked" or 1 <= t["ranked_bin"] <= 256)
        print(f"{name} m={m} kk={kk}: top={t['top']} passes={t['passes']} end={t['end']} ranked_bin={t['ranked_bin']} "
              f"need_eq={need_eq} equal={equal} eq_count={t['eq_count']}")
    for which, (passes, end, ranked_bin) in SELECT_CLAIMS.get(name, {}).items():
        for kk in (kks if which == "all" else [m // 2]):
            t = traces[kk]
            assert (t["passes"], t["end"]) == (passes, end), (kk, t)
            assert ranked_bin is None or t["ranked_bin"] == ranked_bin, (kk, t)
    half = traces[m // 2] if m >= 2 else None
    if name.startswith("uniform"):
        assert m == int(name.split("_")[1]) and all(t["end"] == "ranked" for t in traces.values())
        assert all(t["top"] >= 62 for t in traces.values())
        if m == 5000:
            assert any(t["passes"] == 1 for t in traces.values())         # 5000 / 256 per bin: ranked after the first digit
    if name in ("bit63_small", "bit63_big"):
        assert all(t["top"] == 64 for t in traces.values())               # maskbits = 0
        assert len(np.unique(keys)) == 2 and int(keys.max() ^ keys.min()) == 1 << 63
    if name == "bit63_big":
        assert all((keys == U64(t["thr"])).sum() == 300 for t in traces.values())
    if name == "bit0":
        assert all(t["top"] == 1 for t in traces.values()) and int(keys.max() ^ keys.min()) == 1
    if name == "share_top56":
        assert all(t["top"] == 8 for t in traces.values()) and m <= 256   # lo == 0: a bin of <= 256 keys, still not ranked
        assert len(np.unique(keys >> U64(8))) == 1
    if name in ("bin_256", "bin_257"):
        size = int(name[-3:])
        assert ((keys >> U64(56)) == U64(0x40)).sum() == size and half["top"] == 64
        if size == 257:
            assert 1 <= half["ranked_bin"] < 257
    if name in ("copies_300", "copies_256"):
        copies = int(name[-3:])
        thr, need_eq, equal = pc.ref_select(keys, m // 2)
        assert equal == copies and 1 < need_eq < copies                   # kk cuts the tie
        assert len(np.unique(keys)) == m - copies + 1
        assert half["eq_count"] == (256 if copies == 256 else -1)
    if name.startswith("five_values"):
        vals, counts = np.unique(keys, return_counts=True)
        assert len(vals) == 5
        if name.endswith("small"):
            assert counts.max() <= 256 and all(t["end"] == "ranked" and t["eq_count"] > 1 for t in traces.values())
        else:
            assert counts.min() > 256
    if name == "f64_scores":
        assert mode == 1 and data.dtype == np.float64 and not np.isnan(data).any()
        x = data
        assert ((x == 0) & np.signbit(x)).sum() > 20 and ((x == 0) & ~np.signbit(x)).sum() > 20
        assert np.isinf(x).sum() > 40 and (x == np.inf).any() and (x == -np.inf).any() and (x < 0).sum() > 200
        tiny = np.finfo(np.float64).tiny
        assert ((x != 0) & (np.abs(x) < tiny) & (x > 0)).any() and ((x != 0) & (np.abs(x) < tiny) & (x < 0)).any()
        assert np.unique(x, return_counts=True)[1].max() > 40             # equal scores at many positions
        # the order of the keys is the order of the doubles with -0.0 < +0.0, and kk = m // 2 lands between the zeros
        order = np.lexsort((np.arange(m), ~np.signbit(x), x))
        assert np.array_equal(order, np.lexsort((np.arange(m), keys)))
        thr = pc.ref_select(keys, m // 2)[0]
        assert thr in (1 << 63, (1 << 63) - 1)                             # +0.0 or -0.0
        assert all(t["top"] == 64 for t in traces.values())
    else:
        assert mode == 0 and data.dtype == np.uint64


def test_select_cases_cover_every_branch_of_the_issue():
    ends, passes, bins = set(), set(), set()
    for name in pc.SELECT_NAMES:
        keys = pc.select_case(name)[2]
        for kk in pc.select_kks(len(keys)):
            t = pc.select_trace(keys, kk)
            ends.add(t["end"])
            passes.add(t["passes"])
            bins.add(t["ranked_bin"])
    assert ends == {"all_equal", "ranked", "out_of_bits"} and {0, 1, 2, 8} <= passes and {1, 256} <= bins and max(bins) == 256
    assert {len(pc.select_case(f"uniform_{m}")[2]) for m in (2, 1023, 1024, 1025, 5000)} == {2, 1023, 1024, 1025, 5000}


def test_f64_key_orders_the_doubles():
    x = np.array([-np.inf, -1e300, -1.0, -2.0 ** -1060, -5e-324, -0.0, 0.0, 5e-324, 2.0 ** -1060, 1.0, 1e300, np.inf])
    key = pc.f64_key(x)
    assert (np.diff(key.astype(object)) > 0).all() and int(key[6]) == 1 << 63 and int(key[5]) == (1 << 63) - 1


def test_select_trace_on_hand_made_keys():
    # two keys that differ in bit 9: top = 10, one pass over bits [2, 10), lo = 2 > 0: ranked
    t = pc.select_trace(np.array([0x200, 0x000], dtype=np.uint64), 2)
    assert (t["top"], t["passes"], t["end"], t["ranked_bin"], t["thr"], t["need_eq"], t["eq_count"]) == (10, 1, "ranked", 1, 0x200, 1, 1)
    # 300 + 300 keys that differ in bit 20: [12, 20) keeps 300, [4, 12) keeps 300, [0, 4) runs out of bits
    k = np.array([0] * 300 + [1 << 19] * 300, dtype=np.uint64)
    t = pc.select_trace(k, 450)
    assert (t["top"], t["passes"], t["end"], t["thr"], t["need_eq"], t["eq_count"]) == (20, 3, "out_of_bits", 1 << 19, 150, -1)


# ---- union-find -----------------------------------------------------------------------------------------------------------------------------------
UF_SHAPE = {  # name: (n, m, components)
    "single_self_loop": (1, 1, 1), "self_loops": (100, 500, 100), "same_pair": (50, 10000, 49), "path": (4096, 4095, 1),
    "star_last": (4096, 4095, 1), "star_first": (4096, 4095, 1), "two_trees": (4096, 50000, None),
    "random_graph": (4096, 100000, 1), "random_forest": (20000, 15000, 5000),
}


@pytest.mark.parametrize("name", pc.UF_NAMES)
def test_union_find_case_is_what_its_name_says(name):
    n, a, b = pc.uf_case(name)
    roots = pc.ref_roots(name)
    want_n, want_m, want_comps = UF_SHAPE[name]
    comps = len(np.unique(roots))
    assert (n, len(a), len(b)) == (want_n, want_m, want_m) and a.dtype == b.dtype == np.int32
    assert a.min() >= 0 and b.min() >= 0 and a.max() < n and b.max() < n
    assert want_comps is None or comps == want_comps
    assert (roots <= np.arange(n)).all() and np.array_equal(roots[roots], roots)         # the smallest member, a root
    for r in np.unique(roots)[:50]:
        assert np.flatnonzero(roots == r).min() == r
    if name in ("single_self_loop", "self_loops"):
        assert np.array_equal(a, b)
    if name == "same_pair":
        assert {(int(x), int(y)) for x, y in zip(a, b)} == {(7, 31), (31, 7)} and roots[31] == 7
    if name == "path":
        assert (np.abs(a - b) == 1).all() and len({(min(x, y)) for x, y in zip(a.tolist(), b.tolist())}) == 4095
        assert not np.array_equal(np.minimum(a, b), np.arange(4095))                     # in random order
    if name == "star_last":
        assert (np.maximum(a, b) == 4095).all() and len(np.unique(np.minimum(a, b))) == 4095
    if name == "star_first":
        assert (np.minimum(a, b) == 0).all() and len(np.unique(np.maximum(a, b))) == 4095
    if name == "two_trees":
        hub = (a <= 1)
        assert hub.mean() > 0.98 and (a[hub] % 2 == b[hub] % 2).all() and (a[hub] == 0).sum() > 20000 and (a[hub] == 1).sum() > 20000
        link = a % 2 != b % 2
        assert 100 < link.sum() < 1500 and roots[0] == 0 and roots[1] == 0
        assert (roots[np.unique(b)] == 0).all()
    if name == "random_forest":
        uf = pc.HostUnionFind(n)
        assert all(uf.unite(x, y) for x, y in zip(a.tolist(), b.tolist()))               # no edge closes a cycle
    print(f"{name}: n={n} m={len(a)} components={comps}")


def test_spanning_forest_check_catches_what_it_must():
    n, a, b = pc.uf_case("random_graph")
    roots = pc.ref_roots("random_graph")
    uf = pc.HostUnionFind(n)
    joined = np.array([uf.unite(x, y) for x, y in zip(a.tolist(), b.tolist())])
    assert joined.sum() == n - 1 and pc.spanning_forest_defect(n, a, b, joined, roots) is None
    twice = joined.copy()
    twice[np.flatnonzero(~joined)[0]] = True                                             # one merge reported twice
    assert "joined flags" in pc.spanning_forest_defect(n, a, b, twice, roots)
    moved = joined.copy()
    moved[np.flatnonzero(joined)[-1]] = False
    moved[np.flatnonzero(~joined & (a != b))[0]] = True                                  # the right count, the wrong edges
    assert pc.spanning_forest_defect(n, a, b, moved, roots) is not None
