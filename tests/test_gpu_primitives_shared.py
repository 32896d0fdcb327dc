"""The primitives the kernel files share, each tested by itself through csrc/primitives_debug.hip against the exact
statements of tests/primitives_cases.py: the wave moves and exchanges of wave_ops.h, wave_incl_scan / block_excl_scan /
lower_bound of scan.h, blockscan_kernel, the radix sort pass, the radix select and the lock-free union-find.  Every
comparison is of integers or bit patterns, but wave_allsum against math.fsum.  Output buffers start as -7 and must keep it
wherever the primitive has nothing to write; input padding holds 0x7f7f7f7f.  tests/test_primitives_cases_host.py shows on
the CPU that every case reaches the edge it is named for."""
import ctypes as C
import math

import numpy as np
import pytest

import primitives_cases as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VP, I, L = C.c_void_p, C.c_int, C.c_long
U64 = np.uint64


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _entry(name, argtypes, restype=I):
    from mused_amd import _lib

    fn = getattr(_lib.lib(), name)
    fn.restype, fn.argtypes = restype, argtypes
    return fn


def _call(fn, *args):
    """Tensors go in as they are and stay alive until the launch is enqueued: their memory is not handed out again before."""
    from mused_amd import _lib
    from mused_amd.engine import stream_ptr

    _lib.check(fn(*[p(a) if isinstance(a, torch.Tensor) else a for a in args], stream_ptr()))


def dev(a):
    """A host array on the device; uint64 travels as the int64 of the same bits."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).cuda()


def full(n, dtype=torch.int32, value=pc.SENTINEL):
    return torch.full((n,), value, dtype=dtype, device="cuda")


def host(t, dtype=None):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def p(t):
    from mused_amd.engine import ptr

    return None if t is None else ptr(t)


# ---- wave operations --------------------------------------------------------------------------------------------------------------------
def run_wave_ops(in_bits):
    """-> {op: 256 uint64 bit patterns}, the int32 scan, the uint64 scan."""
    fn = _entry("mused_debug_wave_ops", [VP] * 7)
    iin, uin = pc.wave_scan_input()
    out, iout, uout = full(10 * 256, torch.int64), full(256), full(256, torch.int64)
    _call(fn, dev(in_bits), dev(iin), dev(uin), out, iout, uout)
    rows = host(out, np.uint64).reshape(10, 256)
    return dict(zip(pc.WAVE_OPS, rows)), host(iout), host(uout, np.uint64)


@pytest.fixture(scope="module")
def wave_moves():
    return run_wave_ops(pc.wave_move_input())


@pytest.fixture(scope="module")
def wave_adds():
    return run_wave_ops(pc.wave_add_input().view(np.uint64))


@pytest.mark.parametrize("op", list(pc.MOVE_SOURCE))
def test_wave_move_brings_the_bits_of_its_source_lane(wave_moves, op):
    a = pc.wave_move_input()[:256]
    got = wave_moves[0][op]
    want = pc.ref_move(op, a)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (op, bad[:8], [hex(int(x)) for x in got[bad[:4]]], [hex(int(x)) for x in want[bad[:4]]])


@pytest.mark.parametrize("op,bit", [("swap16_add", 16), ("swap32_add", 32)])
def test_swap_add_keeps_a_below_the_bit_and_b_above(wave_adds, op, bit):
    v = pc.wave_add_input()
    want = pc.ref_swap_add(v[:256], v[256:], bit).view(np.uint64)
    got = wave_adds[0][op]
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (op, bad[:8])


@pytest.fixture(scope="module")
def wave_near():
    return run_wave_ops(pc.wave_near_input().view(np.uint64))


@pytest.mark.parametrize("which", ["wide", "near"])
def test_wave_allsum_is_one_value_per_wave_within_the_pairwise_bound(wave_adds, wave_near, which):
    a = (pc.wave_add_input() if which == "wide" else pc.wave_near_input())[:256]
    got = (wave_adds if which == "wide" else wave_near)[0]["wave_allsum"].reshape(4, 64)
    for w in range(4):
        x = a[64 * w:64 * w + 64]
        assert len(np.unique(got[w])) == 1, (w, "the 64 lanes do not hold the same bits")
        s = float(got[w][:1].view(np.float64)[0])
        exact, mag = math.fsum(x), math.fsum(np.abs(x))
        print(f"wave {w}: allsum {s!r}, fsum {exact!r}, |error| / sum|v| = {abs(s - exact) / mag:.3e}")
        assert abs(s - exact) <= pc.ALLSUM_BOUND * mag


def test_wave_incl_scan_int_and_u64(wave_adds, wave_moves):
    iin, uin = pc.wave_scan_input()
    for _, iout, uout in (wave_adds, wave_moves):                # (the scans do not depend on the fp64 input)
        assert np.array_equal(iout, pc.ref_wave_scan(iin))
        assert np.array_equal(uout, pc.ref_wave_scan(uin))


# ---- block_excl_scan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("threads", pc.SCAN_THREADS)
def test_block_excl_scan_three_calls_back_to_back(threads, dtype):
    fn = _entry("mused_debug_block_scan", [VP, VP, VP, I, I, I, VP])
    T = pc.SCAN_DTYPES[dtype]
    tt = torch.int32 if dtype == 0 else torch.int64
    for which in (0, 1):
        rows = pc.scan_launch(threads, dtype, which)
        n = rows.size
        out, totals = full(n + 64, tt), full(n + 64, tt)
        _call(fn, dev(rows.reshape(-1)), out, totals, threads, dtype, pc.SCAN_CALLS)
        excl, tot = pc.ref_excl_scan(rows)
        o, t = host(out, T), host(totals, T)
        assert np.array_equal(o[:n].reshape(rows.shape), excl), (threads, dtype, which)
        got_tot = t[:n].reshape(rows.shape)
        assert (got_tot == tot[:, None]).all(), (threads, dtype, which, np.argwhere(got_tot != tot[:, None])[:4])
        sentinel = np.int64(pc.SENTINEL).astype(T)
        assert (o[n:] == sentinel).all() and (t[n:] == sentinel).all()


def test_block_scan_entry_refuses_other_workgroup_sizes():
    fn = _entry("mused_debug_block_scan", [VP, VP, VP, I, I, I, VP])
    from mused_amd.engine import stream_ptr

    buf = full(4096)
    for threads, dtype, calls in ((0, 0, 3), (96, 0, 3), (1088, 0, 3), (64, 2, 3), (64, 0, 0), (64, 0, 9)):
        assert fn(p(buf), p(buf), p(buf), threads, dtype, calls, stream_ptr()) != 0


# ---- blockscan_kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", pc.BLOCKSCAN_TOTAL)
@pytest.mark.parametrize("m", pc.BLOCKSCAN_M)
def test_blockscan_kernel_scans_in_place(m, total):
    fn = _entry("mused_debug_blockscan", [VP, I, VP, VP])
    for pattern in pc.BLOCKSCAN_VALUES:
        v = pc.blockscan_values(pattern, m)
        a = full(m + 8)
        a[:m] = dev(v) if m else a[:0]
        sep = full(4)
        tot_ptr = {"null": None, "separate": sep, "alias": VP(a.data_ptr() + 4 * m)}[total]
        _call(fn, a, m, tot_ptr)
        got, s = host(a), host(sep)
        want = np.cumsum(v, dtype=np.int64) - v
        assert np.array_equal(got[:m], want.astype(np.int32)), (m, total, pattern)
        assert got[m] == (int(v.sum()) if total == "alias" else pc.SENTINEL), (m, total, pattern)
        assert (got[m + 1:] == pc.SENTINEL).all()
        assert s[0] == (int(v.sum()) if total == "separate" else pc.SENTINEL) and (s[1:] == pc.SENTINEL).all()


# ---- lower_bound ----------------------------------------------------------------------------------------------------------------------------
def test_lower_bound_on_ranges_duplicates_and_gaps():
    fn = _entry("mused_debug_lower_bound", [VP, VP, VP, VP, I, VP, VP])
    a, lo, hi, v = pc.lower_bound_case()
    nq = len(v)
    out = full(nq + 64)
    _call(fn, dev(a), dev(lo), dev(hi), dev(v), nq, out)
    got = host(out)
    want = pc.ref_lower_bound(a, lo, hi, v)
    bad = np.flatnonzero(got[:nq] != want)
    assert len(bad) == 0, [(int(lo[q]), int(hi[q]), int(v[q]), int(got[q]), int(want[q])) for q in bad[:6]]
    assert (got[nq:] == pc.SENTINEL).all()


# ---- radix sort --------------------------------------------------------------------------------------------------------------------------------
def run_sort(key, n, cap, passes, by_pointer):
    """-> key_out, val_out, gather_out, each `cap` long.  Input entries [n, cap) are poison; by_pointer: the live count is
    read on the device and the value given is a wrong one."""
    fn = _entry("mused_debug_radix_sort", [VP, I, I, VP, I, VP, VP, VP, VP, VP, L, VP])
    ws_bytes = _entry("mused_debug_radix_sort_ws_bytes", [I], L)(cap)
    assert ws_bytes > 0
    kin = np.full(cap, pc.POISON, dtype=np.int32)
    kin[:n] = key
    ws = full(ws_bytes // 4 + 1, value=0)           # zeros: a value the sort lost still indexes gather_src inside it
    count = dev(np.array([n], dtype=np.int32)) if by_pointer else None
    outs = [full(cap) for _ in range(3)]
    _call(fn, dev(kin), cap, cap if by_pointer else n, count, passes, dev(pc.sort_gather_src(n)), outs[0], outs[1],
          outs[2], ws, ws_bytes)
    return [host(o) for o in outs]


@pytest.mark.parametrize("passes", pc.SORT_PASSES)
@pytest.mark.parametrize("pattern", pc.SORT_PATTERNS)
def test_radix_sort_is_the_stable_sort(pattern, passes):
    for n in pc.SORT_N:
        key = pc.sort_keys(pattern, n, passes)
        order = pc.ref_sort(key)
        src = pc.sort_gather_src(n)
        for cap, by_pointer in ((n, False), (n + pc.SORT_CAP_EXTRA, True)):
            key_out, val_out, gather_out = run_sort(key, n, cap, passes, by_pointer)
            where = (pattern, passes, n, cap)
            assert np.array_equal(val_out[:n], order), where
            assert np.array_equal(key_out[:n], key[order]), where
            assert np.array_equal(gather_out[:n], src[order]), where
            for o in (key_out, val_out, gather_out):
                assert (o[n:] == pc.SENTINEL).all(), where


def test_radix_sort_without_a_gather_and_bad_arguments():
    fn = _entry("mused_debug_radix_sort", [VP, I, I, VP, I, VP, VP, VP, VP, VP, L, VP])
    from mused_amd.engine import stream_ptr

    n, passes = 1025, 2
    key = pc.sort_keys("uniform", n, passes)
    ws_bytes = _entry("mused_debug_radix_sort_ws_bytes", [I], L)(n)
    ws = full(ws_bytes // 4 + 1, value=0)
    ko, vo = full(n), full(n)
    _call(fn, dev(key), n, n, None, passes, None, ko, vo, None, ws, ws_bytes)
    order = pc.ref_sort(key)
    assert np.array_equal(host(vo), order) and np.array_equal(host(ko), key[order])
    k = dev(key)
    assert _entry("mused_debug_radix_sort_ws_bytes", [I], L)(0) == -1
    for cap, passes, wsb in ((0, 2, ws_bytes), (n, 0, ws_bytes), (n, 5, ws_bytes), (n, 2, ws_bytes - 1)):
        assert fn(p(k), cap, min(cap, n), None, passes, None, p(ko), p(vo), None, p(ws), wsb, stream_ptr()) != 0


# ---- radix select --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.SELECT_NAMES)
def test_radix_select_threshold(name):
    fn = _entry("mused_debug_radix_select", [VP, I, I, VP, I, VP, VP, VP, VP])
    mode, data, keys = pc.select_case(name)
    m = len(keys)
    kks = pc.select_kks(m)
    asked = np.array(kks + [0, m + 1], dtype=np.int32)                      # the last two: refused on the device, nothing written
    nk = len(asked)
    pad = np.full(64, pc.POISON, dtype=np.int32).view(data.dtype)          # behind the keys: nothing may read it
    thr, need, eqc = full(nk + 2, torch.int64), full(nk + 2), full(nk + 2)
    _call(fn, dev(np.concatenate([data, pad])), m, mode, dev(asked), nk, thr, need, eqc)
    thr, need, eqc = host(thr, np.uint64), host(need), host(eqc)
    for b, kk in enumerate(kks):
        want_thr, want_need, equal = pc.ref_select(keys, kk)
        t = pc.select_trace(keys, kk)
        want_eq = equal if t["end"] == "ranked" else -1
        assert (int(thr[b]), int(need[b]), int(eqc[b])) == (want_thr, want_need, want_eq), (name, kk, t)
    assert (thr[len(kks):] == U64(pc.SENTINEL & pc.M64)).all()
    assert (need[len(kks):] == pc.SENTINEL).all() and (eqc[len(kks):] == pc.SENTINEL).all()


# ---- union-find ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.UF_NAMES)
def test_union_find_components_and_joined_flags(name):
    fn = _entry("mused_debug_unite", [VP, I, VP, VP, I, VP, VP, VP])
    n, a, b = pc.uf_case(name)
    m = len(a)
    parent, roots, joined = full(n + 8), full(n + 8), full(m + 8)
    _call(fn, parent, n, dev(a), dev(b), m, joined, roots)
    parent, roots, joined = host(parent), host(roots), host(joined)
    want = pc.ref_roots(name)
    assert np.array_equal(roots[:n], want)                                   # each row's smallest component member
    assert (parent[:n] <= np.arange(n)).all() and (parent[:n] >= 0).all()
    assert np.array_equal(want[parent[:n]], want)                            # a parent is a member of the row's component
    assert set(np.unique(joined[:m])) <= {0, 1}
    assert joined[:m].sum() == n - len(np.unique(want))                      # one flag per merge, exactly
    assert pc.spanning_forest_defect(n, a, b, joined[:m], want) is None
    assert not joined[:m][a == b].any()
    for o, k in ((parent, n), (roots, n), (joined, m)):
        assert (o[k:] == pc.SENTINEL).all()


def test_unite_entry_needs_an_edge():
    fn = _entry("mused_debug_unite", [VP, I, VP, VP, I, VP, VP, VP])
    from mused_amd.engine import stream_ptr

    buf = full(8)
    assert fn(p(buf), 1, p(buf), p(buf), 0, p(buf), p(buf), stream_ptr()) != 0
    assert fn(p(buf), 0, p(buf), p(buf), 1, p(buf), p(buf), stream_ptr()) != 0
