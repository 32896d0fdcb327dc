"""mused_knn_fused / mused_knn_fused_hop (csrc/knn_fused.hip) through the C ABI against references of their own: the exact
int64 neighbours of integer rows (l2), longdouble cosine scores with an asserted gap, and the classic path bit for bit, at
the caps, schedules and shapes tests/knn_fused_cases.py names (tests/test_knn_fused_cases_host.py asserts on the CPU that
each case reaches its path).  Hop mode is held to its contract on the device: outputs equal to a computation from scratch or
a raised flag, bit 1 when a kept list stops proving its row's k smallest, sticky until n_new = 0."""
import ctypes as C

import numpy as np
import pytest

import knn_fused_cases as kc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t):
    return 0 if t.dtype == torch.float32 else 1


GUARD = 256


def _fused(L, dX, k, metric, cap, d=None, want_idx=True, want_mask=True):
    """dX: (n, ld) device rows of which the first d columns count.  Outputs with one extra pitch word / row preset to -1,
    the workspace between two guard bands of 0xA5 bytes.  Returns (idx, mask, overflow word, guards intact)."""
    n, ld = dX.shape
    d = ld if d is None else d
    nb = L.lib().mused_knn_fused_ws_bytes(n, cap)
    buf = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert (buf.data_ptr() + GUARD) % 256 == 0
    w = kc.words_for(n) + 1
    idx = torch.full((n + 1, k), -1, dtype=torch.int32, device="cuda") if want_idx else None
    mask = torch.full((n, w), -1, dtype=torch.int64, device="cuda") if want_mask else None
    ovf = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    L.call("mused_knn_fused", P(dX), _dt(dX), n, d, ld, k, metric, C.c_void_p(buf.data_ptr() + GUARD), nb, cap, P(idx), P(mask),
           w if want_mask else 0, P(ovf), S())
    torch.cuda.synchronize()
    intact = bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nb:] == 0xA5).all())
    return (idx.cpu().numpy() if want_idx else None, mask.cpu().numpy().view(np.uint64) if want_mask else None,
            int(ovf.item()), intact)


def _classic(L, dX, k, metric, d=None):
    n, ld = dX.shape
    d = ld if d is None else d
    ws = torch.empty(n * n, dtype=torch.float64, device="cuda")
    nr = torch.empty(n, dtype=torch.float64, device="cuda")
    w = kc.words_for(n)
    idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
    mask = torch.empty((n, w), dtype=torch.int64, device="cuda")
    L.call("mused_knn_topk", P(dX), _dt(dX), n, d, ld, k, metric, P(ws), P(nr), P(idx), P(mask), w, S())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), mask.cpu().numpy().view(np.uint64)


def _check_outputs(idx, mask, n, k, ref_idx, ref_mask, what):
    w = kc.words_for(n)
    assert np.array_equal(idx[:n], ref_idx), f"{what}: neighbour lists differ in rows {np.flatnonzero((idx[:n] != ref_idx).any(axis=1))[:8]}"
    assert (idx[n:] == -1).all(), f"{what}: wrote behind out_idx"
    assert np.array_equal(mask[:, :w], ref_mask), f"{what}: masks differ in rows {np.flatnonzero((mask[:, :w] != ref_mask).any(axis=1))[:8]}"
    assert not mask[:, w:].any(), f"{what}: the extra pitch word is not zero"


# ---- tumbling: every case, every variant -----------------------------------------------------------------------------------
@pytest.mark.parametrize("vname", kc.VARIANT_NAMES)
@pytest.mark.parametrize("name", kc.NAMES)
def test_case_against_reference_and_classic(L, name, vname):
    c = kc.case(name)
    metric = kc.variant(vname)[1]
    dX = dev(kc.rows_as(name, vname))
    idx, mask, ovf, intact = _fused(L, dX, c.k, metric, c.cap)
    assert ovf == 0, "a candidate list overflowed"
    assert intact, "bytes outside mused_knn_fused_ws_bytes(n, cap) were written"
    w = kc.words_for(c.n)
    if kc.has_reference(vname):
        ref = kc.reference_lists(name, vname)
        _check_outputs(idx, mask, c.n, c.k, ref, kc.mask_of(ref, c.n, w), "reference")
    i_cl, m_cl = _classic(L, dX, c.k, metric)
    _check_outputs(idx, mask, c.n, c.k, i_cl, m_cl, "classic path")


@pytest.mark.parametrize("dtype,extra,loads", kc.PITCHES)
def test_padded_rows(L, dtype, extra, loads):
    """ld > d with NaN in the padding: nothing of it may reach a product (scalar-load and vector-load variants)."""
    c = kc.case(kc.PADDED)
    X = kc.rows(c.name, "wide")
    d = X.shape[1]
    assert kc.loads_vector(dtype, d + extra) == (loads == "vector")
    Xp = np.full((c.n, d + extra), np.nan, dtype=dtype)
    Xp[:, :d] = X
    dX = dev(Xp)
    idx, mask, ovf, intact = _fused(L, dX, c.k, 0, c.cap, d=d)
    assert ovf == 0 and intact
    ref = kc.reference_lists(c.name, "l2_f64_wide")
    _check_outputs(idx, mask, c.n, c.k, ref, kc.mask_of(ref, c.n, kc.words_for(c.n)), "reference")
    i_cl, m_cl = _classic(L, dX, c.k, 0, d=d)
    _check_outputs(idx, mask, c.n, c.k, i_cl, m_cl, "classic path")


@pytest.mark.parametrize("name", ["sel4_a0", kc.PADDED, "k1_two_tiles"])
def test_null_outputs(L, name):
    """out_mask = NULL with mask_words = 0 (what engine.knn_lists passes) and out_idx = NULL: the other output is the same."""
    c = kc.case(name)
    dX = dev(kc.rows_as(name, "l2_f32_narrow"))
    idx, mask, ovf, _ = _fused(L, dX, c.k, 0, c.cap)
    i_only, none, ovf_i, intact_i = _fused(L, dX, c.k, 0, c.cap, want_mask=False)
    none2, m_only, ovf_m, intact_m = _fused(L, dX, c.k, 0, c.cap, want_idx=False)
    assert ovf == ovf_i == ovf_m == 0 and intact_i and intact_m and none is None and none2 is None
    assert np.array_equal(i_only, idx) and np.array_equal(m_only, mask)
    ref = kc.reference_lists(name, "l2_f32_narrow")
    assert np.array_equal(i_only[:c.n], ref)


def _raw(L, fn, *args):
    rc = getattr(L.lib(), fn)(*args)
    msg = L.lib().mused_last_error()
    return rc, (msg.decode() if msg else "")


@pytest.mark.parametrize("what", ["cap<k", "cap>1024", "k>n", "k=0", "ld<d", "mask_words", "ws_bytes", "metric", "dtype",
                                  "hop:cap<k", "hop:k>n", "hop:mask_words", "hop:ws_bytes", "hop:metric", "hop:dtype",
                                  "hop:position"])
def test_argument_errors_write_nothing(L, what):
    n, d, k, cap, metric, dt = 200, 8, 10, 256, 0, 0
    ld, lo_abs, n_new = d, 0, 0
    w = kc.words_for(n)
    words = w
    nb = L.lib().mused_knn_fused_ws_bytes(n, cap)
    assert nb > 0 and L.lib().mused_knn_fused_ws_bytes(0, cap) == -1 and L.lib().mused_knn_fused_ws_bytes(n, 0) == -1
    bytes_given = nb
    hop = what.startswith("hop:")
    key = what[4:] if hop else what
    if key == "cap<k":
        cap = k - 1
    elif key == "cap>1024":
        cap = 1025
    elif key == "k>n":
        k = n + 1
    elif key == "k=0":
        k = 0
    elif key == "ld<d":
        ld = d - 1
    elif key == "mask_words":
        words = w - 1
    elif key == "ws_bytes":
        bytes_given = nb - 1
    elif key == "metric":
        metric = 2
    elif key == "dtype":
        dt = 2
    elif key == "position":
        lo_abs = kc.POSITION_LIMIT - n
    dX = dev(np.random.default_rng(1).standard_normal((n, d)).astype(np.float32))
    ws = torch.full((nb + 1024,), 0xA5, dtype=torch.uint8, device="cuda")     # (room for the larger cap of "cap>1024": unused)
    idx = torch.full((n, max(k, 1)), -1, dtype=torch.int32, device="cuda")
    mask = torch.full((n, w), -1, dtype=torch.int64, device="cuda")
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    if hop:
        rc, msg = _raw(L, "mused_knn_fused_hop", P(dX), dt, n, d, ld, k, metric, P(ws), bytes_given, cap, lo_abs, n_new,
                       P(idx), P(mask), words, P(flag), S())
    else:
        rc, msg = _raw(L, "mused_knn_fused", P(dX), dt, n, d, ld, k, metric, P(ws), bytes_given, cap, P(idx), P(mask), words,
                       P(flag), S())
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith("mused_"), (rc, msg)
    assert bool((ws == 0xA5).all()) and bool((idx == -1).all()) and bool((mask == -1).all()) and int(flag.item()) == 7
    if hop and key == "position":           # one row earlier is the last valid position
        rc, _ = _raw(L, "mused_knn_fused_hop", P(dX), dt, n, d, ld, k, metric, P(ws), nb, cap, lo_abs - 1, 0, P(idx), P(mask),
                     words, P(flag), S())
        torch.cuda.synchronize()
        assert rc == 0 and int(flag.item()) == 0


# ---- hop mode -----------------------------------------------------------------------------------------------------------------
class Hop:
    """One workspace driven through a sequence of windows of one stream.  call() runs mused_knn_fused_hop for the window
    whose rows are stream rows [row0, row0 + W) at stream position lo_abs (row0 + lo_shift), then mused_knn_fused on the same
    rows, and asserts the contract: the flag is non-zero, or lists and mask equal the from-scratch ones bit for bit; a flag
    raised before stays up through every reuse call; a from-scratch call (n_new = 0 or >= W) clears it and is exact."""

    def __init__(self, L, X, W, k, metric, cap, lo_shift=0):
        self.L, self.dX, self.W, self.k, self.metric, self.cap, self.lo_shift = L, dev(X), W, k, metric, cap, lo_shift
        self.nb = L.lib().mused_knn_fused_ws_bytes(W, cap)
        self.buf = torch.full((self.nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.flag = self.reused = 0
        self.flags, self.exact, self.masks = [], [], []
        self._scratch = {}

    def scratch(self, row0):
        if row0 not in self._scratch:
            idx, mask, ovf, _ = _fused(self.L, self.dX[row0:row0 + self.W], self.k, self.metric, self.cap)
            assert ovf == 0
            self._scratch[row0] = (idx[:self.W], mask[:, :kc.words_for(self.W)])
        return self._scratch[row0]

    def call(self, row0, n_new):
        W, k = self.W, self.k
        rows = self.dX[row0:row0 + W]
        w = kc.words_for(W)
        idx = torch.full((W, k), -1, dtype=torch.int32, device="cuda")
        mask = torch.full((W, w), -1, dtype=torch.int64, device="cuda")
        flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        self.L.call("mused_knn_fused_hop", P(rows), _dt(rows), W, rows.shape[1], rows.shape[1], k, self.metric,
                    C.c_void_p(self.buf.data_ptr() + GUARD), self.nb, self.cap, row0 + self.lo_shift, n_new, P(idx), P(mask), w,
                    P(flag), S())
        torch.cuda.synchronize()
        f = int(flag.item())
        i_ref, m_ref = self.scratch(row0)
        mask = mask.cpu().numpy().view(np.uint64)
        same = np.array_equal(idx.cpu().numpy(), i_ref) and np.array_equal(mask, m_ref)
        where = f"window at row {row0} (n_new = {n_new})"
        assert f in (0, 1, 2, 3), where
        assert f != 0 or same, f"{where}: flag 0 and outputs that differ from a computation from scratch"
        if n_new == 0 or n_new >= W:
            assert f == 0 and same, f"{where}: a computation from scratch must clear the flag and be exact (flag {f})"
        elif self.flag != 0:
            assert f != 0, f"{where}: the flag raised earlier ({self.flag}) came back as 0 without a computation from scratch"
        self.flag = f
        self.reused += 1 if (0 < n_new < W and f == 0) else 0
        self.flags.append(f)
        self.exact.append(same)
        self.masks.append(mask)
        return f

    def guards_intact(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.nb:] == 0xA5).all())


def _run_friendly(L, q, lo_shift=0):
    h = Hop(L, kc.friendly_stream(q.hop), q.W, q.k, q.metric, q.cap, lo_shift)
    for t in range(q.windows):
        h.call(t * q.hop, 0 if t == 0 else q.hop)
    assert h.guards_intact()
    return h


@pytest.mark.parametrize("q", [q for q in kc.FRIENDLY if q.cap == 1024], ids=lambda q: q.name)
def test_hop_friendly_stream_raises_no_flag(L, q):
    """A blob stream at cap = 1024 (what the engine uses): every window reuses and none is flagged, so the contract above is
    not met vacuously."""
    h = _run_friendly(L, q)
    assert h.flags == [0] * q.windows and all(h.exact)


@pytest.mark.parametrize("q", [q for q in kc.FRIENDLY if q.cap == 512], ids=lambda q: q.name)
def test_hop_friendly_stream_small_cap(L, q):
    """cap = 512: a = 1 and kthr = 40 (asserted by the host test).  The flag MAY come up here; contract and stickiness only.
    Observed on the MI355X: in each of the four sequences all 8 calls came back unflagged (flags [0] * 8) and bit-identical
    to a computation from scratch, the 7 reuse calls included."""
    h = _run_friendly(L, q)
    print(f"{q.name}: flags {h.flags}, exact {h.exact}, accepted reuse calls {h.reused}")


@pytest.mark.parametrize("q", [q for q in kc.FRIENDLY if q.cap == 1024 and q.metric == 0], ids=lambda q: q.name)
def test_hop_positions_near_the_limit(L, q):
    """The same windows at stream positions just below 2^30: absolute column ids near the limit, slot_base = lo mod W
    arbitrary.  Masks and flags equal those of the sequence started at 0."""
    lo0 = kc.POSITION_LIMIT - q.W - 8 * q.hop
    a, b = _run_friendly(L, q), _run_friendly(L, q, lo_shift=lo0)
    assert a.flags == b.flags == [0] * q.windows
    assert all(np.array_equal(x, y) for x, y in zip(a.masks, b.masks))


def test_hop_bit_1_comes_up_when_a_kept_list_proves_nothing(L):
    """10 rows of the near block stay, 590 rows 50 * sqrt(10) away enter: a staying row keeps at most 10 columns and admits
    none of the entering ones (its threshold, set by the select between the two phases of its five-tile window, is of order
    10), so its list holds fewer than k candidates.  The device has to say so (bit 1), keep saying so through the next reuse
    call, stop after a computation from scratch, and stay quiet on the reuse call after that."""
    h = Hop(L, kc.shift_stream(), kc.SHIFT_W, kc.SHIFT_K, 0, 1024)
    for lo, n_new in kc.SHIFT_CALLS:
        h.call(lo, n_new)
    assert h.flags[0] == 0 and h.exact[0]
    assert h.flags[kc.SHIFT_FLAGGED_AT] & 2, h.flags
    assert not h.exact[kc.SHIFT_FLAGGED_AT], "the flagged window came out right: the case no longer needs the flag"
    assert h.flags[3] != 0                                  # sticky (also asserted by Hop.call)
    assert h.flags[4] == 0 and h.exact[4]                   # n_new = 0
    assert h.flags[5] == 0 and h.exact[5]                   # reuse on the rebuilt state
    assert h.guards_intact()


def test_hop_lists_grow_over_many_small_hops(L):
    """60 windows of hop 8: the lists of the staying rows are never compacted in between.  Contract on every window; a
    raised flag stays up until this driver asks for a computation from scratch (two calls later)."""
    q = kc.GROWTH
    h = Hop(L, kc.growth_stream(), q.W, q.k, q.metric, q.cap)
    flagged_for = 0
    for t in range(q.windows + 1):
        fresh = t == 0 or flagged_for >= 2
        f = h.call(t * q.hop, 0 if fresh else q.hop)
        flagged_for = flagged_for + 1 if f else 0
    print(f"growth: flags {h.flags}")
    assert h.guards_intact()
    assert h.reused >= 1                                    # some reuse call was accepted: the contract was not met vacuously


@pytest.mark.parametrize("n_new", [0, kc.SHIFT_W, kc.SHIFT_W + 5])
def test_hop_from_scratch_clears_a_raised_flag(L, n_new):
    """n_new = 0 and n_new >= n both compute from scratch: the raised flag is cleared, the state is good for reuse."""
    h = Hop(L, kc.shift_stream(), kc.SHIFT_W, kc.SHIFT_K, 0, 1024)
    for lo, nn in kc.SHIFT_CALLS[:kc.SHIFT_FLAGGED_AT + 1]:
        h.call(lo, nn)
    assert h.flags[-1] & 2
    lo = kc.SHIFT_CALLS[kc.SHIFT_FLAGGED_AT + 1][0]
    assert h.call(lo, n_new) == 0 and h.exact[-1]
    assert h.call(lo + 50, 50) == 0 and h.exact[-1]


def test_hop_single_phase_window_keeps_complete_lists(L):
    """The distribution shift at W = 300 (three tiles: one band launch, then the final select): no threshold is ever lowered,
    so every list holds every window column, nothing has to be flagged and every reuse call is exact."""
    h = Hop(L, kc.single_phase_stream(), kc.SINGLE_W, kc.SHIFT_K, 0, 1024)
    for lo, n_new in kc.SINGLE_CALLS:
        h.call(lo, n_new)
    assert h.flags == [0] * len(kc.SINGLE_CALLS) and all(h.exact) and h.guards_intact()


def test_engine_repeats_a_window_the_device_flags(L):
    """The same stream through WindowEngine.knn_adjacency_hop: the repeat-from-scratch branch runs because the device asked
    for it, and every mask equals a fresh engine's."""
    from mused_amd.engine import WindowEngine

    Xd = dev(kc.shift_stream())
    W, k = kc.SHIFT_W, kc.SHIFT_K
    eng, fresh = WindowEngine(W), WindowEngine(W)
    for lo, _ in kc.SHIFT_CALLS:
        a = eng.knn_adjacency_hop(Xd[lo:lo + W], k, "l2", key="m", lo=lo)
        b = fresh.knn_adjacency(Xd[lo:lo + W], k, "l2")
        assert torch.equal(a.mask, b.mask), f"window at {lo} differs"
    assert eng.hop_recomputes >= 1 and eng.knn_fallbacks == 0 and fresh.knn_fallbacks == 0
    assert eng.hop_windows == len(kc.SHIFT_CALLS)
    eng.close(), fresh.close()
