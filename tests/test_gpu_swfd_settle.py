"""On the GPU: the settle kernel of the sliding-window sketch (csrc/swfd.hip, swfd_settle_kernel) -- the rotation's
scatter and the append of the call's next block in one launch, with a zero range that ends at the rows in use -- against
the kernel pair it replaces.  Every comparison is bit for bit: get() by the rule of test_gpu_swfd_edges.py::_same_get,
both exported halves byte for byte.  Three ways to feed the same rows: one call per checkpoint (every interior block of
the call is settled by the rotation before it), one call per block (no call spans a rotation: nothing is fused), and
MUSED_SWFD_SETTLE=0 (the scatter + append pair).  Cases and the blob parser: tests/swfd_cases.py."""
import numpy as np
import pytest

import swfd_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SWITCHES = ("MUSED_SWFD_DEDUPE", "MUSED_SWFD_LIST", "MUSED_SWFD_ORDERS", "MUSED_SWFD_KACT", "MUSED_SWFD_SKIP_DEAD",
            "MUSED_SWFD_GRAM_SPLIT", "MUSED_SWFD_PREROT", "MUSED_SWFD_PREROT_SWEEPS", "MUSED_EIG_TRD", "MUSED_SWFD_SETTLE")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(monkeypatch, N, R, d, l, settle=True, **kw):
    """A handle created under a clean environment (the switches are read at creation), MUSED_SWFD_SETTLE=0 if asked."""
    from mused_amd.swfd import SeqBasedSWFD

    with monkeypatch.context() as m:
        for name in SWITCHES:
            m.delenv(name, raising=False)
        if not settle:
            m.setenv("MUSED_SWFD_SETTLE", "0")
        return SeqBasedSWFD(N=N, R=R, d=d, sketch_dim=l, **kw)


def _case_dev(monkeypatch, name, settle=True):
    c = sc.CASES[name]
    return _dev(monkeypatch, c.N, sc.case_stream(name)[1], c.d, c.l, settle=settle)


def _raw(sk, kind):
    return sk.export_half(kind).cpu().numpy()


def _record(sk):
    return sk.get(), _raw(sk, 0), _raw(sk, 1)


def _same_get(a, b):
    return sc.same_bits(a[0], b[0]) and sc.same_bits(a[1], b[1]) and a[2] == b[2] and sc.same_bits(a[3], b[3])


def _same_record(a, b):
    return _same_get(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _rotation_cuts(N, l, n, extra=()):
    """Every row count in (0, n] at which a rotation runs (multiples of l inside an epoch, epoch ends), and `extra`."""
    cuts = {i for i in range(1, n + 1) if i % N == 0 or (i % N) % l == 0}
    return sorted(cuts | {e for e in extra if 0 < e <= n} | {n})


def _feed_per_block(sk, Xd, a, b, N, l):
    """Rows a .. b in calls that end at every rotation: each call's rows are the first block of a call."""
    t = a
    for e in _rotation_cuts(N, l, b):
        if e <= a:
            continue
        sk.fit(Xd[t:e])
        t = e
    assert t == b


def _pending(i, N, l):
    return 0 if i % N == 0 else (i % N) % l


def _checkpoints(c, n):
    return sorted({c.N, 2 * c.N, 3 * c.N, 4 * c.N, c.N + c.l + 2, n})


# ---- the cases have what they are here for -----------------------------------------------------------------------------
def _trace_properties(name):
    """From the specification's trace: states with frozen MAIN levels, AUX levels whose kept-row count fell inside an
    epoch (and the largest fall), pairs of neighbouring AUX levels with bit-identical kept rows."""
    _, trace = sc.oracle_trace(name)
    frozen = sum(1 for s in trace if s["frozen"])
    drops, deepest, twins = 0, 0, 0
    for prev, cur in zip(trace[:-1], trace[1:]):
        for j, (a, b) in enumerate(zip(prev["halves"][1], cur["halves"][1])):
            if prev["epoch_start"] == cur["epoch_start"] and len(b["K"]) < len(a["K"]):
                drops += 1
                deepest = max(deepest, len(a["K"]) - len(b["K"]))
    for s in trace:
        aux = s["halves"][1]
        twins += sum(1 for a, b in zip(aux[:-1], aux[1:]) if len(a["K"]) and sc.same_bits(a["K"], b["K"]))
    return frozen, drops, deepest, twins


@pytest.mark.parametrize("name", ["l4", "l6_ragged_epoch", "l8_d5"])
def test_cases_freeze_levels_drop_kept_rows_and_hold_duplicates(name):
    frozen, drops, deepest, twins = _trace_properties(name)
    print(f"{name}: states with frozen levels {frozen}, kept-count falls {drops} (up to {deepest}), duplicate pairs {twins}")
    assert frozen > 0 and drops > 0 and deepest >= 2 and twins > 0


def test_case_N5_l8_never_fuses():
    """N < l: every block ends an epoch, so the next row always starts one and no rotation takes rows ahead."""
    c = sc.CASES["N5_l8"]
    assert c.N < c.l
    _, trace = sc.oracle_trace("N5_l8")
    assert not any(s["frozen"] for s in trace)


# ---- a. fused == unfused == the kernel pair ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l4", "l6_ragged_epoch", "l8_d5", "l3_odd", "l2_d1", "N5_l8"])
def test_fused_equals_unfused_equals_the_pair(name, monkeypatch):
    """At every epoch end, at N + l + 2 rows (the call ends inside a block the rotation has placed, the next call goes on
    behind it) and at the end of the stream: get() and both halves agree in every byte."""
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    n = len(X)
    Xd = _cuda(X)
    fused, blockwise, pair = _case_dev(monkeypatch, name), _case_dev(monkeypatch, name), _case_dev(monkeypatch, name, settle=False)
    t = 0
    for cp in _checkpoints(c, n):
        fused.fit(Xd[t:cp])
        pair.fit(Xd[t:cp])
        _feed_per_block(blockwise, Xd, t, cp, c.N, c.l)
        t = cp
        assert fused.rows_seen == blockwise.rows_seen == pair.rows_seen == cp
        ref = _record(blockwise)
        assert _same_record(_record(fused), ref), (name, cp, "one call per checkpoint")
        assert _same_record(_record(pair), ref), (name, cp, "MUSED_SWFD_SETTLE=0")
    assert ref[0][1][0] > 0.0 or c.l == 1
    for sk in (fused, blockwise, pair):
        sk.close()


# ---- b. row sources and alignment --------------------------------------------------------------------------------------------
def _binary_stream(n, d, seed):
    return (np.random.default_rng(seed).random((n, d)) < 0.1).astype(np.float64)


def _strided(Z, dtype, fill, pitch, offset, lanes_stride=None):
    """Z (n, d) or (B, n, d) as a view of a flat tensor filled with `fill`: first element `offset` elements into the
    allocation, row pitch `pitch`, lanes `lanes_stride` apart."""
    if Z.ndim == 2:
        n, d = Z.shape
        flat = torch.full((offset + n * pitch + 8,), fill, dtype=dtype, device="cuda")
        view = flat.as_strided((n, d), (pitch, 1), offset)
    else:
        B, n, d = Z.shape
        flat = torch.full((offset + B * lanes_stride + 8,), fill, dtype=dtype, device="cuda")
        view = flat.as_strided((B, n, d), (lanes_stride, pitch, 1), offset)
    view.copy_(torch.from_numpy(Z).to(dtype).cuda())
    return view


def _pack_bits(Z, pitch):
    """0/1 rows as bitmask rows of `pitch` 64-bit words, every bit behind column d and every padding word SET."""
    n, d = Z.shape
    full = np.ones((n, pitch * 64), dtype=np.uint8)
    full[:, :d] = Z
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.int64)


def _append_raw(sk, t, dtype, n_rows, ld, lane_stride=None):
    from mused_amd._lib import call
    from mused_amd.engine import ptr, stream_ptr

    if lane_stride is None:
        call("mused_swfd_append", sk._h, ptr(t), dtype, n_rows, ld, stream_ptr())
    else:
        call("mused_swfd_append_lanes", sk._h, ptr(t), dtype, n_rows, ld, lane_stride, stream_ptr())
    keep = getattr(sk, "_held", [])
    keep.append(t)
    sk._held = keep


@pytest.mark.parametrize("d", [1, 5, 63, 64, 65, 130])
def test_row_sources_and_alignments_give_the_same_bits(d, monkeypatch):
    """One 0/1 stream (exact in every type) from F64 / F32 / I64 / bit rows, each from views of NaN- or junk-filled
    allocations: 16-byte aligned with an even pitch (the 16-byte path when d is even), first element one element in (8 but
    not 16 bytes aligned for the 8-byte types), an odd pitch (every other row off), bit rows one word in with two junk words
    per row; three lanes whose stride is no multiple of the pitch.  Fed in calls that span rotations and end inside a block:
    every one equals contiguous F64 rows fed block by block, in get() and in both halves."""
    from mused_amd._lib import BITS, F32, F64, I64

    l, B = 4, 3
    N = max(d, 3 * l + 1)
    n = 2 * N + 7
    cuts = [0, N + l + 2, n]                    # ends two rows into a block that the rotation has placed
    Z = np.stack([_binary_stream(n, d, 1000 * d + b) for b in range(B)])
    R = max(float(Z.sum(2).max()), 1.0)
    w = (d + 63) // 64
    even, odd = d + 2 + (d & 1), d + 3 - (d & 1)
    assert even % 2 == 0 and odd % 2 == 1
    i64min = torch.iinfo(torch.int64).min

    # the reference: contiguous F64 rows, a call per block
    refs, singles = [], []
    for b in range(B):
        sk, Zd, out = _dev(monkeypatch, N, R, d, l), _cuda(Z[b]), []
        for a, e in zip(cuts[:-1], cuts[1:]):
            _feed_per_block(sk, Zd, a, e, N, l)
            out.append(_record(sk))
        refs.append(out)
        singles.append(sk)
    assert refs[0][-1][0][1][0] > 0.0

    sources = []
    for tag, dtype, code, fill in (("f64", torch.float64, F64, float("nan")), ("f32", torch.float32, F32, float("nan")),
                                   ("i64", torch.int64, I64, i64min)):
        for how, pitch, offset in (("even pitch", even, 0), ("one element in", even, 1), ("odd pitch", odd, 0)):
            if tag != "f64" and how == "even pitch" and d not in (64, 130):
                continue                          # (the aligned view of the other types: at the even d only)
            sources.append((f"{tag} {how}", _strided(Z[0], dtype, fill, pitch, offset), code, pitch))
    bits_in = torch.full((1 + n * (w + 2) + 8,), -1, dtype=torch.int64, device="cuda")
    bits_view = bits_in.as_strided((n, w + 2), (w + 2, 1), 1)
    bits_view.copy_(_cuda(_pack_bits(Z[0], w + 2)))
    sources.append(("bits one word in, junk behind d", bits_view, BITS, w + 2))
    sources.append(("bits tight pitch", _cuda(_pack_bits(Z[0], w)), BITS, w))
    for tag, view, code, pitch in sources:
        assert view.stride(0) == pitch
        sk = _dev(monkeypatch, N, R, d, l)
        for k, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
            _append_raw(sk, view[a:e], code, e - a, pitch)
            assert _same_record(_record(sk), refs[0][k]), (d, tag, e)
        sk.close()

    # three lanes, lane stride no multiple of the pitch
    ls_f, ls_b = n * odd + 5, n * (w + 2) + 1
    assert ls_f % odd and ls_b % (w + 2)
    lanes_f64 = _strided(Z, torch.float64, float("nan"), odd, 1, ls_f)
    lanes_f32 = _strided(Z, torch.float32, float("nan"), even, 0, n * even + 2 * even - 1)
    flat = torch.full((B * ls_b + 8,), -1, dtype=torch.int64, device="cuda")
    lanes_bits = flat.as_strided((B, n, w + 2), (ls_b, w + 2, 1), 0)
    lanes_bits.copy_(_cuda(np.stack([_pack_bits(Z[b], w + 2) for b in range(B)])))
    for tag, view, code in (("f64 lanes", lanes_f64, F64), ("f32 lanes", lanes_f32, F32), ("bit lanes", lanes_bits, BITS)):
        sk = _dev(monkeypatch, N, R, d, l, lanes=B)
        for k, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
            _append_raw(sk, view[:, a:e], code, e - a, view.stride(1), lane_stride=view.stride(0))
            Bl, sl, ll, dl = sk.get()
            for b in range(B):
                assert _same_get((Bl[b], sl[b], int(ll[b]), dl[b]), refs[b][k][0]), (d, tag, b, e)
        sk.close()
    for sk in singles:
        sk.close()


# ---- c. the zero tail ------------------------------------------------------------------------------------------------------
def _assert_zero_tails(sk, c, tag):
    """Every live level of both halves: the rows from nk + pending on are all-zero bit patterns.  (A frozen MAIN level is
    outside the invariant: below the top, not in the first epoch, a snapshot of the current epoch lost.)"""
    i = sk.rows_seen
    pend = _pending(i, c.N, c.l)
    e0 = ((i - 1) // c.N) * c.N if i else 0
    checked = 0
    for kind in (0, 1):
        for j, lv in enumerate(sc.parse_half(_raw(sk, kind), sk.L, c.l, c.d)):
            if kind == 0 and i > c.N and j < sk.L - 1 and lv["dropped"] > e0:
                continue
            assert lv["nk"] + pend <= 2 * c.l, (tag, kind, j)
            assert not sc.bits(lv["buf"][lv["nk"] + pend:]).any(), (tag, kind, j, lv["nk"], pend)
            checked += 1
    return checked


@pytest.mark.parametrize("name", ["l6_ragged_epoch", "l8_d5"])
def test_zero_tail_behind_the_rows_in_use(name, monkeypatch):
    assert _trace_properties(name)[1] > 0          # (kept counts do fall in this case)
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    n = len(X)
    Xd = _cuda(X)
    sk = _case_dev(monkeypatch, name)
    # one call per checkpoint, and one block more behind each (the tail after a single rotation with nothing placed ahead)
    t = 0
    for cp in sorted(set(_checkpoints(c, n)) | {c.N + 5 * c.l, 2 * c.N + 3 * c.l + 1}):
        sk.fit(Xd[t:cp])
        t = cp
        assert _assert_zero_tails(sk, c, f"{name} t={cp}") > sk.L
    # a blob whose rows behind the rows in use were overwritten with ones, imported; then one more block
    t = c.N + 5 * c.l                                # a rotation boundary inside the second epoch: nothing pending
    A, Bk = _case_dev(monkeypatch, name), _case_dev(monkeypatch, name)
    A.fit(Xd[:t])
    Bk.fit(_cuda(X[::-1][:t]))
    nbuf = sk.L * 2 * c.l * c.d * 8
    for kind in (0, 1):
        raw = _raw(A, kind).copy()
        bufs = raw[:nbuf].view(np.float64).reshape(sk.L, 2 * c.l, c.d)
        for j, lv in enumerate(sc.parse_half(raw, sk.L, c.l, c.d)):
            bufs[j, lv["nk"]:] = 1.0
        Bk.import_half(kind, torch.from_numpy(raw).cuda())
    dirty = sc.parse_half(_raw(Bk, 1), sk.L, c.l, c.d)
    assert all(sc.bits(lv["buf"][lv["nk"]:]).all() for lv in dirty)      # (the ones are there)
    Bk.fit(Xd[t:t + c.l])                            # one block: one rotation
    assert _assert_zero_tails(Bk, c, f"{name} after import") > sk.L
    Bk.fit(Xd[t + c.l:t + 3 * c.l + 1])              # and a call that spans rotations behind it
    assert _assert_zero_tails(Bk, c, f"{name} after import, second call") > sk.L
    # begin_epoch(0) on a used handle
    A.begin_epoch(0)
    assert A.rows_seen == 0
    for kind in (0, 1):
        assert all(not sc.bits(lv["buf"]).any() for lv in sc.parse_half(_raw(A, kind), sk.L, c.l, c.d))
    A.fit(Xd[:c.N + 2 * c.l + 1])
    assert _assert_zero_tails(A, c, f"{name} after begin_epoch(0)") > sk.L
    fresh = _case_dev(monkeypatch, name)
    fresh.fit(Xd[:c.N + 2 * c.l + 1])
    assert _same_get(A.get(), fresh.get())           # (ring slots that are not live keep what the earlier stream left)
    for kind in (0, 1):
        pa, pf = (sc.parse_half(_raw(h, kind), sk.L, c.l, c.d) for h in (A, fresh))
        assert all(sc.live_equal(a, b) for a, b in zip(pa, pf)), kind
    for h in (sk, A, Bk, fresh):
        h.close()


# ---- d. frozen levels ----------------------------------------------------------------------------------------------------
def test_frozen_levels_keep_the_bytes_of_the_pair(monkeypatch):
    """l4 at row counts where the specification has frozen MAIN levels (rotation boundaries and inside blocks): the whole
    MAIN half -- frozen levels, whose buffers only take the raw rows, included -- equals the block-by-block handle's."""
    name = "l4"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    Xd = _cuda(X)
    _, trace = sc.oracle_trace(name)
    with_frozen = [s["i"] for s in trace if s["frozen"]]
    assert len(with_frozen) >= 4
    cps = sorted({with_frozen[k * (len(with_frozen) - 1) // 3] for k in range(4)})
    assert any(_pending(i, c.N, c.l) for i in cps)          # (one of them inside a block)
    fused, blockwise = _case_dev(monkeypatch, name), _case_dev(monkeypatch, name)
    t = 0
    for cp in cps:
        fused.fit(Xd[t:cp])
        _feed_per_block(blockwise, Xd, t, cp, c.N, c.l)
        t = cp
        main = sc.parse_half(_raw(fused, 0), fused.L, c.l, c.d)
        e0 = ((cp - 1) // c.N) * c.N
        frozen_dev = {j for j in range(fused.L - 1) if main[j]["dropped"] > e0}
        state = next(s for s in trace if s["i"] == cp)
        assert frozen_dev == set(state["frozen"]) and frozen_dev, cp
        assert _same_record(_record(fused), _record(blockwise)), cp
    fused.close()
    blockwise.close()
