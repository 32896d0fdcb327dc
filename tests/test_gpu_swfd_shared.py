"""On the GPU: the shared pending rows of the sliding-window sketch (csrc/swfd.hip, `Swfd::pendbuf`) --
one copy of a lane's pending rows instead of one per sketch -- against MUSED_SWFD_SHARED=0, the mode in which every sketch
buffer holds them.  Every comparison is bit for bit: get() by the rule of test_gpu_swfd_edges.py::_same_get, both exported
halves byte for byte.  And the GEMM operand with a second row segment (csrc/gemm_f64.h, GemmArgs::tail) alone, against the
same launch on the materialised operand.  Cases and the blob parser: tests/swfd_cases.py."""
import ctypes as C

import numpy as np
import pytest

import swfd_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SWITCHES = ("MUSED_SWFD_DEDUPE", "MUSED_SWFD_LIST", "MUSED_SWFD_ORDERS", "MUSED_SWFD_KACT", "MUSED_SWFD_SKIP_DEAD",
            "MUSED_SWFD_GRAM_SPLIT", "MUSED_SWFD_PREROT", "MUSED_SWFD_PREROT_SWEEPS", "MUSED_EIG_TRD", "MUSED_SWFD_SETTLE",
            "MUSED_SWFD_SHARED")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(monkeypatch, N, R, d, l, shared=True, env=None, **kw):
    """A handle created under a clean environment (the switches are read at creation), MUSED_SWFD_SHARED=0 if asked."""
    from mused_amd.swfd import SeqBasedSWFD

    with monkeypatch.context() as m:
        for name in SWITCHES:
            m.delenv(name, raising=False)
        if not shared:
            m.setenv("MUSED_SWFD_SHARED", "0")
        for k, v in (env or {}).items():
            m.setenv(k, v)
        sk = SeqBasedSWFD(N=N, R=R, d=d, sketch_dim=l, **kw)
        on = _lib_fn("mused_swfd_debug_shared")(sk._h)
        want = shared and not any(m_ in (env or {}) for m_ in ("MUSED_SWFD_SETTLE", "MUSED_SWFD_PREROT"))
        assert on == (1 if want else 0), (shared, env, on)      # (the mode under test is the mode that runs)
        return sk


def _lib_fn(name):
    from mused_amd import _lib

    fn = getattr(_lib.lib(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p]
    return fn


def _case_dev(monkeypatch, name, shared=True, env=None):
    c = sc.CASES[name]
    return _dev(monkeypatch, c.N, sc.case_stream(name)[1], c.d, c.l, shared=shared, env=env)


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


def _rotation_cuts(N, l, n):
    return sorted({i for i in range(1, n + 1) if i % N == 0 or (i % N) % l == 0} | {n})


def _feed_per_block(sk, Xd, a, b, N, l):
    """Rows a .. b in calls that end at every rotation: no call spans one, every block goes through the stand-alone append."""
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
    """Epoch ends (the first one closes the twin epoch), N + l + 2 and 2 N + 1 (rows pending; the second right behind an
    epoch start), a rotation boundary inside the second epoch, the end of the stream."""
    return sorted({c.N, 2 * c.N, 3 * c.N, 4 * c.N, c.N + c.l + 2, 2 * c.N + 1, c.N + 5 * c.l, n})


# ---- a. shared == MUSED_SWFD_SHARED=0 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["l4", "l6_ragged_epoch", "l8_d5", "l3_odd", "l2_d1", "N5_l8", "l8"])
def test_shared_equals_unshared(name, monkeypatch):
    """Three ways to feed a shared handle -- one call per checkpoint (interior blocks settled by the rotation), a call per
    block (the stand-alone append), ragged chunks that end inside blocks -- against the unshared handle at every checkpoint,
    and at every chunk end for the ragged one.  The cases freeze MAIN levels, drop kept rows and hold duplicate levels
    (test_gpu_swfd_settle.py checks that they do)."""
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    n = len(X)
    Xd = _cuda(X)
    ref, fused, blockwise = (_case_dev(monkeypatch, name, shared=False), _case_dev(monkeypatch, name),
                             _case_dev(monkeypatch, name))
    t = 0
    for cp in _checkpoints(c, n):
        ref.fit(Xd[t:cp])
        fused.fit(Xd[t:cp])
        _feed_per_block(blockwise, Xd, t, cp, c.N, c.l)
        t = cp
        want = _record(ref)
        assert _same_record(_record(fused), want), (name, cp, "one call per checkpoint")
        assert _same_record(_record(blockwise), want), (name, cp, "a call per block")
    assert want[0][1][0] > 0.0
    ref2, ragged = _case_dev(monkeypatch, name, shared=False), _case_dev(monkeypatch, name)
    t, with_pending = 0, 0
    for b in sc.case_blocks(name):
        ref2.fit(Xd[t:t + b])
        ragged.fit(Xd[t:t + b])
        t += b
        with_pending += _pending(t, c.N, c.l) > 0
        assert _same_record(_record(ragged), _record(ref2)), (name, t, "ragged chunks")
    assert t == n and (with_pending > 0 or c.l == 1)       # (chunks did end inside blocks)
    for sk in (ref, fused, blockwise, ref2, ragged):
        sk.close()


def test_frozen_levels_are_there_and_equal(monkeypatch):
    """l4 at the row counts where the specification has frozen MAIN levels: the device has them frozen too, and the MAIN half
    of the shared handle is the unshared one's, frozen levels included."""
    name = "l4"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    Xd = _cuda(X)
    _, trace = sc.oracle_trace(name)
    with_frozen = [s["i"] for s in trace if s["frozen"]]
    cps = sorted({with_frozen[k * (len(with_frozen) - 1) // 5] for k in range(6)})
    assert any(_pending(i, c.N, c.l) for i in cps)
    ref, sh = _case_dev(monkeypatch, name, shared=False), _case_dev(monkeypatch, name)
    t = 0
    for cp in cps:
        ref.fit(Xd[t:cp])
        sh.fit(Xd[t:cp])
        t = cp
        main = sc.parse_half(_raw(sh, 0), sh.L, c.l, c.d)
        e0 = ((cp - 1) // c.N) * c.N
        assert {j for j in range(sh.L - 1) if main[j]["dropped"] > e0}, cp
        assert _same_record(_record(sh), _record(ref)), cp
    ref.close()
    sh.close()


@pytest.mark.parametrize("env", [{"MUSED_SWFD_DEDUPE": "0"}, {"MUSED_SWFD_LIST": "0"}, {"MUSED_SWFD_KACT": "0"},
                                 {"MUSED_SWFD_SKIP_DEAD": "0"}, {"MUSED_SWFD_GRAM_SPLIT": "4"}])
def test_shared_equals_unshared_under_the_switches(env, monkeypatch):
    """The launch modes the rotation's products have (no list, no K bound, the batched split-K Gram of long rows) and the
    sketches without frozen or duplicate levels."""
    name = "split_d100" if "MUSED_SWFD_GRAM_SPLIT" in env else "l6_ragged_epoch"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    Xd = _cuda(X)
    ref, sh = _case_dev(monkeypatch, name, shared=False, env=env), _case_dev(monkeypatch, name, env=env)
    t = 0
    for cp in (c.N + c.l + 2, 2 * c.N + 3 * c.l + 1, 3 * c.N):
        ref.fit(Xd[t:cp])
        sh.fit(Xd[t:cp])
        t = cp
        assert _same_record(_record(sh), _record(ref)), (env, cp)
    ref.close()
    sh.close()


@pytest.mark.parametrize("env", [{"MUSED_SWFD_SETTLE": "0"}, {"MUSED_SWFD_PREROT": "1"}])
def test_the_mode_is_off_with_the_other_paths(env, monkeypatch):
    """MUSED_SWFD_SETTLE=0 and MUSED_SWFD_PREROT=1 run the code they ran: with them the switch changes nothing."""
    name = "l4"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    Xd = _cuda(X)
    a, b = _case_dev(monkeypatch, name, shared=False, env=env), _case_dev(monkeypatch, name, env=env)
    t = 0
    for cp in (c.N + c.l + 2, 2 * c.N + 3):
        a.fit(Xd[t:cp])
        b.fit(Xd[t:cp])
        t = cp
        assert _same_record(_record(a), _record(b)), (env, cp)
    a.close()
    b.close()


# ---- b. lanes == singles -------------------------------------------------------------------------------------------------
def test_three_lanes_equal_three_singles(monkeypatch):
    """Three lanes with different streams (the case's, reversed, and rolled by 17 rows), fed in ragged chunks: every lane's
    get() is the single shared handle's, which is the unshared one's by the tests above."""
    name = "l6_ragged_epoch"
    c = sc.CASES[name]
    X, R = sc.case_stream(name)
    Z = np.stack([X, X[::-1], np.roll(X, 17, axis=0)])
    Zd = _cuda(Z)
    lanes = _dev(monkeypatch, c.N, R, c.d, c.l, lanes=3)
    singles = [_dev(monkeypatch, c.N, R, c.d, c.l) for _ in range(3)]
    t = 0
    for b in sc.case_blocks(name):
        lanes.fit_lanes(Zd[:, t:t + b])
        for k, sk in enumerate(singles):
            sk.fit(Zd[k, t:t + b])
        t += b
        Bl, sl, ll, dl = lanes.get()
        for k, sk in enumerate(singles):
            assert _same_get((Bl[k], sl[k], int(ll[k]), dl[k]), sk.get()), (t, k)
    for sk in singles + [lanes]:
        sk.close()


# ---- c. row sources ----------------------------------------------------------------------------------------------------------
def _append_raw(sk, t, dtype, n_rows, ld):
    from mused_amd._lib import call
    from mused_amd.engine import ptr, stream_ptr

    call("mused_swfd_append", sk._h, ptr(t), dtype, n_rows, ld, stream_ptr())
    keep = getattr(sk, "_held", [])
    keep.append(t)
    sk._held = keep


def _strided(Z, dtype, fill, pitch, offset):
    n, d = Z.shape
    flat = torch.full((offset + n * pitch + 8,), fill, dtype=dtype, device="cuda")
    view = flat.as_strided((n, d), (pitch, 1), offset)
    view.copy_(torch.from_numpy(Z).to(dtype).cuda())
    return view


def _pack_bits(Z, pitch):
    n, d = Z.shape
    full = np.ones((n, pitch * 64), dtype=np.uint8)
    full[:, :d] = Z
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.int64)


@pytest.mark.parametrize("d", [5, 64, 65, 130])
def test_row_sources_through_the_settle_and_the_append(d, monkeypatch):
    """One 0/1 stream (exact in every type) as F64 / F32 / I64 / bit rows; aligned with an even pitch (the 16-byte path when
    d is even) and one element into a NaN-filled allocation with an odd pitch (misaligned).  Each source is fed twice: in
    calls that span rotations (the settle kernel writes pendbuf) and a call per block plus a call that ends inside one (the
    stand-alone append does).  The reference is the unshared handle on contiguous F64 rows."""
    from mused_amd._lib import BITS, F32, F64, I64

    l = 4
    N = max(d, 3 * l + 1)
    n = 2 * N + 7
    cuts = [0, N + l + 2, n]
    Z = (np.random.default_rng(7000 + d).random((n, d)) < 0.1).astype(np.float64)
    R = max(float(Z.sum(1).max()), 1.0)
    w = (d + 63) // 64
    even, odd = d + 2 + (d & 1), d + 3 - (d & 1)
    ref, Zd, want = _dev(monkeypatch, N, R, d, l, shared=False), _cuda(Z), []
    for a, e in zip(cuts[:-1], cuts[1:]):
        ref.fit(Zd[a:e])
        want.append(_record(ref))
    ref.close()
    assert want[-1][0][1][0] > 0.0
    i64min = torch.iinfo(torch.int64).min
    sources = []
    for tag, dtype, code, fill in (("f64", torch.float64, F64, float("nan")), ("f32", torch.float32, F32, float("nan")),
                                   ("i64", torch.int64, I64, i64min)):
        sources.append((f"{tag} aligned", _strided(Z, dtype, fill, even, 0), code, even))
        sources.append((f"{tag} misaligned", _strided(Z, dtype, fill, odd, 1), code, odd))
    bits_in = torch.full((1 + n * (w + 2) + 8,), -1, dtype=torch.int64, device="cuda")
    bits_view = bits_in.as_strided((n, w + 2), (w + 2, 1), 1)
    bits_view.copy_(_cuda(_pack_bits(Z, w + 2)))
    sources.append(("bits one word in", bits_view, BITS, w + 2))
    sources.append(("bits tight", _cuda(_pack_bits(Z, w)), BITS, w))
    for tag, view, code, pitch in sources:
        spanning, blockwise = _dev(monkeypatch, N, R, d, l), _dev(monkeypatch, N, R, d, l)
        for k, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
            _append_raw(spanning, view[a:e], code, e - a, pitch)
            assert _same_record(_record(spanning), want[k]), (d, tag, e, "settle")
            t = a
            for cut in [x for x in _rotation_cuts(N, l, e) if x > a]:
                _append_raw(blockwise, view[t:cut], code, cut - t, pitch)
                t = cut
            assert _same_record(_record(blockwise), want[k]), (d, tag, e, "append")
        spanning.close()
        blockwise.close()


# ---- d. blobs across the modes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", ["boundary", "pending"])
@pytest.mark.parametrize("to_shared", [True, False])
def test_blobs_cross_the_modes(t0, to_shared, monkeypatch):
    """Both halves exported from a handle of one mode in its second epoch (on a rotation boundary; with rows pending and
    MAIN levels frozen), imported into a handle of the other mode that has seen as many other rows: the halves read back
    equal, and from there on the same rows give the same bits in get() and in both halves."""
    name = "l6_ragged_epoch"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    Xd = _cuda(X)
    t = c.N + 5 * c.l + (0 if t0 == "boundary" else 4)
    assert _pending(t, c.N, c.l) == (0 if t0 == "boundary" else 4)
    A, Bk = _case_dev(monkeypatch, name, shared=not to_shared), _case_dev(monkeypatch, name, shared=to_shared)
    A.fit(Xd[:t])
    Bk.fit(_cuda(X[::-1][:t]))
    assert not _same_get(A.get(), Bk.get())
    for kind in (0, 1):
        Bk.import_half(kind, A.export_half(kind))
    assert _same_record(_record(Bk), _record(A)), "right after the import"
    for b in sc.blocks(c.l, 2 * c.N):
        A.fit(Xd[t:t + b])
        Bk.fit(Xd[t:t + b])
        t += b
        assert _same_get(A.get(), Bk.get()), t
        for kind in (0, 1):
            pa, pb = (sc.parse_half(_raw(h, kind), A.L, c.l, c.d) for h in (A, Bk))
            assert all(sc.live_equal(a, b_) for a, b_ in zip(pa, pb)), (t, kind)
    A.close()
    Bk.close()


def test_hand_over_across_the_modes(monkeypatch):
    """begin_epoch with the AUX half of the predecessor, the handles alternating between the modes: the last one's get()
    is the sequential unshared sketch's."""
    name = "l6_ragged_epoch"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    Xd = _cuda(X)
    seq = _case_dev(monkeypatch, name, shared=False)
    blob = None
    for e in range(4):
        seq.fit(Xd[e * c.N:(e + 1) * c.N])
        sk = _case_dev(monkeypatch, name, shared=(e % 2 == 0))
        sk.begin_epoch(e * c.N, blob)
        sk.fit(Xd[e * c.N:(e + 1) * c.N])
        blob = sk.export_half(1)
        assert _same_get(sk.get(), seq.get()), e
        pa, pb = (sc.parse_half(r, seq.L, c.l, c.d) for r in (blob.cpu().numpy(), _raw(seq, 1)))
        assert all(sc.live_equal(a, b_) for a, b_ in zip(pa, pb)), e      # (dead ring slots keep an earlier epoch's rows)
        sk.close()
    seq.close()


def test_a_dirty_tail_is_not_read(monkeypatch):
    """A blob whose buffer rows behind the rows in use were overwritten with ones (the unshared mode's Gram product would
    read them: it is the shared handle that is held to ignoring them).  Imported into a shared handle, the ones read back
    in the export; after one block and its rotation get() and both halves are those of the handle that imported the clean
    blob, in either mode, and every live level has its zero tail."""
    name = "l8_d5"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    Xd = _cuda(X)
    t = c.N + 5 * c.l
    A = _case_dev(monkeypatch, name, shared=False)
    A.fit(Xd[:t])
    clean_sh, clean_un, dirty = (_case_dev(monkeypatch, name), _case_dev(monkeypatch, name, shared=False),
                                 _case_dev(monkeypatch, name))
    for h in (clean_sh, clean_un, dirty):
        h.fit(_cuda(X[::-1][:t]))
    nbuf = A.L * 2 * c.l * c.d * 8
    e0 = ((t - 1) // c.N) * c.N
    for kind in (0, 1):
        raw = _raw(A, kind)
        for h in (clean_sh, clean_un):
            h.import_half(kind, torch.from_numpy(raw).cuda())
        raw = raw.copy()
        bufs = raw[:nbuf].view(np.float64).reshape(A.L, 2 * c.l, c.d)
        for j, lv in enumerate(sc.parse_half(raw, A.L, c.l, c.d)):
            if not (kind == 0 and j < A.L - 1 and lv["dropped"] > e0):      # (a frozen level keeps its bytes in every mode)
                bufs[j, lv["nk"]:] = 1.0
        dirty.import_half(kind, torch.from_numpy(raw).cuda())
        assert np.array_equal(_raw(dirty, kind), raw), kind
    for h in (clean_sh, clean_un, dirty):
        h.fit(Xd[t:t + c.l])
    want = _record(clean_un)
    assert _same_record(_record(clean_sh), want)
    assert _same_record(_record(dirty), want)
    for h in (A, clean_sh, clean_un, dirty):
        h.close()


# ---- e. the operand alone ------------------------------------------------------------------------------------------------
SENT = -1.2345678912345e300
BATCH, PER_LANE = 4, 2
_PTR3 = [C.c_void_p, C.c_long, C.c_long] * 3


def _fn(name, argtypes):
    from mused_amd import _lib

    fn = getattr(_lib.lib(), name)
    fn.restype = C.c_int
    fn.argtypes = argtypes
    return fn


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _launch(a_kc, b_kc, A, lda, sA, B, ldb, sB, M, N, K, kact=None, lst=None, tail=None, nsplit=1, kchunk=0):
    """One batched launch into a sentinel-filled C.  tail = None: the library's ordinary launches (list / K bound: the entry
    of test_gpu_gemm_active.py; split over K: mused_gemm_f64_batched_splitk).  tail = (rows, lane stride, split array,
    its stride, pend, the row of zeros, plain_diag): the same launch with the second row segment."""
    from mused_amd import _lib

    out = torch.full((BATCH, M, N), SENT, dtype=torch.float64, device="cuda")
    part = torch.empty(BATCH * max(nsplit, 1) * M * N, dtype=torch.float64, device="cuda")
    dl = None if lst is None else _i32([len(lst)] + list(lst) + [0] * (BATCH - len(lst)))
    dk = None if kact is None else _i32(kact)
    if tail is not None:
        rows, ls, split, stride, pend, zero_row, plain_diag = tail
        fn = _fn("mused_debug_gemm_f64_batched_tail",
                 [C.c_int, C.c_int] + _PTR3 + [C.c_int] * 4 + [C.c_void_p] * 3
                 + [C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p])
        _lib.check(fn(a_kc, b_kc, _p(A), lda, sA, _p(B), ldb, sB, _p(out), N, M * N, M, N, K, BATCH, _p(dl), _p(dk), _p(rows),
                      ls, PER_LANE, _p(split), stride, pend, _p(zero_row), plain_diag, _p(part), kchunk, nsplit, _stream()))
    elif nsplit > 1:
        fn = _fn("mused_gemm_f64_batched_splitk",
                 [C.c_int, C.c_int] + [C.c_void_p, C.c_long, C.c_long] * 2 + [C.c_void_p, C.c_void_p] + [C.c_int] * 6
                 + [C.c_void_p, C.c_void_p])
        _lib.check(fn(a_kc, b_kc, _p(A), lda, sA, _p(B), ldb, sB, _p(part), _p(out), M, N, K, BATCH, kchunk, nsplit, None,
                      _stream()))
    else:
        fn = _fn("mused_debug_gemm_f64_batched_active",
                 [C.c_int, C.c_int] + _PTR3 + [C.c_int] * 4 + [C.c_double] + [C.c_void_p] * 3)
        _lib.check(fn(a_kc, b_kc, _p(A), lda, sA, _p(B), ldb, sB, _p(out), N, M * N, M, N, K, BATCH, 1.0, _p(dl), _p(dk),
                      _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _place(a, offset):
    """`a` in a NaN-filled allocation, its first element `offset` doubles in (1: off the 16-byte boundary)."""
    flat = torch.full((offset + a.size + 8,), float("nan"), dtype=torch.float64, device="cuda")
    flat[offset:offset + a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    return flat[offset:]


def _sketch_operands(n, d, ell, pend, nks, pitch, offset, seed):
    """BATCH sketch-like buffers (n rows of d doubles, row pitch `pitch`): the MATERIALISED ones hold kept rows, the
    lane's first pend tail rows and +0.0; the SPLIT ones hold the kept rows and NaN from the split on (rows nobody may
    read); the lanes' tails hold ell rows each, NaN from row pend on; the row of zeros.  The padding behind column d is NaN
    everywhere."""
    rng = np.random.default_rng(seed)
    kept = rng.standard_normal((BATCH, n, d))
    tails = rng.standard_normal((BATCH // PER_LANE, ell, d))
    full = np.full((BATCH, n, pitch), np.nan)
    full[:, :, :d] = 0.0
    holey = np.full((BATCH, n, pitch), np.nan)
    for z, nk in enumerate(nks):
        full[z, :nk, :d] = kept[z, :nk]
        full[z, nk:nk + pend, :d] = tails[z // PER_LANE, :pend]
        holey[z, :nk, :d] = kept[z, :nk]
    tp = np.full((BATCH // PER_LANE, ell, pitch), np.nan)
    tp[:, :pend, :d] = tails[:, :pend]
    zero_row = np.full(pitch, np.nan)
    zero_row[:d] = 0.0
    return _place(full, offset), _place(holey, offset), _place(tp, offset), _place(zero_row, offset)


def _split_sets(n, pend):
    """The splits {0, 1, 15, 16, 17, n - pend} (those that leave room for the tail), as batches of BATCH entries."""
    sp = sorted({v for v in (0, 1, 15, 16, 17, n - pend) if 0 <= v <= n - pend})
    sets = [[sp[(i + z) % len(sp)] for z in range(BATCH)] for i in range(0, len(sp), BATCH)]
    assert {v for s_ in sets for v in s_} == set(sp)
    return sets


def _layouts(d):
    """(name, pitch, offset): 16-byte loads (even pitch, aligned base) and 8-byte loads (odd pitch, base one double in)."""
    return [("vector", d + (d & 1), 0), ("scalar", d + 1 - (d & 1), 1)]


@pytest.mark.parametrize("d", [5, 24, 250])
@pytest.mark.parametrize("n", [16, 48, 130, 256])
def test_gram_operand_with_a_tail(n, d, monkeypatch):
    """C[z] = op[z] op[z]^T (order n, depth d), op[z] split at nk[z] with pend tail rows: the bits of the ordinary launch on
    the materialised operand -- with the diagonal tiles of the symmetric launch as the process has them and with the
    ordinary ones, plain and split over K, through the 16-byte and the 8-byte loads."""
    ell = n // 2
    nsplit = 4 if d > 64 else 2
    kchunk = (((d + nsplit - 1) // nsplit + 15) // 16) * 16
    for how, pitch, offset in _layouts(d):
        for pend in (0, 1, ell):
            for nks in _split_sets(n, pend):
                full, holey, tail, zrow = _sketch_operands(n, d, ell, pend, nks, pitch, offset, 1000 * n + 10 * d + pend)
                split = torch.zeros(BATCH * 4, dtype=torch.int32, device="cuda")
                split[::4] = _i32(nks)
                sA = n * pitch
                for ns, kc in ((1, 0), (nsplit, kchunk)):
                    want = _launch(1, 1, full, pitch, sA, full, pitch, sA, n, n, d, nsplit=ns, kchunk=kc)
                    assert not np.isnan(want).any() and (want != SENT).all()
                    for plain_diag in (0, 1):
                        got = _launch(1, 1, holey, pitch, sA, holey, pitch, sA, n, n, d, nsplit=ns, kchunk=kc,
                                      tail=(tail, ell * pitch, split, 4, pend, zrow, plain_diag))
                        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (n, d, how, pend, nks, ns, plain_diag)


@pytest.mark.parametrize("d", [5, 24, 250])
@pytest.mark.parametrize("n", [16, 48, 130, 256])
def test_k_rows_operand_with_a_tail(n, d):
    """The rotate product T[z] = W[z] op[z] (W: n / 2 x n, K-contiguous; op: the n x d sketch operand as K rows), op[z] split
    at nk[z]: over all n rows, and with the K bound per entry the sketch uses (rows in use rounded up to 16) together with
    a list that leaves one entry out -- the bits of the ordinary launch on the materialised operand."""
    ell = n // 2
    M = ell
    W = _place(np.random.default_rng(n + d).standard_normal((BATCH, M, n)), 0)
    lst = [3, 0, 2]
    for how, pitch, offset in _layouts(d):
        for pend in (0, 1, ell):
            for nks in _split_sets(n, pend):
                full, holey, tail, zrow = _sketch_operands(n, d, ell, pend, nks, pitch, offset, 2000 * n + 10 * d + pend)
                split = _i32(nks)
                kact = [min(n, (nk + pend + 15) // 16 * 16) for nk in nks]
                for kb, li in ((None, None), (kact, lst)):
                    want = _launch(1, 0, W, n, M * n, full, pitch, n * pitch, M, d, n, kact=kb, lst=li)
                    got = _launch(1, 0, W, n, M * n, holey, pitch, n * pitch, M, d, n, kact=kb, lst=li,
                                  tail=(tail, ell * pitch, split, 1, pend, zrow, 0))
                    assert not np.isnan(want).any()
                    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (n, d, how, pend, nks, kb is not None)
                    if li is not None:
                        assert (got[1] == SENT).all()
