"""On the GPU: P P^T of a lane's pending rows formed once, ahead of the rotations, and copied into the Gram tiles that hold
nothing else (csrc/gemm_f64.h, GemmArgs::fill; csrc/swfd.hip, `Swfd::ppt`).

GEMM level: the symmetric launch on a split operand with the fill source against the ordinary symmetric launch on the
materialised operand, bit for bit -- this is also the check of the premise (an entry of a v_mfma_f64_16x16x4 K chain does not
depend on where in a tile it is computed).  Handle level: the default against MUSED_SWFD_PPT=0, get() and both exported
halves byte for byte after every call."""
import ctypes as C

import numpy as np
import pytest

import swfd_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SWITCHES = ("MUSED_SWFD_DEDUPE", "MUSED_SWFD_LIST", "MUSED_SWFD_ORDERS", "MUSED_SWFD_KACT", "MUSED_SWFD_SKIP_DEAD",
            "MUSED_SWFD_GRAM_SPLIT", "MUSED_SWFD_PREROT", "MUSED_SWFD_PREROT_SWEEPS", "MUSED_EIG_TRD", "MUSED_SWFD_SETTLE",
            "MUSED_SWFD_SHARED", "MUSED_SWFD_PPT", "MUSED_SWFD_PPT_CHUNK")

SENT = -777.25
LANES = 2
PER_LANE = 2
BATCH = LANES * PER_LANE
LISTED = [3, 0, 2]          # entry 1 is left out
GROUPS = 2                  # the P P^T launch forms two blocks per lane; the Gram launch is given the second


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


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


def _place(a, offset, dtype=torch.float64):
    """`a` in a NaN-filled allocation, its first element `offset` elements in (1: off the 16-byte boundary)."""
    flat = torch.full((offset + a.size + 8,), float("nan"), dtype=dtype, device="cuda")
    flat[offset:offset + a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda().to(dtype)
    return flat[offset:]


def _layouts(d):
    """(name, row pitch of the fp64 arrays, of the fp32 array, offset): 16-byte loads (aligned base, rows a multiple of 16
    bytes) and 8- / 4-byte loads (odd pitch, base one element in)."""
    return [("vector", d + (d & 1), (d + 3) // 4 * 4, 0), ("scalar", d + 1 - (d & 1), d + 1 - (d & 1), 1)]


def _nk_sets(n, pend):
    """The splits that leave room for the tail, three at a time on the listed entries (the entry left out gets the first)."""
    sp = sorted({v for v in (0, 1, 15, 16, 17, 127, 128, 129, n - pend) if 0 <= v <= n - pend})
    sets = []
    for i in range(0, len(sp), len(LISTED)):
        nks = [sp[0]] * BATCH
        for j, z in enumerate(LISTED):
            nks[z] = sp[(i + j) % len(sp)]
        sets.append(nks)
    assert {s_[z] for s_ in sets for z in LISTED} == set(sp)
    return sets


def _ordinary(full, pitch, n, d, lst):
    fn = _fn("mused_debug_gemm_f64_batched_active",
             [C.c_int, C.c_int] + [C.c_void_p, C.c_long, C.c_long] * 3 + [C.c_int] * 4 + [C.c_double] + [C.c_void_p] * 3)
    from mused_amd import _lib

    out = torch.full((BATCH, n, n), SENT, dtype=torch.float64, device="cuda")
    _lib.check(fn(1, 1, _p(full), pitch, n * pitch, _p(full), pitch, n * pitch, _p(out), n, n * n, n, n, d, BATCH, 1.0,
                  _p(lst), None, _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _gram_rows(src, dtype, pitch, lane_stride, pend, d, ell, plain_diag):
    """P P^T of GROUPS blocks of pend rows per lane, read in place: out[group][lane] (ell x ell, NaN outside the pend x pend
    corner)."""
    from mused_amd import _lib

    fn = _fn("mused_debug_gemm_gram_rows",
             [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_long, C.c_void_p, C.c_long, C.c_long] + [C.c_int] * 4
             + [C.c_void_p])
    out = torch.full((GROUPS, LANES, ell, ell), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(fn(_p(src), dtype, pitch, lane_stride, LANES, pend * pitch, _p(out), ell, ell * ell, pend, d, GROUPS * LANES,
                  plain_diag, _stream()))
    return out


def _filled(holey, pitch, n, d, lst, tail, split, pend, zrow, plain_diag, fill, ell):
    from mused_amd import _lib

    fn = _fn("mused_debug_gemm_f64_batched_tail_fill",
             [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p,
              C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_int,
              C.c_void_p])
    out = torch.full((BATCH, n, n), SENT, dtype=torch.float64, device="cuda")
    _lib.check(fn(_p(holey), pitch, n * pitch, _p(out), n, n * n, n, d, BATCH, _p(lst), _p(tail), ell * pitch, PER_LANE,
                  _p(split), 4, pend, _p(zrow), plain_diag, _p(fill), ell * ell, ell, _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("d", [5, 24, 250])
@pytest.mark.parametrize("n", [16, 130, 256, 272, 400])
def test_gram_with_copied_tiles(n, d):
    """C[z] = op[z] op[z]^T (order n, depth d), op[z] = [nk[z] kept rows; the lane's pend tail rows; +0.0], with P P^T of the
    tail rows as the fill source: the bits of the ordinary symmetric launch on the materialised operand, every entry of the
    listed matrices written, the matrix left out untouched.  P P^T comes from a two-level batched launch (lane, block) on
    the rows in place, once from fp32 rows and once from fp64 rows, and is itself the ordinary Gram product of those rows."""
    from mused_amd._lib import F32, F64

    ell = n // 2
    lst = _i32([len(LISTED)] + LISTED + [0] * (BATCH - len(LISTED)))
    for how, pitch, pitch32, offset in _layouts(d):
        for pend in sorted({0, 1, min(16, ell), ell}):
            rng = np.random.default_rng(1000 * n + 10 * d + pend)
            # the rows a lane receives: GROUPS blocks of pend rows, fp32 values (so that both sources hold the same numbers)
            rows = rng.standard_normal((LANES, GROUPS * pend, d)).astype(np.float32).astype(np.float64)
            src64 = np.full((LANES, GROUPS * pend, pitch), np.nan)
            src64[:, :, :d] = rows
            src32 = np.full((LANES, GROUPS * pend, pitch32), np.nan)
            src32[:, :, :d] = rows
            sources = [(_place(src64, offset), F64, pitch), (_place(src32, offset, torch.float32), F32, pitch32)]
            tails = rows[:, pend:2 * pend]                      # the second block
            tp = np.full((LANES, ell, pitch), np.nan)
            tp[:, :pend, :d] = tails
            tail = _place(tp, offset)
            zr = np.full(pitch, np.nan)
            zr[:d] = 0.0
            zrow = _place(zr, offset)
            for nks in _nk_sets(n, pend):
                kept = rng.standard_normal((BATCH, n, d))
                full = np.full((BATCH, n, pitch), np.nan)
                full[:, :, :d] = 0.0
                holey = np.full((BATCH, n, pitch), np.nan)      # NaN from the split on: rows nobody may read
                for z, nk in enumerate(nks):
                    full[z, :nk, :d] = kept[z, :nk]
                    full[z, nk:nk + pend, :d] = tails[z // PER_LANE]
                    holey[z, :nk, :d] = kept[z, :nk]
                full, holey = _place(full, offset), _place(holey, offset)
                split = torch.zeros(BATCH * 4, dtype=torch.int32, device="cuda")
                split[::4] = _i32(nks)
                want = _ordinary(full, pitch, n, d, lst)
                assert not np.isnan(want[LISTED]).any() and (want[LISTED] != SENT).all() and (want[1] == SENT).all()
                for plain_diag in (0, 1):
                    for src, dtype, sp in sources:
                        pp = _gram_rows(src, dtype, sp, GROUPS * pend * sp, pend, d, ell, plain_diag)
                        tag = (n, d, how, pend, nks, plain_diag, dtype)
                        if pend:
                            torch.cuda.synchronize()
                            corner = pp[:, :, :pend, :pend].cpu().numpy()
                            blocks = rows.reshape(LANES, GROUPS, pend, d).transpose(1, 0, 2, 3)
                            assert np.allclose(corner, blocks @ blocks.transpose(0, 1, 3, 2), rtol=1e-12, atol=1e-12), tag
                            assert np.isnan(pp.cpu().numpy()[:, :, pend:, :]).all(), tag
                        got = _filled(holey, pitch, n, d, lst, tail, split, pend, zrow, plain_diag, pp[1], ell)
                        assert np.array_equal(got.view(np.int64), want.view(np.int64)), tag


# ---- the handle ----------------------------------------------------------------------------------------------------------
def _dev(monkeypatch, N, R, d, l, ppt=True, env=None, **kw):
    """A handle created under a clean environment (the switches are read at creation), MUSED_SWFD_PPT=0 if asked, and
    MUSED_SWFD_PPT=1 where the default of the order is off."""
    from mused_amd.swfd import SeqBasedSWFD

    with monkeypatch.context() as m:
        for name in SWITCHES:
            m.delenv(name, raising=False)
        if not ppt:
            m.setenv("MUSED_SWFD_PPT", "0")
        elif 2 * l <= 128:
            m.setenv("MUSED_SWFD_PPT", "1")              # (a Gram matrix of one tile: off unless asked for)
        for k, v in (env or {}).items():
            m.setenv(k, v)
        sk = SeqBasedSWFD(N=N, R=R, d=d, sketch_dim=l, **kw)
        chunk = _fn("mused_swfd_debug_ppt", [C.c_void_p])(sk._h)
        assert (chunk > 0) == ppt, (ppt, env, chunk)      # (the mode under test is the mode that runs)
        if env and "MUSED_SWFD_PPT_CHUNK" in env:
            assert chunk == int(env["MUSED_SWFD_PPT_CHUNK"])
        return sk


def _record(sk):
    """get() and both exported halves (a handle with several lanes exports nothing: get() of every lane)."""
    if sk.lanes != 1:
        return sk.get(), np.zeros(0), np.zeros(0)
    return sk.get(), sk.export_half(0).cpu().numpy(), sk.export_half(1).cpu().numpy()


def _same_record(a, b):
    return (all(sc.same_bits(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])
            and np.array_equal(a[2], b[2]))


def _rows(l, d, lanes, dtype, seed):
    """(lanes, n, d) rows on the device, n = 2 N + l + 5 with N = 3 l + 16 (a short block ends every epoch, two epoch changes),
    and R."""
    N = 3 * l + 16
    n = 2 * N + l + 5
    X = np.stack([sc.stream(N, d, n, seed + b, (N // 3, N // 2, 6.0)) for b in range(lanes)])
    if dtype is np.int64:
        X = np.rint(X).astype(np.int64)
    else:
        X = X.astype(dtype)
    R = float((X.astype(np.float64) ** 2).sum(-1).max())
    return torch.from_numpy(X).cuda(), N, n, R


def _feed(sk, Xd, a, b):
    if sk.lanes == 1:
        sk.fit(Xd[0, a:b])
    else:
        sk.fit_lanes(Xd[:, a:b])


def _calls(how, N, l, n):
    sizes = [N] if how == "window" else [1, l - 1, l + 1, N + 1]
    out, t, i = [], 0, 0
    while t < n:
        b = min(sizes[i % len(sizes)], n - t)
        out.append((t, t + b))
        t += b
        i += 1
    return out


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("d", [24, 130])
@pytest.mark.parametrize("l", [50, 72, 128, 160])
def test_ppt_equals_ppt_off(l, d, lanes, monkeypatch):
    """The default handle against MUSED_SWFD_PPT=0 after every call: a whole window per call (every block complete: its
    P P^T comes from the batched launch) and ragged calls (blocks completed across calls take the fall-back), from fp32,
    fp64 and int64 rows (int64: no P P^T at all)."""
    for dtype in (np.float32, np.float64, np.int64):
        Xd, N, n, R = _rows(l, d, lanes, dtype, 100 * l + d)
        for how in ("window", "ragged"):
            ref = _dev(monkeypatch, N, R, d, l, ppt=False, lanes=lanes)
            dev = _dev(monkeypatch, N, R, d, l, lanes=lanes)
            for a, b in _calls(how, N, l, n):
                _feed(ref, Xd, a, b)
                _feed(dev, Xd, a, b)
                assert _same_record(_record(dev), _record(ref)), (l, d, lanes, dtype.__name__, how, b)
            ref.close()
            dev.close()


def test_ppt_default_by_order(monkeypatch):
    """Unset, the switch follows the order: on from two tiles up (16 blocks a launch at these sizes), off for one tile."""
    from mused_amd.swfd import SeqBasedSWFD

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for l, want in ((50, 0), (64, 0), (65, 16), (128, 16)):
        sk = SeqBasedSWFD(N=3 * l, R=16.0, d=24, sketch_dim=l)
        assert _fn("mused_swfd_debug_ppt", [C.c_void_p])(sk._h) == want, l
        sk.close()


def test_ppt_chunk_smaller_than_a_call(monkeypatch):
    """Two blocks per chunk, eight blocks per call: the workspace is reused inside a call."""
    l, d, lanes = 72, 24, 3
    Xd, N, n, R = _rows(l, d, lanes, np.float32, 7)
    ref = _dev(monkeypatch, N, R, d, l, ppt=False, lanes=lanes)
    dev = _dev(monkeypatch, N, R, d, l, lanes=lanes, env={"MUSED_SWFD_PPT_CHUNK": "2"})
    for a, b in ((0, 2 * N + 3), (2 * N + 3, n)):
        _feed(ref, Xd, a, b)
        _feed(dev, Xd, a, b)
        assert _same_record(_record(dev), _record(ref)), b
    ref.close()
    dev.close()


def test_ppt_lanes_equal_single_handles(monkeypatch):
    """Three lanes in lock-step hold what three single-lane handles hold (one P P^T launch for all lanes against one each)."""
    l, d, lanes = 128, 24, 3
    Xd, N, n, R = _rows(l, d, lanes, np.float64, 11)
    multi = _dev(monkeypatch, N, R, d, l, lanes=lanes)
    singles = [_dev(monkeypatch, N, R, d, l) for _ in range(lanes)]
    for a, b in _calls("window", N, l, n):
        multi.fit_lanes(Xd[:, a:b])
        for z, sk in enumerate(singles):
            sk.fit(Xd[z, a:b])
        B, sig, lvl, delta = multi.get()
        for z, sk in enumerate(singles):
            g = sk.get()
            assert sc.same_bits(B[z], g[0]) and sc.same_bits(sig[z], g[1]) and lvl[z] == g[2] and sc.same_bits(delta[z], g[3]), (b, z)
    multi.close()
    for sk in singles:
        sk.close()


def test_ppt_with_imported_state(monkeypatch):
    """import_half and begin_epoch with a blob between calls: the imported pending rows take the fall-back, the blocks
    behind them the batched launch again."""
    l, d = 72, 24
    Xd, N, n, R = _rows(l, d, 1, np.float64, 23)
    donor = _dev(monkeypatch, N, R, d, l, ppt=False)
    donor.fit(Xd[0, :N + l + 7])                       # rows pending in the exported state
    main, aux = donor.export_half(0), donor.export_half(1)
    pair = []
    for ppt in (False, True):
        sk = _dev(monkeypatch, N, R, d, l, ppt=ppt)
        sk.fit(Xd[0, :N + l + 7])
        sk.import_half(0, main)
        sk.import_half(1, aux)
        sk.fit(Xd[0, N + l + 7:2 * N])
        rec = [_record(sk)]
        sk.begin_epoch(2 * N, sk.export_half(1))
        sk.fit(Xd[0, 2 * N:n])
        rec.append(_record(sk))
        pair.append(rec)
        sk.close()
    donor.close()
    for a, b in zip(*pair):
        assert _same_record(b, a)
