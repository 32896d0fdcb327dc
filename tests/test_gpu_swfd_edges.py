"""On the GPU: the sliding-window sketch (csrc/swfd.hip, mused_amd/swfd.py) at its edges -- the state of EVERY sketch (all
2 L of them, not the one level get() reads) against the specification after every ragged block, the row sources (pitched
F32 / F64 / I64 rows, bit rows off the word boundary with junk behind column d, strided lanes) bit for bit against
contiguous F64 rows, batching invariance on the device, the environment switches, and the state exchange between handles.
Cases, the instrumented specification and the blob parser: tests/swfd_cases.py (checked on the CPU by
tests/test_swfd_cases_host.py).  Parity unpinned, as for every SWFD test: the specification is oracle/swfd_oracle.py."""
import ctypes as C

import numpy as np
import pytest

import swfd_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SWITCHES = ("MUSED_SWFD_DEDUPE", "MUSED_SWFD_LIST", "MUSED_SWFD_ORDERS", "MUSED_SWFD_KACT", "MUSED_SWFD_SKIP_DEAD",
            "MUSED_SWFD_GRAM_SPLIT", "MUSED_SWFD_PREROT", "MUSED_SWFD_PREROT_SWEEPS", "MUSED_EIG_TRD")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(N, R, d, l, **kw):
    from mused_amd.swfd import SeqBasedSWFD

    return SeqBasedSWFD(N=N, R=R, d=d, sketch_dim=l, **kw)


def _case_dev(name, **kw):
    c = sc.CASES[name]
    return _dev(c.N, sc.case_stream(name)[1], c.d, c.l, **kw)


def _raw(sk, kind):
    return sk.export_half(kind).cpu().numpy()


def _halves(sk):
    return [sc.parse_half(_raw(sk, k), sk.L, sk.ell, sk.d) for k in (0, 1)]


def _same_get(a, b):
    return sc.same_bits(a[0], b[0]) and sc.same_bits(a[1], b[1]) and a[2] == b[2] and sc.same_bits(a[3], b[3])


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()     # (a copy: the shared streams are read only)


def _append_raw(sk, t, dtype, n_rows, ld, lane_stride=None):
    """Straight through the C ABI: rows at t's address with the given pitch (elements; 64-bit words for bit rows)."""
    from mused_amd._lib import call
    from mused_amd.engine import ptr, stream_ptr

    if lane_stride is None:
        call("mused_swfd_append", sk._h, ptr(t), dtype, n_rows, ld, stream_ptr())
    else:
        call("mused_swfd_append_lanes", sk._h, ptr(t), dtype, n_rows, ld, lane_stride, stream_ptr())
    sk._keepalive = t


def _clean_env(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


# ---- a. every sketch's state equals the specification's ---------------------------------------------------------------
def _check_state(dev, state, tag, skip_frozen):
    got = sc.compare_get(dev, state["get"], tag)
    pend = state["pending"]
    p = len(pend)
    for kind, (dev_half, ora_half) in enumerate(zip(_halves(dev), state["halves"])):
        for j, (lv, o) in enumerate(zip(dev_half, ora_half)):
            if kind == 0 and skip_frozen and j in state["frozen"]:
                continue
            where = f"{tag} kind {kind} level {j}"
            nk = lv["nk"]
            slots = sc.ring_slots(lv)
            assert nk == len(o["K"]), where
            assert lv["count"] == len(o["qt"]), where
            assert [int(x) for x in lv["qt"][slots]] == o["qt"], where
            assert lv["dropped"] == o["dropped"], where
            tol = 1e-8 * o["lam_max"]
            K = lv["buf"][:nk]
            np.testing.assert_allclose(K.T @ K, o["K"].T @ o["K"], rtol=0, atol=tol, err_msg=where)
            for ts in sorted(set(o["qt"])):
                vd = lv["ring"][[s for s in slots if lv["qt"][s] == ts]]
                vo = o["qv"][[q for q, t in enumerate(o["qt"]) if t == ts]]
                np.testing.assert_allclose(vd.T @ vd, vo.T @ vo, rtol=0, atol=tol, err_msg=f"{where} snapshots of t={ts}")
            assert sc.same_bits(lv["buf"][nk:nk + p], pend), where            # the pending rows: raw, bit for bit
            assert not sc.bits(lv["buf"][nk + p:]).any(), where               # +0.0 behind them
    return got


def _run_against_trace(name, skip_frozen):
    X, _ = sc.case_stream(name)
    _, trace = sc.oracle_trace(name)
    dev = _case_dev(name)
    assert dev.L == len(trace[0]["halves"][0])
    t = 0
    for b, state in zip(sc.case_blocks(name), trace):
        dev.fit(_cuda(X[t:t + b]))
        t += b
        assert dev.rows_seen == state["i"] == t
        _check_state(dev, state, f"{name} t={t}", skip_frozen)
    dev.close()


@pytest.mark.parametrize("name", ["l4", "l3_odd", "l6_ragged_epoch", "l8", "l2_d1", "l8_d5", "N5_l8"])
def test_every_sketch_state_equals_the_specification(name, monkeypatch):
    """After every block: get() by the rule of test_gpu_path.py, then for all 2 L sketches the kept-row count, the ring
    (count, timestamps from `head`), `dropped` exactly; the Gram matrix of the kept rows and, per timestamp, the sum of
    v v^T over its snapshots within 1e-8 of the sketch's largest lam0 so far; pending rows bit for bit, +0.0 behind them.
    MAIN levels the device has frozen (swfd_rep_kernel) are skipped."""
    _clean_env(monkeypatch)
    _run_against_trace(name, skip_frozen=True)


def test_every_sketch_state_with_nothing_frozen(monkeypatch):
    """MUSED_SWFD_SKIP_DEAD=0: every MAIN level keeps rotating and must equal the specification too."""
    _clean_env(monkeypatch, MUSED_SWFD_SKIP_DEAD="0")
    _run_against_trace("l4", skip_frozen=False)


def test_l1_and_a_query_before_any_row_are_zero(monkeypatch):
    _clean_env(monkeypatch)
    for name in ("l1", "l4", "l3_odd", "l2_d1"):
        dev = _case_dev(name)
        B, sig, lvl, delta = dev.get()          # (get() raises on a non-zero status word)
        assert not sc.bits(B).any() and not sc.bits(sig).any() and lvl == 0 and delta == 0.0, name
        dev.close()
    X, _ = sc.case_stream("l1")
    _, trace = sc.oracle_trace("l1")
    dev = _case_dev("l1")
    t = 0
    for b, state in zip(sc.case_blocks("l1"), trace):
        dev.fit(_cuda(X[t:t + b]))
        t += b
        B, sig, lvl, delta = sc.compare_get(dev, state["get"], f"l1 t={t}")
        assert not B.any() and not sig.any() and lvl == 0 and delta == 0.0
    for half in _halves(dev):
        for lv in half:
            assert lv["nk"] == 0 and lv["count"] == 0 and lv["dropped"] == 0 and not sc.bits(lv["buf"]).any()
    dev.close()


# ---- b. row sources give the same bits -----------------------------------------------------------------------------------
def _binary_stream(n, d, seed):
    Z = (np.random.default_rng(seed).random((n, d)) < 0.1).astype(np.float64)
    return Z


def _pack_bits(Z, pitch, junk):
    """0/1 rows as bitmask rows of `pitch` 64-bit words (bit c of a row = element c); junk: every bit behind column d and
    every padding word set."""
    n, d = Z.shape
    full = np.ones((n, pitch * 64), dtype=np.uint8) if junk else np.zeros((n, pitch * 64), dtype=np.uint8)
    full[:, :d] = Z
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.int64)


def _pitched(Z, dtype, fill):
    n, d = Z.shape
    T = torch.full((n, d + 3), fill, dtype=dtype, device="cuda")
    T[:, :d] = torch.from_numpy(Z).to(dtype).cuda()
    return T


@pytest.mark.parametrize("d", [63, 64, 65, 130])
def test_row_sources_give_the_same_bits(d, monkeypatch):
    """One 0/1 stream (exact in every type), N = d as SWFDMC wires it: pitched F64 / F32 / I64 rows with NaN / INT64_MIN in
    the padding, bit rows at the minimal pitch and at a wider one with every unused bit set == contiguous F64 rows, bit
    for bit in get() and in both exported halves, inside a block and at the end."""
    from mused_amd._lib import BITS

    _clean_env(monkeypatch)
    l, N = 4, d
    n = 2 * N + 7
    Z = _binary_stream(n, d, d)
    R = max(float(Z.sum(1).max()), 1.0)
    cuts = [0, 37, n]                      # 37 rows: inside a block of l = 4
    w = (d + 63) // 64
    Zd = _cuda(Z)
    f64p, f32p = _pitched(Z, torch.float64, float("nan")), _pitched(Z, torch.float32, float("nan"))
    i64p = _pitched(Z, torch.int64, torch.iinfo(torch.int64).min)
    tight, wide = _cuda(_pack_bits(Z, w, False)), _cuda(_pack_bits(Z, w + 2, True))
    sources = {
        "f64": lambda sk, a, b: sk.fit(Zd[a:b]),
        "f64 pitched": lambda sk, a, b: sk.fit(f64p[a:b, :d]),
        "f32 pitched": lambda sk, a, b: sk.fit(f32p[a:b, :d]),
        "i64 pitched": lambda sk, a, b: sk.fit(i64p[a:b, :d]),
        "bits": lambda sk, a, b: _append_raw(sk, tight[a:b], BITS, b - a, w),
        "bits wide junk": lambda sk, a, b: _append_raw(sk, wide[a:b], BITS, b - a, w + 2),
    }
    assert f64p[:, :d].stride(0) == d + 3 and not f64p[:, :d].is_contiguous()
    ref = None
    for tag, feed in sources.items():
        sk = _dev(N, R, d, l)
        out = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            feed(sk, a, b)
            out.append((sk.get(), _raw(sk, 0), _raw(sk, 1)))
        assert sk.rows_seen == n
        sk.close()
        if ref is None:
            ref = out
            assert ref[-1][0][1][0] > 0.0          # (the sketch is not empty)
            continue
        for (g, m, a_), (g0, m0, a0) in zip(out, ref):
            assert _same_get(g, g0), (d, tag)
            assert np.array_equal(m, m0) and np.array_equal(a_, a0), (d, tag)


def test_lanes_from_strided_views_equal_single_sketches(monkeypatch):
    """lanes = 3 fed from views of larger tensors (lane_stride is not n * ld), F64 and bit rows, one lane all zero for its
    first N rows: every lane equals its single sketch bit for bit."""
    from mused_amd._lib import BITS

    _clean_env(monkeypatch)
    d, l, B = 65, 4, 3
    N = d
    n = 2 * N + 7
    Z = np.stack([_binary_stream(n, d, 200 + b) for b in range(B)])
    Z[1, :N] = 0.0
    R = max(float(Z.sum(2).max()), 1.0)
    w = (d + 63) // 64
    big = torch.full((B, n + 5, d + 3), float("nan"), dtype=torch.float64, device="cuda")
    big[:, 2:2 + n, :d] = _cuda(Z)
    view = big[:, 2:2 + n, :d]
    assert view.stride(0) != n * view.stride(1)
    bigm = torch.full((B, n + 5, w + 2), -1, dtype=torch.int64, device="cuda")
    bigm[:, 2:2 + n] = _cuda(np.stack([_pack_bits(Z[b], w + 2, True) for b in range(B)]))
    singles = [_dev(N, R, d, l) for _ in range(B)]
    lanes_f, lanes_b = _dev(N, R, d, l, lanes=B), _dev(N, R, d, l, lanes=B)
    for a, b in [(0, 37), (37, n)]:
        lanes_f.fit_lanes(view[:, a:b])
        _append_raw(lanes_b, bigm[:, 2 + a:2 + b], BITS, b - a, w + 2, lane_stride=(n + 5) * (w + 2))
        for k in range(B):
            singles[k].fit(_cuda(Z[k, a:b]))
        for tag, lanes in (("f64", lanes_f), ("bits", lanes_b)):
            Bl, sl, ll, dl = lanes.get()
            for k in range(B):
                assert _same_get((Bl[k], sl[k], int(ll[k]), dl[k]), singles[k].get()), (tag, k, b)
    assert singles[0].get()[1][0] > 0.0
    for sk in singles + [lanes_f, lanes_b]:
        sk.close()


# ---- c. batching invariance on the device --------------------------------------------------------------------------------
def test_any_batching_gives_the_same_sketch_on_the_device(monkeypatch):
    """Per-row appends, one call, ragged blocks and NumPy rows staged 7 at a time: identical bits of get() and of both
    halves at every epoch end and at the end (N = 100 is no multiple of l = 6)."""
    _clean_env(monkeypatch)
    name = "l6_ragged_epoch"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    n = len(X)
    Xd = _cuda(X)
    cps = [c.N, 2 * c.N, 3 * c.N, 4 * c.N, n]

    def record(sk):
        return sk.get(), _raw(sk, 0), _raw(sk, 1)

    def per_row():
        sk, out, t = _case_dev(name), [], 0
        for cp in cps:
            for r in range(t, cp):
                sk.fit(Xd[r:r + 1])
            t = cp
            out.append(record(sk))
        sk.close()
        return out

    def one_call():
        out = []
        for cp in cps:
            sk = _case_dev(name)
            sk.fit(Xd[:cp])
            out.append(record(sk))
            sk.close()
        return out

    def ragged():
        sk, out, t = _case_dev(name), [], 0
        ends = sorted(set(np.cumsum(sc.case_blocks(name)).tolist()) | set(cps))
        for e in ends:
            sk.fit(Xd[t:e])
            t = e
            if e in cps:
                out.append(record(sk))
        sk.close()
        return out

    def staged_numpy():
        sk, out, t = _case_dev(name, stage_rows=7), [], 0
        for cp in cps:
            sk.fit(X[t:cp])
            t = cp
            out.append(record(sk))
        sk.close()
        return out

    ref = per_row()
    for tag, way in (("one call", one_call), ("ragged", ragged), ("numpy staged", staged_numpy)):
        for cp, (g, m, a), (g0, m0, a0) in zip(cps, way(), ref):
            assert _same_get(g, g0), (tag, cp)
            assert np.array_equal(m, m0) and np.array_equal(a, a0), (tag, cp)


# ---- d. switches ------------------------------------------------------------------------------------------------------------
def _orders(sk):
    from mused_amd import _lib

    st = (C.c_longlong * 18)()
    fn = _lib.lib().mused_swfd_debug_orders
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p]
    return list(st) if fn(sk._h, st) == 1 else None


_RUNS = {}


def _run(name, monkeypatch, **env):
    """The case's ragged blocks under the given switches: ([(get, MAIN blob, AUX blob) after every block], order counts).
    The default configuration runs once per case."""
    key = (name, tuple(sorted(env.items())))
    if key in _RUNS:
        return _RUNS[key]
    with monkeypatch.context() as m:
        _clean_env(m, **env)
        sk = _case_dev(name)
    X, _ = sc.case_stream(name)
    out, t = [], 0
    for b in sc.case_blocks(name):
        sk.fit(_cuda(X[t:t + b]))
        t += b
        out.append((sk.get(), _raw(sk, 0), _raw(sk, 1)))
    res = (out, _orders(sk))
    sk.close()
    if not env:
        _RUNS[key] = res
    return res


def _report(tag, run, ref):
    dev = max(np.abs(g[0].T @ g[0] - g0[0].T @ g0[0]).max() / max(g0[1][0] ** 2, 1e-300) for (g, _, _), (g0, _, _) in zip(run, ref))
    same = all(_same_get(g, g0) for (g, _, _), (g0, _, _) in zip(run, ref))
    print(f"SWITCH {tag}: max |B^T B - default| / sigma_1^2 = {dev:.3e}; get() bit-identical to the default: {same}")


def _against_oracle(name, run, tag):
    _, trace = sc.oracle_trace(name)
    assert len(run) == len(trace)
    for (g, _, _), state in zip(run, trace):
        sc.compare_get(g, state["get"], f"{tag} t={state['i']}")


@pytest.mark.parametrize("switch", ["MUSED_SWFD_LIST", "MUSED_SWFD_DEDUPE", "MUSED_SWFD_SKIP_DEAD"])
def test_exact_switches_change_no_bit(switch, monkeypatch):
    """The switches csrc/swfd.hip states to be exact: get() after every block and the AUX half are bit-identical to the
    default configuration.  MUSED_SWFD_SKIP_DEAD=0: the MAIN half differs on frozen levels, and only there."""
    ref, _ = _run("l8", monkeypatch)
    run, _ = _run("l8", monkeypatch, **{switch: "0"})
    _, trace = sc.oracle_trace("l8")
    c = sc.CASES["l8"]
    L = len(trace[0]["halves"][0])
    frozen_differs = False
    for (g, m, a), (g0, m0, a0), state in zip(run, ref, trace):
        assert _same_get(g, g0), (switch, state["i"])
        assert np.array_equal(a, a0), (switch, state["i"])
        if switch != "MUSED_SWFD_SKIP_DEAD":
            continue
        for j, (lv, lv0) in enumerate(zip(sc.parse_half(m, L, c.l, c.d), sc.parse_half(m0, L, c.l, c.d))):
            same = (all(np.array_equal(np.asarray(lv[k]), np.asarray(lv0[k])) for k in lv)
                    and sc.same_bits(lv["buf"], lv0["buf"]) and sc.same_bits(lv["ring"], lv0["ring"]))
            if j in state["frozen"]:
                frozen_differs |= not same
            else:
                assert same, (state["i"], j)
    if switch == "MUSED_SWFD_SKIP_DEAD":
        assert frozen_differs        # (else nothing was ever frozen: the switch was not exercised)


@pytest.mark.parametrize("env", [{"MUSED_SWFD_KACT": "0"}, {"MUSED_SWFD_PREROT": "1"}, {"MUSED_EIG_TRD": "0"}],
                         ids=["KACT=0", "PREROT=1", "EIG_TRD=0"])
def test_switches_stay_within_the_specification(env, monkeypatch):
    """Every block against the specification by the rule of test_gpu_path.py; the deviation from the default configuration
    is printed, not asserted.  MUSED_EIG_TRD=0 is the Jacobi configuration (pre-rotation on by default)."""
    tag = " ".join(f"{k}={v}" for k, v in env.items())
    ref, _ = _run("l8", monkeypatch)
    run, _ = _run("l8", monkeypatch, **env)
    _against_oracle("l8", run, tag)
    _report(tag, run, ref)


def test_gram_split_with_a_narrow_last_chunk(monkeypatch):
    """MUSED_SWFD_GRAM_SPLIT=4 at d = 100: k-chunks of 32 columns, the last one 4 wide (production splits at d >= 8192 only)."""
    ref, _ = _run("split_d100", monkeypatch)
    run, _ = _run("split_d100", monkeypatch, MUSED_SWFD_GRAM_SPLIT="4")
    _against_oracle("split_d100", ref, "split_d100 default")
    _against_oracle("split_d100", run, "GRAM_SPLIT=4")
    _report("MUSED_SWFD_GRAM_SPLIT=4", run, ref)


def test_orders_switch_at_l128(monkeypatch):
    """MUSED_SWFD_ORDERS = 0 / 1 / 32 against the default (offsets rounded to 16) at l = 128, d = 40: every block within the
    specification, and the histogram of the orders solved shows that the switch acted: 0 solves everything at order 256,
    32 moves solves into higher buckets.  The buckets are 16 orders wide, (16 b, 16 b + 16]: exact offsets (1) fall into
    the buckets of the default by construction, so that histogram is asserted EQUAL."""
    name = "l128_d40"
    ref, h16 = _run(name, monkeypatch)
    _against_oracle(name, ref, "ORDERS default")
    hist = {"16": h16}
    for v in ("0", "1", "32"):
        run, hist[v] = _run(name, monkeypatch, MUSED_SWFD_ORDERS=v)
        _against_oracle(name, run, f"ORDERS={v}")
        _report(f"MUSED_SWFD_ORDERS={v}", run, ref)
    for v, h in hist.items():
        print(f"ORDERS={v}: rotations {h[0]}, solves {h[1]}, by order bucket {h[2:]}")
        assert h[0] == hist["16"][0] and h[1] == hist["16"][1] and sum(h[2:]) == h[1]
    assert hist["0"][2:] == [0] * 15 + [hist["0"][1]]
    assert hist["16"][2:] != hist["0"][2:] and hist["32"][2:] != hist["0"][2:] and hist["32"][2:] != hist["16"][2:]
    assert hist["1"][2:] == hist["16"][2:]


@pytest.mark.parametrize("env", [{"MUSED_SWFD_PREROT": "1"}, {"MUSED_EIG_TRD": "0"}], ids=["PREROT=1", "EIG_TRD=0"])
def test_prerotation_block_boundaries(env, monkeypatch):
    """Pre-rotation on (N = 90, l = 8): an append that ends inside a block, so that the next call completes the block from raw
    rows before its pre-rotated blocks; an append over an epoch end whose last block is short (2 rows, zero padded) and
    that ends inside the first block of the next epoch."""
    from oracle.swfd_oracle import SeqBasedSWFD as Ora

    c = sc.CASES["l8"]
    X, R = sc.case_stream("l8")
    with monkeypatch.context() as m:
        _clean_env(m, **env)
        dev = _case_dev("l8")
    ora = Ora(N=c.N, R=R, d=c.d, sketch_dim=c.l)
    t = 0
    for b in [5, 19, 56, 16, 90, 100, len(X) - 286]:
        dev.fit(_cuda(X[t:t + b]))
        ora.fit(X[t:t + b])
        t += b
        sc.compare_get(dev, ora, f"{env} t={t}")
    assert t == len(X)
    dev.close()


# ---- e. state exchange ------------------------------------------------------------------------------------------------------
def test_hand_over_chain_equals_the_sequential_sketch(monkeypatch):
    """Four handles, one epoch each (N = 100 is no multiple of l = 6), every one started from the AUX half of its
    predecessor: the last one's get() equals the sequential sketch bit for bit, and so does its MAIN half on every level
    that is not frozen."""
    _clean_env(monkeypatch)
    name = "l6_ragged_epoch"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    Xd = _cuda(X)
    seq = _case_dev(name)
    blob, chain = None, []
    for e in range(4):
        seq.fit(Xd[e * c.N:(e + 1) * c.N])
        sk = _case_dev(name)
        sk.begin_epoch(e * c.N, blob)
        sk.fit(Xd[e * c.N:(e + 1) * c.N])
        assert sk.rows_seen == (e + 1) * c.N
        blob = sk.export_half(1)
        chain.append(sk)
        assert _same_get(sk.get(), seq.get()), e
    last = chain[-1]
    main_seq, main_last = _halves(seq)[0], _halves(last)[0]
    frozen = {j for j in range(seq.L - 1) if main_seq[j]["dropped"] > 3 * c.N}
    assert frozen and len(frozen) < seq.L - 1        # (both kinds of level are there)
    for j in range(seq.L):
        if j not in frozen:
            assert sc.live_equal(main_last[j], main_seq[j]), j
    aux_seq, aux_last = _halves(seq)[1], _halves(last)[1]
    assert all(sc.live_equal(a, b) for a, b in zip(aux_last, aux_seq))
    for sk in chain + [seq]:
        sk.close()


def test_begin_epoch_zero_resets_a_used_handle(monkeypatch):
    """begin_epoch(0) without a blob on a handle that has seen 2 N rows == a fresh handle, bit for bit."""
    _clean_env(monkeypatch)
    name = "l4"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    used, fresh = _case_dev(name), _case_dev(name)
    used.fit(_cuda(X[::-1][:2 * c.N]))
    used.get()
    used.begin_epoch(0)
    assert used.rows_seen == 0
    t = 0
    for b in sc.case_blocks(name):
        if t >= 2 * c.N + 13:
            break
        used.fit(_cuda(X[t:t + b]))
        fresh.fit(_cuda(X[t:t + b]))
        t += b
        assert _same_get(used.get(), fresh.get()), t
        for hu, hf in zip(_halves(used), _halves(fresh)):
            assert all(sc.live_equal(a, b_) for a, b_ in zip(hu, hf)), t
    used.close()
    fresh.close()


def test_import_half_round_trip(monkeypatch):
    """Both halves of A, exported in its second epoch on a rotation boundary, imported into B, which has seen as many
    DIFFERENT rows: from there on the same rows give the same bits."""
    _clean_env(monkeypatch)
    name = "l6_ragged_epoch"
    c = sc.CASES[name]
    X, _ = sc.case_stream(name)
    t = c.N + 5 * c.l
    A, Bk = _case_dev(name), _case_dev(name)
    A.fit(_cuda(X[:t]))
    Bk.fit(_cuda(X[::-1][:t]))              # (the same rows in another order: the same R bound)
    assert not _same_get(A.get(), Bk.get())
    for kind in (0, 1):
        Bk.import_half(kind, A.export_half(kind))
    assert Bk.rows_seen == A.rows_seen == t
    assert _same_get(A.get(), Bk.get())
    for b in sc.blocks(c.l, 2 * c.N):
        A.fit(_cuda(X[t:t + b]))
        Bk.fit(_cuda(X[t:t + b]))
        t += b
        assert _same_get(A.get(), Bk.get()), t
    for ha, hb in zip(_halves(A), _halves(Bk)):
        assert all(sc.live_equal(a, b_) for a, b_ in zip(ha, hb))
    A.close()
    Bk.close()


def test_argument_errors_change_nothing(monkeypatch):
    from mused_amd._lib import BITS, F64, MusedError

    _clean_env(monkeypatch)
    d, l = 130, 4
    N = d
    Z = _binary_stream(N + 30, d, 7)
    R = max(float(Z.sum(1).max()), 1.0)
    sk, lanes = _dev(N, R, d, l), _dev(N, R, d, l, lanes=2)
    Zd = _cuda(Z)
    sk.fit(Zd)
    lanes.fit_lanes(torch.stack([Zd, Zd.flip(0)]))
    blob = sk.export_half(1)
    mask = _cuda(_pack_bits(Z, 3, False))

    def unchanged(h, rows, before, what):
        assert h.rows_seen == rows, what
        after = h.get()
        assert all(sc.same_bits(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)) for x, y in zip(after, before)), what

    before, before_l = sk.get(), lanes.get()
    state = [_raw(sk, 0), _raw(sk, 1)]
    errors = [
        ("begin_epoch off an epoch boundary", MusedError, lambda: sk.begin_epoch(N + 1, blob)),
        ("begin_epoch without a blob off an epoch boundary", MusedError, lambda: sk.begin_epoch(N - 1)),
        ("begin_epoch with a short blob", ValueError, lambda: sk.begin_epoch(N, blob[:-1])),
        ("import_half with a short blob", ValueError, lambda: sk.import_half(0, blob[:-1])),
        ("export_half kind 2", MusedError, lambda: sk.export_half(2)),
        ("import_half kind -1", MusedError, lambda: sk.import_half(-1, blob)),
        ("bit rows with a pitch of 2 words", MusedError, lambda: _append_raw(sk, mask, BITS, 4, 2)),
        ("rows with a pitch of d - 1", MusedError, lambda: _append_raw(sk, Zd, F64, 4, d - 1)),
        ("unknown dtype", MusedError, lambda: _append_raw(sk, Zd, 7, 4, d)),
    ]
    for what, exc, fn in errors:
        with pytest.raises(exc):
            fn()
        unchanged(sk, N + 30, before, what)
    assert np.array_equal(_raw(sk, 0), state[0]) and np.array_equal(_raw(sk, 1), state[1])
    lane_blob = torch.zeros(lanes.half_bytes(), dtype=torch.uint8, device="cuda")
    for what, fn in [("export_half on two lanes", lambda: lanes.export_half(0)),
                     ("import_half on two lanes", lambda: lanes.import_half(1, lane_blob)),
                     ("begin_epoch with a blob on two lanes", lambda: lanes.begin_epoch(N, lane_blob))]:
        with pytest.raises(MusedError):
            fn()
        unchanged(lanes, N + 30, before_l, what)
    sk.close()
    lanes.close()
