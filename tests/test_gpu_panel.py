"""On the GPU: the LU and Householder panel kernels (csrc/panel.hip) through mused_lu_permute_l and mused_qr_economic, against
tests/panel_cases.py -- the structure of P L, its backward error, the pivot order (pivstep, the first n words of ws_int) and, on
the exact cases, the bits of the plain restatement; orthogonality, span, triangularity and the sign convention of Q; every case
once with pitch r and once with a wider pitch whose padding is NaN, with guard words behind the panel and both workspaces;
2^200 and 2^-200 times the panel; the column-at-a-time (MUSED_LU_BLOCKED=0) and one-launch-per-column (MUSED_LU_MODE=2)
variants in a fresh child each, bit for bit against the default blocked one; the chain through mused_rsvd_reduce where it
enters panel.hip; and the argument checks of the two entries."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import panel_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64
SENT = -12345.678
INT_SENT = -7
LU_PAD, QR_PADY, QR_PADQ = 3, 3, 5
PITCHES = ("tight", "padded")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    _LU.clear()
    _QR.clear()


def P(t):
    return C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pitched(Y, pad):
    """the panel in a buffer of pitch r + pad with NaN behind every row and one more row of NaN"""
    n, r = Y.shape
    buf = np.full((n + 1, r + pad), np.nan)
    buf[:n, :r] = Y
    return torch.from_numpy(buf).cuda()


def outside_untouched(buf, n, r):
    a = buf.cpu().numpy()
    assert np.isnan(a[:n, r:]).all() and np.isnan(a[n]).all(), "written outside the n x r panel"
    return a[:n, :r]


def guarded(n_words, dtype, sent):
    return torch.full((n_words + GUARD,), sent, dtype=dtype, device="cuda")


def guard_untouched(t, n_words, sent, what):
    assert bool((t[n_words:] == sent).all()), f"written behind {what}"


def lu_device(Y, pad):
    """mused_lu_permute_l: (PL[:, :k], pivstep) of the device, with the workspaces sized exactly as the header documents"""
    from mused_amd import _lib

    n, r = Y.shape
    k = min(n, r)
    dY = pitched(Y, pad)
    ni, nf = n + (n + 15) // 16, 4 * (r + n)
    wi, wf = guarded(ni, torch.int32, INT_SENT), guarded(nf, torch.float64, SENT)
    _lib.call("mused_lu_permute_l", P(dY), n, r, r + pad, P(wi), P(wf), S())
    torch.cuda.synchronize()
    out = outside_untouched(dY, n, r)
    guard_untouched(wi, ni, INT_SENT, "ws_int")
    guard_untouched(wf, nf, SENT, "ws_f64")
    return np.ascontiguousarray(out[:, :k]), wi[:n].cpu().numpy()


def qr_device(Y, pady, padq):
    """mused_qr_economic: Q of the device; Y may be destroyed, nothing else may change"""
    from mused_amd import _lib

    n, r = Y.shape
    dY, dQ = pitched(Y, pady), pitched(np.full((n, r), 7.0), padq)
    nf = r + ((n + 511) // 512) * r + 2 * n
    wf = guarded(nf, torch.float64, SENT)
    _lib.call("mused_qr_economic", P(dY), n, r, r + pady, P(dQ), r + padq, P(wf), S())
    torch.cuda.synchronize()
    outside_untouched(dY, n, r)
    guard_untouched(wf, nf, SENT, "ws_f64")
    return np.ascontiguousarray(outside_untouched(dQ, n, r))


_LU, _QR = {}, {}


def lu_run(c, pitch):
    """the default-mode result of a case, computed once (read-only)"""
    if (c.name, pitch) not in _LU:
        out = lu_device(pc.panel(c), LU_PAD if pitch == "padded" else 0)
        for a in out:
            a.setflags(write=False)
        _LU[c.name, pitch] = out
    return _LU[c.name, pitch]


def qr_run(c, pitch):
    if (c.name, pitch) not in _QR:
        Q = qr_device(pc.panel(c), *((QR_PADY, QR_PADQ) if pitch == "padded" else (0, 0)))
        Q.setflags(write=False)
        _QR[c.name, pitch] = Q
    return _QR[c.name, pitch]


def show(name, ratios, restated):
    print(f"{name}: " + " ".join(f"{k} {v:.3g} (device / restatement {v / restated[k]:.3g})" if restated.get(k) else f"{k} {v:.3g}"
                                 for k, v in ratios.items()))


# ---- LU --------------------------------------------------------------------------------------------------------------
def test_default_mode_runs_the_routes_the_table_names():
    from mused_amd import _lib

    L = _lib.lib()
    assert L.mused_lu_mode() == 1, "MUSED_LU_MODE / MUSED_LU_BLOCKED are set: this file needs the default"
    for c in pc.LU_TABLE:
        assert L.mused_lu_path(c.n, c.r) == (0 if pc.lu_route(c) == "column" else 1), c.name


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("c", pc.LU_TABLE, ids=pc.LU_IDS)
def test_lu_case(c, pitch):
    PL, ps = lu_run(c, pitch)
    ratios, bad = pc.lu_verdict(c, PL, ps)
    show(f"{c.name} {pitch}", ratios, {"backward": pc.lu_backward_ratio(pc.panel(c), *pc.lu_restated(c))})
    assert not bad, bad


def test_lu_pitch_does_not_change_a_bit():
    for c in pc.LU_TABLE:
        a, b = lu_run(c, "tight"), lu_run(c, "padded")
        assert np.array_equal(pc.bits(a[0]), pc.bits(b[0])) and np.array_equal(a[1], b[1]), c.name


@pytest.mark.parametrize("c", pc.LU_SCALED, ids=[c.name for c in pc.LU_SCALED])
def test_lu_is_scale_invariant(c):
    PL, ps = lu_run(c, "tight")
    for s in pc.SCALES:
        PLs, pss = lu_device(pc.panel(c) * s, 0)
        assert np.array_equal(pss, ps) and np.array_equal(pc.bits(PLs), pc.bits(PL)), (c.name, s)


def _child(out):
    """the whole LU table at both pitches in this process's LU variant"""
    from mused_amd import _lib

    res = {"mode": np.array(_lib.lib().mused_lu_mode())}
    for c in pc.LU_TABLE:
        res[c.name + "_path"] = np.array(_lib.lib().mused_lu_path(c.n, c.r))
        for pitch in PITCHES:
            res[f"{c.name}_{pitch}_PL"], res[f"{c.name}_{pitch}_ps"] = lu_device(pc.panel(c), LU_PAD if pitch == "padded" else 0)
    np.savez(out, **res)


@pytest.mark.parametrize("var,value,mode", [("MUSED_LU_BLOCKED", "0", 0), ("MUSED_LU_MODE", "2", 2)])
def test_variant_gives_the_blocked_kernels_bits(tmp_path, var, value, mode):
    """csrc/panel.hip promises that the column-at-a-time, blocked and one-launch-per-column variants are bit-identical.  The
    variant is read once per process, so the other two run in a fresh child each, started once.  At n = 10,241 the default
    itself runs the column-at-a-time kernels (mused_lu_path == 0): those cases are compared like every other."""
    from mused_amd import _lib

    out = str(tmp_path / f"lu_mode{mode}.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("MUSED_LU_BLOCKED", "MUSED_LU_MODE")}
    env[var] = value
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    z = np.load(out)
    assert int(z["mode"]) == mode, "the child did not run the variant it was started for"
    assert any(_lib.lib().mused_lu_path(c.n, c.r) == 0 for c in pc.LU_TABLE)
    for c in pc.LU_TABLE:
        assert int(z[c.name + "_path"]) == mode, c.name
        for pitch in PITCHES:
            PL, ps = lu_run(c, pitch)
            assert np.array_equal(z[f"{c.name}_{pitch}_ps"], ps), f"{c.name} {pitch}: another pivot order"
            assert np.array_equal(pc.bits(z[f"{c.name}_{pitch}_PL"]), pc.bits(PL)), f"{c.name} {pitch}: P L differs in its bits"


# ---- QR --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("c", pc.QR_TABLE, ids=pc.QR_IDS)
def test_qr_case(c, pitch):
    Q = qr_run(c, pitch)
    ratios, bad = pc.qr_verdict(c, Q)
    show(f"{c.name} {pitch}", ratios, pc.qr_ratios(pc.panel(c), pc.qr_restated(c)[0])[0])
    assert not bad, bad
    if c.data == "zeros":
        assert np.array_equal(Q, np.eye(c.n, c.r))


def test_qr_pitch_does_not_change_a_bit():
    for c in pc.QR_TABLE:
        assert np.array_equal(pc.bits(qr_run(c, "tight")), pc.bits(qr_run(c, "padded"))), c.name


@pytest.mark.parametrize("c", pc.QR_SCALED, ids=[c.name for c in pc.QR_SCALED])
def test_qr_is_scale_invariant(c):
    Q = qr_run(c, "tight")
    for s in pc.SCALES:
        assert np.array_equal(pc.bits(qr_device(pc.panel(c) * s, 0, 0)), pc.bits(Q)), (c.name, s)


# ---- the chain ---------------------------------------------------------------------------------------------------------
def _knn_window(n, d, k, eng):
    from mused_amd import matrix_operations as mo
    from oracle import mo_oracle as omo

    X = np.random.default_rng([n, 0]).standard_normal((n, d))
    return omo.create_adjacency_matrix(X, "", k), mo.adjacency_on_device(X, "", k, engine=eng)


@pytest.mark.parametrize("n_iter", [0, 1, 5])
def test_chain_in_lu_mode_on_a_full_rank_window(n_iter):
    """rsvd_mode "lu" (a mode-2 handle): LU after every product and the Householder QR, on a k-NN adjacency whose rank (292)
    is far above the r = 30 columns of the panel -- tests/test_gpu_path.py runs this handle on its rank-deficient window only."""
    from mused_amd.engine import WindowEngine
    from oracle import mo_oracle as omo

    e = WindowEngine(300)
    e.rsvd_mode = "lu"
    try:
        A, adj = _knn_window(300, 12, 10, e)
        assert np.linalg.matrix_rank(A) >= 30 + 100
        sig_o = omo.randomized_svd_reduce(A, 20, 3, n_iter=n_iter)[1]
        sig_d = e.svd_reduce(adj, 20, 3, n_iter=n_iter)[1].cpu().numpy()
        np.testing.assert_allclose(sig_d, sig_o, rtol=1e-9)
        assert e.rsvd_fallbacks == 0
    finally:
        e.close()


@pytest.mark.parametrize("n,d,k,reduced_dim", [(20, 6, 5, 15), (400, 12, 10, 280)], ids=["r_above_n", "r_above_286"])
def test_chain_default_mode_routes_into_the_panel_kernels(n, d, k, reduced_dim):
    """The default (Cholesky-QR) mode gives way to lu_permute_l / qr_economic where r = n_comp + 10 > n (25 columns in 20 rows:
    k = n, pitch r > rc from the second product on) and where r > 286 (290)."""
    from mused_amd.engine import WindowEngine
    from oracle import mo_oracle as omo

    e = WindowEngine(n)
    try:
        assert e.rsvd_mode == "cholqr"
        A, adj = _knn_window(n, d, k, e)
        n_comp = min(reduced_dim, n - 1)
        assert n_comp + 10 > (n if n < 100 else 286)
        info = {}
        sig_o = omo.randomized_svd_reduce(A, reduced_dim, 3, info=info)[1]
        sa = info["sigma_all"]
        assert sa[n_comp - 1] - sa[n_comp] > 1e-6 * sa[0], "the cut falls inside a multiple singular value: another seed"
        sig_d = e.svd_reduce(adj, reduced_dim, 3)[1].cpu().numpy()
        np.testing.assert_allclose(sig_d, sig_o, rtol=0, atol=1e-8 * sig_o[0])
    finally:
        e.close()


# ---- rejected arguments ------------------------------------------------------------------------------------------------
def test_argument_checks():
    from mused_amd import _lib

    L = _lib.lib()
    Y = torch.zeros(64, dtype=torch.float64, device="cuda")
    Q = torch.zeros(64, dtype=torch.float64, device="cuda")
    wi = torch.zeros(64, dtype=torch.int32, device="cuda")
    wf = torch.zeros(256, dtype=torch.float64, device="cuda")

    def lu(y, n, r, ld, i, f):
        return L.mused_lu_permute_l(y, n, r, ld, i, f, S()), L.mused_last_error().decode()

    def qr(y, n, r, ldy, q, ldq, f):
        return L.mused_qr_economic(y, n, r, ldy, q, ldq, f, S()), L.mused_last_error().decode()

    for args in [(P(Y), 8, 4, 3, P(wi), P(wf)), (P(Y), 8, 0, 4, P(wi), P(wf)), (P(Y), 0, 4, 4, P(wi), P(wf)),
                 (None, 8, 4, 4, P(wi), P(wf)), (P(Y), 8, 4, 4, None, P(wf)), (P(Y), 8, 4, 4, P(wi), None)]:
        code, msg = lu(*args)
        assert code != 0 and "mused_lu_permute_l" in msg, (args[1:4], msg)
    for args in [(P(Y), 8, 4, 3, P(Q), 4, P(wf)), (P(Y), 8, 4, 4, P(Q), 3, P(wf)), (P(Y), 3, 4, 4, P(Q), 4, P(wf)),
                 (P(Y), 8, 0, 4, P(Q), 4, P(wf)), (None, 8, 4, 4, P(Q), 4, P(wf)), (P(Y), 8, 4, 4, None, 4, P(wf)),
                 (P(Y), 8, 4, 4, P(Q), 4, None)]:
        code, msg = qr(*args)
        assert code != 0 and "mused_qr_economic" in msg, (args[1:4], msg)
    torch.cuda.synchronize()
    assert not Y.any() and not Q.any() and not wi.any() and not wf.any(), "a rejected call wrote something"
    assert L.mused_lu_permute_l(P(Y), 8, 4, 4, P(wi), P(wf), S()) == 0   # and the library goes on working
    torch.cuda.synchronize()


if __name__ == "__main__":
    _child(sys.argv[1])
