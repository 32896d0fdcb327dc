"""On the GPU: one Cholesky-QR pass of the eigenstep (csrc/rsvd.hip: gram_reduce_kernel, chol_kernel, trsm_rows_kernel,
panel_sub_kernel, the two-block path) through mused_rsvd_cholqr, against the rounding-error bounds of tests/cholqr_cases.py
evaluated in np.longdouble -- Gram, factor, solve, the projected second block, two passes as the final basis, the weak-pivot
word on either side of its line -- and the argument checks of the entry."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cholqr_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_MAX, R_MAX = 1000, 2 * cc.MAX_R
GUARD = 64
SENT = -12345.678
WEAK_SENT = -9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def P(t):
    return C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def create(n_max, r_max):
    from mused_amd import _lib

    h = C.c_void_p()
    _lib.call("mused_rsvd_create", n_max, r_max, 1, 0, C.byref(h))
    return h


@pytest.fixture(scope="module")
def handle():
    from mused_amd import _lib

    h = create(N_MAX, R_MAX)
    yield h
    _FIRST.clear()
    _lib.call("mused_rsvd_destroy", h)


def one_pass(h, Y):
    """mused_rsvd_cholqr on a contiguous n x r panel: (Q, G, L unpacked, weak) of the device, every output followed by a band
    of sentinels that must come back untouched."""
    from mused_amd import _lib

    n, r = Y.shape
    rb = r if r <= cc.MAX_R else r - r // 2
    dY = torch.from_numpy(np.array(Y, order="C")).cuda()
    sizes = (n * r, rb * rb, rb * (rb + 1) // 2)
    dQ, dG, dL = (torch.full((s + GUARD,), SENT, dtype=torch.float64, device="cuda") for s in sizes)
    dW = torch.full((1 + GUARD,), WEAK_SENT, dtype=torch.int32, device="cuda")
    _lib.call("mused_rsvd_cholqr", h, P(dY), n, r, P(dQ), P(dG), P(dL), P(dW), S())
    torch.cuda.synchronize()
    assert np.array_equal(dY.cpu().numpy(), Y), "the input panel was written to"
    outs = []
    for t, s in zip((dQ, dG, dL), sizes):
        a = t.cpu().numpy()
        assert np.all(a[s:] == SENT), "written behind an output"
        outs.append(a[:s])
    w = dW.cpu().numpy()
    assert np.all(w[1:] == WEAK_SENT)
    return outs[0].reshape(n, r), outs[1].reshape(rb, rb), cc.unpack(outs[2], rb), int(w[0])


_FIRST = {}


def run_pass(h, c):
    """the first pass of a case on the device, computed once (read-only)"""
    if c.name not in _FIRST:
        out = one_pass(h, cc.panel(c))
        for a in out[:3]:
            a.setflags(write=False)
        _FIRST[c.name] = out
    return _FIRST[c.name]


@pytest.mark.parametrize("c", cc.TABLE, ids=cc.IDS)
def test_one_pass_keeps_every_bound(handle, c):
    Y = cc.panel(c)
    Q, G, L, weak = run_pass(handle, c)
    assert np.isfinite(Q).all() and np.isfinite(G).all() and np.isfinite(L).all()
    assert np.array_equal(G, G.T), "the Gram is symmetric bit for bit"
    assert np.all(np.triu(L, 1) == 0)
    ratios = cc.pass_ratios(Y, Q, G, L)
    print(f"{c.name}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f" weak {weak}")
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert weak == int(c.weak)


@pytest.mark.parametrize("c", cc.SOUND, ids=[c.name for c in cc.SOUND])
def test_two_passes_make_the_final_basis(handle, c):
    Q1 = run_pass(handle, c)[0]
    Q, _, _, weak = one_pass(handle, Q1)
    assert weak == 0
    orth, restated = cc.orthogonality(Q), cc.restated_orthogonality(c)
    print(f"{c.name}: max |Q^T Q - I| = {orth:.3g} (fp64 restatement {restated:.3g}, bound {cc.yamamoto(c.n, c.r):.3g})")
    assert orth <= 4 * restated
    assert orth <= cc.yamamoto(c.n, c.r)


@pytest.mark.parametrize("c", cc.TWO_BLOCK, ids=[c.name for c in cc.TWO_BLOCK])
def test_first_block_equals_a_single_block_call(handle, c):
    """The first r // 2 columns go through the same kernels on the same numbers, with pitch r in the one call and pitch r // 2
    in the other: bit for bit the same."""
    r1 = c.blocks[0]
    Q = run_pass(handle, c)[0]
    Q1 = one_pass(handle, np.ascontiguousarray(cc.panel(c)[:, :r1]))[0]
    assert np.array_equal(Q[:, :r1].view(np.int64), Q1.view(np.int64))


def test_a_pass_is_reproducible_and_leaves_the_handle_usable(handle):
    c = next(c for c in cc.TABLE if c.name == "gauss_n333_r145")
    a = run_pass(handle, c)
    b = one_pass(handle, cc.panel(c))
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    assert a[3] == b[3]


def test_argument_checks(handle):
    from mused_amd import _lib

    Lib = _lib.lib()
    buf = torch.zeros(N_MAX * R_MAX + GUARD, dtype=torch.float64, device="cuda")
    w = torch.zeros(4, dtype=torch.int32, device="cuda")

    def rc(h, n, r):
        code = Lib.mused_rsvd_cholqr(h, P(buf), n, r, P(buf), P(buf), P(buf), P(w), S())
        return code, Lib.mused_last_error().decode()

    for n, r, word in [(10, 11, "r = 11 columns in n = 10 rows"), (N_MAX + 1, 5, "n_max"), (10, 0, "r = 0"), (0, 1, "n = 0")]:
        code, msg = rc(handle, n, r)
        assert code != 0 and "mused_rsvd_cholqr" in msg and word in msg, (n, r, msg)
    assert Lib.mused_rsvd_cholqr(handle, None, 10, 5, P(buf), P(buf), P(buf), P(w), S()) != 0
    small = create(64, 8)
    try:
        code, msg = rc(small, 64, 9)
        assert code != 0 and "r_max" in msg
        code, msg = rc(small, 65, 8)
        assert code != 0 and "n_max" in msg
        _lib.call("mused_rsvd_set_mode", small, 2)
        code, msg = rc(small, 64, 8)
        assert code != 0 and "mode 2" in msg
    finally:
        _lib.call("mused_rsvd_destroy", small)
    wide = create(300, 2 * cc.MAX_R + 1)
    try:
        code, msg = rc(wide, 300, 2 * cc.MAX_R + 1)
        assert code != 0 and str(2 * cc.MAX_R) in msg
    finally:
        _lib.call("mused_rsvd_destroy", wide)
    torch.cuda.synchronize()
