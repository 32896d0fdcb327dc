"""The order-256 direct eigensolver with a PER-MATRIX active order and a compacted list of the matrices to solve
(csrc/trd.hip: `offs`, `list`): a Gram matrix that is zero from row and column n on is solved as the order-n matrix it is,
in the same launch as matrices of other orders, and workgroup i of the batch serves matrix list[i]."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ACT = [128, 129, 143, 160, 200, 224, 255, 256]
NEED = 128
OFFS = [256 - max(n, NEED) for n in N_ACT]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def run_offs(Gs, offs=None, lst=None, rep=None, done_init=-1):
    """mused_debug_trd_offs on a batch: (G out, d, e, lam, res, done)."""
    from mused_amd import _lib
    from mused_amd.engine import ptr, stream_ptr

    fn = _lib.lib().mused_debug_trd_offs
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p]
    B = len(Gs)
    G = torch.from_numpy(np.ascontiguousarray(np.stack(Gs))).cuda()
    d = torch.zeros(B, 256, dtype=torch.float64, device="cuda")
    e = torch.zeros(B, 256, dtype=torch.float64, device="cuda")
    lam = torch.zeros(B, 128, dtype=torch.float64, device="cuda")
    res = torch.zeros(B, 128, dtype=torch.float64, device="cuda")
    done = torch.full((B,), done_init, dtype=torch.int32, device="cuda")
    dev = lambda a: None if a is None else torch.tensor(list(a), dtype=torch.int32, device="cuda")  # noqa: E731
    o, l, r = dev(offs), dev(lst), dev(rep)
    p = lambda t: None if t is None else ptr(t)  # noqa: E731
    _lib.check(fn(ptr(G), NEED, 0, B, ptr(d), ptr(e), ptr(lam), ptr(res), ptr(done), p(o), p(l), 0 if lst is None else len(lst),
                  p(r), stream_ptr()))
    torch.cuda.synchronize()
    return G.cpu().numpy(), d.cpu().numpy(), e.cpu().numpy(), lam.cpu().numpy(), res.cpu().numpy(), done.cpu().numpy()


@pytest.fixture(scope="module")
def batch():
    """Eight Gram matrices in the 256-layout: n_act random rows, then zero rows; the batch solved with every matrix at its own
    order, and LAPACK's spectra."""
    rng = np.random.default_rng(6)
    Gs = []
    for n in N_ACT:
        buf = np.zeros((256, 300))
        buf[:n] = rng.standard_normal((n, 300))
        Gs.append(buf @ buf.T)
    ref = [np.linalg.eigvalsh(G)[::-1] for G in Gs]
    return Gs, ref, run_offs(Gs, offs=OFFS)


def test_every_matrix_at_its_own_order_matches_lapack(batch):
    Gs, ref, (out, d, e, lam, res, done) = batch
    for b, (G, n_act, off) in enumerate(zip(Gs, N_ACT, OFFS)):
        n = 256 - off
        w = ref[b]
        scale = np.abs(w).max()
        assert done[b] == 1, (n_act, res[b].max())
        assert not d[b, :off].any() and not e[b, :off].any()                    # the skipped steps
        np.testing.assert_allclose(lam[b], w[:128], rtol=0, atol=1e-13 * scale)
        cols = out[b].T                                                            # (256, 256): column c
        nrm = np.linalg.norm(cols[:, :128], axis=0)
        np.testing.assert_allclose(nrm, np.maximum(w[:128], 0), rtol=0, atol=1e-12 * scale)
        assert not cols[n:, :128].any()                                            # rows behind the order: exact zeros
        assert not cols[:, 128:].any()                                             # columns behind the formed ones
        sig = (w[:128] - w[127]) > 1e-10 * w[0]
        V = cols[:, :128][:, sig] / nrm[sig]
        assert np.abs(V.T @ V - np.eye(V.shape[1])).max() < 1e-9
        assert np.abs(G @ V - V * w[:128][sig]).max() < 1e-11 * scale


def test_a_matrix_does_not_depend_on_its_batch(batch):
    Gs, _, full = batch
    for b in range(len(Gs)):
        one = run_offs([Gs[b]], offs=[OFFS[b]])
        for a_full, a_one in zip(full, one):
            assert np.array_equal(a_full[b], a_one[0]), (N_ACT[b],)


def test_offset_zero_equals_the_order_256_solver(batch):
    from mused_amd import _lib
    from mused_amd.engine import ptr, stream_ptr

    Gs, _, full = batch
    b = N_ACT.index(256)
    fn = _lib.lib().mused_debug_trd
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    G = torch.from_numpy(np.ascontiguousarray(Gs[b][None])).cuda()
    d, e = (torch.zeros(1, 256, dtype=torch.float64, device="cuda") for _ in range(2))
    lam, res = (torch.zeros(1, 128, dtype=torch.float64, device="cuda") for _ in range(2))
    done = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(fn(ptr(G), 1, ptr(d), ptr(e), ptr(lam), ptr(res), ptr(done), stream_ptr()))
    torch.cuda.synchronize()
    plain = [t.cpu().numpy() for t in (G, d, e, lam, res, done)]
    for a_full, a_plain in zip(full, plain):
        assert np.array_equal(a_full[b], a_plain[0])


def test_list_serves_the_listed_matrices_and_leaves_the_others(batch):
    """list = a permutation of a subset; matrix 2 is a duplicate of matrix 5 (rep[2] = 5) and matrix 6 a frozen sketch (rep = -1):
    neither is listed.  Listed matrices: the bits of the unlisted solve; unlisted ones untouched, the duplicate and the frozen
    one marked done (the Jacobi skips them), matrix 0 -- its own representative, but not listed -- not even that."""
    Gs, _, full = batch
    rep = [0, 1, 5, 3, 4, 5, -1, 7]
    lst = [7, 3, 5, 1, 4]
    out, d, e, lam, res, done = run_offs(Gs, offs=OFFS, lst=lst, rep=rep, done_init=-7)
    for b in lst:
        assert done[b] == 1
        assert np.array_equal(out[b], full[0][b]) and np.array_equal(lam[b], full[3][b])
        assert np.array_equal(d[b], full[1][b]) and np.array_equal(e[b], full[2][b]) and np.array_equal(res[b], full[4][b])
    for b in (0, 2, 6):
        assert np.array_equal(out[b], Gs[b])
    assert done[0] == -7 and done[2] == 1 and done[6] == 1
