"""The two kernels behind mused_spmm_binary (csrc/spmm.hip: rows, wide), each forced in turn at the smallest shapes at which
it can go wrong: the dispatcher reports the kernel, and the result is, as int64 bit patterns, the sequential fp64 sum
in list order starting from 0.0, with nothing written outside the n x r panel.  Then the eigenstep with and without
`out_components` (the svd_flip signs applied in the stores of the last product instead of a pass over V), on every kernel."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS, WIDE = 0, 1
PATHS = {"rows": ROWS, "wide": WIDE}
# below, at and above the 4 rows of a workgroup, a ragged last workgroup (these are also the edges of the measured `panels`
# kernel that was not kept: 7 rows per wave, 28 per workgroup)
NS = (1, 6, 7, 8, 29, 257)
# empty rows, every remainder of the 4-neighbour step, steps of 1 .. 5 trips
DEGREES = (5, 0, 1, 2, 3, 4, 7, 8, 9, 23)
# a single lane, one / two / three loads of a 192-column trip of `wide` and a second trip, its second load on 1 and 31 lanes
RS = (2, 14, 16, 18, 126, 128, 130, 138, 190, 192, 194, 266)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    yield _lib
    _lib.call("mused_spmm_force_path", -1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_lists(n):
    """Neighbour lists of n rows with the degrees of DEGREES in turn, ascending; a neighbour may repeat (it must once n is
    smaller than the degree), and every third list of two or more names rows 0 and n - 1."""
    rng = np.random.default_rng(1000 + n)
    lists = []
    for i in range(n):
        d = DEGREES[i % len(DEGREES)]
        nb = np.sort(rng.choice(n, d, replace=d > n))
        if d >= 2 and i % 3 == 0:
            nb[0], nb[-1] = 0, n - 1
        if d >= 3 and i % 4 == 2:
            nb[1] = nb[2]
        lists.append(nb.astype(np.int32))
    return lists


@pytest.fixture(scope="module")
def lists_by_n():
    out = {n: make_lists(n) for n in NS}
    big = out[257]
    assert {len(nb) for nb in big} == set(DEGREES)
    assert any(len(nb) > len(set(nb)) for nb in big) and any(nb[0] == 0 and nb[-1] == 256 for nb in big if len(nb) >= 2)
    return out


def sequential_sum(lists, Q):
    want = np.zeros((len(lists), Q.shape[1]))
    for i, nb in enumerate(lists):
        for j in nb:
            want[i] = want[i] + Q[j]
    return want


def run_spmm(L, lists, Q, ldq, ldy, q_offset=0):
    """mused_spmm_binary on Q stored at pitch ldq, `q_offset` doubles behind a 256-byte aligned base, NaN behind every row of Q and
    of Y and in one row below Y.  Returns (path reported for exactly this call, Y as stored: n + 1 rows of ldy)."""
    n, r = Q.shape
    Qp = np.full(n * ldq + q_offset, np.nan)
    Qp[q_offset:].reshape(n, ldq)[:, :r] = Q
    d_Q = dev(Qp)[q_offset:]
    rowptr = np.concatenate([[0], np.cumsum([len(nb) for nb in lists])]).astype(np.int32)
    col = np.concatenate(lists + [np.zeros(1, np.int32)]).astype(np.int32)   # (never an empty device array)
    d_rowptr, d_col = dev(rowptr), dev(col)
    Y = torch.full((n + 1, ldy), np.nan, dtype=torch.float64, device="cuda")
    path = L.lib().mused_spmm_binary_path(n, r, ldq, ldy, d_Q.data_ptr() % 16, Y.data_ptr() % 16)
    L.call("mused_spmm_binary", P(d_rowptr), P(d_col), n, P(d_Q), ldq, r, P(Y), ldy, S())
    torch.cuda.synchronize()
    return path, Y.cpu().numpy()


def check(got, want):
    n, r = want.shape
    assert np.isnan(got[:n, r:]).all() and np.isnan(got[n]).all(), "written outside the n x r panel"
    assert np.array_equal(got[:n, :r].view(np.int64), want.view(np.int64))


def rows_of_mixed_size(n, r, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, r)) * np.exp(rng.uniform(-8.0, 8.0, (n, 1)))   # order matters


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("path", list(PATHS))
def test_forced_path_every_shape(L, lists_by_n, path, r):
    """Even r, rows of Q 16-byte aligned (ldq = r + 2): the forced kernel runs, for ldy odd (8-byte stores) and even (16-byte)."""
    L.call("mused_spmm_force_path", PATHS[path])
    for n in NS:
        Q = rows_of_mixed_size(n, r, 7 * r + n)
        want = sequential_sum(lists_by_n[n], Q)
        for ldy in (r + 3, r + 4):
            got_path, got = run_spmm(L, lists_by_n[n], Q, r + 2, ldy)
            assert got_path == PATHS[path]
            check(got, want)


@pytest.mark.parametrize("path", list(PATHS))
def test_fallback_to_rows(L, lists_by_n, path):
    """Odd r, an odd pitch of Q, or a base 8 bytes off a 16-byte boundary: today's kernel whatever is forced, same bits."""
    L.call("mused_spmm_force_path", PATHS[path])
    for n in (29, 257):
        for r, ldq, off in ((1, 4, 0), (137, 138, 0), (138, 141, 0), (138, 140, 1), (16, 18, 1)):
            Q = rows_of_mixed_size(n, r, 31 * r + n + off)
            got_path, got = run_spmm(L, lists_by_n[n], Q, ldq, r + 4, q_offset=off)
            assert got_path == ROWS
            check(got, sequential_sum(lists_by_n[n], Q))


def test_default_per_shape_class(L):
    """Unforced: a panel beyond one XCD's 4 MB L2 takes `wide` (the eigenstep at n = 10^4), a smaller one today's kernel (n = 2,000)."""
    L.call("mused_spmm_force_path", -1)
    path = L.lib().mused_spmm_binary_path
    assert [path(10000, r, r, r, 0, 0) for r in (138, 128, 266, 256)] == [WIDE] * 4
    assert [path(2000, r, r, r, 0, 0) for r in (60, 50)] == [ROWS] * 2
    assert path(10000, 137, 137, 137, 0, 0) == ROWS and path(10000, 138, 138, 138, 8, 0) == ROWS


@pytest.fixture(scope="module")
def knn_window(L):
    """One small kNN mask (n = 257, k = 5) and its A / A^T neighbour lists, built as the eigenstep builds them."""
    from mused_amd.engine import Adjacency, WindowEngine

    n, k = 257, 5
    X = np.random.default_rng(5).standard_normal((n, 24))
    eng = WindowEngine(n)
    adj = eng.knn_adjacency(torch.from_numpy(X).cuda(), k)
    mT = torch.empty_like(adj.mask)
    L.call("mused_adj_transpose", P(adj.mask), n, adj.words, P(mT), S())
    out = []
    for a in (adj, Adjacency(mT, n)):
        rowptr, col = a.neighbour_lists()
        rp, cl = rowptr.cpu().numpy(), col.cpu().numpy()
        out.append([cl[rp[i]:rp[i + 1]] for i in range(n)])
    torch.cuda.synchronize()
    assert {len(nb) for nb in out[0]} <= {k - 1, k} and len({len(nb) for nb in out[1]}) > 2   # (self is dropped from its k)
    yield adj, out
    eng.close()


@pytest.mark.parametrize("path", list(PATHS))
def test_knn_lists_and_transpose(L, knn_window, path):
    L.call("mused_spmm_force_path", PATHS[path])
    n = 257
    for r in (138, 128):
        Q = rows_of_mixed_size(n, r, r)
        for lists in knn_window[1]:
            got_path, got = run_spmm(L, lists, Q, r, r)
            assert got_path == PATHS[path]
            check(got, sequential_sum(lists, Q))


def test_reduce_signs_in_the_store(L, knn_window):
    """mused_rsvd_reduce at n = 257, r = 26 with and without out_components, on each kernel: embedding and sigma bit for bit
    the same in all four runs (a handle records its kernels at its first call: one handle per run)."""
    adj = knn_window[0]
    n, r, n_comp = 257, 26, 16
    q0 = dev(np.random.RandomState(0).normal(size=(n, r)))
    runs = {}
    for path in PATHS:
        L.call("mused_spmm_force_path", PATHS[path])
        assert L.lib().mused_spmm_binary_path(n, n_comp, n_comp, n_comp, 0, 0) == PATHS[path]
        for comps in (False, True):
            h = C.c_void_p()
            L.call("mused_rsvd_create", n, r, n * 5, 0, C.byref(h))
            L.call("mused_rsvd_set_mode", h, 1)   # Cholesky-QR without the recorded Householder fallback, as the engine runs it
            L.call("mused_rsvd_set_q0", h, P(q0), n, r, S())
            L.call("mused_memcpy_d2d", C.c_void_p(L.lib().mused_rsvd_mask_buffer(h)), P(adj.mask), n * adj.words * 8, S())
            emb = torch.full((n, n_comp), np.nan, dtype=torch.float64, device="cuda")
            sig = torch.full((n_comp,), np.nan, dtype=torch.float64, device="cuda")
            V = torch.full((n, n_comp), np.nan, dtype=torch.float64, device="cuda") if comps else None
            for _ in range(2):   # the second call replays the recorded graph
                L.call("mused_rsvd_reduce", h, n, n_comp, r, 5, P(emb), P(sig), P(V) if comps else None, S())
            torch.cuda.synchronize()
            L.call("mused_rsvd_destroy", h)
            runs[(path, comps)] = (emb.cpu().numpy(), sig.cpu().numpy(), V.cpu().numpy() if comps else None)
    ref_emb, ref_sig, ref_V = runs[("rows", True)]
    assert np.isfinite(ref_emb).all() and np.isfinite(ref_sig).all() and (ref_sig[:-1] >= ref_sig[1:]).all()
    # svd_flip leaves the entry of largest magnitude of every component positive
    assert (ref_V[np.abs(ref_V).argmax(axis=0), np.arange(n_comp)] > 0).all()
    for key, (emb, sig, V) in runs.items():
        assert np.array_equal(emb.view(np.int64), ref_emb.view(np.int64)), key
        assert np.array_equal(sig.view(np.int64), ref_sig.view(np.int64)), key
        if V is not None:
            assert np.array_equal(V.view(np.int64), ref_V.view(np.int64)), key
