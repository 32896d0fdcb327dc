"""The edge values of the valued eigenstep (csrc/adj_values.hip): mused_adj_csr_values on asymmetric masks against the NumPy
restatement of tests/spmm_valued_cases.py (the sum of the weights in modality order, the transposed lists valued from
(col, i)), bit for bit, with nothing written behind the last entry; mused_adj_csr_values_dense for the three dtypes; and the
arguments both refuse."""
import ctypes as C

import numpy as np
import pytest

import spmm_valued_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = -7.25


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_values(L, d_masks, weights, n, rowptr, col, transposed):
    nnz = len(col)
    d_rowptr, d_col = dev(rowptr), dev(np.concatenate([col, np.zeros(1, np.int32)]))
    out = torch.full((nnz + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    arr = (C.c_void_p * len(d_masks))(*[m.data_ptr() for m in d_masks])
    w = (C.c_double * len(weights))(*weights)
    L.call("mused_adj_csr_values", arr, w, len(d_masks), n, d_masks[0].shape[1], P(d_rowptr), P(d_col), int(transposed), P(out),
           S())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[nnz:] == SENTINEL).all(), "written behind the last entry"
    return got[:nnz]


@pytest.mark.parametrize("n", [1, 64, 65, 1025, 4097])
@pytest.mark.parametrize("M", [1, 2, 3, 5])
def test_values_from_masks(L, M, n):
    """n = 4097: a 65th word per row.  Both orientations; the lists come from the OR of the masks, as the eigenstep's do."""
    masks = sc.make_masks(n, M, 100 * M + n)
    pattern = np.logical_or.reduce(masks)
    d_masks = [dev(sc.pack_mask(A)) for A in masks]
    weights = [0.3, 0.7, 1.9, 1.0, 0.5][:M]
    for transposed, pat in ((False, pattern), (True, pattern.T)):
        rowptr, col = sc.lists_of(pat)
        got = device_values(L, d_masks, weights, n, rowptr, col, transposed)
        assert sc.same_bits(got, sc.values_from_masks(masks, weights, rowptr, col, transposed))
        assert (got > 0).all()


def test_device_lists_are_the_host_lists(L):
    """The lists the values are checked on above are those mused_adj_degrees / mused_adj_csr_fill build from the OR mask."""
    from mused_amd.engine import Adjacency

    masks = sc.make_masks(65, 3, 365)
    pattern = np.logical_or.reduce(masks)
    rowptr, col = Adjacency(dev(sc.pack_mask(pattern)), 65).neighbour_lists()
    want_rowptr, want_col = sc.lists_of(pattern)
    assert np.array_equal(rowptr.cpu().numpy(), want_rowptr) and np.array_equal(col.cpu().numpy(), want_col)


@pytest.mark.parametrize("weights", sc.ORDER_WEIGHTS)
def test_modality_order_decides_the_last_bit(L, weights):
    n = 65
    masks = sc.make_masks(n, 3, 303)
    pattern = np.logical_or.reduce(masks)
    d_masks = [dev(sc.pack_mask(A)) for A in masks]
    for transposed, pat in ((False, pattern), (True, pattern.T)):
        rowptr, col = sc.lists_of(pat)
        got = device_values(L, d_masks, list(weights), n, rowptr, col, transposed)
        assert sc.same_bits(got, sc.values_from_masks(masks, weights, rowptr, col, transposed))
        assert got.max() == (2.0 ** 53 if weights[0] > 1 else 2.0 ** 53 + 2.0)


def dense_case(n, dtype, seed):
    rng = np.random.default_rng(seed)
    D = np.where(rng.random((n, n)) < min(1.0, 4.0 / n), rng.standard_normal((n, n)) * 3.0, 0.0)
    D[0, n - 1] = -2.5
    if dtype == np.int64:
        D = np.trunc(D * 4.0)
    return D.astype(dtype)


def device_dense_values(L, D, ld, rowptr, col, transposed):
    n = D.shape[0]
    nnz = len(col)
    store = np.full((n, ld), 99.0).astype(D.dtype)
    store[:, :n] = D
    d_D, d_rowptr, d_col = dev(store), dev(rowptr), dev(np.concatenate([col, np.zeros(1, np.int32)]))
    out = torch.full((nnz + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = {np.dtype(np.float32): L.F32, np.dtype(np.float64): L.F64, np.dtype(np.int64): L.I64}[D.dtype]
    L.call("mused_adj_csr_values_dense", P(d_D), code, n, ld, P(d_rowptr), P(d_col), int(transposed), P(out), P(flag), S())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[nnz:] == SENTINEL).all(), "written behind the last entry"
    return got[:nnz], int(flag.item())


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int64])
def test_values_from_dense(L, dtype, n):
    """Negative and fractional entries, a row pitch beyond n, both orientations: the entries as fp64, no flag."""
    D = dense_case(n, dtype, 11 * n)
    for transposed, M in ((False, D), (True, D.T)):
        rowptr, col = sc.lists_of(M != 0)
        got, flag = device_dense_values(L, D, n + 3, rowptr, col, transposed)
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        assert sc.same_bits(got, M[rows, col].astype(np.float64)) and flag == 0
    assert (D < 0).any() and (dtype == np.int64 or n == 1 or (D != np.trunc(D)).any())


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nonfinite_raises_the_flag(L, dtype, bad):
    D = dense_case(65, dtype, 5)
    D[7, 64] = bad
    for transposed, M in ((False, D), (True, D.T)):
        rowptr, col = sc.lists_of(M != 0)
        _, flag = device_dense_values(L, D, 65, rowptr, col, transposed)
        assert flag == 1


def test_bad_arguments(L):
    n = 65
    masks = sc.make_masks(n, 2, 1)
    d_masks = [dev(sc.pack_mask(A)) for A in masks]
    rowptr, col = sc.lists_of(np.logical_or.reduce(masks))
    d_rowptr, d_col = dev(rowptr), dev(col)
    out = torch.full((len(col),), SENTINEL, dtype=torch.float64, device="cuda")
    f = L.lib().mused_adj_csr_values
    ERR_ARG = -1

    def go(M=2, weights=(1.0, 2.0), ptrs=None, rp=d_rowptr, ci=d_col, vals=out, null_masks=False, null_weights=False):
        ptrs = [m.data_ptr() for m in d_masks] if ptrs is None else ptrs
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        w = (C.c_double * max(len(weights), 1))(*weights)
        return f(None if null_masks else arr, None if null_weights else w, M, n, 2, P(rp) if rp is not None else None,
                 P(ci) if ci is not None else None, 0, P(vals) if vals is not None else None, S())

    assert go() == 0
    assert go(M=0) == ERR_ARG
    nine = [d_masks[0].data_ptr()] * 9
    assert go(M=9, weights=(1.0,) * 9, ptrs=nine) == ERR_ARG
    for w in (0.0, -1.0, np.nan, np.inf):
        assert go(weights=(1.0, w)) == ERR_ARG
    assert go(ptrs=[d_masks[0].data_ptr(), None]) == ERR_ARG
    assert go(null_masks=True) == ERR_ARG and go(null_weights=True) == ERR_ARG
    assert go(rp=None) == ERR_ARG and go(ci=None) == ERR_ARG and go(vals=None) == ERR_ARG
    torch.cuda.synchronize()
    g = L.lib().mused_adj_csr_values_dense
    D = dev(dense_case(n, np.float64, 2))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert g(None, L.F64, n, n, P(d_rowptr), P(d_col), 0, P(out), P(flag), S()) == ERR_ARG
    assert g(P(D), L.F64, n, n - 1, P(d_rowptr), P(d_col), 0, P(out), P(flag), S()) == ERR_ARG
    assert g(P(D), L.F64, n, n, P(d_rowptr), P(d_col), 0, P(out), None, S()) == ERR_ARG
    assert g(P(D), L.F64, n, n, P(d_rowptr), P(d_col), 0, None, P(flag), S()) == ERR_ARG
    assert g(P(D), L.BITS, n, n, P(d_rowptr), P(d_col), 0, P(out), P(flag), S()) == -4   # MUSED_ERR_UNSUPPORTED, as mused_adj_from_dense
