"""mused_spmm_valued (csrc/spmm_valued.hip: rows, wide), each kernel forced in turn on the grid of tests/test_gpu_spmm_paths.py,
with values that are negative, subnormal, +-0.0 and 2^50 apart and a Q that holds -0.0.  The stored result is, as int64 bit
patterns, the restatement of tests/spmm_valued_cases.py (acc = acc + (v * q), in list order, from 0.0 -- the variants that
test_spmm_valued_host.py shows to differ would fail here), nothing is written outside the n x r panel, the two kernels agree,
and with every value 1.0 the result is mused_spmm_binary's bit for bit.  (The C entries take no col_sign: the sign-in-store
rule of the valued kernels is covered through the eigenstep, tests/test_gpu_weighted_fusion.py, M = 1 and w = 1.0 with and
without out_components.)"""
import ctypes as C

import numpy as np
import pytest

import spmm_valued_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


_CASES = {}


def case(n, r):
    """(lists, values, Q, restatement) of one shape, computed once and shared by every test."""
    if (n, r) not in _CASES:
        lists = sc.make_lists(n)
        vals = sc.make_values(lists, 50 + n)
        Q = sc.make_q(n, r, 7 * r + n)
        _CASES[(n, r)] = (lists, vals, Q, sc.restate(lists, vals, Q))
    return _CASES[(n, r)]


def run(L, lists, vals, Q, ldq, ldy, q_offset=0, binary=False):
    """mused_spmm_valued (or mused_spmm_binary) on Q stored at pitch ldq, `q_offset` doubles behind a 256-byte aligned base,
    NaN behind every row of Q and of Y, in one row below Y and behind the last value.  Returns (the path the dispatcher
    reports for exactly this call, Y as stored: n + 1 rows of ldy)."""
    n, r = Q.shape
    Qp = np.full(n * ldq + q_offset, np.nan)
    Qp[q_offset:].reshape(n, ldq)[:, :r] = Q
    d_Q = dev(Qp)[q_offset:]
    rowptr = np.concatenate([[0], np.cumsum([len(nb) for nb in lists])]).astype(np.int32)
    d_rowptr = dev(rowptr)
    d_col = dev(np.concatenate(lists + [np.zeros(1, np.int32)]).astype(np.int32))   # (never an empty device array)
    d_val = dev(np.concatenate(list(vals) + [np.full(1, np.nan)]))
    Y = torch.full((n + 1, ldy), np.nan, dtype=torch.float64, device="cuda")
    path = L.lib().mused_spmm_binary_path(n, r, ldq, ldy, d_Q.data_ptr() % 16, Y.data_ptr() % 16)
    if binary:
        L.call("mused_spmm_binary", P(d_rowptr), P(d_col), n, P(d_Q), ldq, r, P(Y), ldy, S())
    else:
        L.call("mused_spmm_valued", P(d_rowptr), P(d_col), P(d_val), n, P(d_Q), ldq, r, P(Y), ldy, S())
    torch.cuda.synchronize()
    return path, Y.cpu().numpy()


def check(got, want):
    n, r = want.shape
    assert np.isnan(got[:n, r:]).all() and np.isnan(got[n]).all(), "written outside the n x r panel"
    assert sc.same_bits(got[:n, :r], want)


@pytest.mark.parametrize("r", sc.RS)
@pytest.mark.parametrize("path", list(sc.PATHS))
def test_forced_path_every_shape(L, path, r):
    """Even r, rows of Q 16-byte aligned (ldq = r + 2): the forced kernel runs, for ldy odd (8-byte stores) and even (16-byte)."""
    L.call("mused_spmm_force_path", sc.PATHS[path])
    for n in sc.NS:
        lists, vals, Q, want = case(n, r)
        for ldy in (r + 3, r + 4):
            got_path, got = run(L, lists, vals, Q, r + 2, ldy)
            assert got_path == sc.PATHS[path]
            check(got, want)


@pytest.mark.parametrize("r", (2, 138, 194, 266))
def test_rows_equals_wide(L, r):
    for n in (29, 257):
        lists, vals, Q, _ = case(n, r)
        out = {}
        for path, code in sc.PATHS.items():
            L.call("mused_spmm_force_path", code)
            got_path, out[path] = run(L, lists, vals, Q, r, r)
            assert got_path == code
        assert sc.same_bits(out["rows"][:n], out["wide"][:n])


@pytest.mark.parametrize("path", list(sc.PATHS))
def test_fallback_to_rows(L, path):
    """Odd r, an odd pitch of Q, or a base 8 bytes off a 16-byte boundary: `rows` whatever is forced, same bits."""
    L.call("mused_spmm_force_path", sc.PATHS[path])
    for n in (29, 257):
        lists = sc.make_lists(n)
        vals = sc.make_values(lists, 50 + n)
        for r, ldq, off in ((1, 4, 0), (137, 138, 0), (138, 141, 0), (138, 140, 1), (16, 18, 1)):
            Q = sc.make_q(n, r, 31 * r + n + off)
            got_path, got = run(L, lists, vals, Q, ldq, r + 4, q_offset=off)
            assert got_path == sc.ROWS
            check(got, sc.restate(lists, vals, Q))


@pytest.mark.parametrize("r", (2, 18, 138, 192, 266))
@pytest.mark.parametrize("path", list(sc.PATHS))
def test_all_ones_is_the_binary_kernel_bit_for_bit(L, path, r):
    """The product by 1.0 is exact: the valued kernel stores what mused_spmm_binary stores, -0.0 in Q and empty rows included."""
    L.call("mused_spmm_force_path", sc.PATHS[path])
    for n in sc.NS:
        lists, _, Q, _ = case(n, r)
        ones = [np.ones(len(nb)) for nb in lists]
        for ldy in (r + 3, r + 4):
            p_v, got = run(L, lists, ones, Q, r + 2, ldy)
            p_b, ref = run(L, lists, ones, Q, r + 2, ldy, binary=True)
            assert p_v == p_b == sc.PATHS[path]
            assert np.array_equal(got.view(np.int64), ref.view(np.int64))   # the NaN padding included


def test_bad_arguments(L):
    n, r = 6, 4
    lists, vals, Q, _ = case(n, 14)
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    f = L.lib().mused_spmm_valued
    assert f(P(i), P(i), None, n, P(t), r, r, P(t), r, S()) == -1
    assert f(None, P(i), P(t), n, P(t), r, r, P(t), r, S()) == -1
    assert f(P(i), P(i), P(t), n, P(t), r - 1, r, P(t), r, S()) == -1
    assert f(P(i), P(i), P(t), 0, P(t), r, r, P(t), r, S()) == -1
