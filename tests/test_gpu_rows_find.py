"""mused_rows_find (csrc/rows_find.hip) against its specification, mused_amd.rows_find.rows_find: positions of query rows among
held rows by bit equality, duplicates handed out in order of position.  Every case runs twice and must give the same output."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pitched(A, pitch):
    """A on the device with rows `pitch` doubles apart; the padding holds NaN of another bit pattern, which nothing may read."""
    buf = torch.full((max(1, len(A)), pitch), float("nan"), dtype=torch.float64, device="cuda")
    buf.view(torch.int64)[:] |= 0x5a5a
    if len(A):
        buf[:len(A), :A.shape[1]] = torch.tensor(A, device="cuda")
    return buf


def find(X, Q, pad=3):
    from mused_amd import _lib
    from mused_amd.engine import ptr

    n, q, d = len(X), len(Q), X.shape[1]
    Xd, Qd = _pitched(X, d + pad), _pitched(Q, d + 2 * pad)
    nbytes = int(_lib.lib().mused_rows_find_ws_bytes(n, q, d))
    assert 0 < nbytes <= 40 * (n + q) + 1024 * ((n + q + 1023) // 1024) + 9 * 256 + 12     # O(n + q)
    outs = []
    for _ in range(2):
        ws = torch.full((nbytes,), 0xa5, dtype=torch.uint8, device="cuda")                 # the workspace carries nothing
        idx = torch.full((max(1, q),), -7, dtype=torch.int32, device="cuda")
        info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        _lib.call("mused_rows_find", ptr(Xd), Xd.stride(0), n, ptr(Qd), Qd.stride(0), q, d, ptr(idx), ptr(info), ptr(ws), nbytes,
                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        outs.append((idx[:q].cpu().numpy().astype(np.int64), info.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


@functools.lru_cache(maxsize=None)
def _held(n, d):
    """n rows of which about a fifth repeat earlier ones; d = 1: integer values below n / 2, so many values are held several
    times and, as doubles whose low words are all zero, land in few distinct slots of any table before probing."""
    rng = np.random.default_rng(n + d)
    if d == 1:
        return rng.integers(0, max(2, n // 2), (n, 1)).astype(np.float64)
    X = rng.standard_normal((n, d))
    rep = rng.random(n) < 0.2
    X[rep] = X[rng.integers(0, n, int(rep.sum()))]
    return X


# the sort's edges, d = 1: n + q = 1024 and 1025 (one tile of the radix passes exactly, and one element into the second); a
# table of 65,535 and of 65,539 slots (the largest group id crosses 2^16: two passes, then three)
SORT_EDGES = [(1023, 1, 1), (1024, 1, 1), (32766, 1, 1), (32768, 1, 1)]


@pytest.mark.parametrize("n,d,q", [(n, d, q) for q in [1, 127, 128, 129] for d in [1, 2, 50] for n in [1, 300, 20000]] + SORT_EDGES)
def test_against_the_rule(n, d, q):
    from mused_amd.rows_find import rows_find

    X = _held(n, d)
    rng = np.random.default_rng(q)
    Q = X[rng.integers(0, n, q)].copy()                    # rows held, many asked for more often than they are held
    miss = rng.random(q) < 0.25
    Q[miss] = Q[miss] + 0.5 if d == 1 else rng.standard_normal((int(miss.sum()), d))
    want = rows_find(X, Q)
    got, info = find(X, Q)
    assert np.array_equal(got, want)
    assert tuple(info) == ((want >= 0).sum(), (want < 0).sum(), 0, 0)
    if n == 20000 and q >= 127:
        assert (want >= 0).any() and (want < 0).any()


def test_duplicates_signed_zeros_nan_and_the_last_bit():
    from mused_amd.rows_find import rows_find

    a, b = [1.5, -2.0], [0.25, 7.0]
    X = np.array([b, a, b, a, b, a, [0.0, 1.0], [-0.0, 1.0], [1.0, np.nan], [1.0, 2.0]])
    other_nan = np.array([1.0, np.nan])
    other_nan.view(np.int64)[1] ^= 1
    Q = np.array([a, a, a, a, [-0.0, 1.0], [0.0, 1.0], [0.0, -1.0], [1.0, np.nan], other_nan, [1.0, np.nextafter(2.0, 3.0)],
                  [np.nextafter(1.0, 0.0), 2.0], [1.0, 2.0]])
    want = np.array([1, 3, 5, -1, 7, 6, -1, 8, -1, -1, -1, 9])
    assert np.array_equal(rows_find(X, Q), want)
    got, info = find(X, Q)
    assert np.array_equal(got, want) and tuple(info) == (7, 5, 0, 0)
    got, info = find(X, X[::-1].copy())                    # the rows held, asked for in reverse: every position once
    assert np.array_equal(np.sort(got), np.arange(len(X))) and np.array_equal(got, rows_find(X, X[::-1]))


def test_empty_sides_and_refusals():
    from mused_amd import _lib
    from mused_amd._lib import MusedError
    from mused_amd.engine import ptr

    X = np.arange(6.0).reshape(3, 2)
    got, info = find(X, np.empty((0, 2)))
    assert len(got) == 0 and tuple(info) == (0, 0, 0, 0)
    got, info = find(np.empty((0, 2)), X)
    assert np.array_equal(got, [-1, -1, -1]) and tuple(info) == (0, 3, 0, 0)
    ws_bytes = _lib.lib().mused_rows_find_ws_bytes
    assert ws_bytes(-1, 1, 2) == -1 and ws_bytes(1, -1, 2) == -1 and ws_bytes(1, 1, 0) == -1 and ws_bytes(1 << 24, 1, 2) == -1
    Xd = torch.tensor(X, device="cuda")
    idx = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    need = int(ws_bytes(3, 3, 2))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n, q, d, ld, nbytes in ((3, 3, 2, 2, need - 1), (3, 3, 2, 1, need), (3, 3, 0, 2, need), (-1, 3, 2, 2, need), (3, -1, 2, 2, need)):
        with pytest.raises(MusedError):
            _lib.call("mused_rows_find", ptr(Xd), ld, n, ptr(Xd), 2, q, d, ptr(idx), ptr(info), ptr(ws), nbytes, st)
    torch.cuda.synchronize()
    assert (idx == -7).all() and (info == -7).all()
