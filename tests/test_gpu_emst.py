"""csrc/emst.hip through the C ABI (mused_emst) against its specification mused_amd/hdbscan.py emst_boruvka: the device's
edge SET must equal the specification's on inputs that are decided far beyond rounding (tests/test_hdbscan_host.py checks
that for the same inputs), the flags must rise on the inputs built for them, and one larger input is checked by its
invariants alone."""
import ctypes as C
import math

import numpy as np
import pytest

import hdbscan_cases as hc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rows_on_device(X, ld):
    """(n, d) fp64 CUDA view of X with row pitch ld (0: contiguous); the padding holds NaN, which nothing may read."""
    n, d = X.shape
    if not ld:
        return torch.from_numpy(np.array(X)).cuda()
    buf = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :d] = torch.from_numpy(np.array(X)).cuda()
    return buf[:, :d]


def _cabi(Xd, short_by=0):
    """mused_emst itself -> (edge_a, edge_b int32 NumPy, edge_d2 fp64 NumPy, info 4 int32 NumPy)."""
    from mused_amd import _lib
    from mused_amd.engine import ptr

    n, d = Xd.shape
    nbytes = _lib.lib().mused_emst_ws_bytes(n)
    assert 0 < nbytes <= 56 * n + 4 * ((n + 127) // 128) + 12 * 256   # O(n): no n x n array, list or bitmask
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ea = torch.full((max(n - 1, 1),), -7, dtype=torch.int32, device="cuda")
    eb = torch.full((max(n - 1, 1),), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((max(n - 1, 1),), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    _lib.call("mused_emst", ptr(Xd), n, d, Xd.stride(0), ptr(ea), ptr(eb), ptr(d2), ptr(info), ptr(ws), nbytes - short_by,
              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return ea.cpu().numpy()[:n - 1], eb.cpu().numpy()[:n - 1], d2.cpu().numpy()[:n - 1], info.cpu().numpy()


def _tau(X, a, b, d2):
    """tau(i, j) = 2 (d + 8) 2^-52 (|x_i|^2 + |x_j|^2) + 4 ulp(d2(i, j)) (csrc/emst.hip, mused_amd/hdbscan.py)."""
    sq = np.einsum("ij,ij->i", X, X)
    return 2.0 * (X.shape[1] + 8) * 2.0 ** -52 * (sq[a] + sq[b]) + 4.0 * np.spacing(d2)


@pytest.mark.parametrize("name", hc.CASE_NAMES)
def test_edge_set_equals_the_specification(name):
    X, _, ld = hc.case(name)
    n = len(X)
    want = hc.spec_tree(name)
    Xd = _rows_on_device(X, ld)
    a, b, d2, info = _cabi(Xd)
    print(f"{name}: info {info.tolist()}, specification rounds {want.rounds}")
    assert info.tolist()[:2] == [0, n - 1] and info[3] == 0
    assert 1 <= info[2] <= max(1, math.ceil(math.log2(n)))
    assert a.min() >= 0 and b.min() >= 0 and max(a.max(), b.max()) < n
    assert hc.edge_set(a, b) == hc.edge_set(want.a, want.b) and len(hc.edge_set(a, b)) == n - 1
    exact = ((X[a].astype(np.longdouble) - X[b].astype(np.longdouble)) ** 2).sum(axis=1)
    assert (np.abs(d2.astype(np.longdouble) - exact) <= _tau(X, a, b, d2)).all()
    # the same edge set from a second call: it does not depend on scheduling (the order of the edges may)
    a2, b2, _, info2 = _cabi(Xd)
    assert hc.edge_set(a2, b2) == hc.edge_set(a, b) and info2.tolist() == info.tolist()


@pytest.mark.parametrize("name", hc.AMBIGUOUS_NAMES)
def test_exact_ties_raise_flag_1(name):
    from mused_amd import hdbscan as spec

    X, _, ld = hc.case(name)
    _, _, _, info = _cabi(_rows_on_device(X, ld))
    assert info[0] & spec.FLAG_AMBIGUOUS and not info[0] & spec.FLAG_NONFINITE
    assert info[1] == len(X) - 1                           # under the total order still a spanning tree


def test_nan_row_raises_flag_2():
    from mused_amd import hdbscan as spec

    X, _, ld = hc.case(hc.NAN_NAME)
    _, _, _, info = _cabi(_rows_on_device(X, ld))
    assert info[0] & spec.FLAG_NONFINITE
    assert info[1] == 0 and info[2] == 0                   # no round runs on rows that are not finite


def test_short_workspace_and_bad_shapes_are_rejected_with_a_status():
    from mused_amd import _lib
    from mused_amd._lib import MusedError

    X, _, _ = hc.case("gauss_n129_d50")
    Xd = _rows_on_device(X, 0)
    with pytest.raises(MusedError):
        _cabi(Xd, short_by=1)
    L = _lib.lib()
    assert L.mused_emst_ws_bytes(0) == -1 and L.mused_emst_ws_bytes((1 << 19) + 1) == -1 and L.mused_emst_ws_bytes(1 << 19) > 0
    a, b, _, info = _cabi(Xd[:1])                          # one row: no edge, no round
    assert len(a) == 0 and info.tolist() == [0, 0, 0, 0]


def test_invariants_at_20000_rows():
    """(20000, 8): 157 row tiles, far more workgroups than the device holds at once.  No comparison with scikit-learn's
    estimator at this size: n - 1 edges that span without a cycle, every row's nearest-neighbour pair among them (the
    nearest neighbour of a row is the smallest edge of the cut around it, so it is in every minimum spanning tree), rounds
    within their bound."""
    from sklearn.neighbors import NearestNeighbors

    n, d = 20000, 8
    X = hc.blobs(n, d, seed=11)
    a, b, d2, info = _cabi(_rows_on_device(X, 0))
    print("info", info.tolist())
    assert info.tolist()[:2] == [0, n - 1] and 1 <= info[2] <= math.ceil(math.log2(n))
    edges = hc.edge_set(a, b)
    assert len(edges) == n - 1
    parent = np.arange(n)                                  # host union-find: spanning and acyclic
    for u, v in zip(a.tolist(), b.tolist()):
        while parent[u] != u:
            parent[u] = parent[parent[u]]
            u = parent[u]
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        assert u != v, "a cycle"
        parent[max(u, v)] = min(u, v)
    dist, nb = NearestNeighbors(n_neighbors=2).fit(X).kneighbors(X)
    assert (dist[:, 1] > 0).all()                          # (no duplicates: column 0 is the row itself)
    i = np.arange(n)
    assert hc.edge_set(i, nb[:, 1]) <= edges
