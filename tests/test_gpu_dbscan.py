"""csrc/dbscan.hip against sklearn.cluster.DBSCAN: through the C ABI (mused_dbscan) and through
matrix_operations.perform_dbscan_clustering_on_device.  Labels must be EQUAL, the ambiguity flag clear and no call may
have gone to the host, on inputs whose smallest |d2 - eps^2| lies far above the rounding margin (tests/test_dbscan_host.py
checks that for the same inputs); two cases raise a flag on purpose."""
import ctypes as C

import numpy as np
import pytest

import dbscan_cases as dc

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
        return torch.from_numpy(np.ascontiguousarray(X)).cuda()
    buf = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :d] = torch.from_numpy(X).cuda()
    return buf[:, :d]


def _cabi(Xd, eps, ms):
    """mused_dbscan itself -> (labels int32 NumPy, info 4 int32 NumPy)."""
    from mused_amd import _lib
    from mused_amd.engine import ptr

    n, d = Xd.shape
    nbytes = _lib.lib().mused_dbscan_ws_bytes(n)
    assert 0 < nbytes <= 24 * n + 4 * ((n + 127) // 128) + 7 * 256   # O(n): no n x n array, list or bitmask
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    labels = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    _lib.call("mused_dbscan", ptr(Xd), n, d, Xd.stride(0), float(eps), int(ms), ptr(labels), ptr(info), ptr(ws), nbytes,
              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return labels.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_labels_equal_sklearn(name):
    from mused_amd import matrix_operations as mo

    _, X, eps, ms, ld = dc.case(name)
    want = dc.sklearn_labels(name)
    Xd = _rows_on_device(X, ld)
    labels, info = _cabi(Xd, eps, ms)
    assert info[0] == 0, "a flag on an input that is decided far beyond rounding"
    assert np.array_equal(labels, want)
    assert info[1] == want.max() + 1 and info[2] == len(dc.sklearn_core(name))   # clusters, core rows
    before = mo.dbscan_fallbacks
    for arg in (Xd, X):                                    # device tensor (pitched where the case says so), ndarray
        got = mo.perform_dbscan_clustering_on_device(arg, eps, ms)
        assert got.dtype == np.int64 and np.array_equal(got, want)
    assert mo.dbscan_fallbacks == before


def test_exact_eps_raises_the_flag_and_the_host_answers():
    from sklearn.cluster import DBSCAN

    from mused_amd import dbscan as spec
    from mused_amd import matrix_operations as mo

    X = np.random.default_rng(2).standard_normal((200, 4))
    X[1] = X[0]
    X[1, 2] = X[0, 2] + 0.75                              # rows 0 and 1 eps apart along one axis
    eps, ms = 0.75, 3
    _, info = _cabi(_rows_on_device(X, 0), eps, ms)
    assert info[0] & spec.FLAG_AMBIGUOUS and not info[0] & spec.FLAG_NONFINITE
    before = mo.dbscan_fallbacks
    got = mo.perform_dbscan_clustering_on_device(torch.from_numpy(X).cuda(), eps, ms)
    assert mo.dbscan_fallbacks == before + 1
    assert np.array_equal(got, DBSCAN(eps=eps, min_samples=ms).fit_predict(X))
    # a hair away from it the device answers itself
    _, info = _cabi(_rows_on_device(X, 0), 0.7501, ms)
    assert info[0] == 0


def test_nan_row_behaves_as_the_host_call():
    from mused_amd import dbscan as spec
    from mused_amd import matrix_operations as mo

    X = np.random.default_rng(3).standard_normal((150, 6))
    X[77, 3] = np.nan
    _, info = _cabi(_rows_on_device(X, 0), 1.0, 3)
    assert info[0] & spec.FLAG_NONFINITE
    with pytest.raises(ValueError) as host:
        mo.perform_dbscan_clustering(X, 1.0, 3)
    before = mo.dbscan_fallbacks
    with pytest.raises(ValueError) as dev:
        mo.perform_dbscan_clustering_on_device(torch.from_numpy(X).cuda(), 1.0, 3)
    assert str(dev.value) == str(host.value)
    assert mo.dbscan_fallbacks == before + 1


def test_host_switch_and_rejected_arguments(monkeypatch):
    from mused_amd import matrix_operations as mo

    _, X, eps, ms, _ = dc.case("duplicates")
    want = dc.sklearn_labels("duplicates")
    calls = []
    real = mo.perform_dbscan_clustering
    monkeypatch.setattr(mo, "perform_dbscan_clustering", lambda *a, **k: calls.append(1) or real(*a, **k))
    before = mo.dbscan_fallbacks
    assert np.array_equal(mo.perform_dbscan_clustering_on_device(torch.from_numpy(X).cuda(), eps, ms), want) and not calls
    monkeypatch.setenv("MUSED_DBSCAN", "host")
    assert np.array_equal(mo.perform_dbscan_clustering_on_device(torch.from_numpy(X).cuda(), eps, ms), want) and calls
    monkeypatch.delenv("MUSED_DBSCAN")
    with pytest.raises(Exception):                         # scikit-learn's own parameter check
        mo.perform_dbscan_clustering_on_device(X, 0.0, ms)
    assert mo.dbscan_fallbacks == before                   # neither was a fallback
    from mused_amd._lib import MusedError
    with pytest.raises(MusedError):
        _cabi(_rows_on_device(X, 0), -1.0, ms)
