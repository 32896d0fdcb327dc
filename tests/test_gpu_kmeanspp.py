"""Device k-means++ seeding (csrc/kmeanspp.hip) against scikit-learn: the moments of KMeans.fit, the seeds of
`kmeans_plusplus` from the host's draws, the ambiguity flag with its fallback, and `perform_clustering_on_device` end to
end without a host copy of the embedding."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from sklearn.cluster import KMeans, kmeans_plusplus  # noqa: E402
from sklearn.datasets import make_blobs  # noqa: E402

from mused_amd import matrix_operations as mo  # noqa: E402
from test_kmeanspp_host import replay_kmeanspp  # noqa: E402

BLOB_CASES = [(2000, 50, 8), (2049, 128, 20), (2000, 50, 150), (10000, 8, 1024), (4096, 512, 16), (150001, 8, 4)]
# every seeding input has n >= 10 k: none of them may raise the ambiguity flag
SEED_CASES = ([("blobs",) + c + (s,) for c in BLOB_CASES for s in range(3)]
              + [("noise", 2000, 16, 50, s) for s in range(3)]
              + [("blobs", 2000, 50, 1, 0), ("blobs", 2000, 50, 2, 0)])   # k = 2: the first added centre is the last step


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _align(b):
    return (b + 255) & ~255


@functools.lru_cache(maxsize=None)
def rows(kind, n, d, k, seed):
    if kind == "noise":
        X = np.random.RandomState(seed).standard_normal((n, d))
    else:
        X, _ = make_blobs(n, d, centers=max(k, 3), random_state=seed)
    X = np.ascontiguousarray(X, dtype=np.float64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def sk_seeds(kind, n, d, k, seed):
    """(centred rows, scikit-learn's indices) with the reference's own replay checked on the way: an input on which the
    CPU replay with the same draws already leaves scikit-learn's choice is a tie, not a test of the kernel."""
    X = rows(kind, n, d, k, seed)
    Xc = X - X.mean(axis=0)
    _, idx = kmeans_plusplus(Xc, k, random_state=np.random.RandomState(seed))
    first, U = mo.kmeanspp_draws(n, k, seed)
    assert np.array_equal(replay_kmeanspp(Xc, k, first, U), idx), "the input is ambiguous for the reference itself"
    Xc.setflags(write=False)
    return Xc, idx


@functools.lru_cache(maxsize=None)
def sk_labels(kind, n, d, k, seed):
    return KMeans(n_clusters=k, random_state=seed).fit_predict(rows(kind, n, d, k, seed))


def device_moments(Xd):
    from mused_amd import _lib
    from mused_amd import engine as eng

    n, d = Xd.shape
    mean = torch.full((d,), float("nan"), dtype=torch.float64, device="cuda")
    tol = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.call("mused_kmeans_moments", eng.ptr(Xd), Xd.stride(0), n, d, eng.ptr(mean), eng.ptr(tol),
              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return mean.cpu().numpy(), float(tol.cpu().numpy()[0])


def device_seed(X, k, seed):
    """-> (indices, centres, info, closest_dist_sq) of mused_kmeans_seed on the rows X (host), NumPy's column means."""
    from mused_amd import _lib
    from mused_amd import engine as eng

    n, d = X.shape
    first, U = mo.kmeanspp_draws(n, k, seed)
    Xd = torch.tensor(X, device="cuda")
    mean = torch.from_numpy(X.mean(axis=0)).cuda()
    Ud = torch.from_numpy(U if k > 1 else np.zeros((1, 1))).cuda()
    ws_bytes = int(_lib.lib().mused_kmeans_seed_ws_bytes(n, d, k))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    cen = torch.full((k, d), float("nan"), dtype=torch.float64, device="cuda")
    idx = torch.full((k,), -1, dtype=torch.int32, device="cuda")
    info = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    _lib.call("mused_kmeans_seed", eng.ptr(Xd), Xd.stride(0), n, d, k, eng.ptr(mean), first, eng.ptr(Ud), U.shape[1],
              eng.ptr(cen), eng.ptr(idx), eng.ptr(info), eng.ptr(ws), ws_bytes,
              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    off = _align(8 * n * d) + _align(8 * n)   # the layout include/mused_hip.h documents
    closest = ws[off:off + 8 * n].view(torch.float64).cpu().numpy()
    return idx.cpu().numpy(), cen.cpu().numpy(), info.cpu().numpy(), closest


# ---- moments ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,ld", [(1, 3, 3), (257, 50, 50), (2049, 512, 512), (257, 50, 64)])
def test_moments_are_numpys(n, d, ld):
    rs = np.random.RandomState(n + d)
    big = rs.standard_normal((n, ld)) * rs.uniform(0.1, 30.0, size=ld) + rs.uniform(-5.0, 5.0, size=ld)
    Xd = torch.from_numpy(big).cuda()[:, :d]
    X = np.ascontiguousarray(big[:, :d])
    assert Xd.stride(0) == ld
    mean, tol = device_moments(Xd)
    assert np.array_equal(mean, X.mean(axis=0))   # bit for bit
    ref = float(np.mean(np.var(X, axis=0)) * 1e-4)
    print(f"tol {tol!r} ref {ref!r}")
    assert abs(tol - ref) <= d * 2.0 ** -52 * ref   # d positive terms added in another order


# ---- seeding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,d,k,seed", SEED_CASES)
def test_seeds_are_sklearns(kind, n, d, k, seed):
    Xc, ref = sk_seeds(kind, n, d, k, seed)
    idx, cen, info, closest = device_seed(rows(kind, n, d, k, seed), k, seed)
    assert list(info) == [0, k], f"ambiguity flag / centres chosen: {info}"
    assert np.array_equal(idx, ref)
    assert np.array_equal(cen, Xc[ref])   # the centred rows, bit for bit
    if n * k <= 2_000_000:
        # closest_dist_sq of the finished run against plain differences to the chosen rows: what |x|^2 + |c|^2 - 2 x.c
        # can lose in d fused multiply-adds and the two sums of squares
        from scipy.spatial.distance import cdist

        xs = (Xc ** 2).sum(1)
        d2 = cdist(Xc, Xc[ref], "sqeuclidean").min(axis=1)
        assert np.all(np.abs(closest - d2) <= 4 * (d + 8) * 2.0 ** -52 * (xs + xs.max()))


@pytest.mark.parametrize("kind,n,d,k,seed", [("blobs", 2049, 128, 20, 0), ("blobs", 150001, 8, 4, 1)])
def test_two_runs_give_the_same_bits(kind, n, d, k, seed):
    X = rows(kind, n, d, k, seed)
    a, b = device_seed(X, k, seed), device_seed(X, k, seed)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[3].view(np.int64), b[3].view(np.int64))
    assert np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


# ---- ties -----------------------------------------------------------------------------------------------------------
def test_tie_is_flagged_and_sklearn_clusters_the_window():
    """150 two-point blobs, 300 rows, k = 150: candidates of one blob have potentials equal to the last digits, and a
    fixed-order sum decides otherwise than BLAS (a NumPy restatement left scikit-learn's choice at centre 147).  The kernel
    must say so; through perform_clustering_on_device the window leaves the device path (k * d > 8192 here: scikit-learn's
    KMeans) and is counted."""
    X, _ = make_blobs(300, 128, centers=150, random_state=0)
    _, _, info, _ = device_seed(np.ascontiguousarray(X), 150, 0)
    assert info[0] == 1 and info[1] == 150
    before = mo.km_fallbacks
    got = mo.perform_clustering_on_device(torch.from_numpy(X).cuda(), 150, 0)
    assert mo.km_fallbacks == before + 1
    assert np.array_equal(got, KMeans(n_clusters=150, random_state=0).fit_predict(X))


def test_exact_tie_takes_the_host_seeded_path(monkeypatch):
    """Two distinct points, 20 copies of each, k = 2: both trials of the second centre land on copies of the point the
    first centre is not, their potentials are the same number, and with this seed they are different rows -- a tie that
    no rounding bound is needed for.  Flag, one fallback, one host copy, scikit-learn's labels."""
    seed = 0
    a, b = np.random.RandomState(5).standard_normal((2, 8))
    X = np.ascontiguousarray(np.concatenate([np.tile(a, (20, 1)), np.tile(b, (20, 1))]))
    first, U = mo.kmeanspp_draws(40, 2, seed)
    far = np.arange(20, 40) if first < 20 else np.arange(0, 20)   # the rows with a distance: equal shares of the potential
    cand = far[np.minimum((U[0] * 20).astype(int), 19)]
    assert U.shape == (1, 2) and cand[0] != cand[1] and np.all(np.abs(U[0] * 20 - np.round(U[0] * 20)) > 1e-6)
    _, _, info, _ = device_seed(X, 2, seed)
    assert list(info) == [1, 2]
    calls = []
    real = mo._km_host_copy
    monkeypatch.setattr(mo, "_km_host_copy", lambda *args: calls.append(1) or real(*args))
    before = mo.km_fallbacks
    got = mo.perform_clustering_on_device(torch.from_numpy(X).cuda(), 2, seed)
    assert mo.km_fallbacks == before + 1 and calls == [1]
    assert np.array_equal(got, KMeans(n_clusters=2, random_state=seed).fit_predict(X))


def test_duplicated_rows_give_sklearns_labels():
    X, _ = make_blobs(600, 16, centers=6, random_state=3)
    X = np.ascontiguousarray(np.repeat(X, 2, axis=0))   # every row twice: equal potentials wherever both copies are tried
    _, _, info, _ = device_seed(X, 6, 3)
    before = mo.km_fallbacks
    got = mo.perform_clustering_on_device(torch.from_numpy(X).cuda(), 6, 3)
    assert mo.km_fallbacks == before + int(info[0])
    assert np.array_equal(got, KMeans(n_clusters=6, random_state=3).fit_predict(X))


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,seed", [c + (s,) for c in BLOB_CASES if c[1] * c[2] <= 8192 for s in range(3)])
def test_clustering_without_a_host_copy(n, d, k, seed, monkeypatch):
    X = rows("blobs", n, d, k, seed)
    calls = []
    real = mo._km_host_copy
    monkeypatch.setattr(mo, "_km_host_copy", lambda *a: calls.append(1) or real(*a))
    monkeypatch.delenv("MUSED_KMEANS_SEED", raising=False)
    before = mo.km_fallbacks
    got = mo.perform_clustering_on_device(torch.tensor(X, device="cuda"), k, seed)
    assert np.array_equal(got, sk_labels("blobs", n, d, k, seed))
    assert calls == [] and mo.km_fallbacks == before   # the embedding never went to the host


def test_host_switch_takes_the_host_seeded_path(monkeypatch):
    X = rows("blobs", 2000, 50, 8, 0)
    calls = []
    real = mo._km_host_copy
    monkeypatch.setattr(mo, "_km_host_copy", lambda *a: calls.append(1) or real(*a))
    monkeypatch.setenv("MUSED_KMEANS_SEED", "host")
    before = mo.km_fallbacks
    got = mo.perform_clustering_on_device(torch.tensor(X, device="cuda"), 8, 0)
    assert np.array_equal(got, sk_labels("blobs", 2000, 50, 8, 0))
    assert calls == [1] and mo.km_fallbacks == before   # asked for, not a fallback
