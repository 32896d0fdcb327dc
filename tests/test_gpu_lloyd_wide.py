"""On the GPU: mused_kmeans_lloyd_wide (csrc/kmeans.hip), the Lloyd iterations for any k <= 1024, d <= 512 -- against the
high-precision reference on the cases of tests/lloyd_wide_cases.py (k * d > 8192), bit for bit against mused_kmeans_lloyd
on every case both accept, run to run, the empty-cluster flag, the wrapper with and without MUSED_KMEANS_WIDE=host, a
two-window pipeline run, the argument checks, and the E step it shares with mused_kmeans_lloyd and mused_kmeans_assign."""
import ctypes as C
import functools

import numpy as np
import pytest

import lloyd_cases as lc
import lloyd_wide_cases as lw

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_lloyd import (INFO_SENT, LAB_SENT, MUSED_ERR_ARG, Buffers, P, S, assert_matches_reference,  # noqa: E402
                            bits, dev)
from test_gpu_lloyd import first_run as narrow_first_run  # noqa: E402

WIDE = "mused_kmeans_lloyd_wide"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class WideBuffers(Buffers):
    """The arguments of a call with the workspace mused_kmeans_lloyd_wide asks for (0xFF bytes).  For a shape it rejects:
    its formula (include/mused_hip.h does not fix one; csrc/kmeans.hip: the narrow entry's plus k x d shifts)."""

    def __init__(self, X, mean, C0, ld=0):
        from mused_amd import _lib

        super().__init__(X, mean, C0, ld)
        self.ws_bytes = int(_lib.lib().mused_kmeans_wide_ws_bytes(self.n, self.d, self.k))
        if self.ws_bytes < 0:
            self.ws_bytes = int(_lib.lib().mused_kmeans_ws_bytes(self.n, self.d, self.k)) + 8 * self.k * self.d
        self.ws = torch.full((self.ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda")


def run_wide(c):
    """mused_kmeans_lloyd_wide on a case -> (labels, centres, info), the guard bands checked."""
    from mused_amd import _lib

    X, mean, C0, tol = lc.inputs(c)
    b = WideBuffers(X, mean, C0, c.ld)
    _lib.call(WIDE, *b.args(tol, c.max_iter))
    return b.read()


_RUNS = {}


def first_run(c):
    if c not in _RUNS:
        _RUNS[c] = run_wide(c)
    return _RUNS[c]


def assert_same_bits(a, b, what):
    assert a[2] == b[2], f"{what}: info {a[2]} against {b[2]}"
    assert np.array_equal(a[0], b[0]), f"{what}: {np.count_nonzero(a[0] != b[0])} labels differ"
    assert np.array_equal(bits(a[1]), bits(b[1])), f"{what}: the centres differ in their bits"


# ---- 1. the wide cases against the reference ----------------------------------------------------------------------
@pytest.mark.parametrize("c", lw.EXACT, ids=[c.name for c in lw.EXACT])
def test_wide_case_is_the_references(c):
    assert c.k * c.d > 8192
    got = first_run(c)
    r = lc.reference(c)
    if c in lw.MAX_ITER:
        assert got[2][:2] == [c.max_iter, 0]
    if c is lw.FORCED_TOL:
        assert got[2][:2] == [lw.FORCED_TOL_ITER, 2]
    assert r.empty == 0
    assert_matches_reference(c, got)


def test_one_case_runs_pitched():
    assert [(c.name, c.ld - c.d) for c in lw.TABLE if c.ld] == [(lw.PITCHED, 3)]


# ---- 2. the narrow entry's bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", lc.EXACT, ids=[c.name for c in lc.EXACT])
def test_narrow_shapes_give_the_narrow_entrys_bits(c):
    """Every sum of the wide kernels is taken in the order of the kernels behind mused_kmeans_lloyd, so on the shapes both
    accept (k * d <= 8192) labels, info and the centres' bits are the same."""
    assert_same_bits(run_wide(c), narrow_first_run(c), c.name)


# ---- 3. run to run ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_ref_s1", "wide_k1024_s0"])
def test_two_runs_give_the_same_bits(name):
    c = next(c for c in lw.TABLE if c.name == name)
    assert_same_bits(run_wide(c), first_run(c), name)


# ---- 4. the empty flag past the old limit -------------------------------------------------------------------------
def test_empty_cluster_raises_the_flag():
    assert lc.reference(lw.EMPTY).empty == 1
    _, _, info = run_wide(lw.EMPTY)
    assert info[2] == 1


def test_wrapper_leaves_the_device_path_on_an_empty_cluster(monkeypatch):
    """The rows of wide_min_s0 through perform_clustering_on_device, the last seed moved to 1e3 on its way to the Lloyd
    iterations: the wide entry runs once and reports the empty cluster, the window is counted and scikit-learn's KMeans
    gives the labels."""
    from sklearn.cluster import KMeans

    from mused_amd import _lib
    from mused_amd import matrix_operations as mo

    c = lw.TABLE[0]
    X = lc.inputs(c)[0]
    infos, sk_calls = [], []
    real_call, real_lloyd, real_sk = _lib.call, mo._km_lloyd, mo.perform_clustering

    def call(name, *args):
        real_call(name, *args)
        if name.startswith("mused_kmeans_lloyd"):
            infos.append((name, list(args[10])))

    def lloyd(Xd, n, d, k, mean_d, cen_d, tol, st):
        cen_d[-1] = 1e3
        return real_lloyd(Xd, n, d, k, mean_d, cen_d, tol, st)

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(mo, "_km_lloyd", lloyd)
    monkeypatch.setattr(mo, "perform_clustering", lambda *a: sk_calls.append(1) or real_sk(*a))
    monkeypatch.delenv("MUSED_KMEANS_SEED", raising=False)
    monkeypatch.delenv("MUSED_KMEANS_WIDE", raising=False)
    before = mo.km_fallbacks
    got = mo.perform_clustering_on_device(torch.tensor(X, device="cuda"), c.k, c.seed)
    print(f"lloyd calls {infos} scikit-learn calls {sk_calls}")
    assert len(infos) == 1 and infos[0][0] == WIDE and infos[0][1][2] == 1
    assert sk_calls == [1] and mo.km_fallbacks == before + 1
    assert np.array_equal(got, KMeans(c.k, random_state=c.seed).fit_predict(X))


# ---- 5. the wrapper -----------------------------------------------------------------------------------------------
# none of these raised the seed kernel's ambiguity flag on the device
WRAPPER_CASES = ([(n, d, k, s) for n, d, k in [(2000, 100, 150), (2049, 256, 40), (1500, 60, 140)] for s in range(3)]
                 + [(20000, 100, 150, 0)])


@functools.lru_cache(maxsize=None)
def blob_rows(n, d, k, seed):
    from sklearn.datasets import make_blobs

    X = np.ascontiguousarray(make_blobs(n, d, centers=k, random_state=seed)[0], dtype=np.float64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def sk_labels(n, d, k, seed):
    from sklearn.cluster import KMeans

    return KMeans(n_clusters=k, random_state=seed).fit_predict(blob_rows(n, d, k, seed))


@pytest.mark.parametrize("n,d,k,seed", WRAPPER_CASES)
def test_clustering_without_a_host_copy(n, d, k, seed, monkeypatch):
    from mused_amd import _lib
    from mused_amd import matrix_operations as mo

    X = blob_rows(n, d, k, seed)
    copies, names = [], []
    real_copy, real_call = mo._km_host_copy, _lib.call
    monkeypatch.setattr(mo, "_km_host_copy", lambda *a: copies.append(1) or real_copy(*a))
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real_call(name, *a))
    monkeypatch.delenv("MUSED_KMEANS_SEED", raising=False)
    monkeypatch.delenv("MUSED_KMEANS_WIDE", raising=False)
    Xd = torch.tensor(X, device="cuda")
    before = mo.km_fallbacks
    got = mo.perform_clustering_on_device(Xd, k, seed)
    assert np.array_equal(got, sk_labels(n, d, k, seed))
    assert copies == [] and mo.km_fallbacks == before   # the embedding never went to the host
    assert [x for x in names if "lloyd" in x] == [WIDE]
    # the switch: the window goes to scikit-learn on a host copy and is counted, as before the wide entry existed
    monkeypatch.setenv("MUSED_KMEANS_WIDE", "host")
    del names[:]
    host = mo.perform_clustering_on_device(Xd, k, seed)
    assert copies == [1] and mo.km_fallbacks == before + 1 and names == []
    assert np.array_equal(host, got)


def test_host_seeded_path_reaches_the_wide_entry(monkeypatch):
    """MUSED_KMEANS_SEED=host (and the seed kernel's ambiguity flag) seed on the host and iterate on the device: _km_lloyd
    routes by shape there too."""
    from mused_amd import _lib
    from mused_amd import matrix_operations as mo

    n, d, k, seed = WRAPPER_CASES[0]
    names = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real_call(name, *a))
    monkeypatch.setenv("MUSED_KMEANS_SEED", "host")
    monkeypatch.delenv("MUSED_KMEANS_WIDE", raising=False)
    before = mo.km_fallbacks
    got = mo.perform_clustering_on_device(torch.tensor(blob_rows(n, d, k, seed), device="cuda"), k, seed)
    assert names == [WIDE] and mo.km_fallbacks == before   # asked for, not a fallback
    assert np.array_equal(got, sk_labels(n, d, k, seed))


# ---- 6. the window loop -------------------------------------------------------------------------------------------
def test_two_windows_of_a_stream_stay_on_the_device(monkeypatch):
    """Two windows (W = 400, reduced_dim 100, k_basis 10) of synth.blob_stream(800, 32, seed 1, 100 centres): 96 and 98
    distinct labels, so k * d = 9600 and 9800.  On the CPU oracle's embedding of the two windows, from scikit-learn's
    k-means++ seeds, lloyd_reference converges strictly in 3 and 3 iterations with scikit-learn's labels, no empty
    cluster, e-margins 2.1e-3 and 2.9e-3 and s-margins 8.5e4 and 9.9e4 (the table's bounds: 1e-9 and 1e-6), and the CPU
    replay of k-means++ with the host's draws picks scikit-learn's rows.  Seed 1, not 0: in the first window of seed 0 two
    candidates for centre 83 on different rows have the same potential to the last bit, the seed kernel says so and that
    window is seeded on the host (one counted fallback that has nothing to do with k * d)."""
    from mused_amd import matrix_operations as mo
    from mused_amd import synth
    from mused_amd.pipeline import StreamPipeline

    W, ell, k_basis, seed = 400, 100, 10, 1
    X, labels = synth.blob_stream(2 * W, 32, seed, n_centres=100)
    assert [len(np.unique(labels[i * W:(i + 1) * W])) for i in range(2)] == [96, 98]
    monkeypatch.delenv("MUSED_KMEANS_SEED", raising=False)

    def run():
        with StreamPipeline(W, ell, k_basis, seed, "sSVDMC", modality_types=[""]) as pipe:
            return np.asarray(pipe.run([X.astype(np.float64)], labels), dtype=np.int64)

    monkeypatch.delenv("MUSED_KMEANS_WIDE", raising=False)
    before = mo.km_fallbacks
    dev = run()
    assert mo.km_fallbacks == before
    monkeypatch.setenv("MUSED_KMEANS_WIDE", "host")
    host = run()
    assert mo.km_fallbacks == before + 2
    assert len(dev) == 2 * W and np.array_equal(dev, host)


# ---- 7. rejected arguments ----------------------------------------------------------------------------------------
def test_bad_arguments_rejected_without_launch():
    """k = 1025, d = 513, k > n, ld < d and a workspace one byte short: MUSED_ERR_ARG, and labels, centres and info untouched."""
    from mused_amd import _lib

    lib = _lib.lib()
    rng = np.random.default_rng(0)
    for n, d, k, over, msg in [(1100, 8, 1025, {}, b"k <= 1024 and d <= 512"), (40, 513, 17, {}, b"k <= 1024 and d <= 512"),
                               (16, 482, 17, {}, b"bad arguments"), (300, 482, 17, {"ld": 481}, b"bad arguments"),
                               (300, 482, 17, {"ws_bytes": -1}, b"workspace too small")]:
        X, C0 = rng.standard_normal((n, d)), rng.standard_normal((k, d))
        b = WideBuffers(X, X.mean(axis=0), C0)
        if "ws_bytes" in over:
            over = {"ws_bytes": b.ws_bytes - 1}
        assert lib.mused_kmeans_lloyd_wide(*b.args(1e-4, 300, **over)) == MUSED_ERR_ARG
        assert msg in lib.mused_last_error(), lib.mused_last_error()
        lab, cen, info = b.read()
        assert (lab == LAB_SENT).all() and info == [INFO_SENT] * 4
        assert np.array_equal(bits(cen), bits(C0))


# ---- 8. one E step behind the three entries -----------------------------------------------------------------------
SHARED_E_STEP = [(WIDE, 300, 482, 17),                   # k d = 8194, the last chunk holds 44 rows
                 (WIDE, 1100, 16, 1024),                 # mused_kmeans_assign walks two centre tiles (1016 + 8), Lloyd one
                 ("mused_kmeans_lloyd", 300, 16, 40)]    # the staged kernel, 64 rows per sub-tile


@pytest.mark.parametrize("entry,n,d,k", SHARED_E_STEP, ids=[f"{e}-{n}x{d}x{k}" for e, n, d, k in SHARED_E_STEP])
def test_assign_gives_the_lloyd_entrys_final_labels(entry, n, d, k):
    """The three entries promise one E step (first-minimum rule, centre norms and tiles: csrc/kmeans_common.h; the streamed
    kernels of csrc/kmeans.hip and csrc/minibatch.hip are copies of each other).  With mean = 0 the centring is exact
    (Xc == X) and with max_iter = 1 a Lloyd entry ends with an E step on the centres it returns, so mused_kmeans_assign on
    those centres gives its labels element for element.  Gaussian rows of tests/lloyd_cases.py (continuous: no two
    distances tie), seeded with their first k rows (each seed keeps at least itself: no empty cluster)."""
    from mused_amd import _lib

    lib = _lib.lib()
    if entry != WIDE:
        assert lib.mused_kmeans_assign_rows(d, k) == 64
    X = lc.inputs(lc.Case("shared_e_step", n, d, k, 0, 0))[0]
    b = (WideBuffers if entry == WIDE else Buffers)(X, np.zeros(d), X[:k])
    _lib.call(entry, *b.args(lc.sklearn_tolerance(X), 1))
    lab, cen, info = b.read()
    assert info[1] != 1, "max_iter = 1 converged strictly on this case, so no final E step ran: pick another seed"
    assert info[0] == 1 and info[2] == 0, info
    Xd, Cd = dev(X), dev(cen)
    got = torch.full((n,), LAB_SENT, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.mused_mbkm_ws_bytes(n, d, k)), dtype=torch.uint8, device="cuda")
    _lib.call("mused_kmeans_assign", P(Xd), d, n, d, k, P(Cd), P(got), P(ws), ws.numel(), S())
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), lab), f"{np.count_nonzero(got.cpu().numpy() != lab)} labels differ"
