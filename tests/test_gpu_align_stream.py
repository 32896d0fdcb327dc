"""process_streaming_data(..., align_embeddings=True) for the two chained approaches against a host replay: the tensors the
stream's clusterer receives (recorded from its insert / partial_fit) must be the SciPy chain
aligned_t = E_t @ orthogonal_procrustes(E_t[:W - s], aligned_{t-1}[s:])[0] over the UNALIGNED embeddings E_t of a second run
with align_embeddings=False, within 4 u per window (mused_amd.procrustes.unit) accumulated along the chain."""
import numpy as np
import pytest
from scipy.linalg import orthogonal_procrustes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, ELL, K, RATIO = 256, 8, 5, 2
S = W // RATIO                      # rows a window moves on: windows t - 1 and t share W - S rows
SEED = 0
APPROACHES = ["DBSCAN_incr", "sSVDMC_mini"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(approach, monkeypatch, **kw):
    """One stream of four windows -> (results, the (W, ELL) arrays the clusterer was handed, in window order)."""
    from mused_amd import cluster, incdbscan, synth
    from mused_amd.pipeline import process_streaming_data

    n = W + 3 * S
    X, labels = synth.blob_stream(n, 16, SEED, n_centres=4)
    seen = []

    def host(rows):
        return rows.cpu().numpy().copy() if isinstance(rows, torch.Tensor) else np.array(rows)

    with monkeypatch.context() as mp:
        if approach == "DBSCAN_incr":
            real = incdbscan.IncrementalDBSCAN.insert
            mp.setattr(incdbscan.IncrementalDBSCAN, "insert", lambda self, rows: (seen.append(host(rows)), real(self, rows))[1])
        else:
            real = cluster.MiniBatchKMeans.partial_fit
            mp.setattr(cluster.MiniBatchKMeans, "partial_fit", lambda self, rows, *a, **k: (seen.append(host(rows)), real(self, rows, *a, **k))[1])
        res = process_streaming_data({}, [X.astype(np.float64)], [""], W, ELL, K, 4, 0, approach, labels, RATIO, 0.0, "types", False,
                                     0.15, 3, **kw)
    assert len(seen) == 4 and all(e.shape == (W, ELL) and e.dtype == np.float64 for e in seen)
    return res, seen


@pytest.fixture(scope="module")
def runs():
    """approach -> (aligned run, align_embeddings=False run, a run that never heard of the argument), made once."""
    from mused_amd import matrix_operations as mo

    out = {}
    mp = pytest.MonkeyPatch()
    try:
        for a in APPROACHES:
            before = mo.procrustes_fallbacks
            on = _run(a, mp, align_embeddings=True)
            out[a] = (on, _run(a, mp, align_embeddings=False), _run(a, mp), mo.procrustes_fallbacks - before)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("approach", APPROACHES)
def test_clusterer_receives_the_scipy_chain(runs, approach):
    from mused_amd import procrustes as pr

    (res, got), (_, raw), _, fallbacks = runs[approach]
    assert fallbacks == 0
    assert np.array_equal(got[0], raw[0])                     # window 0 defines the frame: handed over as it is
    chain, d = [raw[0]], 0.0                                  # d: how far the device's chain may have left the replay's (entrywise)
    for t in range(1, 4):
        E = raw[t]
        A = E[:W - S]
        prod = (ELL + 2) * 2.0 ** -52 * np.linalg.norm(E, axis=1).max()    # E R, two evaluations of an ELL-term sum
        # against SciPy on the DEVICE's own previous window: one Procrustes problem, 4 u
        B_dev = got[t - 1][S:]
        R_own = orthogonal_procrustes(A, B_dev)[0]
        row1 = np.abs(E).sum(1).max()
        assert np.abs(got[t] - E @ R_own).max() <= row1 * 4 * pr.unit(A, B_dev) + prod
        # against the replay's chain: B differs by at most d entrywise, |dM|_F <= |A|_F sqrt(m r) d, |dR| <= |dM|_F / sigma_r
        B = chain[-1][S:]
        R = orthogonal_procrustes(A, B)[0]
        sig_r = np.linalg.svd(A.T @ B, compute_uv=False)[-1]
        assert sig_r > 2.0 ** -10 * np.linalg.svd(A.T @ B, compute_uv=False)[0]      # far from the flag
        tol_R = 4 * pr.unit(A, B) + np.linalg.norm(A) * np.sqrt(A.size) * d / sig_r
        d = row1 * tol_R + prod
        chain.append(E @ R)
        err = np.abs(got[t] - chain[-1]).max()
        print(f"{approach} window {t}: |device - replay| = {err:.3e}, allowed {d:.3e}")
        assert err <= d
        # an isometry of the window: the Gram matrix of its rows is unchanged to rounding
        # (|R R^T - I|_2 <= ELL max|R^T R - I| <= 8 ELL^2 2^-52, and the rounding of the two products of every entry)
        assert np.abs(got[t] @ got[t].T - E @ E.T).max() <= (8 * ELL * ELL + 4 * (ELL + 2)) * 2.0 ** -52 * np.linalg.norm(E, axis=1).max() ** 2


@pytest.mark.parametrize("approach", APPROACHES)
def test_residual_lists(runs, approach):
    (res, got), (_, raw), _, _ = runs[approach]
    r, u = res["alignment_residuals"], res["alignment_unaligned"]
    assert len(r) == 4 and len(u) == 4 and np.isnan(r[0]) and np.isnan(u[0])
    for t in range(1, 4):
        assert 0.0 <= r[t] <= u[t]
        A, B = raw[t][:W - S], got[t - 1][S:]
        nb = np.linalg.norm(B)
        assert abs(u[t] - np.linalg.norm(A - B) / nb) <= 1e-12 * max(u[t], 1.0)
        assert abs(r[t] - np.linalg.norm(got[t][:W - S] - B) / nb) <= 1e-12 * max(u[t], 1.0)
    assert np.asarray(res["all_clusters"]).shape == (4 * W,)


@pytest.mark.parametrize("approach", APPROACHES)
def test_off_is_the_run_that_never_heard_of_it(runs, approach):
    _, (res_off, raw), (res_plain, plain), _ = runs[approach]
    assert "alignment_residuals" not in res_off and "alignment_residuals" not in res_plain
    assert np.array_equal(np.asarray(res_off["all_clusters"]), np.asarray(res_plain["all_clusters"]))
    assert all(np.array_equal(a, b) for a, b in zip(raw, plain))


def test_host_kmeans_gets_the_same_treatment(monkeypatch):
    """MUSED_KMEANS=host: scikit-learn's MiniBatchKMeans takes the host copy, aligned by SciPy."""
    from sklearn.cluster import MiniBatchKMeans as Sk

    from mused_amd import procrustes as pr
    from mused_amd import synth
    from mused_amd.pipeline import process_streaming_data

    monkeypatch.setenv("MUSED_KMEANS", "host")
    seen = []
    real = Sk.partial_fit
    monkeypatch.setattr(Sk, "partial_fit", lambda self, X, *a, **k: (seen.append(np.array(X)), real(self, X, *a, **k))[1])
    X, labels = synth.blob_stream(W + 3 * S, 16, SEED, n_centres=4)
    args = ({}, [X.astype(np.float64)], [""], W, ELL, K, 4, 0, "sSVDMC_mini", labels, RATIO, 0.0, "types", False, 0.15, 3)
    res = process_streaming_data(*args, align_embeddings=True)
    on, seen = seen, []
    process_streaming_data(*args)
    assert len(on) == 4 and len(seen) == 4 and np.array_equal(on[0], seen[0])
    for t in range(1, 4):
        A, B = seen[t][:W - S], on[t - 1][S:]
        R = orthogonal_procrustes(A, B)[0]
        allowed = np.abs(seen[t]).sum(1).max() * 4 * pr.unit(A, B) + (ELL + 2) * 2.0 ** -52 * np.linalg.norm(seen[t], axis=1).max()
        assert np.abs(on[t] - seen[t] @ R).max() <= allowed
    assert len(res["alignment_residuals"]) == 4 and all(a <= b for a, b in zip(res["alignment_residuals"][1:], res["alignment_unaligned"][1:]))


def test_constructor_refuses_what_cannot_be_aligned():
    from mused_amd.pipeline import StreamPipeline

    with pytest.raises(ValueError, match="share no rows"):
        StreamPipeline(W, ELL, K, 0, "DBSCAN_incr", step_window_ratio=1, align_embeddings=True)
    with pytest.raises(ValueError, match="clusters every window on its own"):
        StreamPipeline(W, ELL, K, 0, "sSVDMC", step_window_ratio=2, align_embeddings=True)
    with pytest.raises(ValueError, match="window_slots must be 1"):
        StreamPipeline(W, ELL, K, 0, "sSVDMC_mini", step_window_ratio=2, n_clusters_total=4, window_slots=2, align_embeddings=True)
