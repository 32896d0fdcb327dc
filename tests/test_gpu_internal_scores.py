"""The public side of csrc/silhouette.hip: metrics_evaluation.compute_internal_metrics / silhouette_samples_on_device,
matrix_operations.select_n_clusters_on_device, and the pipeline's n_clusters_range / internal_scores arguments -- a stream
clustered and judged without one true label."""
import numpy as np
import pytest

import silhouette_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = ["n257_d17_straddle", "singletons", "any_int32_labels", "n1000_d129"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _close(got, ref, score_b, db_b, ch_b):
    assert set(got) == {"silhouette", "davies_bouldin", "calinski_harabasz"}
    assert all(type(v) is float for v in got.values())
    assert abs(got["silhouette"] - ref[0]) <= score_b
    assert abs(got["davies_bouldin"] - ref[1]) <= db_b
    assert abs(got["calinski_harabasz"] - ref[2]) <= ch_b * abs(ref[2])


@pytest.mark.parametrize("name", CASES)
def test_compute_internal_metrics_numpy_and_device_inputs(name):
    from mused_amd import metrics_evaluation as me

    c = next(c for c in sc.CASES if c.name == name)
    ref_s, ref_db, ref_ch = sc.reference(name)
    sb, score_b, db_b, ch_b = sc.bounds(name)
    ref = (float(ref_s.mean()), ref_db, ref_ch)
    _close(me.compute_internal_metrics(c.X, c.labels), ref, score_b, db_b, ch_b)
    Xd, ld = torch.tensor(c.X, device="cuda"), torch.tensor(c.labels.astype(np.int64), device="cuda")
    on_dev = me.compute_internal_metrics(Xd, ld)
    _close(on_dev, ref, score_b, db_b, ch_b)
    assert on_dev == me.compute_internal_metrics(c.X, c.labels)      # the same bits from either kind of input
    s = me.silhouette_samples_on_device(Xd, ld, stream=torch.cuda.Stream())
    assert s.is_cuda and s.dtype == torch.float64
    assert (np.abs(s.cpu().numpy() - ref_s) <= sb).all()


@pytest.mark.parametrize("name,X,labels,text", sc.error_cases(), ids=[e[0] for e in sc.error_cases()])
def test_flags_become_sklearn_errors(name, X, labels, text):
    from mused_amd import metrics_evaluation as me

    for call in (me.compute_internal_metrics, me.silhouette_samples_on_device):
        with pytest.raises(ValueError) as err:
            call(X, labels)
        assert str(err.value) == text


def test_host_switch_returns_sklearn_floats(monkeypatch):
    from sklearn import metrics as skm

    from mused_amd import metrics_evaluation as me

    c = next(c for c in sc.CASES if c.name == "n129_d16")
    monkeypatch.setenv("MUSED_SCORE", "host")
    got = me.compute_internal_metrics(torch.tensor(c.X, device="cuda"), c.labels)
    assert got == {"silhouette": float(skm.silhouette_score(c.X, c.labels)), "davies_bouldin": sc.reference(c.name)[1],
                   "calinski_harabasz": sc.reference(c.name)[2]}
    s = me.silhouette_samples_on_device(c.X, c.labels)
    assert np.array_equal(s.cpu().numpy(), sc.reference(c.name)[0])


def test_selector_on_four_blobs():
    from sklearn import metrics as skm

    from mused_amd import matrix_operations as mo

    X, _ = sc.four_blobs()
    Xd = torch.tensor(X, device="cuda")
    best, labels, scores = mo.select_n_clusters_on_device(Xd, range(2, 8), 0)
    assert best == 4 and sorted(scores) == [2, 3, 4, 5, 6, 7]
    assert np.array_equal(labels, mo.perform_clustering_on_device(Xd, 4, 0))
    for k, s in scores.items():
        lab = mo.perform_clustering_on_device(Xd, k, 0)
        assert abs(s - float(skm.silhouette_score(X, lab))) <= sc.score_bound(X, lab)
    assert mo.select_n_clusters_on_device(Xd, [7, 4, 4, 2], 0, stream=torch.cuda.Stream())[0] == 4
    for bad in ([], [1, 2], [2, 400], [2.0, 3], [True, 3], 5, None):
        with pytest.raises(ValueError):
            mo.select_n_clusters_on_device(Xd, bad, 0)


ARGS = (256, 6, 12, 3, 0)   # window_size, reduced_dim, k_basis, n_clusters_total, seed
TAIL = (1, 0.0, "types", False, 1.5, 2)


@pytest.fixture(scope="module")
def stream():
    from mused_amd import synth

    mods, labels = synth.two_modality_blob_stream(3 * 256, 16, 5, n_centres=3)
    return [np.ascontiguousarray(m) for m in mods], np.asarray(labels)


def test_stream_without_true_labels(stream):
    from mused_amd import metrics_evaluation as me
    from mused_amd.pipeline import StreamPipeline, process_streaming_data

    mods, _ = stream
    res = process_streaming_data({}, mods, ["", ""], *ARGS, "sSVDMC", None, *TAIL, n_clusters_range=(2, 6), internal_scores=True)
    assert len(res["all_clusters"]) == 3 * 256
    assert len(res["chosen_k"]) == 3 and all(type(k) is int and 2 <= k <= 6 for k in res["chosen_k"])
    assert len(res["internal_scores"]) == 3
    # the same run with the trace at hand: the raw labels of every window
    with StreamPipeline(256, 6, 12, 0, "sSVDMC", ["", ""], n_clusters_range=(2, 6), internal_scores=True) as pipe:
        out = pipe.run(mods, None)
        trace, chosen, scores = list(pipe.trace), list(pipe.chosen_k), list(pipe.internal_scores)
    assert np.array_equal(out, res["all_clusters"]) and chosen == res["chosen_k"] and scores == res["internal_scores"]
    dev = [torch.from_numpy(m).cuda() for m in mods]
    with StreamPipeline(256, 6, 12, 0, "sSVDMC", ["", ""]) as again:
        for w in range(3):
            emb = again.window_device([m[w * 256 : (w + 1) * 256] for m in dev])[0]
            torch.cuda.synchronize()
            raw = np.asarray(trace[w]["raw"])
            assert len(np.unique(raw)) == chosen[w]
            E = emb.cpu().numpy().astype(np.float64)
            want = me.compute_internal_metrics(emb, raw)
            _close(scores[w], (want["silhouette"], want["davies_bouldin"], want["calinski_harabasz"]),
                   sc.score_bound(E, raw), sc.davies_bouldin_bound(E, raw), sc.calinski_harabasz_bound(E, raw))


def test_approaches_without_a_k_per_window_refuse(stream, monkeypatch):
    from mused_amd.pipeline import process_batch_data, process_streaming_data

    mods, labels = stream
    for approach in ("sSVDMC_mini", "DBSCAN_incr"):
        with pytest.raises(ValueError):
            process_streaming_data({}, mods, ["", ""], *ARGS, approach, None, *TAIL, n_clusters_range=(2, 6))
    for bad in ((1, 6), (4, 3), (2, 256), (2.0, 6), (2,), 5):
        with pytest.raises(ValueError):
            process_streaming_data({}, mods, ["", ""], *ARGS, "sSVDMC", None, *TAIL, n_clusters_range=bad)
    with pytest.raises(ValueError):
        process_batch_data({}, mods, ["", ""], 6, 12, 3, 0, "DBSCAN_batch", None, 0.0, "types", False, 1.5, 2, 5, 256,
                           n_clusters_range=(2, 6))
    monkeypatch.setenv("MUSED_KMEANS", "host")
    with pytest.raises(ValueError):
        process_streaming_data({}, mods, ["", ""], *ARGS, "sSVDMC", None, *TAIL, n_clusters_range=(2, 6))


def test_batch_chooses_its_k(stream):
    from mused_amd.pipeline import process_batch_data

    mods, _ = stream
    res = process_batch_data({}, mods, ["", ""], 6, 12, 3, 0, "SVDMC_batch", None, 0.0, "types", False, 1.5, 2, 5, 256,
                             n_clusters_range=(2, 5), internal_scores=True)
    assert len(res["chosen_k"]) == 1 and 2 <= res["chosen_k"][0] <= 5
    assert len(np.unique(res["all_clusters"])) == res["chosen_k"][0]
    assert len(res["internal_scores"]) == 1 and -1.0 <= res["internal_scores"][0]["silhouette"] <= 1.0


def test_single_valued_window_records_nans(stream):
    """One true label per window: k-means with k = 1, labels with a single value, no silhouette -- NaNs, no error."""
    from mused_amd.pipeline import process_streaming_data

    mods, labels = stream
    res = process_streaming_data({}, mods, ["", ""], *ARGS, "sSVDMC", np.zeros_like(labels), *TAIL, internal_scores=True)
    assert len(res["internal_scores"]) == 3 and "chosen_k" not in res
    assert all(np.isnan(list(w.values())).all() for w in res["internal_scores"])


def test_defaults_change_nothing(stream):
    """(Passes without the feature's kernels: the default path runs none of them.)"""
    from mused_amd.pipeline import process_streaming_data

    mods, labels = stream
    a = process_streaming_data({}, mods, ["", ""], *ARGS, "sSVDMC", labels, *TAIL)
    b = process_streaming_data({}, mods, ["", ""], *ARGS, "sSVDMC", labels, *TAIL, n_clusters_range=None, internal_scores=False)
    assert np.array_equal(a["all_clusters"], b["all_clusters"])
    assert "chosen_k" not in b and "internal_scores" not in b
