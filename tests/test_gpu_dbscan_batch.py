"""The reference's batch approach "DBSCAN_batch" (process_batch_data, main.py:132-167) with DBSCAN on the device embedding:
the labels of the reference's own run (tests/golden/make_dbscan_golden.py), without the host DBSCAN and without a
fallback; MUSED_DBSCAN=host, the former path, gives the same labels."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDENS = ["batch_dbscan_blob_s0_e150_m2", "batch_dbscan_blob_s0_e050_m5", "batch_dbscan_sed4_s7_e150_m2"]
# (clusters, noise rows) of the reference's runs
SUMMARY = {"batch_dbscan_blob_s0_e150_m2": (4, 0), "batch_dbscan_blob_s0_e050_m5": (38, 2683),
           "batch_dbscan_sed4_s7_e150_m2": (8, 1984)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _inputs(g):
    from mused_amd import synth

    n, d, ell, k, seed, n_clusters, ms = (int(x) for x in g["meta"])
    kind = str(g["kind"])
    if kind == "blob":
        X, labels = synth.blob_stream(n, d, seed, n_centres=4)
        mods, types_ = [X.astype(np.float64)], [""]
    else:
        types_ = ["location", "time", "username", "text"]
        cols, labels = synth.metadata_stream(n, seed)
        cols["text"], _ = synth.text_stream(n, seed)
        mods = [cols[t] for t in types_]
    assert types_ == [str(x) for x in g["types"]]
    assert [synth.array_digest(m) if m.dtype.kind == "f" else "" for m in mods] == [str(x) for x in g["input_digest"]]
    return mods, types_, labels, (ell, k, n_clusters, seed, float(g["eps"]), ms)


def _run(g, timings=None):
    from mused_amd.pipeline import process_batch_data

    mods, types_, labels, (ell, k, n_clusters, seed, eps, ms) = _inputs(g)
    res = process_batch_data({}, mods, types_, ell, k, n_clusters, seed, "DBSCAN_batch", labels, 0.0, "all", False, eps,
                             ms, 3, 2000, timings=timings)
    return np.asarray(res["all_clusters"])


@pytest.mark.parametrize("name", GOLDENS)
def test_dbscan_batch_labels_match_reference_golden(name, monkeypatch):
    from mused_amd import matrix_operations as mo

    g = load_golden(name)
    want = g["all_clusters"]
    assert (len(set(want[want >= 0])), int((want < 0).sum())) == SUMMARY[name]
    margin, tau = g["margin"]
    assert tau < margin                       # the reference's own embedding decides every pair beyond rounding

    def no_host(*a, **k):
        raise AssertionError("DBSCAN_batch called the host DBSCAN")

    monkeypatch.setattr(mo, "perform_dbscan_clustering", no_host)
    before = mo.dbscan_fallbacks
    timings = {}
    got = _run(g, timings)
    assert mo.dbscan_fallbacks == before
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert timings["clustering"] > 0


@pytest.mark.parametrize("name", GOLDENS)
def test_dbscan_batch_host_switch_gives_the_same_labels(name, monkeypatch):
    from mused_amd import matrix_operations as mo

    g = load_golden(name)
    calls = []
    real = mo.perform_dbscan_clustering
    monkeypatch.setattr(mo, "perform_dbscan_clustering", lambda *a, **k: calls.append(1) or real(*a, **k))
    monkeypatch.setenv("MUSED_DBSCAN", "host")
    assert np.array_equal(_run(g), g["all_clusters"])
    assert calls == [1]
