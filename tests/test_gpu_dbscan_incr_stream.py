"""process_streaming_data(..., "DBSCAN_incr", ...) against a host replay of the same windows: the pipeline's own per-window
embeddings (taken from the inserts it makes), sklearn's DBSCAN.fit_predict on their concatenation, the last W labels, then
the host's Hungarian matching with min_overlap = 3 (main.py:87-91, :110).  `all_clusters` must be equal exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, ELL, K = 256, 8, 5
# (eps, min_samples).  1.5, 2: the reference's values -- the rows of these embeddings have entries of the order W^-1/2, so every
# row lies within 1.5 of every other and each refit is one cluster.  0.15, 3: an eps of the embeddings' own scale, at which a
# window splits into about 20 clusters with border and noise rows and inserts merge clusters of earlier windows.
PARAMS = [(1.5, 2), (0.15, 3)]
# The stream seed was picked so that no insert of any of these streams raises the kernel's ambiguity flag (a pair of embedding rows
# within rounding of eps): the tests assert that no insert went to the host.
SEED = 0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _replay(embeddings, eps, ms):
    from sklearn.cluster import DBSCAN

    from mused_amd import matrix_operations as mo

    out, prev = [], None
    for t in range(len(embeddings)):
        labels = DBSCAN(eps=eps, min_samples=ms).fit_predict(np.concatenate(embeddings[:t + 1]))[-W:]
        matched = mo.match_clusters(prev, labels, method="hungarian", min_overlap=3)
        if matched is None or len(matched) == 0:   # main.py:114-116
            matched = np.full(W, 0)
        prev = matched
        out.extend(matched)
    return np.array(out)


@pytest.mark.parametrize("eps, ms", PARAMS)
@pytest.mark.parametrize("ratio", [1, 2])
def test_stream_equals_the_host_replay(ratio, eps, ms, monkeypatch):
    from mused_amd import incdbscan, synth
    from mused_amd import matrix_operations as mo
    from mused_amd.pipeline import process_streaming_data

    n = W + 3 * (W // ratio)                               # 4 windows
    X, labels = synth.blob_stream(n, 16, SEED, n_centres=4)
    embeddings = []
    real = incdbscan.IncrementalDBSCAN.insert

    def recording(self, rows):
        embeddings.append(rows.cpu().numpy().copy() if isinstance(rows, torch.Tensor) else np.array(rows))
        return real(self, rows)

    monkeypatch.setattr(incdbscan.IncrementalDBSCAN, "insert", recording)
    before = mo.dbscan_incr_fallbacks
    res = process_streaming_data({}, [X.astype(np.float64)], [""], W, ELL, K, 4, 0, "DBSCAN_incr", labels, ratio, 0.0, "types",
                                 False, eps, ms)
    assert mo.dbscan_incr_fallbacks == before
    assert len(embeddings) == 4 and all(e.shape[0] == W and e.dtype == np.float64 for e in embeddings)
    got = np.asarray(res["all_clusters"])
    assert got.shape == (4 * W,) and np.array_equal(got, _replay(embeddings, eps, ms))


def test_unknown_approach_is_still_rejected():
    from mused_amd.pipeline import StreamPipeline

    with pytest.raises(ValueError, match="is not on the device hot path"):
        StreamPipeline(W, ELL, K, 0, "DBSCAN_centr")
