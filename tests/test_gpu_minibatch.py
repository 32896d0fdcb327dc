"""On the GPU: the device MiniBatchKMeans (mused_amd/cluster.py, csrc/minibatch.hip) against scikit-learn's, and the
reference's "sSVDMC_mini" approach (main.py:82-86) through the device pipeline against its golden event labels."""
import hashlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, regen_inputs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MINI_GOLDENS = ["c1_stream_mini_blob_s0", "c1_stream_mini150_blob_s0", "refdef_stream_mini_blob_s0"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _open(name):
    # opened directly: a missing fixture fails instead of skipping
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def _blob_batches(steps, n, d, seed, centres=6):
    rng = np.random.default_rng(seed)
    mu = rng.normal(scale=3.0, size=(centres, d))
    return [mu[rng.integers(0, centres, n)] + rng.normal(size=(n, d)) for _ in range(steps)]


def _against_sklearn(batches, k, seed, to_dev, **kw):
    from sklearn.cluster import MiniBatchKMeans as SkMiniBatch

    from mused_amd.cluster import MiniBatchKMeans

    ours = MiniBatchKMeans(n_clusters=k, random_state=seed, **kw)
    ref = SkMiniBatch(n_clusters=k, random_state=seed, **kw)
    for t, X in enumerate(batches):
        Xd = to_dev(X)
        lab = ours.partial_fit(Xd).predict(Xd)
        lab_ref = ref.partial_fit(X).predict(X)
        assert np.array_equal(lab, lab_ref), f"step {t}: {np.count_nonzero(lab != lab_ref)} labels differ"
        assert np.array_equal(ours.labels_, ref.labels_), f"step {t}"
        assert np.array_equal(ours._counts, ref._counts), f"step {t}: counts differ"
        assert np.array_equal(ours.cluster_centers_, ref.cluster_centers_), f"step {t}: centres differ"
    return ours, ref


def _cuda(X):
    return torch.from_numpy(X).cuda()


@pytest.mark.parametrize("n,d,k", [(500, 16, 4), (500, 50, 150), (2000, 128, 150), (300, 1, 5), (300, 3, 7)])
def test_device_minibatch_bitwise_sklearn(n, d, k):
    """Labels, counts and centres equal scikit-learn's bit for bit over 6 consecutive batches; (2000, 128, 150) is beyond
    the k * d <= 8192 LDS ceiling of the Lloyd path."""
    _against_sklearn(_blob_batches(6, n, d, 0), k, 0, _cuda, batch_size=n)


@pytest.mark.parametrize("n,d,k,steps", [(3000, 512, 64, 3), (4096, 32, 1024, 2)])
def test_device_minibatch_bitwise_sklearn_at_limits(n, d, k, steps):
    """At the declared limits of the device kernels (d = 512: 16-row tiles with 16 lanes per row and a second feature
    accumulator; k = 1024: the centres in three LDS tiles of the E step) on k well-separated blobs."""
    rng = np.random.default_rng(n + d + k)
    mu = 10.0 * rng.normal(size=(k, d))
    batches = [mu[rng.integers(0, k, n)] + 0.1 * rng.normal(size=(n, d)) for _ in range(steps)]
    _against_sklearn(batches, k, 0, _cuda, batch_size=n)


def test_device_minibatch_trim_branch():
    """n = 64, k = 48, reassignment_ratio = 0.5: the argsort trim of the reassignment (tests/test_minibatch_host.py)."""
    rng = np.random.default_rng(1)
    _against_sklearn([rng.normal(size=(64, 8)) for _ in range(12)], 48, 0, _cuda, batch_size=64, reassignment_ratio=0.5)


def test_device_minibatch_numpy_and_strided_inputs():
    """NumPy batches (uploaded by the class) and a strided device view (ld > d), with the init subsample."""
    batches = _blob_batches(8, 400, 24, 3)
    _against_sklearn(batches, 10, 2, lambda X: X, batch_size=128)

    def strided(X):
        big = torch.zeros((X.shape[0], X.shape[1] + 13), dtype=torch.float64, device="cuda")
        big[:, 5 : 5 + X.shape[1]] = torch.from_numpy(X).cuda()
        v = big[:, 5 : 5 + X.shape[1]]
        assert v.stride(0) > v.shape[1]
        return v

    _against_sklearn(batches, 10, 2, strided, batch_size=128)


def test_device_minibatch_rejects_unsupported():
    from mused_amd.cluster import MiniBatchKMeans

    X = _blob_batches(1, 100, 4, 0)[0]
    m = MiniBatchKMeans(4, random_state=0)
    with pytest.raises(ValueError):
        m.partial_fit(torch.from_numpy(X.astype(np.float32)).cuda())
    with pytest.raises(ValueError):
        m.partial_fit(_cuda(X), sample_weight=np.ones(len(X)))
    with pytest.raises(ValueError):
        MiniBatchKMeans(4, random_state=0).partial_fit(_cuda(X[:3]))


@pytest.mark.parametrize("name", MINI_GOLDENS)
@pytest.mark.parametrize("async_labels", [True, False])
def test_mini_stream_event_labels_bit_exact(name, async_labels):
    """Whole-run `all_clusters` of the reference (approach sSVDMC_mini) through StreamPipeline."""
    from mused_amd.pipeline import StreamPipeline

    g = _open(name)
    mods, labels, (n, d, W, ell, k, seed) = regen_inputs(g)
    with StreamPipeline(W, ell, k, seed, "sSVDMC_mini", async_labels=async_labels,
                        n_clusters_total=int(g["n_clusters_total"])) as pipe:
        out = pipe.run(mods, labels)
        assert pipe.km_device_windows == n // W
    assert np.array_equal(out.astype(np.int64), g["all_clusters"])
    assert hashlib.sha256(out.astype(np.int64).tobytes()).hexdigest() == str(g["labels_sha"])


def test_mini_stream_window_slots_and_process_streaming_data():
    """Four window slots (adjacency / eigenstep of consecutive windows overlap, the clusterer stays in window order), and
    the same labels through process_streaming_data."""
    from mused_amd import pipeline

    g = _open("c1_stream_mini150_blob_s0")
    mods, labels, (n, d, W, ell, k, seed) = regen_inputs(g)
    ncl = int(g["n_clusters_total"])
    with pipeline.StreamPipeline(W, ell, k, seed, "sSVDMC_mini", window_slots=4, n_clusters_total=ncl) as pipe:
        assert pipe._nslots == 4
        out = pipe.run(mods, labels)
    assert np.array_equal(out.astype(np.int64), g["all_clusters"])
    res = pipeline.process_streaming_data({}, [mods[0]], [""], W, ell, k, ncl, seed, "sSVDMC_mini", labels, 1, 0.0, "all",
                                          False, 1.5, 2)
    assert np.array_equal(np.asarray(res["all_clusters"], dtype=np.int64), g["all_clusters"])


def test_mini_requires_n_clusters_total():
    from mused_amd.pipeline import StreamPipeline

    with pytest.raises(ValueError, match="n_clusters_total"):
        StreamPipeline(500, 16, 50, 0, "sSVDMC_mini")
