"""Weighted modality fusion through the eigenstep: S = sum_m w_m A_m instead of the OR mask, and any square real matrix behind
`perform_svd_reduction_valued`.

  * M = 1, w = 1.0 is the binary eigenstep bit for bit (embedding, sigma, components) on either SpMM kernel, with the svd_flip
    signs in the stores of the last product (no components asked for) and without.
  * Against scikit-learn's TruncatedSVD and the oracle's restatement of it, on S built on the host from the oracle's adjacency
    per modality.  Tolerances: the project's own for the eigenstep (tests/test_gpu_path.py: sigma rtol 1e-8; embedding
    atol 1e-7 max|e_ref| on the columns with sigma > 1e-6 sigma_1).
  * The dense entry.  Where the matrix is rank deficient (the 4 x 4 constant matrix has ONE nonzero singular value) the
    singular values below 1e-6 sigma_1 are rounding noise of size eps * sigma_1 in either implementation: they are compared
    with atol = 1e-8 sigma_1, the others with the rtol above.
  * One engine, masks in different tensors and different weights from call to call, a binary call in between: every result
    is a fresh engine's bit for bit (the recorded graph reads masks and weights through the handle).
  * The pipeline with `modality_weights` against a host restatement written here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WEIGHTS = ((1.0, 1.0, 1.0), (1.0, 0.5, 0.25), (0.3, 0.7, 1.9))


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    yield _lib
    _lib.call("mused_spmm_force_path", -1)


def bits(t):
    return t.cpu().numpy().view(np.int64)


_MODS = {}


def modalities(n, k):
    """Three blob modalities of n rows (two share a label sequence) and the oracle's adjacency of each, computed once."""
    if (n, k) not in _MODS:
        from mused_amd import synth
        from oracle import mo_oracle as omo

        mods, _ = synth.two_modality_blob_stream(n, 16, 3, n_centres=4)
        third, _ = synth.blob_stream(n, 12, 4, n_centres=5)
        mods = [m.astype(np.float64) for m in mods + [third]]
        _MODS[(n, k)] = (mods, [omo.create_adjacency_matrix(m, "", k) for m in mods])
    return _MODS[(n, k)]


def weighted_sum(adjs, weights):
    """S on the host: per entry, from 0.0, the weights of the modalities that have the edge, in modality order."""
    S = np.zeros(adjs[0].shape)
    for A, w in zip(adjs, weights):
        S = np.where(A != 0, S + w, S)
    return S


def device_parts(eng, mods, k):
    return [eng.knn_adjacency(torch.from_numpy(m).cuda(), k) for m in mods]


def check_against(emb, sig, e_ref, s_ref, rank_deficient=False):
    s_ref = np.asarray(s_ref)
    big = s_ref > 1e-6 * s_ref[0]
    if rank_deficient:
        np.testing.assert_allclose(sig, s_ref, rtol=1e-8, atol=1e-8 * s_ref[0])
    else:
        np.testing.assert_allclose(sig, s_ref, rtol=1e-8)
    np.testing.assert_allclose(emb[:, big], e_ref[:, big], atol=1e-7 * np.abs(e_ref).max())


@pytest.mark.parametrize("path", [0, 1])
def test_one_modality_weight_one_is_the_binary_eigenstep(L, path):
    from mused_amd.engine import WindowEngine

    n, k, ell = 257, 5, 16
    mods, _ = modalities(n, k)
    L.call("mused_spmm_force_path", path)
    assert L.lib().mused_spmm_binary_path(n, ell + 10, ell + 10, ell + 10, 0, 0) == path
    eng = WindowEngine(n)
    try:
        adj = device_parts(eng, mods[:1], k)[0]
        for comps in (False, True):
            ref = eng.svd_reduce(eng.fuse([adj]), ell, 0, nnz_cap=n * k, want_components=comps)
            got = eng.svd_reduce(eng.fuse_weighted([adj], [1.0]), ell, 0, nnz_cap=n * k, want_components=comps)
            assert len(got) == len(ref) == (3 if comps else 2)
            for g, r in zip(got, ref):
                assert np.isfinite(r.cpu().numpy()).all() and np.array_equal(bits(g), bits(r))
    finally:
        eng.close()


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("n,k,M", [(600, 15, 3), (257, 5, 2)])
def test_against_truncated_svd(L, n, k, M, weights):
    from sklearn.decomposition import TruncatedSVD

    from mused_amd.engine import WindowEngine
    from oracle import mo_oracle as omo

    L.call("mused_spmm_force_path", -1)
    ell, seed = 12, 7
    mods, adjs = modalities(n, k)
    w = list(weights[:M])
    S = weighted_sum(adjs[:M], w)
    eng = WindowEngine(n)
    try:
        wadj = eng.fuse_weighted(device_parts(eng, mods[:M], k), w)
        assert np.array_equal(wadj.to_dense().cpu().numpy().view(np.int64), S.view(np.int64))
        assert np.array_equal(wadj.pattern.to_dense().cpu().numpy() != 0, S != 0)
        emb, sig = eng.svd_reduce(wadj, ell, seed, nnz_cap=n * k * M)
        flags, _ = eng.rsvd_status()
        assert flags == 0
        emb, sig = emb.cpu().numpy(), sig.cpu().numpy()
    finally:
        eng.close()
    e_ref, s_ref, _ = omo.randomized_svd_reduce(S, ell, seed)
    check_against(emb, sig, e_ref, s_ref)
    tsvd = TruncatedSVD(n_components=ell, random_state=seed)
    e_sk = tsvd.fit_transform(S)
    check_against(emb, sig, e_sk, tsvd.singular_values_)


def sk_reduce(matrix, reduced_dim, seed):
    from sklearn.decomposition import TruncatedSVD

    t = TruncatedSVD(n_components=min(reduced_dim, matrix.shape[1] - 1), random_state=seed)
    return t.fit_transform(matrix), t.singular_values_


def test_dense_entry_constant_matrix(L):
    from mused_amd import matrix_operations as mo
    from mused_amd.engine import default_engine

    A = np.full((4, 4), 0.5)
    e_ref, s_ref = sk_reduce(A, 2, 0)
    got = mo.perform_svd_reduction_valued(A, 2, 0)
    assert got.shape == (4, 2) and got.dtype == np.float64
    _, sig = default_engine(4).svd_reduce_dense(A, 2, 0)
    check_against(got, sig.cpu().numpy(), e_ref, s_ref, rank_deficient=True)
    with pytest.raises(NotImplementedError):
        mo.perform_svd_reduction(A, 2, 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dense_entry_sparse_gaussian(L, dtype):
    from mused_amd import matrix_operations as mo
    from mused_amd.engine import WindowEngine

    rng = np.random.default_rng(9)
    n = 600
    A = np.where(rng.random((n, n)) < 0.05, rng.standard_normal((n, n)), 0.0).astype(dtype)
    e_ref, s_ref = sk_reduce(A.astype(np.float64), 10, 3)
    got = mo.perform_svd_reduction_valued(A, 10, 3)
    eng = WindowEngine(n)
    try:
        wide = torch.from_numpy(np.concatenate([A, np.full((n, 8), 7.0, dtype=dtype)], axis=1)).cuda()   # a row pitch beyond n
        emb, sig = eng.svd_reduce_dense(wide[:, :n], 10, 3)
        emb, sig = emb.cpu().numpy(), sig.cpu().numpy()
    finally:
        eng.close()
    check_against(emb, sig, e_ref, s_ref)
    # (the process-wide engine behind perform_svd_reduction_valued may hold a handle sized for wider panels, whose eigensolver
    # pads the Gram to another order: equal to rounding, not to the bit)
    check_against(got, sig, e_ref, s_ref)


def test_dense_entry_refuses(L):
    from mused_amd import matrix_operations as mo

    A = np.where(np.random.default_rng(1).random((65, 65)) < 0.2, 1.5, 0.0)
    for bad in (np.nan, np.inf):
        B = A.copy()
        B[3, 64] = bad
        with pytest.raises(ValueError, match="Input contains NaN or infinity"):
            mo.perform_svd_reduction_valued(B, 4, 0)
    with pytest.raises(ValueError):
        mo.perform_svd_reduction_valued(np.ones((4, 5)), 2, 0)
    with pytest.raises(ValueError):
        mo.perform_svd_reduction_valued(np.ones(4), 2, 0)
    for bad in (1e80, -1e-80):   # beyond 2^200 / below 2^-200 the chain's Gram products leave the fp64 range
        B = A.copy()
        B[3, 64] = bad
        with pytest.raises(ValueError, match="magnitudes within"):
            mo.perform_svd_reduction_valued(B, 4, 0)
    assert np.isfinite(mo.perform_svd_reduction_valued(A, 4, 0)).all()   # the engine is usable after a refused call
    assert np.array_equal(mo.perform_svd_reduction_valued(np.zeros((5, 5)), 2, 0), np.zeros((5, 2)))   # TruncatedSVD's answer


def test_weights_are_checked():
    from mused_amd import matrix_operations as mo
    from mused_amd.engine import check_weights

    for bad in ((1.0, 0.0), (1.0, -2.0), (1.0, np.nan), (np.inf, 1.0), (), (1.0,) * 9, ("a", 1.0)):
        with pytest.raises(ValueError):
            check_weights(bad)
    with pytest.raises(ValueError):
        check_weights((1.0, 2.0), 3)
    A, B = np.eye(3), np.array([[0, 2.0, 0], [0, 0, 0], [1, 0, 1]])
    S = mo.fuse_matrices_weighted([A, B], (0.5, 0.25))
    assert S.dtype == np.float64 and np.array_equal(S, 0.5 * (A != 0) + 0.25 * (B != 0))


def test_graph_is_safe_when_masks_and_weights_change(L):
    from mused_amd.engine import WindowEngine

    L.call("mused_spmm_force_path", -1)
    n, k, ell, seed = 257, 5, 12, 1
    mods, _ = modalities(n, k)

    def fresh(parts_of, weights):
        e = WindowEngine(n)
        try:
            parts = parts_of(e)
            if weights is None:
                out = e.svd_reduce(e.fuse(parts), ell, seed, nnz_cap=3 * n * k, want_components=True)
            else:
                out = e.svd_reduce(e.fuse_weighted(parts, weights), ell, seed, nnz_cap=3 * n * k, want_components=True)
            return [bits(t) for t in out]
        finally:
            e.close()

    first = lambda e: device_parts(e, mods[:2], k)
    second = lambda e: device_parts(e, [mods[2], mods[0]], k)
    calls = [(first, [1.0, 0.5]), (second, [1.0, 0.5]), (first, None), (second, [0.3, 1.9]), (first, [1.0, 0.5])]
    want = [fresh(p, w) for p, w in calls]
    assert not np.array_equal(want[0][0], want[1][0]) and not np.array_equal(want[1][0], want[3][0])
    eng = WindowEngine(n)
    try:
        keep = []   # every call's masks live in tensors of their own
        for (parts_of, w), ref in zip(calls, want):
            parts = [type(a)(a.mask.clone(), a.n) for a in parts_of(eng)]
            keep.append(parts)
            fused = eng.fuse(parts) if w is None else eng.fuse_weighted(parts, w)
            got = eng.svd_reduce(fused, ell, seed, nnz_cap=3 * n * k, want_components=True)
            for g, r in zip(got, ref):
                assert np.array_equal(bits(g), r)
    finally:
        eng.close()


# ---- the pipeline ------------------------------------------------------------------------------------------------------

W, ELL, K, SEED = 256, 8, 10, 0
PIPE_WEIGHTS = (1.0, 0.5)


@pytest.fixture(scope="module")
def stream():
    from mused_amd import synth

    mods, labels = synth.two_modality_blob_stream(3 * W, 16, 11, n_centres=4, sep=4.0)
    return [m.astype(np.float64) for m in mods], labels


def host_embedding(mods, lo, hi, weights):
    from oracle import mo_oracle as omo

    S = weighted_sum([omo.create_adjacency_matrix(m[lo:hi], "", K) for m in mods], weights)
    return sk_reduce(S, ELL, SEED)[0]


def host_stream_labels(mods, labels, weights, mini):
    """main.py's window loop with the fusion replaced by sum_m w_m A_m: TruncatedSVD, scikit-learn's KMeans (or the stream's
    one MiniBatchKMeans), the reference's match_clusters."""
    from sklearn.cluster import KMeans, MiniBatchKMeans

    from oracle import mo_oracle as omo

    clusterer = MiniBatchKMeans(n_clusters=4, random_state=SEED, batch_size=W) if mini else None
    prev, out = None, []
    for lo in range(0, len(labels), W):
        reduced = host_embedding(mods, lo, lo + W, weights)
        if mini:
            raw = clusterer.partial_fit(reduced).predict(reduced)
        else:
            raw = KMeans(n_clusters=len(np.unique(labels[lo:lo + W])), random_state=SEED).fit_predict(reduced)
        prev = omo.match_clusters(prev, raw, method="hungarian", min_overlap=3)
        out.extend(prev)
    return np.array(out)


def run_stream(mods, labels, approach, **kw):
    from mused_amd.pipeline import process_streaming_data

    res = process_streaming_data({}, mods, ["", ""], W, ELL, K, 4, SEED, approach, labels, 1, 0.0, "types", False, 0.5, 5, **kw)
    return np.asarray(res["all_clusters"])


@pytest.mark.parametrize("approach", ["sSVDMC", "sSVDMC_mini"])
def test_stream_with_weights(L, stream, approach):
    mods, labels = stream
    got = run_stream(mods, labels, approach, modality_weights=PIPE_WEIGHTS)
    assert len(got) == 3 * W
    assert np.array_equal(got, host_stream_labels(mods, labels, PIPE_WEIGHTS, approach == "sSVDMC_mini"))


def test_stream_without_weights_is_unchanged(L, stream):
    mods, labels = stream
    assert np.array_equal(run_stream(mods, labels, "sSVDMC", modality_weights=None), run_stream(mods, labels, "sSVDMC"))


def test_batch_with_weights(L):
    from sklearn.cluster import KMeans

    from mused_amd import synth
    from mused_amd.pipeline import process_batch_data

    n = 600
    mods, labels = synth.two_modality_blob_stream(n, 16, 12, n_centres=4, sep=4.0)
    mods = [m.astype(np.float64) for m in mods]
    args = ({}, mods, ["", ""], ELL, K, 4, SEED, "SVDMC_batch", labels, 0.0, "all", False, 0.5, 5, 3, 2000)
    got = np.asarray(process_batch_data(*args, modality_weights=PIPE_WEIGHTS)["all_clusters"])
    want = KMeans(n_clusters=4, random_state=SEED).fit_predict(host_embedding(mods, 0, n, PIPE_WEIGHTS))
    assert np.array_equal(got, want)
    assert np.array_equal(np.asarray(process_batch_data(*args, modality_weights=None)["all_clusters"]),
                          np.asarray(process_batch_data(*args)["all_clusters"]))


def test_pipeline_refuses(L, stream):
    from mused_amd.pipeline import StreamPipeline, SwfdmcLanes

    mods, labels = stream
    with pytest.raises(ValueError):
        run_stream(mods, labels, "SWFDMC", modality_weights=PIPE_WEIGHTS)
    with pytest.raises(ValueError):
        run_stream(mods, labels, "sSVDMC", modality_weights=(1.0, 0.5, 0.25))
    with pytest.raises(ValueError):
        run_stream(mods, labels, "sSVDMC", modality_weights=(1.0, 0.0))
    with pytest.raises(ValueError):
        StreamPipeline(W, ELL, K, SEED, "sSVDMC", ["", ""], feature_sketch=True, modality_weights=PIPE_WEIGHTS)
    with pytest.raises(ValueError):
        SwfdmcLanes(W, ELL, K, SEED, 2, 10.0, modality_types=["", ""], modality_weights=PIPE_WEIGHTS)
