"""`fusion_threshold` and `modality_ks` on the pipeline entries, against a host restatement written here: per-modality
`oracle.mo_oracle.create_adjacency_matrix(m, "", k_m)`, `mused_amd.fusion.fuse_table_numpy`, scikit-learn's TruncatedSVD (or
`oracle.swfd_oracle.SeqBasedSWFD` with R from window 0's fused matrix), scikit-learn's KMeans / MiniBatchKMeans and the
reference's match_clusters.

The stream: three blob modalities on one label sequence, W = 256, l = 8, three windows.  The rules used for label equality are
the majority (tau = 2) and the weights (1, 0.5, 0.75) at tau = 1.5, at k = (20, 20, 20) and (10, 20, 30).  Checked on the CPU
for these inputs: no window has an empty row (the n = 600 batch has some), the eigenstep's k-means clusters hold 24 - 123
rows, and the labels do not move under a relative 1e-6 jitter of the embedding (for the sketch: under the majority rule).  An AND-type rule is NOT used for label
equality: it leaves 36 - 92 empty rows per window and one cluster of ~200 rows.  No test here feeds the eigenstep or the sketch
a mask without an edge."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, ELL, K, SEED, N_CENTRES = 256, 8, 20, 0, 4
KS_EQUAL, KS_MIXED = (20, 20, 20), (10, 20, 30)
MAJORITY = dict(fusion_threshold=2.0)
WEIGHTED = dict(fusion_threshold=1.5, modality_weights=(1.0, 0.5, 0.75))
TYPES = ["", "", ""]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


_STREAM = []


def stream():
    if not _STREAM:
        from mused_amd import synth

        n = 3 * W
        mods, labels = synth.two_modality_blob_stream(n, 16, 11, n_centres=N_CENTRES, sep=4.0)
        rng = np.random.default_rng(12)   # a third modality on the same labels, built the same way
        centres = (4.0 * rng.standard_normal((N_CENTRES, 16))).astype(np.float32)
        third = (centres[labels] + rng.standard_normal((n, 16), dtype=np.float32)).astype(np.float32)
        _STREAM.append(([m.astype(np.float64) for m in mods + [third]], labels))
    return _STREAM[0]


def table_of(rule, M=3):
    from mused_amd import fusion

    return fusion.threshold_table(rule.get("modality_weights") or (1.0,) * M, rule["fusion_threshold"])


_FUSED = {}


def host_fused(lo, hi, ks, rule):
    """The fused int64 0/1 matrix of rows [lo, hi): oracle adjacency per modality at its own k, then the table (rule None: OR)."""
    from mused_amd import fusion
    from oracle import mo_oracle as omo

    key = (lo, hi, tuple(ks), None if rule is None else tuple(sorted((k, str(v)) for k, v in rule.items())))
    if key not in _FUSED:
        mods, _ = stream()
        adjs = [omo.create_adjacency_matrix(m[lo:hi], "", k) for m, k in zip(mods, ks)]
        _FUSED[key] = omo.fuse_matrices(adjs) if rule is None else fusion.fuse_table_numpy(adjs, table_of(rule))
    return _FUSED[key]


def sk_reduce(matrix):
    from sklearn.decomposition import TruncatedSVD

    t = TruncatedSVD(n_components=ELL, random_state=SEED)
    return t.fit_transform(matrix.astype(np.float64)), t.singular_values_


_HOST = {}


def host_stream(ks, rule, approach):
    """main.py's window loop with the restated fusion; returns (labels, [sigma per window] for SWFDMC)."""
    from sklearn.cluster import KMeans, MiniBatchKMeans

    from oracle import mo_oracle as omo
    from oracle.swfd_oracle import SeqBasedSWFD as OraSWFD

    key = (tuple(ks), str(sorted(rule.items())), approach)
    if key in _HOST:
        return _HOST[key]
    _, labels = stream()
    clusterer = MiniBatchKMeans(n_clusters=N_CENTRES, random_state=SEED, batch_size=W) if approach == "sSVDMC_mini" else None
    prev, out, sigmas, swfd = None, [], [], None
    for lo in range(0, len(labels), W):
        fused = host_fused(lo, lo + W, ks, rule)
        assert fused.sum(axis=1).min() > 0, "a window with an empty row: not a case for label equality"
        if approach == "SWFDMC":
            if swfd is None:
                swfd = OraSWFD(N=W, R=omo.max_row_sq_norm(fused), d=W, sketch_dim=ELL)
            for r in range(W):
                swfd.fit(fused[r, :].reshape(1, -1))
            got = swfd.get()
            reduced = got[0] if got[0].shape[0] == W else got[0].T
            sigmas.append(np.asarray(got[1]))
        else:
            reduced = sk_reduce(fused)[0]
        if clusterer is not None:
            raw = clusterer.partial_fit(reduced).predict(reduced)
        else:
            raw = KMeans(n_clusters=len(np.unique(labels[lo:lo + W])), random_state=SEED).fit_predict(reduced)
        prev = omo.match_clusters(prev, raw, method="hungarian", min_overlap=3)
        out.extend(prev)
    _HOST[key] = (np.array(out), sigmas)
    return _HOST[key]


def run_stream(approach, **kw):
    from mused_amd.pipeline import process_streaming_data

    mods, labels = stream()
    res = process_streaming_data({}, mods, TYPES, W, ELL, K, N_CENTRES, SEED, approach, labels, 1, 0.0, "types", False, 0.5, 5,
                                 **kw)
    return np.asarray(res["all_clusters"])


EIGEN_CASES = [(MAJORITY, KS_EQUAL), (WEIGHTED, KS_EQUAL), (MAJORITY, KS_MIXED), (WEIGHTED, KS_MIXED)]


@pytest.mark.parametrize("rule,ks", EIGEN_CASES, ids=["majority", "weighted", "majority-ks", "weighted-ks"])
@pytest.mark.parametrize("approach", ["sSVDMC", "sSVDMC_mini"])
def test_stream(L, approach, rule, ks):
    got = run_stream(approach, modality_ks=ks, **rule)
    assert len(got) == 3 * W
    assert np.array_equal(got, host_stream(ks, rule, approach)[0])


@pytest.mark.parametrize("ks", [KS_EQUAL, KS_MIXED], ids=["k", "ks"])
def test_stream_swfdmc(L, ks):
    from mused_amd.pipeline import StreamPipeline

    mods, labels = stream()
    want, sigmas = host_stream(ks, MAJORITY, "SWFDMC")
    with StreamPipeline(W, ELL, K, SEED, "SWFDMC", modality_types=TYPES, async_labels=False, modality_ks=ks, **MAJORITY) as pipe:
        got = np.asarray(pipe.run(mods, labels))
        assert len(pipe.trace) == len(sigmas) == 3
        for tr, sig in zip(pipe.trace, sigmas):
            np.testing.assert_allclose(tr["sigma"], sig, rtol=0, atol=1e-8 * sig[0])
    assert np.array_equal(got, want)
    assert np.array_equal(run_stream("SWFDMC", modality_ks=ks, **MAJORITY), want)


@pytest.mark.parametrize("rule,ks", EIGEN_CASES, ids=["majority", "weighted", "majority-ks", "weighted-ks"])
def test_batch(L, rule, ks):
    from sklearn.cluster import KMeans

    from mused_amd.pipeline import process_batch_data

    n = 600
    mods, labels = stream()
    args = ({}, [m[:n] for m in mods], TYPES, ELL, K, N_CENTRES, SEED, "SVDMC_batch", labels[:n], 0.0, "all", False, 0.5, 5, 3,
            2000)
    got = np.asarray(process_batch_data(*args, modality_ks=ks, **rule)["all_clusters"])
    fused = host_fused(0, n, ks, rule)   # (at n = 600 some rows lose every edge to the vote: empty rows, as invalid rows give)
    assert fused.any()
    want = KMeans(n_clusters=N_CENTRES, random_state=SEED).fit_predict(sk_reduce(fused)[0])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("ks", [KS_EQUAL, KS_MIXED], ids=["k", "ks"])
def test_lanes_equal_the_sequential_sketch(L, ks):
    from mused_amd.pipeline import SwfdmcLanes

    mods, labels = stream()
    windows = [[torch.from_numpy(m[lo:lo + W]).cuda() for m in mods] for lo in range(0, 3 * W, W)]
    labs = [labels[lo:lo + W] for lo in range(0, 3 * W, W)]
    R = SwfdmcLanes.r_of_first_window(windows[0], W, K, modality_types=TYPES, modality_ks=ks, **MAJORITY)
    assert R == float(host_fused(0, W, ks, MAJORITY).sum(axis=1).max())
    with SwfdmcLanes(W, ELL, K, SEED, 2, R, modality_types=TYPES, modality_ks=ks, **MAJORITY) as lanes:
        out = np.asarray(lanes.run(windows, labs), dtype=np.int64)
    assert np.array_equal(out, run_stream("SWFDMC", modality_ks=ks, **MAJORITY).astype(np.int64))


def bits(t):
    return t.cpu().numpy().view(np.int64)


def test_eigenstep_on_a_majority_mask(L):
    """One window: the mask equals the restated matrix; sigma rtol 1e-8, embedding atol 1e-7 max|e_ref| on the columns with
    sigma > 1e-6 sigma_1, against TruncatedSVD of the restated matrix (the tolerances of the weighted-fusion tests)."""
    from mused_amd.engine import WindowEngine

    mods, _ = stream()
    fused = host_fused(0, W, KS_MIXED, MAJORITY)
    eng = WindowEngine(W)
    try:
        adjs = [eng.knn_adjacency(torch.from_numpy(m[:W]).cuda(), k) for m, k in zip(mods, KS_MIXED)]
        adj = eng.fuse_threshold(adjs, 2.0)
        assert adj.fused and np.array_equal(adj.to_dense().cpu().numpy(), fused)
        weighted = eng.fuse_threshold(adjs, 1.5, (1.0, 0.5, 0.75))
        assert np.array_equal(weighted.to_dense().cpu().numpy(), host_fused(0, W, KS_MIXED, WEIGHTED))
        emb, sig = eng.svd_reduce(adj, ELL, SEED, nnz_cap=W * sum(KS_MIXED))
        assert eng.rsvd_status()[0] == 0
        emb, sig = emb.cpu().numpy(), sig.cpu().numpy()
    finally:
        eng.close()
    e_ref, s_ref = sk_reduce(fused)
    big = s_ref > 1e-6 * s_ref[0]
    np.testing.assert_allclose(sig, s_ref, rtol=1e-8)
    np.testing.assert_allclose(emb[:, big], e_ref[:, big], atol=1e-7 * np.abs(e_ref).max())


def window_embedding(**kw):
    """Embedding and sigma bits of window 0 through the pipeline's device side."""
    from mused_amd.pipeline import StreamPipeline

    mods, _ = stream()
    with StreamPipeline(W, ELL, K, SEED, "sSVDMC", modality_types=TYPES, async_labels=False, **kw) as pipe:
        emb, sig, _ = pipe.window_device([torch.from_numpy(m[:W]).cuda() for m in mods])
        torch.cuda.synchronize()
        return bits(emb), bits(sig)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_identities(L):
    """Bit for bit, labels and the eigenstep's embedding: the keywords at None are a call without them; modality_ks = (k, k, k)
    is k_basis = k; equal weights at tau = 1 is the OR path."""
    plain, plain_emb = run_stream("sSVDMC"), window_embedding()
    assert np.array_equal(run_stream("sSVDMC", fusion_threshold=None, modality_ks=None), plain)
    assert same(window_embedding(fusion_threshold=None, modality_ks=None), plain_emb)
    assert np.array_equal(run_stream("sSVDMC", modality_ks=KS_EQUAL), plain)
    assert same(window_embedding(modality_ks=KS_EQUAL), plain_emb)
    assert np.array_equal(run_stream("sSVDMC", fusion_threshold=1.0), plain)
    assert same(window_embedding(fusion_threshold=1.0), plain_emb)
    assert same(window_embedding(fusion_threshold=1.0, modality_weights=(1.0, 1.0, 1.0)), plain_emb)
    assert not same(window_embedding(**MAJORITY), plain_emb) and not same(window_embedding(modality_ks=KS_MIXED), plain_emb)
    assert np.array_equal(run_stream("SWFDMC", fusion_threshold=1.0, modality_ks=KS_EQUAL), run_stream("SWFDMC"))


def test_the_other_approaches_take_the_mask(L):
    """DBSCAN_incr and the feature sketch under a threshold: tau = 1 is their OR run bit for bit, and the majority mask goes
    through (the feature sketch is beside the fusion: the labels are those of the run without it)."""
    from mused_amd.pipeline import StreamPipeline

    mods, labels = stream()
    assert np.array_equal(run_stream("DBSCAN_incr", fusion_threshold=1.0, modality_ks=KS_EQUAL), run_stream("DBSCAN_incr"))
    assert len(run_stream("DBSCAN_incr", modality_ks=KS_MIXED, **MAJORITY)) == 3 * W
    with StreamPipeline(W, ELL, K, SEED, "sSVDMC", modality_types=TYPES, async_labels=False, feature_sketch=True,
                        modality_ks=KS_MIXED, **WEIGHTED) as pipe:
        got = np.asarray(pipe.run(mods, labels))
        assert pipe.fswfd is not None and pipe.weights is None
    assert np.array_equal(got, host_stream(KS_MIXED, WEIGHTED, "sSVDMC")[0])


def test_matrix_operations_entry(L):
    from mused_amd import matrix_operations as mo
    from mused_amd.compat import matrix_operations as compat
    from mused_amd.engine import Adjacency

    assert compat.fuse_matrices_threshold is mo.fuse_matrices_threshold
    mods, _ = stream()
    adjs = [mo.adjacency_on_device(m[:W], "", k) for m, k in zip(mods, KS_MIXED)]
    dense = [a.to_numpy() for a in adjs]
    for kw, rule in (((2.0,), MAJORITY), ((1.5, (1.0, 0.5, 0.75)), WEIGHTED)):
        want = host_fused(0, W, KS_MIXED, rule)
        on_device = mo.fuse_matrices_threshold(adjs, *kw)
        assert isinstance(on_device, Adjacency) and on_device.fused and np.array_equal(on_device.to_numpy(), want)
        on_host = mo.fuse_matrices_threshold(dense, *kw)
        assert on_host.dtype == np.int64 and np.array_equal(on_host, want)
    with pytest.raises(ValueError):
        mo.fuse_matrices_threshold(dense, 3.5)
    with pytest.raises(ValueError):
        mo.fuse_matrices_threshold(adjs, 1.0, (1.0, 2.0))


def test_refusals(L):
    from mused_amd.engine import check_threshold
    from mused_amd.pipeline import StreamPipeline, SwfdmcLanes, batch_embedding

    mods, labels = stream()
    for bad in ((20, 20), (20, 20, 20, 20), (20, 0, 20), (20, -1, 20), (20, 2.5, 20), "abc", 20):
        with pytest.raises(ValueError):
            run_stream("sSVDMC", modality_ks=bad)
    for tau in (3.5, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            run_stream("sSVDMC", fusion_threshold=tau)
    with pytest.raises(ValueError):
        run_stream("sSVDMC", fusion_threshold=2.5, modality_weights=(1.0, 0.5, 0.75))   # the total is 2.25
    with pytest.raises(ValueError):
        run_stream("sSVDMC", fusion_threshold=1.0, modality_weights=(1.0, 0.5))
    with pytest.raises(ValueError):
        StreamPipeline(W, ELL, K, SEED, "sSVDMC", [""] * 9, fusion_threshold=1.0)         # M = 9
    with pytest.raises(ValueError):
        check_threshold((1.0,) * 9, 1.0)
    with pytest.raises(ValueError):
        check_threshold((0.3, 0.2, 0.1), 0.6000000000000001)
    assert check_threshold((0.1, 0.2, 0.3), 0.6000000000000001) == ([0.1, 0.2, 0.3], 0.6000000000000001)
    with pytest.raises(ValueError):
        batch_embedding([m[:300] for m in mods], TYPES, ELL, K, SEED, modality_ks=(20, 20))
    with pytest.raises(ValueError):
        batch_embedding([m[:300] for m in mods], TYPES, ELL, K, SEED, fusion_threshold=4.0)
    # weights without a threshold: the sketches still refuse
    with pytest.raises(ValueError):
        run_stream("SWFDMC", modality_weights=(1.0, 0.5, 0.75))
    with pytest.raises(ValueError):
        StreamPipeline(W, ELL, K, SEED, "sSVDMC", TYPES, feature_sketch=True, modality_weights=(1.0, 0.5, 0.75))
    with pytest.raises(ValueError):
        SwfdmcLanes(W, ELL, K, SEED, 2, 10.0, modality_types=TYPES, modality_weights=(1.0, 0.5, 0.75))
    with pytest.raises(ValueError):
        SwfdmcLanes.r_of_first_window([torch.from_numpy(m[:W]).cuda() for m in mods], W, K, modality_types=TYPES,
                                      modality_weights=(1.0, 0.5, 0.75))
