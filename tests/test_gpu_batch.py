"""The reference's batch approach (process_batch_data, main.py:132-167) on the device: the whole subset as one window, up
to the reference's default of 150,000 rows, with no n x n matrix (csrc/meta_stream.hip, the index-list masks, the
username relation for any n)."""
import numpy as np
import pytest

from conftest import load_golden, nbr_hash, text_inputs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    import ctypes as C

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host_list(score_row, kk):
    """Columns of the kk smallest (score, column) pairs, ascending columns."""
    order = np.lexsort((np.arange(len(score_row)), score_row))
    return np.sort(order[:kk]), score_row[order[kk - 1]]


def _same_up_to_ties(dev, score_row, kk, rel):
    """Neighbour sets equal, except swaps between candidates within `rel` (relative) of the kk-th score."""
    host, kth = _host_list(score_row, kk)
    if np.array_equal(dev, host):
        return True
    diff = np.setxor1d(dev, host)
    return rel > 0 and bool(np.all(np.abs(score_row[diff] - kth) <= rel * max(abs(kth), 1e-300)))


def _batch_inputs(kind, n, d, seed):
    """The inputs of tests/golden/make_batch_golden.py's cases."""
    from mused_amd import synth

    if kind == "blob":
        X, labels = synth.blob_stream(n, d, seed, n_centres=4)
        return [X.astype(np.float64)], [""], labels
    types_ = ["location", "time", "username", "text"] if kind == "sed4" else ["location", "time", "username", "tags", "text"]
    cols, labels = synth.metadata_stream(n, seed)
    cols["text"], _ = synth.text_stream(n, seed)
    return [cols[t] for t in types_], types_, labels


# ---- 1. the reference's own process_batch_data ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["batch_blob_s0", "batch_sed150_s5", "batch_sed4_s7"])
def test_batch_labels_match_reference_golden(name):
    from mused_amd import matrix_operations as mo
    from mused_amd import synth
    from mused_amd.pipeline import process_batch_data

    g = load_golden(name)
    n, d, ell, k, seed, n_clusters = (int(x) for x in g["meta"])
    mods, types_, labels = _batch_inputs(str(g["kind"]), n, d, seed)
    assert types_ == [str(x) for x in g["types"]]
    assert [synth.array_digest(m) if m.dtype.kind == "f" else "" for m in mods] == [str(x) for x in g["input_digest"]]
    for m, t, h in zip(mods, types_, g["adj_hash"]):
        assert nbr_hash(mo.adjacency_on_device(m, t, k).to_dense().cpu().numpy()) == str(h), t
    res = process_batch_data({}, mods, types_, ell, k, n_clusters, seed, "SVDMC_batch", labels, 0.0, "all", False, 1.5,
                             2, 3, 2000)
    assert res["processing_time"] > 0
    assert np.array_equal(np.asarray(res["all_clusters"], dtype=np.int64), g["all_clusters"])


def test_batch_five_types_golden_adjacency():
    """All five SED2012-style types: the tie-free ones bit-identical to the reference's, "tags" a valid choice between
    its equal scores (the reference's own is its unstable argsort's), and the whole chain runs."""
    from conftest import assert_valid_topk
    from oracle import mo_oracle as omo

    from mused_amd import matrix_operations as mo
    from mused_amd.pipeline import process_batch_data

    g = load_golden("batch_sed5_s9")
    n, d, ell, k, seed, n_clusters = (int(x) for x in g["meta"])
    mods, types_, labels = _batch_inputs(str(g["kind"]), n, d, seed)
    for m, t, h in zip(mods, types_, g["adj_hash"]):
        A = mo.adjacency_on_device(m, t, k).to_dense().cpu().numpy()
        if t == "tags":
            valid, S, kk = omo.metadata_scores(m, t, k)
            assert_valid_topk(A, valid, S, kk)
        else:
            assert nbr_hash(A) == str(h), t
    res = process_batch_data({}, mods, types_, ell, k, n_clusters, seed, "SVDMC_batch", labels, 0.0, "all", False, 1.5,
                             2, 3, 2000)
    assert res["all_clusters"].shape == (n,) and res["all_clusters"].max() < n_clusters


def test_batch_approach_names():
    from mused_amd.pipeline import process_batch_data

    X = np.random.default_rng(0).standard_normal((300, 8))
    res = process_batch_data({}, [X], [""], 4, 5, 3, 0, "DBSCAN_batch", np.zeros(300), 0.0, "all", False, 1.5, 2, 3, 100)
    assert res["all_clusters"].shape == (300,)
    try:
        import hdbscan  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            process_batch_data({}, [X], [""], 4, 5, 3, 0, "HDBSCAN_batch", np.zeros(300), 0.0, "all", False, 1.5, 2, 3, 100)
    with pytest.raises(ValueError):
        process_batch_data({}, [X], [""], 4, 5, 3, 0, "sSVDMC", np.zeros(300), 0.0, "all", False, 1.5, 2, 3, 100)


# ---- 2. chunked selection == the LDS-row kernels where those apply ------------------------------------------------------
def _tag_csr(tag_column):
    vocab, rowptr, ids = {}, [0], []
    for tags in tag_column:
        ids.extend(sorted(vocab.setdefault(t, len(vocab)) for t in set(tags)))
        rowptr.append(len(ids))
    return np.asarray(rowptr, np.int32), np.asarray(ids, np.int32), len(vocab)


@pytest.mark.parametrize("n", [3000, 15000])
@pytest.mark.parametrize("t", ["location", "time", "tags"])
def test_chunked_selection_equals_fused_kernels(n, t):
    from mused_amd import synth
    from mused_amd._lib import call
    from mused_amd.engine import WindowEngine, ptr

    cols, _ = synth.metadata_stream(n, 7, integer_time=True)  # whole hours: many equal time differences
    k = 50
    eng = WindowEngine(n)
    try:
        if t == "tags":
            rowptr, ids, nt = _tag_csr(cols["tags"][:, 0])  # empty tag sets included
            assert (np.diff(rowptr) == 0).any()
            kk = k
            ref = torch.empty((n, kk), dtype=torch.int32, device="cuda")
            post = WindowEngine._postings(rowptr, ids, nt)
            dev = eng._dev_arrays(rowptr, ids, post[0], post[1])
            call("mused_jaccard_knn", *[ptr(a) for a in dev], n, nt, kk, ptr(ref), None, 0, _stream())
            got = [eng.jaccard_lists(rowptr, ids, nt, kk, chunk=c) for c in (1000, 0)]
        else:
            rec = cols[t].copy()
            if t == "location":
                rec[np.isnan(rec).any(axis=1)] = (45.0, 10.0)
                rec[1::5] = rec[0:-1:5][: len(rec[1::5])]  # duplicated geotags: exact ties
            kk = k + 1 if t == "location" else 3 * k + 1
            rec_d = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
            ref = torch.empty((n, kk), dtype=torch.int32, device="cuda")
            call("mused_record_knn", ptr(rec_d), n, 0 if t == "location" else 1, kk, ptr(ref), None, 0, _stream())
            got = [eng.record_lists(rec, t, kk, chunk=c) for c in (1000, 0)]
        torch.cuda.synchronize()
        ref = ref.cpu().numpy()
        for g in got:
            assert np.array_equal(g.cpu().numpy(), ref)
        # the index-list mask equals the LDS-row kernel's mask (dense _scatter_valid below the limit, same selection)
        a_lists = eng.lists_to_adjacency(got[0], n).mask.cpu().numpy()
        if t == "tags":
            a_ref = eng.jaccard_adjacency(rowptr, ids, nt, kk).mask.cpu().numpy()
        else:
            a_ref = eng.record_adjacency(rec, t, kk).mask.cpu().numpy()
        assert np.array_equal(a_lists, a_ref)
    finally:
        eng.close()


# ---- 3. sparse text == scikit-learn ---------------------------------------------------------------------------------------
def test_sparse_text_equals_sklearn_cosine():
    from sklearn.feature_extraction.text import TfidfVectorizer
    from sklearn.metrics.pairwise import cosine_similarity
    from sklearn.preprocessing import normalize

    from mused_amd import synth
    from mused_amd.engine import WindowEngine

    data, _ = synth.sparse_text_stream(5000, 1)
    valid = np.where(np.any(data != "", axis=1))[0]
    vd = data[valid]
    text = np.where(vd[:, 0] != "", vd[:, 0], " ") + " " + np.where(vd[:, 1] != "", vd[:, 1], " ")
    T = TfidfVectorizer().fit_transform(text)  # rows NOT sorted by term: their stored order is the order of the sums
    S = cosine_similarity(T)  # the reference's text_sim (matrix_operations.py:105)
    assert (S == 0).mean() > 0.05  # rows that share no word: zero scores, filled by index order
    k = 50
    kk = k + 1
    eng = WindowEngine(len(valid))
    try:
        for chunk in (0, 1000):
            idx = eng.sparse_cosine_lists(normalize(T, copy=True), kk, chunk=chunk).cpu().numpy()
            for i in range(len(valid)):
                host, _ = _host_list(0.0 - S[i], kk)
                assert np.array_equal(idx[i], host), (chunk, i)
    finally:
        eng.close()


def test_text_golden_through_the_sparse_path():
    from mused_amd import matrix_operations as mo

    g = load_golden("cosine")
    data, _, n, k = text_inputs(g)
    A = mo.adjacency_on_device(data, "text", k, text_sparse=True).to_dense().cpu().numpy()
    assert nbr_hash(A) == str(g["text_adj_hash"])


# ---- 4 / 6. every metadata type at 40,000 and 150,000 rows, sampled rows against host scores ----------------------------
def _sample_rows(valid_mask, n, rng):
    inv = np.where(~valid_mask)[0]
    near = np.concatenate([inv - 1, inv + 1])
    near = near[(near >= 0) & (near < n)]
    rows = np.concatenate([[0, n - 1], near[:48], rng.choice(n, 96, replace=False)])
    return np.unique(rows)


def _row_bits(mask_np, r, n):
    return np.flatnonzero(np.unpackbits(mask_np[r].view(np.uint8), bitorder="little")[:n])


def _host_scores(t, data, valid, r):
    """Host score row of window row r against the valid rows (smaller = closer), oracle/mo_oracle.py arithmetic."""
    if t == "time":
        rec = data[valid]
        a = data[r]
        return np.abs(rec[:, 0] - a[0]) + np.abs(rec[:, 1] - a[1])
    if t == "location":
        rec = np.radians(data[valid].astype(np.float64))
        lat1, lon1 = np.radians(data[r].astype(np.float64))
        a = np.sin((rec[:, 0] - lat1) / 2) ** 2 + np.cos(lat1) * np.cos(rec[:, 0]) * np.sin((rec[:, 1] - lon1) / 2) ** 2
        return 2 * np.arcsin(np.sqrt(a)) * 6371
    raise ValueError(t)


@pytest.mark.parametrize("n", [40000, 150000])
def test_metadata_types_at_batch_scale(n):
    import scipy.sparse as sp

    from mused_amd import matrix_operations as mo
    from mused_amd import synth
    from mused_amd.engine import WindowEngine

    cols, _ = synth.metadata_stream(n, 21, users=2000, integer_time=True)
    k = 50
    rng = np.random.default_rng(n)
    eng = WindowEngine(n)
    try:
        for t in ("location", "time", "tags", "username"):
            data = cols[t]
            if t == "location":
                vmask = ~np.isnan(data).any(axis=1)
                kk = k + 1
            elif t == "time":
                vmask = ~((data[:, 0] == 0.0) | (data[:, 1] == 0.0))
                kk = 3 * k + 1
            else:  # the reference's validity test of both (matrix_operations.py:58, 75): every tag list is valid
                vmask = np.asarray(data[:, 0] != "", dtype=bool)
                kk = k
            valid = np.where(vmask)[0]
            adj = mo.adjacency_on_device(data, t, k, engine=eng)
            deg = adj.degrees()[0].cpu().numpy()
            M = adj.mask.cpu().numpy()
            rows = _sample_rows(vmask, n, rng)
            assert np.all(deg[~vmask] == 0)
            inv_cols = np.where(~vmask)[0][:64]
            for c in inv_cols:  # invalid columns empty
                assert not ((M[:, c >> 6] >> np.int64(c & 63)) & 1).any()
            if t == "username":
                _, ids, counts = np.unique(data[valid, 0], return_inverse=True, return_counts=True)
                full = np.full(n, -1)
                full[valid] = ids
                assert np.array_equal(deg[valid], counts[ids] - 1)
                for r in rows:
                    want = np.where((full == full[r]) & (full >= 0))[0] if full[r] >= 0 else np.array([], np.int64)
                    assert np.array_equal(_row_bits(M, r, n), want[want != r])
                continue
            assert np.all((deg[valid] == kk) | (deg[valid] == kk - 1))
            if t == "tags":
                vocab = {}
                ri, ci = [], []
                for j, tags in enumerate(data[valid, 0]):
                    for tg in set(tags):
                        ri.append(j)
                        ci.append(vocab.setdefault(tg, len(vocab)))
                B = sp.csr_matrix((np.ones(len(ri)), (ri, ci)), shape=(len(valid), len(vocab)))
                sizes = np.asarray(B.sum(axis=1)).ravel()
            pos = np.full(n, -1)
            pos[valid] = np.arange(len(valid))
            for r in rows:
                got = _row_bits(M, r, n)
                if not vmask[r]:
                    assert len(got) == 0
                    continue
                if t == "tags":
                    inter = np.asarray((B[pos[r]] @ B.T).todense()).ravel()
                    li = sizes[pos[r]]
                    s = np.where((li > 0) & (sizes > 0), 0.0 - inter / np.maximum(li + sizes - inter, 1), 0.0)
                    s[pos[r]] = 1.0
                    rel = 0.0
                else:
                    s = _host_scores(t, data, valid, r)
                    rel = 0.0 if t == "time" else 1e-12  # NumPy's sin / cos / asin against the device's: last bits
                host, kth = _host_list(s, kk)
                dev = np.searchsorted(valid, got)
                mine = np.sort(np.append(dev, pos[r])) if len(dev) == kk - 1 else dev
                assert _same_up_to_ties(np.unique(mine), s, kk, rel), (t, r)
    finally:
        eng.close()


def test_username_at_100k_rows():
    from mused_amd.engine import WindowEngine

    n = 100000
    rng = np.random.default_rng(3)
    ids = rng.integers(-1, 3000, size=n).astype(np.int32)
    eng = WindowEngine(n)
    try:
        adj = eng.group_adjacency(ids)
        deg = adj.degrees()[0].cpu().numpy()
        counts = np.bincount(ids[ids >= 0], minlength=3000)
        want = np.where(ids >= 0, counts[np.maximum(ids, 0)] - 1, 0)
        assert np.array_equal(deg, want)
        M = adj.mask.cpu().numpy()
        for r in np.unique(np.concatenate([[0, n - 1, 65534, 65535, 65536], rng.choice(n, 128, replace=False)])):
            exp = np.where((ids == ids[r]) & (np.arange(n) != r))[0] if ids[r] >= 0 else np.array([], np.int64)
            assert np.array_equal(_row_bits(M, r, n), exp), r
    finally:
        eng.close()


# ---- 5. dense rows beyond the LDS bit rows ----------------------------------------------------------------------------------
def test_dense_rows_beyond_the_bit_row_limit():
    from mused_amd import matrix_operations as mo
    from mused_amd import synth
    from mused_amd.engine import WindowEngine

    k = 50
    # n = 20,000: the index-list mask equals the LDS bit-row mask bitwise
    X, _ = synth.blob_stream(20000, 16, 4)
    eng = WindowEngine(20000)
    try:
        Xd = torch.from_numpy(X).cuda()
        a = eng.knn_adjacency(Xd, k).mask.cpu().numpy()
        b = eng.lists_to_adjacency(eng.knn_lists(Xd, k), 20000).mask.cpu().numpy()
        assert np.array_equal(a, b)
    finally:
        eng.close()
    n = 140000
    assert not mo._bit_rows_fit(n, k)
    X, _ = synth.blob_stream(n, 8, 5)
    X64 = X.astype(np.float64)
    eng = WindowEngine(n)
    try:
        adj = mo.adjacency_on_device(X, "", k, engine=eng)
        M = adj.mask.cpu().numpy()
        deg = adj.degrees()[0].cpu().numpy()
        assert np.all((deg == k) | (deg == k - 1))
        rng = np.random.default_rng(9)
        sq = (X64 ** 2).sum(axis=1)
        for r in np.unique(np.concatenate([[0, n - 1], rng.choice(n, 128, replace=False)])):
            s = np.maximum(sq[r] - 2.0 * (X64 @ X64[r]) + sq, 0.0)
            got = _row_bits(M, r, n)
            mine = np.sort(np.append(got, r)) if len(got) == k - 1 else got
            assert _same_up_to_ties(np.unique(mine), s, k, 1e-12), r
    finally:
        eng.close()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
def _sed_modalities(n, seed):
    from mused_amd import synth

    cols, labels = synth.metadata_stream(n, seed, users=2000)
    text, _ = synth.text_stream(n, seed)
    return [cols["location"], cols["time"], cols["username"], cols["tags"], text], \
        ["location", "time", "username", "tags", "text"], labels


def test_batch_40k_against_sklearn():
    import scipy.sparse as sp
    from sklearn.cluster import KMeans
    from sklearn.decomposition import TruncatedSVD

    from mused_amd import matrix_operations as mo
    from mused_amd.engine import WindowEngine

    n, ell, k, seed = 40000, 50, 50, 0
    mods, types_, labels = _sed_modalities(n, 31)
    eng = WindowEngine(n)
    try:
        fused = None
        for m, t in zip(mods, types_):
            a = mo.adjacency_on_device(m, t, k, engine=eng)
            fused = a if fused is None else eng.fuse_into(fused, a)
        rowptr, colidx = fused.neighbour_lists()
        rowptr, colidx = rowptr.cpu().numpy(), colidx.cpu().numpy()
        A = sp.csr_matrix((np.ones(len(colidx)), colidx, rowptr), shape=(n, n))
        emb, sig = eng.svd_reduce(fused, ell, seed, nnz_cap=len(colidx))
        svd = TruncatedSVD(n_components=ell, random_state=seed)
        svd.fit(A)
        np.testing.assert_allclose(sig.cpu().numpy(), svd.singular_values_, rtol=1e-8)
        E = emb.cpu().numpy()
        dev = mo.perform_clustering_on_device(emb, 4, seed, emb_host=E)
        host = KMeans(n_clusters=4, random_state=seed).fit_predict(E)
        assert np.array_equal(np.asarray(dev), host)
    finally:
        eng.close()


def test_batch_150k_five_modalities_runs_in_bounded_memory():
    from mused_amd.pipeline import process_batch_data

    n = 150000
    mods, types_, labels = _sed_modalities(n, 41)
    timings = {}
    res = process_batch_data({}, mods, types_, 50, 50, 4, 0, "SVDMC_batch", labels, 0.0, "all", False, 1.5, 2, 3, 2000,
                             timings=timings)
    print("batch 150k:", timings)
    assert res["all_clusters"].shape == (n,)
    assert set(np.unique(res["all_clusters"])) <= set(range(4))
    assert 0 < timings["edges"] < 2 ** 31
    assert timings["peak_bytes"] < n * n * 8 / 8  # one n x n fp64 matrix: 180 GB
