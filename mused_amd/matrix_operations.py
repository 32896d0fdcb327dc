"""MI355X-native stand-in for the reference's `matrix_operations` module.

Same eight names `main.py:5` imports, same argument meaning, return types and error behaviour:

    create_adjacency_matrix, fuse_matrices, match_clusters, perform_dbscan_clustering,
    perform_svd_reduction, perform_clustering, perform_dbscan_incr_clustering,
    perform_hdbscan_clustering

The numerical hot path (similarity -> kNN adjacency, fusion, randomized-SVD eigenstep) runs in
libmused_hip on the GPU through `mused_amd.engine.WindowEngine`; there is no CPU fallback -- without
the built extension or without a HIP device these functions raise.  The consumers that turn the
embedding into event indices (k-means, Hungarian matching) call
scikit-learn / SciPy on the host exactly where the reference does, so label parity reduces to
embedding parity; `perform_clustering_on_device` gives the same k-means labels from the device
(k-means++ seeding from the host's random draws, Lloyd iterations).

Two call styles:
  * NumPy in / NumPy out  -- drop-in for the reference (dense n x n matrices cross PCIe);
  * device objects        -- pass / receive `engine.Adjacency` and torch CUDA tensors
                             (`adjacency_on_device`, `fuse_matrices` on Adjacency objects,
                             `svd_reduce_on_device`) and nothing W x W ever visits the host.

modality_type "text" (matrix_operations.py:91-110) tokenises the ('title', 'description') strings once with
scikit-learn's analyser (mused_amd/text.py), computes the TF-IDF of a window on the device from the corpus' integer
arrays (csrc/tfidf.hip: TfidfVectorizer().fit_transform's values bit for bit) and runs the cosine / top-(k+1) kernel
there; MUSED_TEXT=host keeps the TfidfVectorizer call per window.  Already vectorised rows can use modality_type="cosine".
The metadata modality types of the SED2012 stream keep their string handling on the host -- per window for
raw rows, once per stream for a corpus of mused_amd/meta.py, whose windows are one launch each (csrc/meta_window.hip) --
and score / select on the device (csrc/meta.hip): "location" (haversine kNN, :22-31), "time" (:33-54), "username" (:56-71),
"tags" (Jaccard, :73-89).  Where the reference's own choice between EQUAL scores is undefined (unstable argsort,
ball-tree traversal) the smaller row index wins here.
"""
from __future__ import annotations

import os
import threading

import numpy as np

from . import engine as _eng
from . import fusion as _fusion

_METADATA_TYPES = ("location", "time", "username", "tags")
# "text": the dense TF-IDF (n x vocabulary fp64) goes to the device while it stays below this many bytes; beyond it (or
# when the caller asks for it) the sparse rows are used as they are (csrc/meta_stream.hip, SPCOS source)
TEXT_DENSE_BYTES = 1 << 30


def _metric_for(modality_type) -> str:
    """Similarity kernel of a DENSE modality type (the metadata types have their own scores)."""
    if modality_type in _METADATA_TYPES:
        raise ValueError(f"modality_type={modality_type!r} is a metadata type, not a dense-row metric")
    return "cosine" if modality_type in ("cosine", "text") else "l2"


def edges_per_row(modality_type, k_basis):
    """Upper bound of the ones a row of create_adjacency_matrix can hold, None when there is none ("username")."""
    k = int(k_basis)
    if modality_type == "username":
        return None
    if modality_type == "time":
        return 3 * k + 1
    if modality_type == "tags":
        return max(k, 0)
    if modality_type in ("location", "cosine", "text"):
        return k + 1
    return max(k, 1)


def _bit_rows_fit(n: int, kk: int) -> bool:
    """mused_knn_fused keeps one bit row per wave in 64 KiB of LDS (csrc/knn_fused.hip)."""
    return 4 * (8 * _eng.words_for(n) + 4 * kk) + 16 <= 64 * 1024


def _dense_knn(eng, X, k_basis, metric, n, valid_idx) -> _eng.Adjacency:
    """kNN adjacency of device rows X (the valid rows of a window of n; valid_idx None: all of them)."""
    kk = max(1, int(k_basis)) if metric == "l2" else min(int(k_basis) + 1, X.shape[0])
    if valid_idx is None and _bit_rows_fit(n, kk):
        return eng.knn_adjacency(X, k_basis, metric)
    if valid_idx is None or n > _eng._FUSED_META_ROWS:
        # beyond the LDS bit rows, or invalid rows at batch scale: neighbour lists, then the mask through the row map
        return eng.lists_to_adjacency(eng.knn_lists(X, k_basis, metric), n, valid_idx)
    return _scatter_valid(eng.knn_adjacency(X, k_basis, metric), valid_idx, n)


def adjacency_on_device(data, modality_type="", k_basis=50, engine=None, text_sparse=None) -> _eng.Adjacency:
    """Device-resident result of create_adjacency_matrix (matrix_operations.py:14-132, `case _`).

    Rows with a non-finite entry are excluded from the kNN and get empty rows / columns
    (matrix_operations.py:114-115, 126-127).  `text_sparse` ("text" only): True = sparse TF-IDF rows on the device,
    False = dense, None = dense unless it exceeds TEXT_DENSE_BYTES."""
    import torch

    if modality_type == "text":
        return _text_adjacency(data, k_basis, engine, sparse=text_sparse)
    if modality_type in _METADATA_TYPES:
        return _metadata_adjacency(data, modality_type, k_basis, engine)
    metric = _metric_for(modality_type)
    if isinstance(data, torch.Tensor):
        X = _eng.to_device_rows(data)
        finite = torch.isfinite(X).all(dim=1)
        all_valid = bool(finite.all().item())
        valid_idx = None if all_valid else torch.nonzero(finite).flatten()
    else:
        a = np.asarray(data)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        fin = np.all(np.isfinite(a), axis=1)
        all_valid = bool(fin.all())
        valid_np = None if all_valid else np.where(fin)[0]
        X = _eng.to_device_rows(a if all_valid else a[valid_np])
        valid_idx = None if all_valid else torch.from_numpy(valid_np).to(X.device)
        if not all_valid:
            finite = None
    n = len(data)
    eng = engine or _eng.default_engine(n)
    if all_valid:
        return _dense_knn(eng, X, k_basis, metric, n, None)
    if isinstance(data, torch.Tensor):
        X = X[valid_idx].contiguous()
    if X.shape[0] == 0:
        w = _eng.words_for(n)
        return _eng.Adjacency(torch.zeros((n, w), dtype=torch.int64, device=eng.device), n)
    return _dense_knn(eng, X, k_basis, metric, n, valid_idx)


def _scatter_valid(sub: _eng.Adjacency, valid_idx, n: int) -> _eng.Adjacency:
    """Adjacency among the valid rows -> window coordinates (rare path: dense round trip on the device)."""
    import torch

    dense = torch.zeros((n, n), dtype=torch.float64, device=sub.mask.device)
    dense[valid_idx.unsqueeze(1), valid_idx.unsqueeze(0)] = sub.to_dense(torch.float64)
    return _eng.Adjacency.from_dense(dense)


def text_on_device() -> bool:
    """MUSED_TEXT (read at every call): "device" (default) = the per-window TF-IDF runs on the device from a corpus
    tokenised once (csrc/tfidf.hip); "host" = scikit-learn's TfidfVectorizer per window, the former path as a whole."""
    import os

    return os.environ.get("MUSED_TEXT", "device") != "host"


def _text_adjacency(data, k_basis, engine=None, sparse=None) -> _eng.Adjacency:
    """matrix_operations.py:91-110: rows with a non-empty title or description are valid; TF-IDF of "title description",
    then cosine similarity and the k_basis + 1 most similar rows per row on the device: dense rows through
    `MUSED_METRIC_COSINE`, or (`sparse`, or a dense TF-IDF beyond TEXT_DENSE_BYTES) the rows scikit-learn's normalize
    returns, as they are stored, through mused_sparse_cosine_knn -- the similarities of cosine_similarity on sparse input
    bit for bit.
    data: a window of a tokenised corpus (mused_amd.text.TextWindow / TextCorpus) or the (n, 2) strings, which are
    tokenised as a corpus of their own.  The TF-IDF itself runs on the device (`_text_adjacency_device`) unless
    MUSED_TEXT=host or the corpus is host-only (`_text_adjacency_host`: the same TfidfVectorizer call as the reference).
    MUSED_TOKENISE=device|host names the tokeniser of raw strings (`text.tokenise_for_device`)."""
    from . import text as _text

    if isinstance(data, _text.TextCorpus):
        data = data.window()
    if not text_on_device():
        return _text_adjacency_host(data.records if isinstance(data, _text.TextWindow) else data, k_basis, engine, sparse)
    win = data if isinstance(data, _text.TextWindow) else _text.tokenise_for_device(data).window()
    if win.corpus.host_only:
        return _text_adjacency_host(win.records, k_basis, engine, sparse)
    return _text_adjacency_device(win, k_basis, engine, sparse)


def _text_adjacency_device(win, k_basis, engine=None, sparse=None) -> _eng.Adjacency:
    """Rows [win.lo, win.hi) of a tokenised corpus: the window's TF-IDF from the corpus' integer arrays in one
    mused_tfidf_window call (document frequencies, column ids, stored order, both normalisations, posting lists), then
    the kernels the host path feeds -- with the n x V_w matrix scattered on the device, or with the sparse rows and the
    posting lists over the corpus' global terms as they are.  One 16-byte read (V_w and the flag word) per window."""
    import torch

    from . import tfidf as _tfidf

    c, s, e = win.corpus, win.lo, win.hi
    n = e - s
    eng = engine or _eng.default_engine(max(n, 1))
    n_docs = int(c.vrank[e] - c.vrank[s])
    if n_docs == 0:
        return _eng.Adjacency(torch.zeros((n, _eng.words_for(n)), dtype=torch.int64, device=eng.device), n)
    if c.rowptr[e] == c.rowptr[s]:
        raise ValueError(_tfidf.EMPTY_VOCABULARY)   # what TfidfVectorizer raises for documents without a token
    w = eng.tfidf_window(c, s, e)
    n_cols = w.read_info()
    if sparse is None:
        sparse = n_docs * n_cols * 8 > TEXT_DENSE_BYTES
    valid_idx = None
    if n_docs != n:
        valid_idx = torch.from_numpy(c.vrow[c.vrank[s]:c.vrank[e]].astype(np.int64) - s).to(eng.device)
    if sparse:
        return eng.lists_to_adjacency(eng.tfidf_cosine_lists(w, min(int(k_basis) + 1, n_docs)), n, valid_idx)
    return _dense_knn(eng, eng.tfidf_dense(w, n_cols), k_basis, "cosine", n, valid_idx)


def _text_adjacency_host(data, k_basis, engine=None, sparse=None) -> _eng.Adjacency:
    """The TF-IDF on the host, per window, with the same TfidfVectorizer call as the reference; the result is uploaded
    (dense, or the sparse rows with posting lists built on the host) for the same device kernels."""
    import torch
    from sklearn.feature_extraction.text import TfidfVectorizer

    data = np.asarray(data)
    n = len(data)
    eng = engine or _eng.default_engine(max(n, 1))
    empty = lambda: _eng.Adjacency(torch.zeros((n, _eng.words_for(n)), dtype=torch.int64, device=eng.device), n)
    valid = np.where(np.any(data != "", axis=1))[0]
    vd = data[valid]
    if len(vd) == 0:
        return empty()
    text = np.where(vd[:, 0] != "", vd[:, 0], " ") + " " + np.where(vd[:, 1] != "", vd[:, 1], " ")
    if not np.any(text != " "):
        return empty()
    T = TfidfVectorizer().fit_transform(text)
    if sparse is None:
        sparse = T.shape[0] * T.shape[1] * 8 > TEXT_DENSE_BYTES
    valid_idx = None if len(valid) == n else torch.from_numpy(valid).to(eng.device)
    if sparse:
        from sklearn.preprocessing import normalize

        Tn = normalize(T, copy=True)  # what cosine_similarity does to its input (the stored order is kept)
        return eng.lists_to_adjacency(eng.sparse_cosine_lists(Tn, min(int(k_basis) + 1, Tn.shape[0])), n, valid_idx)
    V = np.asarray(T.todense(), dtype=np.float64)
    return _dense_knn(eng, _eng.to_device_rows(V), k_basis, "cosine", n, valid_idx)


def meta_on_device() -> bool:
    """MUSED_META (read at every call): "device" (default) = a window of a stream that was encoded once
    (mused_amd.meta.encode) is one launch on the corpus' resident arrays (csrc/meta_window.hip); "host" = the per-window
    host handling of `_metadata_adjacency` on the window's records, the former path as a whole."""
    import os

    return os.environ.get("MUSED_META", "device") != "host"


def _metadata_window_adjacency(win, modality_type, k_basis, eng) -> _eng.Adjacency:
    """Rows [win.lo, win.hi) of an encoded stream (mused_amd.meta.MetaWindow): the early returns of `_metadata_adjacency`
    decided from the host copy of vrank, then one enqueue-only call.  k per type as there: k + 1 ("location": a row is
    its own nearest neighbour), 3 k + 1 ("time"), k ("tags"); the device caps it by the window's valid rows."""
    import torch

    c, s, e = win.corpus, win.lo, win.hi
    n, k = e - s, int(k_basis)
    kk = {"location": k + 1, "time": 3 * k + 1, "username": 1, "tags": k}[modality_type]
    if n == 0 or c.vrank[e] == c.vrank[s] or (modality_type in ("time", "tags") and kk <= 0):
        return _eng.Adjacency(torch.zeros((n, _eng.words_for(n)), dtype=torch.int64, device=eng.device), n)
    return eng.meta_window_adjacency(win, kk)


def _metadata_adjacency(data, modality_type, k_basis, engine=None) -> _eng.Adjacency:
    """matrix_operations.py:22-89.  Row validity, k and the string handling follow the reference branch by branch on
    the host; scores and the selection run on the device.
    data: the rows of one window, or a window of a stream that was encoded once (mused_amd.meta.MetaWindow / MetaCorpus):
    that one runs from the corpus' device arrays (`_metadata_window_adjacency`) unless MUSED_META=host, the corpus is
    host-only, the engine is in classic kNN mode or the window is beyond _FUSED_META_ROWS -- then its records take the
    path below."""
    import torch

    from . import meta as _meta

    if isinstance(data, _meta.MetaCorpus):
        data = data.window()
    if isinstance(data, _meta.MetaWindow):
        if data.corpus.kind != modality_type:
            raise ValueError(f"a {data.corpus.kind!r} corpus was given as modality_type={modality_type!r}")
        engine = engine or _eng.default_engine(max(len(data), 1))
        if (meta_on_device() and not data.corpus.host_only and engine.knn_mode != "classic"
                and len(data) <= _eng._FUSED_META_ROWS):
            return _metadata_window_adjacency(data, modality_type, k_basis, engine)
        data = data.records
    if isinstance(data, torch.Tensor):
        data = data.cpu().numpy()
    data = np.asarray(data)
    n = len(data)
    eng = engine or _eng.default_engine(max(n, 1))
    empty = lambda: _eng.Adjacency(torch.zeros((n, _eng.words_for(n)), dtype=torch.int64, device=eng.device), n)
    k = int(k_basis)
    # batch scale (beyond one row of scores in LDS): neighbour lists of the valid rows, mapped straight into the window's
    # mask (no n x n round trip)
    lists = n > _eng._FUSED_META_ROWS
    if modality_type == "location":  # 'latitude', 'longitude'; k + 1 because a row is its own nearest neighbour
        valid = np.where(~np.isnan(data.astype(np.float64)).any(axis=1))[0]
        if len(valid) == 0:
            return empty()
        rec, kk = data[valid], min(k + 1, len(valid))
        if lists:
            return eng.lists_to_adjacency(eng.record_lists(rec, "location", kk), n, _map(valid, n))
        sub = eng.record_adjacency(rec, "location", kk)
    elif modality_type == "time":  # 'datetaken', 'dateupload'; 0.0 marks a missing stamp
        valid = np.where(~((data[:, 0] == 0.0) | (data[:, 1] == 0.0)))[0]
        if len(valid) == 0 or 3 * k + 1 <= 0:
            return empty()
        rec, kk = data[valid], min(3 * k + 1, len(valid))
        if lists:
            return eng.lists_to_adjacency(eng.record_lists(rec, "time", kk), n, _map(valid, n))
        sub = eng.record_adjacency(rec, "time", kk)
    elif modality_type == "username":
        valid = np.where(data[:, 0] != "")[0]
        if len(valid) == 0:
            return empty()
        _, ids = np.unique(data[valid, 0].astype(str), return_inverse=True)
        if lists:  # id -1 for rows without a name: no edges in their rows or columns
            full = np.full(n, -1, dtype=np.int32)
            full[valid] = ids
            return eng.group_adjacency(full)
        sub = eng.group_adjacency(ids)
    else:  # "tags"
        valid = np.where(data[:, 0] != "")[0]
        if len(valid) == 0 or k <= 0:
            return empty()
        vocab, rowptr, ids = {}, [0], []
        for tags in data[valid, 0]:
            tag_set = set(tags) if tags else set()
            ids.extend(sorted(vocab.setdefault(t, len(vocab)) for t in tag_set))
            rowptr.append(len(ids))
        ids, kk = np.asarray(ids, dtype=np.int32), min(k, len(valid))
        if lists:
            return eng.lists_to_adjacency(eng.jaccard_lists(rowptr, ids, len(vocab), kk), n, _map(valid, n))
        sub = eng.jaccard_adjacency(rowptr, ids, len(vocab), kk)
    if len(valid) == n:
        return sub
    return _scatter_valid(sub, torch.from_numpy(valid).to(eng.device), n)


def _map(valid, n):
    """Row map of lists_to_adjacency: None when every row is valid."""
    return None if len(valid) == n else valid


def create_adjacency_matrix(data, modality_type, k_basis=50):
    """matrix_operations.py:14: (n, n) float64 0/1 matrix, A[i, j] = 1 iff j is one of the
    k selected neighbours of i and j != i."""
    return adjacency_on_device(data, modality_type, k_basis).to_numpy()


def fuse_matrices(matrices):
    """matrix_operations.py:134-141.  A list of `Adjacency` objects gives a fused `Adjacency` (device
    OR of bitmasks); a list of ndarrays gives what the reference returns: a float64 copy for one
    matrix, the int64 logical OR for two or more."""
    if len(matrices) == 0:
        raise IndexError("list index out of range")  # matrices[0] in the reference
    if all(isinstance(m, _eng.Adjacency) for m in matrices):
        eng = _eng.default_engine(matrices[0].n)
        return eng.fuse(list(matrices))
    if len(matrices) == 1:
        return np.array(matrices[0], copy=True)  # plain .copy(): no arithmetic to accelerate
    adjs = [m if isinstance(m, _eng.Adjacency) else _eng.Adjacency.from_dense(np.asarray(m) != 0) for m in matrices]
    eng = _eng.default_engine(adjs[0].n)
    return eng.fuse(adjs).to_dense().cpu().numpy()


def fuse_matrices_weighted(matrices, weights):
    """Fusion by weighted sum instead of OR: S = sum_m w_m (A_m != 0), at most 8 modalities, every weight finite and > 0
    (ValueError otherwise).  A list of `Adjacency` objects gives a `WeightedAdjacency` (nothing is computed until the
    eigenstep reads it); a list of ndarrays gives S as a float64 array, each entry the sum in modality order from 0.0."""
    if len(matrices) == 0:
        raise IndexError("list index out of range")
    if all(isinstance(m, _eng.Adjacency) for m in matrices):
        return _eng.WeightedAdjacency(list(matrices), weights)
    w = _eng.check_weights(weights, len(matrices))
    mats = [np.asarray(m.to_numpy() if isinstance(m, _eng.Adjacency) else m) for m in matrices]
    out = np.zeros(mats[0].shape, dtype=np.float64)
    for a, wm in zip(mats, w):
        if a.shape != out.shape:
            raise ValueError("adjacency shapes differ")
        out = np.where(a != 0, out + wm, out)
    return out


def fuse_matrices_threshold(matrices, threshold, weights=None):
    """Fusion by agreement threshold: entry (i, j) is 1 iff the sum of w_m over the matrices with a nonzero (i, j) -- fp64,
    from 0.0, in modality order; every weight 1.0 without `weights` -- is >= threshold (mused_amd/fusion.py states the rule;
    ValueError for more than 8 matrices, a weight that is not finite and > 0, a threshold that is not finite, not > 0 or above
    the sum of all weights).  OR, AND and "at least t of M" are thresholds of equal weights.  A list of `Adjacency` objects
    gives a device `Adjacency` (one launch, csrc/adj_fuse_table.hip); ndarrays give the int64 0/1 matrix."""
    if len(matrices) == 0:
        raise IndexError("list index out of range")
    if all(isinstance(m, _eng.Adjacency) for m in matrices):
        return _eng.default_engine(matrices[0].n).fuse_threshold(list(matrices), threshold, weights)
    w, tau = _eng.check_threshold([1.0] * len(matrices) if weights is None else _eng.check_weights(weights, len(matrices)),
                                  threshold)
    mats = [np.asarray(m.to_numpy() if isinstance(m, _eng.Adjacency) else m) for m in matrices]
    return _fusion.fuse_table_numpy(mats, _fusion.threshold_table(w, tau))


def max_row_sq_norm(fused) -> float:
    """R of main.py:61: max_i ||fused[i, :]||^2."""
    if isinstance(fused, _eng.Adjacency):
        return _eng.WindowEngine.max_row_sq_norm(fused)
    return _eng.WindowEngine.max_row_sq_norm(_eng.Adjacency.from_dense(fused))


def svd_reduce_on_device(matrix, reduced_dim, seed, nnz_cap=None, engine=None):
    """(embedding, singular_values) as fp64 CUDA tensors; `matrix` an Adjacency, a WeightedAdjacency or a dense 0/1 matrix."""
    adj = matrix if isinstance(matrix, (_eng.Adjacency, _eng.WeightedAdjacency)) else _eng.Adjacency.from_dense(matrix)
    eng = engine or _eng.default_engine(adj.n)
    return eng.svd_reduce(adj, reduced_dim, seed, nnz_cap=nnz_cap)


def perform_svd_reduction(matrix, reduced_dim, seed):
    """matrix_operations.py:143-147: TruncatedSVD(n_components=min(reduced_dim, n_cols - 1),
    random_state=seed).fit_transform(matrix) for the 0/1 fused adjacency -> (n, n_comp) float64."""
    emb, _ = svd_reduce_on_device(matrix, reduced_dim, seed)
    return emb.cpu().numpy()


def perform_svd_reduction_valued(matrix, reduced_dim, seed):
    """TruncatedSVD(n_components=min(reduced_dim, n - 1), random_state=seed).fit_transform(matrix) -> (n, n_comp) float64
    for ANY square real matrix (its nonzeros become neighbour lists with a value per entry: csrc/adj_values.hip,
    csrc/spmm_valued.hip) or a `WeightedAdjacency`.  ValueError for a matrix that is not square and, with scikit-learn's
    message, for a NaN or an infinity.  `perform_svd_reduction` keeps its 0/1 contract."""
    if isinstance(matrix, _eng.WeightedAdjacency):
        emb, _ = _eng.default_engine(matrix.n).svd_reduce(matrix, reduced_dim, seed)
    else:
        if isinstance(matrix, _eng.Adjacency):
            matrix = matrix.to_dense()
        shape = tuple(matrix.shape) if hasattr(matrix, "shape") else np.shape(matrix)
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError(f"the valued eigenstep takes a square matrix, got shape {shape}")
        emb, _ = _eng.default_engine(shape[0]).svd_reduce_dense(matrix, reduced_dim, seed)
    return emb.cpu().numpy()


# ---- host-side consumers (keep on host, same library calls) ----------


def perform_clustering(matrix, n_clusters, seed):
    """matrix_operations.py:149-153."""
    from sklearn.cluster import KMeans

    if hasattr(matrix, "cpu"):
        matrix = matrix.cpu().numpy()
    return KMeans(n_clusters=n_clusters, random_state=seed).fit_predict(matrix)


_KM_WS = {}
_KM_LDS_KD = 8192   # mused_kmeans_lloyd's limit on k * d; mused_kmeans_lloyd_wide takes over beyond it
# windows that perform_clustering_on_device did not finish on the device although it was asked to: seeded by scikit-learn
# on the host (the seed kernel's ambiguity flag) or clustered by scikit-learn's KMeans (a cluster ran empty, k > n,
# k * d > 8192 together with k > 1024, d > 512 or MUSED_KMEANS_WIDE=host)
km_fallbacks = 0
_km_fallback_lock = threading.Lock()


def _km_count_fallback():
    global km_fallbacks
    with _km_fallback_lock:   # the label workers of a pipeline call in parallel
        km_fallbacks += 1


def kmeanspp_draws(n, k, seed):
    """Everything `sklearn.cluster.kmeans_plusplus` takes from its generator for n rows and k centres, drawn before a
    row has been seen: (first, U) with `first` the first centre's row and U the (k - 1, L) uniforms of the further
    centres, L = 2 + int(log(k)) local trials.  scikit-learn's own expressions in its own order (sklearn 1.7
    cluster/_kmeans.py `_kmeans_plusplus`), so a RandomState(seed) ends in the same state either way
    (`seed` may be such a generator: it is advanced)."""
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    first = int(rs.choice(n, p=np.ones(n) / n))   # sample_weight / sample_weight.sum() with unit weights
    L = 2 + int(np.log(k))
    U = np.empty((k - 1, L), dtype=np.float64)
    for c in range(k - 1):
        U[c] = rs.uniform(size=L)
    return first, U


def _km_host_copy(emb_dev, emb_host):
    """The host copy of the embedding, made (or taken from the caller) only where a fallback needs it."""
    return np.ascontiguousarray(emb_host if emb_host is not None else emb_dev.cpu().numpy(), dtype=np.float64)


def _km_workspace(key, nbytes, device):
    import torch

    ws = _KM_WS.get(key)
    if ws is None:
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        if len(_KM_WS) > 16:
            _KM_WS.clear()
        _KM_WS[key] = ws
    return ws


def _km_lloyd(Xd, n, d, k, mean_d, cen_d, tol, st):
    """The Lloyd iterations on stream st -> (int32 labels on the host, empty-cluster flag): mused_kmeans_lloyd where
    k * d <= 8192 (all centres and sums in LDS), mused_kmeans_lloyd_wide (tiles; the same bits) beyond that."""
    import ctypes as C

    import torch

    from . import _lib

    wide = k * d > _KM_LDS_KD
    entry = "mused_kmeans_lloyd_wide" if wide else "mused_kmeans_lloyd"
    nbytes = (_lib.lib().mused_kmeans_wide_ws_bytes if wide else _lib.lib().mused_kmeans_ws_bytes)(n, d, k)
    ws = _km_workspace((Xd.device, n, d, k, st.cuda_stream), nbytes, Xd.device)
    labels = torch.empty(n, dtype=torch.int32, device=Xd.device)
    info = (C.c_int * 4)()
    _lib.call(entry, _eng.ptr(Xd), Xd.stride(0), n, d, k, _eng.ptr(mean_d), _eng.ptr(cen_d),
              tol, 300, _eng.ptr(labels), info, _eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
    return labels.cpu().numpy(), info[2]


def _km_host_seeded(Xd, X, k, seed, st):
    """Seeding by scikit-learn's own kmeans_plusplus on the host copy X, Lloyd iterations on the device."""
    import torch
    from sklearn.cluster import kmeans_plusplus
    from sklearn.utils.extmath import row_norms

    n, d = X.shape
    tol = float(np.mean(np.var(X, axis=0)) * 1e-4)   # KMeans._check_params_vs_input -> _tolerance, before centring
    mean = X.mean(axis=0)
    Xc = X - mean
    centers, _ = kmeans_plusplus(Xc, k, x_squared_norms=row_norms(Xc, squared=True),
                                 random_state=np.random.RandomState(seed))
    with torch.cuda.stream(st):
        mean_d = torch.from_numpy(mean).to(Xd.device)
        cen_d = torch.from_numpy(np.ascontiguousarray(centers)).to(Xd.device)
        out, empty = _km_lloyd(Xd, n, d, k, mean_d, cen_d, tol, st)
    if empty:
        return perform_clustering(X, k, seed)
    return out


def perform_clustering_on_device(emb_dev, n_clusters, seed, emb_host=None, stream=None):
    """The same labels as `perform_clustering` (matrix_operations.py:149-153) with what `KMeans.fit` computes on the
    device (sklearn:cluster/_kmeans.py `fit`: tolerance from the raw rows, X -= X.mean(0), row norms,
    `_init_centroids` -> `_kmeans_plusplus`, `_kmeans_single_lloyd`).  The host draws what k-means++ takes from
    `RandomState(seed)` (`kmeanspp_draws`: the draws do not depend on the rows); mused_kmeans_moments, mused_kmeans_seed
    (csrc/kmeanspp.hip) and mused_kmeans_lloyd -- mused_kmeans_lloyd_wide where k * d > 8192 -- (csrc/kmeans.hip) run on
    the stream, and the host reads the tolerance with the seed kernel's flag (16 bytes) and the labels.  No host copy of
    the embedding is made on that path.
    emb_dev: (n, d) fp64 CUDA tensor; emb_host: its host copy if the caller already has one (read only on a fallback).
    Returns int32 labels (NumPy).
    Fallbacks: the seed kernel's ambiguity flag (a decision of k-means++ within rounding) -> that window with
    scikit-learn's seeding on the host and the device Lloyd iterations; MUSED_KMEANS_SEED=host -> every window that way
    (d > 512 too, where k * d <= 8192); a cluster that runs empty (sklearn relocates it), k > n, or
    k * d > 8192 with k > 1024 or d > 512 -> scikit-learn's KMeans.  MUSED_KMEANS_WIDE=host (read per call) sends every window with
    k * d > 8192 to scikit-learn's KMeans, as before mused_kmeans_lloyd_wide existed.
    Every fallback is counted in `km_fallbacks`, except the host seeding that MUSED_KMEANS_SEED=host asks for."""
    import ctypes as C
    import os

    import torch

    from . import _lib

    n, d = emb_dev.shape
    k = int(n_clusters)
    wide_on_host = k > 1024 or d > 512 or os.environ.get("MUSED_KMEANS_WIDE", "device") == "host"
    if k > n or (k * d > _KM_LDS_KD and wide_on_host):
        _km_count_fallback()
        return perform_clustering(_km_host_copy(emb_dev, emb_host), k, seed)
    st = stream if stream is not None else torch.cuda.current_stream()
    Xd = emb_dev if emb_dev.stride(1) == 1 else emb_dev.contiguous()
    if os.environ.get("MUSED_KMEANS_SEED", "device") == "host" or d > 512:
        return _km_host_seeded(Xd, _km_host_copy(emb_dev, emb_host), k, seed, st)
    first, U = kmeanspp_draws(n, k, seed)
    dev = emb_dev.device
    with torch.cuda.stream(st):
        ws = _km_workspace((dev, n, d, k, st.cuda_stream, "seed"), _lib.lib().mused_kmeans_seed_ws_bytes(n, d, k), dev)
        mean_d = torch.empty(d, dtype=torch.float64, device=dev)
        cen_d = torch.empty((k, d), dtype=torch.float64, device=dev)
        idx_d = torch.empty(k, dtype=torch.int32, device=dev)
        head = torch.empty(2, dtype=torch.float64, device=dev)   # {tol, the two int32 of the seed kernel's info}
        U_d = torch.from_numpy(U).to(dev) if k > 1 else None
        sp = C.c_void_p(st.cuda_stream)
        _lib.call("mused_kmeans_moments", _eng.ptr(Xd), Xd.stride(0), n, d, _eng.ptr(mean_d), _eng.ptr(head), sp)
        _lib.call("mused_kmeans_seed", _eng.ptr(Xd), Xd.stride(0), n, d, k, _eng.ptr(mean_d), first,
                  _eng.ptr(U_d) if k > 1 else None, U.shape[1], _eng.ptr(cen_d), _eng.ptr(idx_d),
                  C.c_void_p(head.data_ptr() + 8), _eng.ptr(ws), ws.numel(), sp)
        head_h = head.cpu().numpy()   # mused_kmeans_lloyd takes the tolerance by value
        tol, ambiguous = float(head_h[0]), int(head_h[1:].view(np.int32)[0])
        if not ambiguous:
            out, empty = _km_lloyd(Xd, n, d, k, mean_d, cen_d, tol, st)
    if ambiguous:
        _km_count_fallback()
        return _km_host_seeded(Xd, _km_host_copy(emb_dev, emb_host), k, seed, st)
    if empty:
        _km_count_fallback()
        return perform_clustering(_km_host_copy(emb_dev, emb_host), k, seed)
    return out


def check_k_candidates(candidates, n):
    """`candidates` as a list of distinct ints in ascending order; ValueError unless it is a non-empty iterable of ints with
    2 <= k <= n - 1."""
    import numbers

    try:
        ks = list(candidates)
    except TypeError:
        raise ValueError(f"candidates must be an iterable of ints, got {candidates!r}") from None
    if not ks:
        raise ValueError("candidates is empty")
    for k in ks:
        if not isinstance(k, numbers.Integral) or isinstance(k, bool) or not 2 <= int(k) <= n - 1:
            raise ValueError(f"candidate k = {k!r}: every k must be an int with 2 <= k <= n - 1 = {n - 1}")
    return sorted({int(k) for k in ks})


def select_n_clusters_on_device(embedding, candidates, seed, stream=None, emb_host=None):
    """k chosen without ground truth: for every k in `candidates`, `perform_clustering_on_device(embedding, k, seed)` and the
    silhouette score of its labels from csrc/silhouette.hip (metrics_evaluation.internal_metrics_raw).  Returns (best_k,
    the labels of best_k, {k: score}); the highest score wins, ties go to the smaller k.  A k whose labels hold a single
    value has no silhouette: its score is NaN and it never wins (all NaN: the smallest k).
    embedding: (n, d) fp64 CUDA tensor; candidates: a non-empty iterable of ints with 2 <= k <= n - 1 (ValueError otherwise);
    emb_host: the embedding's host copy if the caller has one (read only by a k-means fallback); stream: both kernels run on
    it, for which the embedding must be complete (as for perform_clustering_on_device)."""
    import torch

    from . import metrics_evaluation as me

    if not isinstance(embedding, torch.Tensor) or not embedding.is_cuda or embedding.dim() != 2 \
            or embedding.dtype != torch.float64:
        raise ValueError("embedding must be an (n, d) float64 CUDA tensor")
    ks = check_k_candidates(candidates, embedding.shape[0])
    scores, best_k, best_labels = {}, None, None
    for k in ks:   # ascending: a later k replaces the best one only with a strictly higher score
        labels = perform_clustering_on_device(embedding, k, seed, emb_host=emb_host, stream=stream)
        flags, clusters, s, _, _, Xd = me.internal_metrics_raw(embedding, labels, stream, indices=False, wait_current=False)
        if flags & 2:
            me._raise_flags(flags, clusters, Xd)
        scores[k] = s
        if best_k is None or (s == s and not (scores[best_k] >= s)):
            best_k, best_labels = k, labels
    return best_k, best_labels, scores


def _overlap_costs(prev_clusters, new_clusters, min_overlap):
    up, un = np.unique(prev_clusters), np.unique(new_clusters)
    cost = np.full((len(up), len(un)), np.inf)
    for a, p in enumerate(up):
        sel = prev_clusters == p
        for b, q in enumerate(un):
            ov = int(np.count_nonzero(sel & (new_clusters == q)))
            if ov >= min_overlap:
                cost[a, b] = -ov
    return up, un, cost


def _feasible(cost) -> bool:
    inf = np.isinf(cost)
    return not (inf.all() or inf.all(axis=1).any() or inf.all(axis=0).any())


def match_clusters(prev_clusters, new_clusters, method="hungarian", min_overlap=5):
    """matrix_operations.py:155-185: relabel the new window's clusters by the previous window's
    labels through a minimum-cost assignment on positional overlap counts."""
    if prev_clusters is None or len(prev_clusters) == 0:
        return new_clusters
    prev_clusters = np.asarray(prev_clusters)
    new_arr = np.asarray(new_clusters)
    up, un, cost = _overlap_costs(prev_clusters, new_arr, min_overlap)
    if not _feasible(cost):
        return new_clusters
    if method == "hungarian":
        from scipy.optimize import linear_sum_assignment

        rows, cols = linear_sum_assignment(cost)
        relabel = {un[c]: up[r] for r, c in zip(rows, cols)}
        return np.array([relabel.get(c, c) for c in new_arr])
    if method == "pot":
        # matrix_operations.py:187-210 with ot.sinkhorn written out (mused_amd/sinkhorn.py: specified, unpinned)
        from . import sinkhorn as _sk

        plan, _ = _sk.pot_plan(cost)
        relabel = {un[c]: up[r] for c, r in _sk.select(plan).items()}
        return np.array([relabel.get(c, c) for c in new_arr])
    raise ValueError("Invalid method. Choose 'hungarian' or 'pot'.")


# windows that match_clusters_on_device / match_chain_on_device finished with the host specification although the device was
# asked: a flag of the kernel (a decision within rounding, a label outside [0, 1024), more than 256 distinct labels; for
# "hungarian" also a cost matrix without a complete assignment, where the host call raises SciPy's ValueError; with
# wide=True only what the wide Hungarian chain flags: more than 4,096 labels a side, no complete assignment, the step budget,
# and a label that does not fit int32)
match_fallbacks = 0
_MATCH_WS = {}
MATCH_FLAG_SELECT, MATCH_FLAG_STOP, MATCH_FLAG_RANGE, MATCH_FLAG_SIZE = 1, 2, 4, 8
MATCH_FLAG_ASSIGN = 16
# method -> (chain entry, workspace size entry, diagnostic output per window: elements, dtype name)
_MATCH_ENTRIES = {"pot": ("mused_match_pot_chain", "mused_match_pot_ws_bytes", 65536, "float64"),
                  "hungarian": ("mused_match_hung_chain", "mused_match_hung_ws_bytes", 256, "int32")}
_MATCH_LABELS = 1024   # label values the kernel's histogram covers (csrc/match.hip)


def _match_count_fallback():
    global match_fallbacks
    with _km_fallback_lock:
        match_fallbacks += 1


def _labels_to_device(x, device):
    """int32 CUDA labels of a NumPy array or an int32 / int64 CUDA tensor; values outside [0, 1024) become 1024, which the
    kernel flags (the host copy keeps the true values)."""
    import torch

    if isinstance(x, torch.Tensor):
        return x.to(device).clamp(-1, _MATCH_LABELS).to(torch.int32).contiguous()
    a = np.asarray(x)
    a = np.where((a < 0) | (a >= _MATCH_LABELS), _MATCH_LABELS, a).astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _match_stream(stream):
    """The stream the matching runs on: the caller's, behind whatever the current stream holds (tensor arguments)."""
    import torch

    cur = torch.cuda.current_stream()
    if stream is None:
        return cur
    stream.wait_stream(cur)
    return stream


def _labels_to_host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _match_entry(method):
    try:
        return _MATCH_ENTRIES[method]
    except (KeyError, TypeError):
        raise ValueError("Invalid method. Choose 'hungarian' or 'pot'.") from None


def _match_launch(kind, entry, ws_bytes, diag, raw_dev, prev_dev, min_overlap, stream, extra=()):
    """One call of a chain entry over raw_dev (K x W int32 CUDA) against prev_dev (W int32 CUDA or None) -> (matched K x W
    int32 CUDA, info K x 8 int32 NumPy, the diagnostic output K x diag[0] of dtype name diag[1] on the device -- allocated by
    torch's diag[2], "empty" where the entry fills it itself -- or None for diag None).  The workspace is cached per (device,
    stream, kind) and only grows; ws_bytes is its size for this call, or a callable for a size that never changes, asked
    when nothing is cached.  `extra` are the entry's arguments between min_overlap and matched_out.  Synchronises the
    stream."""
    import ctypes as C

    import torch

    from . import _lib

    K, W = raw_dev.shape
    dev = raw_dev.device
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        key = (dev, st.cuda_stream, kind)
        ws = _MATCH_WS.get(key)
        if ws is None or (not callable(ws_bytes) and ws.numel() < ws_bytes):
            if len(_MATCH_WS) > 16:
                _MATCH_WS.clear()
            ws = _MATCH_WS[key] = torch.empty(int(ws_bytes()) if callable(ws_bytes) else ws_bytes, dtype=torch.uint8, device=dev)
        matched = torch.empty((K, W), dtype=torch.int32, device=dev)
        info = torch.empty((K, 8), dtype=torch.int32, device=dev)
        out = getattr(torch, diag[2])((K, diag[0]), dtype=getattr(torch, diag[1]), device=dev) if diag else None
        _lib.call(entry, _eng.ptr(raw_dev), K, W, _eng.ptr(prev_dev) if prev_dev is not None else None, int(min_overlap), *extra,
                  _eng.ptr(matched), _eng.ptr(info), _eng.ptr(out) if diag else None, _eng.ptr(ws), ws.numel(),
                  C.c_void_p(st.cuda_stream))
        info_h = info.cpu().numpy()
    return matched, info_h, out


def match_chain_launch(raw_dev, prev_dev, min_overlap, stream=None, want_plan=False, method="pot"):
    """One mused_match_pot_chain (method "pot") or mused_match_hung_chain ("hungarian") launch over raw_dev (K x W int32
    CUDA) against prev_dev (W int32 CUDA or None) -> (matched K x W int32 CUDA, info K x 8 int32 NumPy, and with want_plan
    the diagnostic output, else None: plans K x 65536 fp64 CUDA for "pot", assign K x 256 int32 CUDA -- the column of each
    row of the P x N cost matrix or -1 -- for "hungarian").  Synchronises the stream."""
    from . import _lib

    entry, ws_entry, diag_len, diag_dtype = _match_entry(method)
    return _match_launch(method, entry, getattr(_lib.lib(), ws_entry), (diag_len, diag_dtype, "zeros") if want_plan else None,
                         raw_dev, prev_dev, min_overlap, stream)


MATCH_WIDE_MAXC = 4096   # distinct labels a side the wide Hungarian chain takes (csrc/match_wide.hip)
MATCH_WIDE_MAX_W = 1 << 20


def match_wide_launch(raw_dev, prev_dev, min_overlap, stream=None, want_assign=False, max_steps=0):
    """One mused_match_hung_wide_chain call (csrc/match_wide.hip: any int32 label values, up to 4,096 distinct labels a side)
    over raw_dev (K x W int32 CUDA, the TRUE label values) against prev_dev (W int32 CUDA or None) -> (matched K x W int32
    CUDA, info K x 8 int32 NumPy, and with want_assign the K x 4096 int32 CUDA columns of each row or -1, else None).
    max_steps: the solver's step budget per window (0: 32 min(P, N)).  Synchronises the stream."""
    from . import _lib

    W = int(raw_dev.shape[1])
    need = int(_lib.lib().mused_match_hung_wide_ws_bytes(W))
    if need < 0:
        raise ValueError(f"match_wide_launch: W = {W} outside [1, 2^20]")
    return _match_launch("hungarian_wide", "mused_match_hung_wide_chain", need,
                         (MATCH_WIDE_MAXC, "int32", "empty") if want_assign else None, raw_dev, prev_dev, min_overlap, stream,
                         extra=(int(max_steps),))


def _labels_to_device_wide(x, device):
    """int32 CUDA labels with their TRUE values (no clamp: the wide chain takes every int32), or None when a value does not
    fit int32 -- such a window is the host's."""
    import torch

    lo, hi = -(1 << 31), (1 << 31) - 1
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.int32 and x.numel() and (int(x.min()) < lo or int(x.max()) > hi):
            return None
        return x.to(device).to(torch.int32).contiguous()
    a = np.asarray(x)
    if a.dtype != np.int32:
        if a.dtype.kind not in "iub" or (a.size and (int(a.min()) < lo or int(a.max()) > hi)):
            return None
        a = a.astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _wide_mode(wide, method):
    """The `wide` keyword of the public functions -> False, True (the narrow chain first, what it flags 4 or 8 to the wide
    one) or "only" (straight to the wide chain: labels known to hold -1).  MUSED_MATCH_WIDE=host, read per call, turns it
    off: flagged windows take the host route as they did before the wide chain existed."""
    if not wide:
        return False
    if method != "hungarian":
        raise ValueError("wide=True is for method 'hungarian' only (the Sinkhorn chain has no wide entry)")
    if os.environ.get("MUSED_MATCH_WIDE", "device") == "host":
        return False
    return "only" if wide == "only" else True


def match_chain_on_device(raw_windows, prev0=None, min_overlap=3, stream=None, method="pot", wide=False, max_steps=0):
    """`distributed.replay_label_chain(raw_windows, match_clusters, method=method)` with the whole chain in one launch of
    csrc/match.hip ("pot") or csrc/match_hung.hip ("hungarian"): matched_t = match_clusters(matched_{t-1}, raw_t, method,
    min_overlap), window 0 against prev0 (None: it passes through).  raw_windows: (K, W) NumPy array or int32 / int64 CUDA
    tensor.  Returns the K * W matched labels (NumPy int64).  A window the kernel flags (head of the kernel's source file) is
    matched by the host `match_clusters` and counted in `match_fallbacks`; the chain is launched again behind it.  Where
    SciPy finds no complete assignment (flag 16) that host call raises its ValueError, as the host chain does.

    wide=True ("hungarian" only): a window the narrow chain flags 4 (a label outside [0, 1024)) or 8 (more than 256 labels
    a side) goes to the wide chain (csrc/match_wide.hip: any int32 value, 4,096 labels a side), which then runs the rest of
    the chain; only what THAT flags (8, 16, 32) or a label that does not fit int32 goes to the host and is counted.
    wide="only" skips the narrow launch.  max_steps: the wide solver's step budget (0: 32 min(P, N))."""
    import torch

    _match_entry(method)
    wide = _wide_mode(wide, method)
    dev = raw_windows.device if isinstance(raw_windows, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    stream = _match_stream(stream)
    with torch.cuda.stream(stream):
        return _match_chain(raw_windows, prev0, min_overlap, stream, dev, method, wide, max_steps)


def _narrow_flags_only(word) -> bool:
    """The narrow chain gave the window up for its own limits alone (flags 4 and 8), not for a missing assignment."""
    word = int(word)
    return bool(word & (MATCH_FLAG_RANGE | MATCH_FLAG_SIZE)) and not word & ~(MATCH_FLAG_RANGE | MATCH_FLAG_SIZE)


def _match_chain(raw_windows, prev0, min_overlap, stream, dev, method, wide=False, max_steps=0):
    import torch

    if not isinstance(raw_windows, torch.Tensor):
        raw_windows = np.asarray(raw_windows)
    if raw_windows.ndim != 2:
        raise ValueError("raw_windows must be (K, W)")
    raw_dev = _labels_to_device(raw_windows, dev) if wide != "only" else None
    K, W = raw_windows.shape
    out = np.empty((K, W), dtype=np.int64)
    if K == 0 or W == 0:
        return out.ravel()
    raw_host = None
    prev_host = None if prev0 is None or len(prev0) == 0 else prev0
    on_wide = wide == "only"   # once a window went to the wide chain the rest of the chain stays there
    t0 = 0
    while t0 < K:
        host_now = False
        if on_wide:
            # the wide upload keeps the true values: the windows up to the first one with a label that does not fit int32
            stop, block = K, _labels_to_device_wide(raw_windows[t0:], dev)
            if block is None:
                if raw_host is None:
                    raw_host = _labels_to_host(raw_windows)
                stop = next(t for t in range(t0, K) if _labels_to_device_wide(raw_host[t], dev) is None)
                block = _labels_to_device_wide(raw_host[t0:stop], dev) if stop > t0 else None
            prev_w = None if prev_host is None else _labels_to_device_wide(prev_host, dev)
            if block is None or (prev_host is not None and prev_w is None) or W > MATCH_WIDE_MAX_W:
                done, host_now = 0, True
            else:
                matched, info, _ = match_wide_launch(block, prev_w, min_overlap, stream, max_steps=max_steps)
                done = int(np.argmin(info[:, 6])) if not info[:, 6].all() else stop - t0
                host_now = t0 + done < K
        else:
            prev_dev = None if prev_host is None else _labels_to_device(prev_host, dev)
            matched, info, _ = match_chain_launch(raw_dev[t0:], prev_dev, min_overlap, stream, method=method)
            done = int(np.argmin(info[:, 6])) if not info[:, 6].all() else K - t0
            if done < K - t0:
                if wide and _narrow_flags_only(info[done, 4]):
                    on_wide = True
                else:
                    host_now = True
        if done:
            out[t0:t0 + done] = matched[:done].cpu().numpy()
            prev_host = out[t0 + done - 1]
        t0 += done
        if host_now and t0 < K:   # the flagged window: host specification, then on from the next one
            if raw_host is None:
                raw_host = _labels_to_host(raw_windows)
            _match_count_fallback()
            out[t0] = match_clusters(None if prev_host is None else _labels_to_host(prev_host), raw_host[t0], method, min_overlap)
            prev_host = out[t0]
            t0 += 1
    return out.ravel()


def match_clusters_on_device(prev_clusters, new_clusters, min_overlap=3, stream=None, method="pot", wide=False, max_steps=0):
    """`match_clusters(prev_clusters, new_clusters, method, min_overlap)` on the device (csrc/match.hip for "pot",
    csrc/match_hung.hip for "hungarian"; NumPy arrays or int32 / int64 CUDA tensors).  Returns what match_clusters returns:
    `new_clusters` itself without a previous window or when the overlap costs are infeasible, the relabelled array
    otherwise.  A window the kernel flags is matched by the host `match_clusters` (which raises SciPy's ValueError where no
    complete assignment exists) and counted in `match_fallbacks`.  wide, max_steps: as for match_chain_on_device -- with
    wide=True a window flagged 4 or 8 goes to csrc/match_wide.hip, and only what that flags goes to the host."""
    import torch

    _match_entry(method)
    wide = _wide_mode(wide, method)
    if prev_clusters is None or len(prev_clusters) == 0:
        return new_clusters
    dev = new_clusters.device if isinstance(new_clusters, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    stream = _match_stream(stream)
    info = None
    with torch.cuda.stream(stream):
        if wide != "only":
            matched, info, _ = match_chain_launch(_labels_to_device(new_clusters, dev).reshape(1, -1),
                                                  _labels_to_device(prev_clusters, dev), min_overlap, stream, method=method)
        if wide and (info is None or (not info[0, 6] and _narrow_flags_only(info[0, 4]))):
            new_w, prev_w = _labels_to_device_wide(new_clusters, dev), _labels_to_device_wide(prev_clusters, dev)
            if new_w is None or prev_w is None or new_w.numel() > MATCH_WIDE_MAX_W:
                info = np.zeros((1, 8), dtype=np.int32)   # not the device's: the host route below
            else:
                matched, info, _ = match_wide_launch(new_w.reshape(1, -1), prev_w, min_overlap, stream, max_steps=max_steps)
    if not info[0, 6]:
        _match_count_fallback()
        return match_clusters(_labels_to_host(prev_clusters), _labels_to_host(new_clusters), method, min_overlap)
    if not info[0, 3]:
        return new_clusters
    return matched[0].cpu().numpy().astype(np.int64)


def perform_dbscan_clustering(data, eps=0.5, min_samples=5):
    """matrix_operations.py:235-238."""
    from sklearn.cluster import DBSCAN

    return DBSCAN(eps=eps, min_samples=min_samples, metric="euclidean").fit_predict(data)


# calls that perform_dbscan_clustering_on_device finished with scikit-learn on the host although the device was asked: the
# kernel's ambiguity flag (a pair within rounding of eps) or its non-finite flag (scikit-learn raises there)
dbscan_fallbacks = 0
DBSCAN_MAX_ROWS = 1 << 19   # csrc/dbscan.hip: what the tile grid of one launch holds


def _dbscan_count_fallback():
    global dbscan_fallbacks
    with _km_fallback_lock:
        dbscan_fallbacks += 1


# inserts that mused_amd.incdbscan.IncrementalDBSCAN answered with scikit-learn's refit on the host although the device was
# asked: the insert whose kernel raised the ambiguity flag and every later insert of that object
dbscan_incr_fallbacks = 0


def _dbscan_incr_count_fallback():
    global dbscan_incr_fallbacks
    with _km_fallback_lock:
        dbscan_incr_fallbacks += 1


def dbscan_launch(X_dev, eps, min_samples, stream=None):
    """One mused_dbscan call on an (n, d) fp64 CUDA tensor (unit stride along the columns) -> (labels n int32 CUDA, info
    4 int32 NumPy = {flags, clusters, core rows, 0}; flags: mused_amd.dbscan.FLAG_*).  Synchronises the stream."""
    import ctypes as C

    import torch

    from . import _lib

    n, d = X_dev.shape
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        ws = torch.empty(int(_lib.lib().mused_dbscan_ws_bytes(n)), dtype=torch.uint8, device=X_dev.device)
        labels = torch.empty(n, dtype=torch.int32, device=X_dev.device)
        info = torch.empty(4, dtype=torch.int32, device=X_dev.device)
        _lib.call("mused_dbscan", _eng.ptr(X_dev), n, d, X_dev.stride(0), float(eps), int(min_samples), _eng.ptr(labels),
                  _eng.ptr(info), _eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
        info_h = info.cpu().numpy()
    return labels, info_h


# ---- DBSCAN's eps from the data (csrc/kdist.hip; the rule: mused_amd/kdist.py) --------------------------------------------
# the eps that the last eps="auto" call of perform_dbscan_clustering_on_device chose (None before the first)
last_chosen_eps = None


def _kdist_rows(X, k):
    """X as an (n, d) fp64 CUDA tensor with unit column stride (uploads and conversions on the current stream), k checked."""
    import numbers

    import torch

    from . import kdist as _kd

    if isinstance(X, torch.Tensor):
        Xd = X if X.is_cuda else X.cuda()
    else:
        a = np.asarray(X)
        if a.dtype.kind not in "fiub":
            raise ValueError("X must be numeric")
        Xd = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    if Xd.dim() != 2 or Xd.shape[0] < 1 or Xd.shape[1] < 1:
        raise ValueError("X must be (n, d) with n, d >= 1")
    if Xd.dtype != torch.float64:
        Xd = Xd.to(torch.float64)
    if Xd.stride(1) != 1 or Xd.stride(0) < Xd.shape[1]:
        Xd = Xd.contiguous()
    n = Xd.shape[0]
    if not isinstance(k, numbers.Integral) or isinstance(k, bool) or not 1 <= k <= min(n, _kd.MAX_K):
        raise ValueError(f"k must be an integer in [1, min(n, {_kd.MAX_K})] (n = {n}), got {k!r}")
    if n > _kd.MAX_ROWS or Xd.shape[1] >= 1 << 20:
        raise ValueError(f"{n} x {Xd.shape[1]} rows: the device k-distances take at most 2^19 rows "
                         "(MUSED_KDIST=host runs the NumPy rule at any size)")
    return Xd, int(k)


def _kdist_host() -> bool:
    """MUSED_KDIST (read at every call): "device" (default) or "host" = the NumPy rule of mused_amd/kdist.py."""
    return os.environ.get("MUSED_KDIST", "device") == "host"


def _kdist_to_host(X):
    return X.detach().cpu().numpy() if hasattr(X, "detach") else np.asarray(X)


def kth_distance_launch(Xd, k, st):
    """mused_kth_distance enqueued on stream `st` (entered by the caller): (kd2 n fp64 CUDA, SQUARED; info 4 int32 CUDA).
    Nothing is read."""
    import ctypes as C

    import torch

    from . import _lib

    n, d = Xd.shape
    ws = _km_workspace(("kth_distance", n, k, Xd.device, st.cuda_stream), _lib.lib().mused_kth_distance_ws_bytes(n, k), Xd.device)
    kd2 = torch.empty(n, dtype=torch.float64, device=Xd.device)
    info = torch.empty(4, dtype=torch.int32, device=Xd.device)
    _lib.call("mused_kth_distance", _eng.ptr(Xd), n, d, Xd.stride(0), k, _eng.ptr(kd2), _eng.ptr(info), _eng.ptr(ws), ws.numel(),
              C.c_void_p(st.cuda_stream))
    return kd2, info


def _kdist_raise_nonfinite():
    raise ValueError("Input contains NaN or infinity.")   # (scikit-learn's check_array text, as mused_amd.dbscan)


def kth_neighbor_distances_on_device(X, k, stream=None):
    """The distance of every row to its k-th nearest row, the row itself counted -- column k - 1 of
    `NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X)[0]` -- as an n fp64 CUDA tensor (csrc/kdist.hip; the rule and its
    bound: mused_amd/kdist.py).  X: (n, d) NumPy array or tensor (taken as fp64), n <= 2^19; 1 <= k <= min(n, 64).
    Raises scikit-learn's ValueError for a non-finite row (the call reads the flag, so it returns after the stream has
    finished) and ValueError for k outside its range.  MUSED_KDIST=host: the NumPy rule on a host copy, uploaded."""
    import torch

    from . import kdist as _kd

    if _kdist_host():
        v = np.sqrt(_kd.kth_sq_distances(_kdist_to_host(X), k))
        return torch.from_numpy(np.ascontiguousarray(v)).cuda()
    st = _match_stream(stream)
    with torch.cuda.stream(st):
        Xd, k = _kdist_rows(X, k)
        kd2, info = kth_distance_launch(Xd, k, st)
        out = torch.sqrt(kd2)
        flags = int(info.cpu().numpy()[0])
    if flags & _kd.FLAG_NONFINITE:
        _kdist_raise_nonfinite()
    return out


def select_eps_on_device(embedding, min_samples, stream=None):
    """DBSCAN's eps from the sorted k-distance curve of `embedding` (k = min_samples, the row itself counted): the midpoint
    between the curve's value at its knee and the next larger value, so that no k-th neighbour pair lies on the threshold
    and the device DBSCAN can use it (mused_amd/kdist.py; csrc/kdist.hip: the pair pass, the sort and the knee all run on
    the device, one 48-byte read).  Returns (eps, info) with info = {"knee": i*, "next": nxt, "v_knee": v[i*],
    "v_next": v[nxt], "curve": the sorted curve as an n fp64 CUDA tensor}.
    embedding: (n, d) NumPy array or tensor, n <= 2^19; 2 <= min_samples <= min(n, 64) in effect: min_samples = 1 gives
    the flat curve of zeros.  Raises scikit-learn's ValueError for a non-finite row and ValueError for min_samples
    outside [1, min(n, 64)] and for a flat curve (all k-distances equal).  MUSED_KDIST=host: the NumPy rule."""
    import ctypes as C

    import torch

    from . import _lib
    from . import kdist as _kd

    if _kdist_host():
        Xh = _kdist_to_host(embedding)
        v = np.sort(np.sqrt(_kd.kth_sq_distances(Xh, min_samples)))
        i, nxt = _kd.knee(v)
        return float(0.5 * (v[i] + v[nxt])), {"knee": i, "next": nxt, "v_knee": float(v[i]), "v_next": float(v[nxt]),
                                             "curve": torch.from_numpy(v).cuda()}
    st = _match_stream(stream)
    with torch.cuda.stream(st):
        Xd, k = _kdist_rows(embedding, min_samples)
        n = Xd.shape[0]
        kd2, info_k = kth_distance_launch(Xd, k, st)
        nb = int(_lib.lib().mused_eps_knee_ws_bytes(n))
        ws = torch.empty(nb, dtype=torch.uint8, device=Xd.device)   # (its head is returned as the curve: not shared)
        res = torch.empty(64, dtype=torch.uint8, device=Xd.device)  # the knee's 48 bytes | the k-distances' info
        # (a flagged mused_kth_distance leaves kd2 as allocated; its flag is looked at first, below)
        _lib.call("mused_eps_knee", _eng.ptr(kd2), n, _eng.ptr(res), _eng.ptr(ws), nb, C.c_void_p(st.cuda_stream))
        res[48:].copy_(info_k.view(torch.uint8))
        h = res.cpu().numpy()                                        # ONE read
        flags_k = int(h[48:52].view(np.int32)[0])
        h = h[:48]
    if flags_k & _kd.FLAG_NONFINITE:
        _kdist_raise_nonfinite()
    idx, num = h.view(np.int64), h.view(np.float64)
    flags = int(idx[5])
    if flags & _kd.FLAG_NONFINITE:
        _kdist_raise_nonfinite()
    if flags & _kd.FLAG_FLAT:
        raise ValueError(_kd.FLAT_TEXT)
    return float(num[4]), {"knee": int(idx[0]), "next": int(idx[1]), "v_knee": float(num[2]), "v_next": float(num[3]),
                           "curve": ws[: 8 * n].view(torch.float64)}


# ---- orthogonal Procrustes: one window's embedding in the previous window's frame (csrc/procrustes.hip; the rule:
# mused_amd/procrustes.py) ------------------------------------------------------------------------------------------------
# calls that orthogonal_procrustes_on_device / align_embedding_on_device answered with SciPy on a host copy of the shared rows
# although the device was asked: a flagged kernel (ill-conditioned A^T B, sweep cap) or more than 128 columns
procrustes_fallbacks = 0


def _procrustes_count_fallback():
    global procrustes_fallbacks
    with _km_fallback_lock:
        procrustes_fallbacks += 1


def _align_host() -> bool:
    """MUSED_ALIGN (read at every call): "device" (default) or "host" = scipy.linalg.orthogonal_procrustes on host copies."""
    return os.environ.get("MUSED_ALIGN", "device") == "host"


def _procrustes_rows(X):
    """X as an (m, r) fp64 CUDA tensor with unit column stride and a row pitch >= r (row-offset and column-prefix views stay
    views; uploads and conversions on the current stream)."""
    import torch

    if isinstance(X, torch.Tensor):
        Xd = X if X.is_cuda else X.cuda()
    else:
        a = np.asarray(X)
        if a.dtype.kind not in "fiub":
            raise ValueError("expected a numeric matrix")
        Xd = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    if Xd.dim() != 2:
        raise ValueError(f"expected matrix, got shape {tuple(Xd.shape)}")
    if Xd.shape[0] < 1 or Xd.shape[1] < 1:
        raise ValueError("expected a matrix with at least one row and one column")
    if Xd.dtype != torch.float64:
        Xd = Xd.to(torch.float64)
    if Xd.stride(1) != 1 or Xd.stride(0) < Xd.shape[1]:
        Xd = Xd.contiguous()
    return Xd


def _procrustes_scipy(A, B):
    """SciPy's call on host copies of two operands -> (R, scale) as NumPy; raises SciPy's ValueError for a non-finite entry."""
    from scipy.linalg import orthogonal_procrustes

    return orthogonal_procrustes(_kdist_to_host(A), _kdist_to_host(B))


def _procrustes_raise_nonfinite():
    from . import procrustes as _pr

    raise ValueError(_pr.NONFINITE_TEXT)


def procrustes_launch(Ad, Bd, st):
    """mused_procrustes enqueued on stream `st` (entered by the caller) for two (m, r) fp64 CUDA operands, r <= 128:
    (R r x r, out 4 fp64 = {scale, sigma_max, sigma_min, 0}, info 4 int32 = {flags, sweeps, 0, 0}, workspace), all on the
    device.  Nothing is read."""
    import ctypes as C

    import torch

    from . import _lib

    m, r = Ad.shape
    ws = _km_workspace(("procrustes", m, r, Ad.device, st.cuda_stream), _lib.lib().mused_procrustes_ws_bytes(m, r), Ad.device)
    R = torch.empty((r, r), dtype=torch.float64, device=Ad.device)
    outf = torch.empty(4, dtype=torch.float64, device=Ad.device)
    info = torch.empty(4, dtype=torch.int32, device=Ad.device)
    _lib.call("mused_procrustes", _eng.ptr(Ad), Ad.stride(0), _eng.ptr(Bd), Bd.stride(0), m, r, _eng.ptr(R), _eng.ptr(outf),
              _eng.ptr(info), _eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
    return R, outf, info, ws


def svd_jacobi_small_launch(M, stream=None):
    """mused_svd_jacobi_small on an (r, r) fp64 CUDA matrix (row pitch >= r), r <= 128: (W = M V r x r, sigma r, info 4 int32 =
    {flags, sweeps, 0, 0}) on the device; the one-sided Jacobi of the Procrustes kernel alone.  Nothing is read."""
    import ctypes as C

    import torch

    from . import _lib

    st = _match_stream(stream)
    with torch.cuda.stream(st):
        Md = _procrustes_rows(M)
        r = Md.shape[1]
        if Md.shape[0] != r:
            raise ValueError(f"expected a square matrix, got {tuple(Md.shape)}")
        W = torch.empty((r, r), dtype=torch.float64, device=Md.device)
        sigma = torch.empty(r, dtype=torch.float64, device=Md.device)
        info = torch.empty(4, dtype=torch.int32, device=Md.device)
        _lib.call("mused_svd_jacobi_small", _eng.ptr(Md), Md.stride(0), r, _eng.ptr(W), _eng.ptr(sigma), _eng.ptr(info),
                  C.c_void_p(st.cuda_stream))
    return W, sigma, info


def _procrustes_pair(A, B):
    Ad, Bd = _procrustes_rows(A), _procrustes_rows(B)
    if Ad.shape != Bd.shape:
        raise ValueError(f"the shapes of A and B differ ({tuple(Ad.shape)} vs {tuple(Bd.shape)})")   # (SciPy's text)
    return Ad, Bd


def orthogonal_procrustes_on_device(A, B, stream=None):
    """`scipy.linalg.orthogonal_procrustes(A, B)` on the device: (R, scale) as fp64 CUDA tensors (r x r and 0-dim), R the
    orthogonal matrix (det +-1) that minimises |A R - B|_F, scale the sum of the singular values of A^T B
    (csrc/procrustes.hip; the rule and its bound: mused_amd/procrustes.py).  A, B: (m, r) NumPy arrays (uploaded) or
    tensors, taken as fp64.  The call reads the kernel's 16 bytes of flags, so it returns after the stream has finished:
    a non-finite entry raises SciPy's ValueError; an ill-conditioned A^T B (sigma_min <= 2^-14 sigma_max: m < r, a zero
    column), the sweep cap or r > 128 is answered by SciPy on a host copy and counted in `procrustes_fallbacks`.
    MUSED_ALIGN=host: SciPy for every call."""
    import torch

    from . import procrustes as _pr

    if _align_host():
        R, scale = _procrustes_scipy(A, B)
        return torch.from_numpy(np.ascontiguousarray(R)).cuda(), torch.tensor(float(scale), dtype=torch.float64).cuda()
    st = _match_stream(stream)
    with torch.cuda.stream(st):
        Ad, Bd = _procrustes_pair(A, B)
        flags = -1
        if Ad.shape[1] <= _pr.MAX_R:
            R, outf, info, _ = procrustes_launch(Ad, Bd, st)
            flags = int(info.cpu().numpy()[0])
            if flags & _pr.FLAG_NONFINITE:
                _procrustes_raise_nonfinite()
        if flags != 0:
            _procrustes_count_fallback()
            R_h, scale_h = _procrustes_scipy(Ad, Bd)
            return (torch.from_numpy(np.ascontiguousarray(R_h)).to(Ad.device),
                    torch.tensor(float(scale_h), dtype=torch.float64, device=Ad.device))
    return R, outf[0]


def align_embedding_on_device(E_new, E_ref, shift, stream=None):
    """One hopping window's embedding in the previous window's frame: (aligned (W, r) fp64 CUDA tensor = E_new R, R,
    residual, unaligned) with R = orthogonal_procrustes(A, B)[0] over the rows the windows share, A = E_new[:W - shift] and
    B = E_ref[shift:]; residual = |A R - B|_F / |B|_F, unaligned = |A - B|_F / |B|_F (Python floats).  The product and the
    three sums are one pass over E_new on the device (mused_procrustes_apply); what is read is the flags and the sums,
    40 bytes.  E_new is not modified.  Flags, r > 128 and MUSED_ALIGN=host as for orthogonal_procrustes_on_device: a
    fallback copies the shared rows to the host for SciPy's R and still multiplies on the device (r <= 128)."""
    import ctypes as C

    import torch

    from . import _lib
    from . import procrustes as _pr

    if _align_host():
        out, R, res, un = _align_scipy(_kdist_to_host(E_new), _kdist_to_host(E_ref), shift)
        return torch.from_numpy(np.ascontiguousarray(out)).cuda(), torch.from_numpy(np.ascontiguousarray(R)).cuda(), res, un
    st = _match_stream(stream)
    with torch.cuda.stream(st):
        En, Er = _procrustes_pair(E_new, E_ref)
        n, r = En.shape
        shift = _align_shift(shift, n)
        m = n - shift
        A, B = En[:m], Er[shift:]
        if r > _pr.MAX_R:
            _procrustes_count_fallback()
            out, R, res, un = _align_scipy(En.cpu().numpy(), Er.cpu().numpy(), shift)
            return torch.from_numpy(np.ascontiguousarray(out)).to(En.device), torch.from_numpy(np.ascontiguousarray(R)).to(En.device), res, un
        R, _, info, ws = procrustes_launch(A, B, st)
        out = torch.empty((n, r), dtype=torch.float64, device=En.device)
        sums = torch.empty(3, dtype=torch.float64, device=En.device)

        def apply(R_):
            _lib.call("mused_procrustes_apply", _eng.ptr(En), En.stride(0), n, r, _eng.ptr(R_), _eng.ptr(out), out.stride(0),
                      _eng.ptr(B), B.stride(0), m, _eng.ptr(sums), _eng.ptr(ws), C.c_void_p(st.cuda_stream))
            return torch.cat([info.to(torch.float64), sums]).cpu().numpy()   # ONE read: {flags, sweeps, 0, 0, three sums}

        rec = apply(R)
        flags = int(rec[0])
        if flags & _pr.FLAG_NONFINITE:
            _procrustes_raise_nonfinite()
        if flags:
            _procrustes_count_fallback()
            R = torch.from_numpy(np.ascontiguousarray(_procrustes_scipy(A, B)[0])).to(En.device)
            rec = apply(R)
    with np.errstate(divide="ignore", invalid="ignore"):
        res, un = float(np.sqrt(rec[4] / rec[5])), float(np.sqrt(rec[6] / rec[5]))
    return out, R, res, un


def _align_shift(shift, n):
    import numbers

    if not isinstance(shift, numbers.Integral) or isinstance(shift, bool) or not 0 < shift < n:
        raise ValueError(f"shift must be an integer in (0, W = {n}): the windows share W - shift rows, got {shift!r}")
    return int(shift)


def _align_scipy(E_new, E_ref, shift):
    """align_embedding_on_device on the host with SciPy's R: (E_new R, R, residual, unaligned), NumPy."""
    E_new = np.asarray(E_new, dtype=np.float64)
    E_ref = np.asarray(E_ref, dtype=np.float64)
    if E_new.ndim != 2 or E_new.shape != E_ref.shape:
        raise ValueError(f"the shapes of A and B differ ({E_new.shape} vs {E_ref.shape})")
    shift = _align_shift(shift, E_new.shape[0])
    A, B = E_new[:E_new.shape[0] - shift], E_ref[shift:]
    R = _procrustes_scipy(A, B)[0]
    nb = np.linalg.norm(B)
    with np.errstate(divide="ignore", invalid="ignore"):
        return E_new @ R, R, float(np.linalg.norm(A @ R - B) / nb), float(np.linalg.norm(A - B) / nb)


def perform_dbscan_clustering_on_device(emb, eps=0.5, min_samples=5, stream=None):
    """`perform_dbscan_clustering(emb, eps, min_samples)` with the pair work on the device (csrc/dbscan.hip; the rule and
    its rounding margin: mused_amd/dbscan.py): scikit-learn's labels as int64 NumPy, O(n) device memory beside the rows.
    emb: (n, d) fp64 CUDA tensor or ndarray.  Where the kernel raises its ambiguity flag (some pair lies within rounding
    of eps) or its non-finite flag, the host `perform_dbscan_clustering` runs on a host copy -- it raises what
    scikit-learn raises -- and the call is counted in `dbscan_fallbacks`.  What the kernel does not take goes to the host
    call uncounted: MUSED_DBSCAN=host (the former path as a whole), rows that are not fp64 (scikit-learn's arithmetic
    follows the dtype), arguments scikit-learn rejects, more than 2^19 rows.
    stream: the kernels run on it behind whatever the current stream holds; the call returns after they have finished (it
    reads the flags), so `emb` need only stay alive until then.
    eps="auto": eps is chosen first, by `select_eps_on_device(emb, min_samples)` (the knee of the sorted k-distance curve;
    it raises for min_samples = 1, a flat curve and non-finite rows), kept in `last_chosen_eps`, and the call goes on with
    that number."""
    import numbers
    import os

    import torch

    on_dev = isinstance(emb, torch.Tensor)
    if isinstance(eps, str):
        if eps != "auto":
            raise ValueError(f'eps must be a number or "auto", got {eps!r}')
        global last_chosen_eps
        eps, _ = select_eps_on_device(emb, min_samples, stream)
        last_chosen_eps = eps

    def host():
        return perform_dbscan_clustering(emb.cpu().numpy() if on_dev else emb, eps=eps, min_samples=min_samples)

    if os.environ.get("MUSED_DBSCAN", "device") == "host":
        return host()
    X = emb if on_dev else np.asarray(emb)
    ok = (isinstance(eps, numbers.Real) and not isinstance(eps, bool) and 0.0 < float(eps) < 1e150
          and isinstance(min_samples, numbers.Integral) and not isinstance(min_samples, bool) and 1 <= min_samples < 2 ** 31
          and X.ndim == 2 and 1 <= X.shape[0] <= DBSCAN_MAX_ROWS and 1 <= X.shape[1] < 2 ** 20
          and X.dtype in (torch.float64, np.float64))
    if not ok:
        return host()
    st = _match_stream(stream)
    with torch.cuda.stream(st):
        Xd = X if on_dev else torch.from_numpy(np.ascontiguousarray(X)).cuda()
        if Xd.stride(1) != 1 or Xd.stride(0) < Xd.shape[1]:
            Xd = Xd.contiguous()
        labels, info = dbscan_launch(Xd, eps, min_samples, st)
        if info[0]:
            _dbscan_count_fallback()
            return host()
        return labels.cpu().numpy().astype(np.int64)


def perform_hdbscan_clustering(data, min_cluster_size=5, min_samples=2):
    """matrix_operations.py:240-243 (needs the optional `hdbscan` package, as the reference does)."""
    import hdbscan

    return hdbscan.HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, metric="euclidean").fit_predict(data)


def perform_hdbscan_clustering_sklearn(data, min_cluster_size=5, min_samples=2):
    """scikit-learn's own estimator on host rows (its labels as int64; rows that are not finite are labelled as it labels
    them): what `perform_hdbscan_clustering_on_device` is pinned to, and its host path."""
    from sklearn.cluster import HDBSCAN

    labels = HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, metric="euclidean").fit_predict(data)
    return np.asarray(labels, dtype=np.int64)


# calls that perform_hdbscan_clustering_on_device finished with scikit-learn on the host although the device was asked: the
# kernel's ambiguity flag (some component's runner-up within rounding of its pick), its non-finite flag, or two tree edges
# of exactly equal weight
hdbscan_fallbacks = 0


def _hdbscan_count_fallback():
    global hdbscan_fallbacks
    with _km_fallback_lock:
        hdbscan_fallbacks += 1


def emst_launch(X_dev, stream=None, events=None):
    """One mused_emst call on an (n, d) fp64 CUDA tensor (unit stride along the columns) -> (edges (2, n - 1) int32 CUDA, d2
    (n - 1) fp64 CUDA, info 4 int32 NumPy = {flags, edges written, rounds run, 0}; flags: mused_amd.hdbscan.FLAG_*).
    Synchronises the stream (the one read of `info`).  events: a pair of torch.cuda.Event(enable_timing=True), recorded
    on the stream right before and right after the C call."""
    import ctypes as C

    import torch

    from . import _lib

    n, d = X_dev.shape
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        ws = torch.empty(int(_lib.lib().mused_emst_ws_bytes(n)), dtype=torch.uint8, device=X_dev.device)
        edges = torch.empty((2, max(n - 1, 1)), dtype=torch.int32, device=X_dev.device)
        d2 = torch.empty(max(n - 1, 1), dtype=torch.float64, device=X_dev.device)
        info = torch.empty(4, dtype=torch.int32, device=X_dev.device)
        if events:
            events[0].record(st)
        _lib.call("mused_emst", _eng.ptr(X_dev), n, d, X_dev.stride(0), _eng.ptr(edges[0]), _eng.ptr(edges[1]), _eng.ptr(d2),
                  _eng.ptr(info), _eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
        if events:
            events[1].record(st)
        info_h = info.cpu().numpy()
    return edges[:, :n - 1], d2[:n - 1], info_h


def perform_hdbscan_clustering_on_device(emb, min_cluster_size=5, min_samples=2, stream=None, timings=None):
    """sklearn.cluster.HDBSCAN(min_cluster_size, min_samples, metric="euclidean").fit_predict(emb) as int64 NumPy labels, with
    the O(n^2 d) part on the device: for min_samples <= 2 the mutual-reachability distance is the distance, so the
    estimator's tree is the Euclidean minimum spanning tree, which csrc/emst.hip computes in O(n) device memory beside the
    rows (the split, the rounding argument and why min_samples >= 3 is not taken: mused_amd/hdbscan.py).  Device: `mused_emst`
    on the caller's stream, one read of its `info`, the 2 (n - 1) edge indices.  Host: the weights with scikit-learn's bits,
    Prim's edge order from row 0, then scikit-learn's own single-linkage, condensed-tree and labelling routines.
    emb: (n, d) fp64 CUDA tensor or ndarray.  Where the kernel raises its ambiguity or non-finite flag, or two tree edges
    weigh exactly the same, `perform_hdbscan_clustering_sklearn` runs on a host copy and the call is counted in
    `hdbscan_fallbacks`.  What the device does not take goes there uncounted: min_samples >= 3 or None, rows that are not
    fp64, fewer than 2 or more than 2^19 rows, arguments scikit-learn rejects (it raises its own errors), a scikit-learn
    without the private routines.  This pins the labels to scikit-learn's HDBSCAN, NOT to the `hdbscan` package
    `perform_hdbscan_clustering` calls.
    stream: the kernels run on it behind whatever the current stream holds; the call returns after they have finished.
    timings: a dict that receives, where the device ran, "emst_ms" (events around the C call), "rounds" and "host_ms"
    (everything behind the read of the edges: host copy of the rows, weights, Prim's order, scikit-learn's routines)."""
    import numbers
    import time

    import torch

    from . import hdbscan as _hd

    on_dev = isinstance(emb, torch.Tensor)

    def host():
        return perform_hdbscan_clustering_sklearn(emb.cpu().numpy() if on_dev else emb, min_cluster_size=min_cluster_size,
                                                  min_samples=min_samples)

    X = emb if on_dev else np.asarray(emb)
    ok = (isinstance(min_cluster_size, numbers.Integral) and not isinstance(min_cluster_size, bool) and 2 <= min_cluster_size < 2 ** 31
          and isinstance(min_samples, numbers.Integral) and not isinstance(min_samples, bool) and 1 <= min_samples <= 2
          and X.ndim == 2 and 2 <= X.shape[0] <= _hd.MAX_ROWS and 1 <= X.shape[1] < 2 ** 20
          and X.dtype in (torch.float64, np.float64) and _hd.sklearn_internals() is not None)
    if not ok:
        return host()
    st = _match_stream(stream)
    with torch.cuda.stream(st):
        Xd = X if on_dev else torch.from_numpy(np.ascontiguousarray(X)).cuda()
        if Xd.stride(1) != 1 or Xd.stride(0) < Xd.shape[1]:
            Xd = Xd.contiguous()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if timings is not None else None
        edges, _, info = emst_launch(Xd, st, events=ev)
        if timings is not None:
            timings.update(emst_ms=ev[0].elapsed_time(ev[1]), rounds=int(info[2]))
        if info[0] or info[1] != X.shape[0] - 1:
            _hdbscan_count_fallback()
            return host()
        e = edges.cpu().numpy()
    t0 = time.perf_counter()
    Xh = emb.cpu().numpy() if on_dev else np.asarray(emb)
    labels, _ = _hd.labels_from_edges(Xh, e[0], e[1], min_cluster_size)
    if timings is not None:
        timings["host_ms"] = 1e3 * (time.perf_counter() - t0)
    if labels is None:
        _hdbscan_count_fallback()
        return host()
    return labels


def perform_dbscan_incr_clustering(data, previous_centroids, previous_labels, eps=0.5, min_samples=5):
    """matrix_operations.py:265-298: DBSCAN on the window, clusters renamed after the closest
    centroid of the previous window."""
    from scipy.spatial.distance import cdist
    from sklearn.cluster import DBSCAN

    if isinstance(eps, str):
        raise ValueError('eps="auto" is chosen on the device (select_eps_on_device); this host helper takes a number')
    if not isinstance(data, np.ndarray):
        data = np.array(data, dtype=np.float32)
    if data.ndim != 2:
        return None, previous_centroids, previous_labels
    labels = DBSCAN(eps=eps, min_samples=min_samples, metric="euclidean").fit_predict(data)
    found = set(labels) - {-1}
    centroids = np.array([data[labels == c].mean(axis=0) for c in found])
    if previous_centroids is not None and len(previous_centroids) > 0:
        nearest = np.argmin(cdist(centroids, previous_centroids), axis=1)
        rename = {new: (previous_labels[old] if old < len(previous_labels) else -1) for new, old in enumerate(nearest)}
        labels = np.array([rename[l] if l in rename else l for l in labels])
    return labels, centroids, np.unique(labels)
