"""The TF-IDF of one window of a tokenised corpus, from the corpus' integer arrays alone.  NumPy only.

PARITY PINNED: scikit-learn is installed, so tests/test_tfidf_host.py compares `tfidf_window` with
`TfidfVectorizer().fit_transform` (indptr, indices and data bit for bit) and `renormalise` with `normalize(T)`.
scikit-learn stays the authority -- MUSED_TEXT=host and every host-only corpus keep calling it; this module is the
statement of the rule the device kernels (csrc/tfidf.hip) follow step by step.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

EMPTY_VOCABULARY = "empty vocabulary; perhaps the documents only contain stop words"

_IDF = {}

# everything the device path produces for a window [s, e): the window CSR in stored order (indptr over the n documents;
# `term` = global term ids, `indices` = window column ids, `data` / `data2` = once / twice normalised values) and the
# per-term posting lists over ALL V global terms (absent terms: empty lists) with the documents' ranks ascending and the
# twice-normalised values -- what mused_sparse_cosine_knn reads
WindowTfidf = namedtuple("WindowTfidf", "n n_cols indptr term indices data data2 postptr postrow postval")


def idf_table(n: int) -> np.ndarray:
    """idf[j] of a term in j of n documents, j = 0 .. n: what TfidfTransformer.fit leaves in `idf_` (smooth_idf:
    full_like(df, n + 1) / (df + 1), log, + 1), computed by NumPy on the host and cached per n -- the device reads the
    table and never calls log, whose result is not guaranteed to equal NumPy's to the bit."""
    t = _IDF.get(n)
    if t is None:
        if len(_IDF) > 64:
            _IDF.clear()
        t = _IDF[n] = np.log((n + 1) / (np.arange(n + 1) + 1.0)) + 1.0
    return t


def _normalise_rows(indptr, data):
    """sklearn.utils.sparsefuncs_fast.inplace_csr_row_normalize_l2 on a copy: per row s = 0; s += v * v over the row in
    stored order (plain multiply and add), rows with s == 0 left alone, v /= sqrt(s).  Vectorised ACROSS rows, entry p of
    every row at a time, so each row's sum keeps its order."""
    out = np.array(data, dtype=np.float64)
    lens = np.diff(indptr)
    sums = np.zeros(len(lens))
    for p in range(int(lens.max()) if len(lens) else 0):
        rows = np.flatnonzero(lens > p)
        v = out[indptr[rows] + p]
        sums[rows] = sums[rows] + v * v
    nz = np.flatnonzero(sums != 0.0)
    scale = np.ones(len(lens))
    scale[nz] = np.sqrt(sums[nz])
    live = np.repeat(sums != 0.0, lens)
    out[live] = out[live] / np.repeat(scale, lens)[live]
    return out


def renormalise(indptr, data):
    """The values after one more L2 normalisation of the rows: what `normalize(T, copy=True)` returns, which is what
    cosine_similarity does to its input (it changes a few thousand values per window: not a no-op)."""
    return _normalise_rows(np.asarray(indptr), data)


def window_tfidf(corpus, s: int, e: int) -> WindowTfidf:
    """The rule, for rows [s, e) of `corpus` (mused_amd.text.TextCorpus).

    Documents are the valid rows in row order: n = vrank[e] - vrank[s].  Per term t, from the window alone: df[t] = the
    number of window documents that contain t, first[t] = the first of them; t is present when df[t] > 0 and its column
    id is its rank among the present terms (alphabetical: CountVectorizer._sort_features).  A row's entries are stored in
    ascending (first[t], position of t's first occurrence in document first[t]) order: CountVectorizer._count_vocab
    numbers the terms in order of first appearance and sorts every row by that number (`X.sort_indices()`), and
    `_sort_features` then renames the columns without sorting again -- rows are NOT sorted by column id.  Values:
    v = cnt * idf[df[t]] (TfidfTransformer.transform: `X.data *= idf_[X.indices]`), then the row normalisation of
    `_normalise_rows` (normalize -> inplace_csr_row_normalize_l2), and once more for `data2`.

    No valid row: an empty result (n = 0).  Valid rows without a present term: scikit-learn's ValueError."""
    if not 0 <= s <= e <= corpus.N:
        raise IndexError(f"window [{s}, {e}) outside a corpus of {corpus.N} rows")
    V = corpus.V
    n = int(corpus.vrank[e] - corpus.vrank[s])
    e0, e1 = int(corpus.rowptr[s]), int(corpus.rowptr[e])
    zi, zf = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64)
    if n == 0:
        return WindowTfidf(0, 0, np.zeros(1, dtype=np.int32), zi, zi, zf, zf, np.zeros(V + 1, dtype=np.int32), zi, zf)
    if e1 == e0:
        raise ValueError(EMPTY_VOCABULARY)
    term, cnt, pos = corpus.term[e0:e1].astype(np.int64), corpus.cnt[e0:e1], corpus.pos[e0:e1].astype(np.int64)
    rows = corpus.vrow[corpus.vrank[s]:corpus.vrank[e]]
    lens = (corpus.rowptr[rows + 1] - corpus.rowptr[rows]).astype(np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    doc = np.repeat(np.arange(n, dtype=np.int64), lens)        # the document (valid rank in the window) of every entry
    df = np.bincount(term, minlength=V)
    present = df > 0
    col = np.cumsum(present) - 1                               # rank among the present terms
    # entries are row-major, so a term's first entry is its entry in document first[t]
    uniq, first_entry = np.unique(term, return_index=True)
    key = np.zeros(V, dtype=np.int64)
    key[uniq] = ((corpus.vrow[corpus.vrank[s] + doc[first_entry]].astype(np.int64) - s) << 32) | pos[first_entry]
    order = np.lexsort((key[term], doc))                       # stored order inside every row
    term_s = term[order]
    raw = cnt[order].astype(np.float64) * idf_table(n)[df[term_s]]
    data = _normalise_rows(indptr, raw)
    data2 = _normalise_rows(indptr, data)
    # posting lists with values, documents ascending inside a term (a stable sort of the row-major entries)
    by_term = np.argsort(term_s, kind="stable")
    postptr = np.concatenate([[0], np.cumsum(df)]).astype(np.int32)
    return WindowTfidf(n, int(present.sum()), indptr.astype(np.int32), term_s.astype(np.int32), col[term_s].astype(np.int32),
                       data, data2, postptr, doc[order][by_term].astype(np.int32), data2[by_term])


def tfidf_window(corpus, s: int, e: int):
    """(n, indptr, indices, data) of TfidfVectorizer().fit_transform on the strings of the valid rows of [s, e)."""
    w = window_tfidf(corpus, s, e)
    return w.n, w.indptr, w.indices, w.data
