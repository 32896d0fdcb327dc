"""mused_amd.text / mused_amd.tfidf against scikit-learn on the host: the one-pass tokenisation and the per-window TF-IDF
rule the device kernels follow reproduce TfidfVectorizer().fit_transform and normalize(T) bit for bit."""
import numpy as np
import pytest

import tfidf_cases as tc
from mused_amd import text, tfidf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name,which,s,e", tc.WINDOWS, ids=tc.WINDOW_IDS)
def test_window_rule_equals_scikit_learn(name, which, s, e):
    T, Tn = tc.sklearn_tfidf(which, s, e)
    n, indptr, indices, data = tfidf.tfidf_window(tc.corpus(which), s, e)
    assert n == T.shape[0]
    assert np.array_equal(indptr, T.indptr) and np.array_equal(indices, T.indices)
    assert np.array_equal(bits(data), bits(T.data))
    w = tc.spec(which, s, e)
    assert w.n_cols == T.shape[1]
    assert np.array_equal(Tn.indptr, T.indptr) and np.array_equal(Tn.indices, T.indices)   # normalize keeps the stored order
    assert np.array_equal(bits(w.data2), bits(Tn.data))
    assert np.array_equal(bits(tfidf.renormalise(indptr, data)), bits(Tn.data))
    # the rows are in first-appearance order, not sorted by column: the order of the sums is part of the rule
    if name in ("mixed_0_200", "sparse_all"):
        assert any(np.any(np.diff(indices[indptr[i]:indptr[i + 1]]) < 0) for i in range(n))


@pytest.mark.parametrize("name,which,s,e", tc.WINDOWS, ids=tc.WINDOW_IDS)
def test_window_postings(name, which, s, e):
    """The posting lists over the GLOBAL term ids hold every entry once, documents ascending, with the twice-normalised
    values; absent terms have empty lists."""
    c, w = tc.corpus(which), tc.spec(which, s, e)
    assert len(w.postptr) == c.V + 1 and w.postptr[0] == 0 and w.postptr[-1] == len(w.term)
    assert np.count_nonzero(np.diff(w.postptr)) == w.n_cols
    doc = np.repeat(np.arange(w.n), np.diff(w.indptr))
    got = set()
    for t in np.flatnonzero(np.diff(w.postptr)):
        rows = w.postrow[w.postptr[t]:w.postptr[t + 1]]
        assert np.all(np.diff(rows) > 0)
        got.update((int(r), int(t), int(v)) for r, v in zip(rows, bits(w.postval[w.postptr[t]:w.postptr[t + 1]])))
    assert got == {(int(r), int(t), int(v)) for r, t, v in zip(doc, w.term, bits(w.data2))}
    # column ids are the ranks of the global ids among the present terms
    present = np.flatnonzero(np.diff(w.postptr))
    assert np.array_equal(present[w.indices], w.term)


def test_long_and_duplicated_rows_are_in_the_cases():
    c = tc.corpus("mixed")
    lens = np.diff(c.rowptr)
    assert lens[tc.LONG_ROW] == 300 and lens[tc.LONG_COPY] == 300 and c.max_row_terms == 300
    assert c.cnt[c.rowptr[tc.LONG_ROW]:c.rowptr[tc.LONG_ROW + 1]].max() == 3   # the repeated word
    assert lens[tc.TOKENLESS_ROW] == 0 and c.vrank[tc.TOKENLESS_ROW + 1] - c.vrank[tc.TOKENLESS_ROW] == 1
    assert lens[tc.HALF_BLANK_ROW] == 0 and c.vrank[tc.HALF_BLANK_ROW + 2] - c.vrank[tc.HALF_BLANK_ROW] == 1


@pytest.mark.parametrize("which", ["mixed", "sparse"])
def test_corpus_invariants(which):
    c, rec = tc.corpus(which), tc.records(which)
    N, V = len(rec), c.V
    for a in (c.rowptr, c.term, c.cnt, c.pos, c.vrank, c.vrow, c.gpostptr, c.gpostrow, c.gpostent):
        assert a.dtype == np.int32 and a.flags.c_contiguous
    assert not c.host_only and c.N == N and len(c) == N and c.nnz == len(c.term) == c.rowptr[-1]
    assert c.vocabulary == sorted(c.vocabulary) and len(set(c.vocabulary)) == V
    valid = np.any(rec != "", axis=1)
    assert np.array_equal(c.vrank, np.concatenate([[0], np.cumsum(valid)]))
    assert np.array_equal(c.vrow, np.flatnonzero(valid))
    assert np.array_equal(c.vrank[c.vrow], np.arange(len(c.vrow)))             # vrow maps a valid rank back to its row
    lens = np.diff(c.rowptr)
    assert np.all(lens[~valid] == 0) and np.all(c.cnt >= 1)
    rows = np.repeat(np.arange(N), lens)
    for i in np.flatnonzero(lens)[:: max(1, N // 60)]:
        t, p = c.term[c.rowptr[i]:c.rowptr[i + 1]], c.pos[c.rowptr[i]:c.rowptr[i + 1]]
        assert np.all(np.diff(t) > 0) and sorted(p) == list(range(len(p)))     # terms ascending; pos a permutation
    # term-major postings: ascending rows, and gpostent leads back to the entry of that (row, term)
    assert c.gpostptr[0] == 0 and c.gpostptr[-1] == c.nnz and len(c.gpostptr) == V + 1
    assert np.array_equal(np.sort(c.gpostent), np.arange(c.nnz))
    assert np.array_equal(c.term[c.gpostent], np.repeat(np.arange(V), np.diff(c.gpostptr)))
    assert np.array_equal(rows[c.gpostent], c.gpostrow)
    inner = np.ones(c.nnz, dtype=bool)
    inner[c.gpostptr[:-1][np.diff(c.gpostptr) > 0]] = False
    assert np.all(np.diff(c.gpostrow)[inner[1:]] > 0)
    # the tokens are scikit-learn's: counts of one document against its analyser
    from sklearn.feature_extraction.text import TfidfVectorizer

    i = int(np.flatnonzero(lens)[3])
    toks = TfidfVectorizer().build_analyzer()(tc.window_strings(which, i, i + 1)[0])
    sl = slice(c.rowptr[i], c.rowptr[i + 1])
    assert {c.vocabulary[t]: n for t, n in zip(c.term[sl], c.cnt[sl])} == {t: toks.count(t) for t in set(toks)}
    first = {}
    for tok in toks:
        first.setdefault(tok, len(first))
    assert [first[c.vocabulary[t]] for t in c.term[sl]] == list(c.pos[sl])


def test_windows_are_views():
    c = tc.corpus("mixed")
    w = c.window(100, 300)
    assert (w.corpus, w.lo, w.hi, len(w), w.shape) == (c, 100, 300, 200, (200, 2))
    assert np.array_equal(w.records, tc.records("mixed")[100:300])
    v = c[100:300][20:50]
    assert (v.lo, v.hi) == (120, 150)
    with pytest.raises(IndexError):
        c.window(10, 601)


def test_all_blank_window_is_empty():
    c = text.tokenise(np.array([["", ""]] * 4 + [["some words", "here"]]))
    w = tfidf.window_tfidf(c, 0, 4)
    assert w.n == 0 and w.n_cols == 0 and list(w.indptr) == [0] and len(w.data) == 0 and not w.postptr.any()
    assert tfidf.tfidf_window(c, 2, 2)[0] == 0
    blank = text.tokenise(np.array([["", ""]] * 3))
    assert blank.V == 0 and blank.nnz == 0 and tfidf.window_tfidf(blank, 0, 3).n == 0


def test_empty_vocabulary_raises_what_scikit_learn_raises():
    from sklearn.feature_extraction.text import TfidfVectorizer

    rec = np.array([["a", ""], ["", "b c"], ["", ""], ["real words", ""]])
    with pytest.raises(ValueError) as ref:
        TfidfVectorizer().fit_transform(["a  ", "  b c"])
    c = text.tokenise(rec)
    with pytest.raises(ValueError) as got:
        tfidf.window_tfidf(c, 0, 3)
    assert str(got.value) == str(ref.value) == tfidf.EMPTY_VOCABULARY
    assert tfidf.window_tfidf(c, 0, 4).n == 3   # one document with tokens is enough
    mc = tc.corpus("mixed")
    with pytest.raises(ValueError, match="empty vocabulary"):
        tfidf.window_tfidf(mc, tc.HALF_BLANK_ROW, tc.HALF_BLANK_ROW + 2)


def test_host_only_at_the_row_length_cap():
    assert text.TFIDF_MAX_ROW_TERMS >= 1024
    row = lambda k: [" ".join(f"tok{i:04d}" for i in range(k)), "tok0000 again"]
    at = text.tokenise(np.array([row(text.TFIDF_MAX_ROW_TERMS - 1), ["short one", ""]]))
    assert at.max_row_terms == text.TFIDF_MAX_ROW_TERMS and not at.host_only
    over = text.tokenise(np.array([row(text.TFIDF_MAX_ROW_TERMS), ["short one", ""]]))
    assert over.max_row_terms == text.TFIDF_MAX_ROW_TERMS + 1 and over.host_only
    with pytest.raises(ValueError):
        over.device_arrays("cpu")
    # the decision is made when the corpus is tokenised, from the cap it is given
    assert text.tokenise(tc.records("mixed"), max_row_terms=299).host_only
    assert not text.tokenise(tc.records("mixed"), max_row_terms=300).host_only


def test_idf_table_is_the_transformers():
    from sklearn.feature_extraction.text import TfidfTransformer
    import scipy.sparse as sp

    n = 37
    X = sp.csr_matrix(np.tril(np.ones((n, n))))   # column j is in n - j documents
    idf = TfidfTransformer().fit(X).idf_
    assert np.array_equal(bits(tfidf.idf_table(n)[n - np.arange(n)]), bits(idf))
    assert tfidf.idf_table(n) is tfidf.idf_table(n)
