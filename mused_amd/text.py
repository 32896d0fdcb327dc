"""One tokenised pass over the ('title', 'description') records of a "text" modality (matrix_operations.py:91-110).

`tokenise(records)` runs scikit-learn's own analyser (`TfidfVectorizer().build_analyzer()`) once over every valid row
and keeps what any window's TF-IDF needs as int32 arrays (`TextCorpus`): the per-window arithmetic -- document
frequencies, idf weights, the stored order of a row's entries, both normalisations, the posting lists -- then runs on
the device from those arrays (csrc/tfidf.hip; the rule itself: mused_amd/tfidf.py), and with step_window_ratio = r a row
is no longer tokenised r times.

Valid rows and their string follow the reference (matrix_operations.py:97,102): a row is valid if either field is
non-empty, its string is where(title != "", title, " ") + " " + where(description != "", description, " ").  Global
term ids are the rank of the token in sorted(vocabulary) (Python str order, the order of scikit-learn's
`_sort_features`).
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np

# the most distinct terms of one document the rows kernel ranks in LDS (csrc/tfidf.hip: TFIDF_MAX_ROW_TERMS)
TFIDF_MAX_ROW_TERMS = 1024
_INT32_END = 2 ** 31

_DEVICE_FIELDS = ("rowptr", "term", "cnt", "pos", "vrank", "vrow", "gpostptr", "gpostrow", "gpostent")


class TextCorpus:
    """Host arrays of a tokenised corpus of N rows, V terms, nnz (row, term) entries; all int32.

        rowptr[N + 1], term[nnz], cnt[nnz]   CSR over ALL rows (invalid rows are empty), terms ascending inside a row
        pos[nnz]                             ordinal of the term's first occurrence within its document (0, 1, ...)
        vrank[N + 1], vrow[n_valid]          prefix count of valid rows; valid rank -> row
        gpostptr[V + 1], gpostrow[nnz]       term-major postings: the rows that contain a term, ascending
        gpostent[nnz]                        the CSR entry a posting refers to

    `vocabulary` is the sorted token list, `records` the (N, 2) strings themselves (the host path reads them),
    `max_row_terms` the longest row.  `host_only`: the corpus is beyond what the device arrays hold (nnz >= 2^31, or a
    document with more than TFIDF_MAX_ROW_TERMS distinct terms) and every window of it takes the host path."""

    def __init__(self, records, vocabulary, rowptr, term, cnt, pos, valid, max_row_terms_cap=TFIDF_MAX_ROW_TERMS):
        self.records = records
        self.vocabulary = vocabulary
        self.N, self.V = len(records), len(vocabulary)
        nnz = int(rowptr[-1])
        self.nnz = nnz
        self.max_row_terms = int(np.diff(rowptr).max()) if self.N else 0
        self.host_only = nnz >= _INT32_END or self.max_row_terms > max_row_terms_cap
        self._dev = {}
        if nnz >= _INT32_END:   # int32 arrays cannot hold it; only the records are kept
            self.rowptr = self.term = self.cnt = self.pos = self.gpostptr = self.gpostrow = self.gpostent = None
        else:
            self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
            self.term = np.ascontiguousarray(term, dtype=np.int32)
            self.cnt = np.ascontiguousarray(cnt, dtype=np.int32)
            self.pos = np.ascontiguousarray(pos, dtype=np.int32)
            order = np.argsort(self.term, kind="stable")   # entries are row-major: rows ascend inside a term
            rows = np.repeat(np.arange(self.N, dtype=np.int32), np.diff(self.rowptr))
            self.gpostptr = np.concatenate([[0], np.cumsum(np.bincount(self.term, minlength=self.V))]).astype(np.int32)
            self.gpostrow = np.ascontiguousarray(rows[order], dtype=np.int32)
            self.gpostent = np.ascontiguousarray(order, dtype=np.int32)
        valid = np.asarray(valid, dtype=bool)
        self.vrank = np.concatenate([[0], np.cumsum(valid)]).astype(np.int32)
        self.vrow = np.flatnonzero(valid).astype(np.int32)

    def __len__(self):
        return self.N

    @property
    def shape(self):
        return (self.N, 2)

    def window(self, lo=0, hi=None) -> "TextWindow":
        """Rows [lo, hi) of the corpus: a view, nothing is copied."""
        hi = self.N if hi is None else hi
        if not 0 <= lo <= hi <= self.N:
            raise IndexError(f"window [{lo}, {hi}) outside a corpus of {self.N} rows")
        return TextWindow(self, int(lo), int(hi))

    def __getitem__(self, rows):
        if not isinstance(rows, slice) or rows.step not in (None, 1):
            raise TypeError("a TextCorpus is sliced by contiguous row ranges")
        lo, hi, _ = rows.indices(self.N)
        return self.window(lo, max(lo, hi))

    def device_arrays(self, device):
        """The int32 arrays as device tensors, uploaded once per corpus and device."""
        import torch

        dev = self._dev.get(str(device))
        if dev is None:
            if self.host_only:
                raise ValueError("a host-only corpus has no device arrays")
            dev = {}
            for name in _DEVICE_FIELDS:
                a = getattr(self, name)
                dev[name] = torch.from_numpy(a if len(a) else np.zeros(1, np.int32)).to(device)
            torch.cuda.current_stream().synchronize()   # resident before any other stream reads them
            self._dev[str(device)] = dev
        return dev


class TextWindow:
    """Rows [lo, hi) of a TextCorpus, what `adjacency_on_device(x, "text", ...)` takes in place of the strings."""

    def __init__(self, corpus: TextCorpus, lo: int, hi: int):
        self.corpus, self.lo, self.hi = corpus, lo, hi

    def __len__(self):
        return self.hi - self.lo

    @property
    def shape(self):
        return (self.hi - self.lo, 2)

    @property
    def records(self):
        return self.corpus.records[self.lo:self.hi]

    def __getitem__(self, rows):
        if not isinstance(rows, slice) or rows.step not in (None, 1):
            raise TypeError("a TextWindow is sliced by contiguous row ranges")
        lo, hi, _ = rows.indices(len(self))
        return TextWindow(self.corpus, self.lo + lo, self.lo + max(lo, hi))


def tokenise(records, max_row_terms=TFIDF_MAX_ROW_TERMS) -> TextCorpus:
    """(N, 2) title / description strings -> TextCorpus.  `max_row_terms`: the row length beyond which the corpus is
    marked host-only (the kernel's cap; smaller values are for tests)."""
    from sklearn.feature_extraction.text import TfidfVectorizer

    records = np.asarray(records)
    if records.ndim != 2 or records.shape[1] != 2:
        raise ValueError(f"text records must be (N, 2) title / description strings, got {records.shape}")
    N = len(records)
    valid = np.any(records != "", axis=1) if N else np.zeros(0, dtype=bool)
    vd = records[valid]
    strings = (np.where(vd[:, 0] != "", vd[:, 0], " ") + " " + np.where(vd[:, 1] != "", vd[:, 1], " ")).tolist()
    analyse = TfidfVectorizer().build_analyzer()
    seen = defaultdict()   # token -> provisional id, in order of first appearance
    seen.default_factory = seen.__len__
    flat, per_doc = [], []
    for doc in strings:
        ids = [seen[tok] for tok in analyse(doc)]
        flat.extend(ids)
        per_doc.append(len(ids))
    vocabulary = sorted(seen)
    V = len(vocabulary)
    rank = np.empty(V, dtype=np.int64)
    rank[[seen[tok] for tok in vocabulary]] = np.arange(V)
    tokens = np.zeros(N, dtype=np.int64)   # tokens per row, repeats included
    tokens[valid] = per_doc
    # one entry per distinct (row, term): np.unique sorts by row, then term, and reports the first token and the count
    row_of = np.repeat(np.arange(N), tokens)
    pair, first, cnt = np.unique(row_of * max(V, 1) + rank[np.asarray(flat, dtype=np.int64)] if flat else
                                 np.zeros(0, dtype=np.int64), return_index=True, return_counts=True)
    rows, term = pair // max(V, 1), pair % max(V, 1)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))])
    # ordinal of the first occurrence among the row's distinct terms: token positions ascend with the rows
    by_first = np.argsort(first)
    pos = np.empty(len(pair), dtype=np.int64)
    pos[by_first] = np.arange(len(pair)) - rowptr[rows[by_first]]
    return TextCorpus(records, vocabulary, rowptr, term, cnt, pos, valid, max_row_terms)
