"""scikit-learn's default analyser on ASCII text as a rule on bytes, and the corpus arrays it leads to.  NumPy only.

PARITY PINNED: scikit-learn is installed, so tests/test_tokens_host.py compares `analyse` with
`TfidfVectorizer().build_analyzer()` on random ASCII strings over all 128 byte values, and `corpus_arrays` with
`mused_amd.text.tokenise` array for array.  scikit-learn stays the authority -- MUSED_TOKENISE=host and every corpus
that is not pure ASCII keep calling it; this module is the statement of the rule the device kernels
(csrc/tokenise.hip) follow step by step.

What `TfidfVectorizer()` does to a document (sklearn/feature_extraction/text.py, `build_analyzer` with the defaults):

    decode           the input is a str already: nothing
    preprocess       lowercase=True -> doc.lower(); strip_accents=None: nothing
                     on ASCII, str.lower() maps 'A'..'Z' to 'a'..'z' and leaves every other character alone
    tokenize         re.compile(r"(?u)\\b\\w\\w+\\b").findall(doc)
                     on ASCII, \\w is [0-9A-Za-z_]; the pattern is greedy and \\b needs a non-word neighbour on both
                     sides, so the matches are exactly the MAXIMAL runs of word bytes of length >= 2 (a one-byte
                     run is no token; NUL, control bytes, tab and newline are as good a separator as a blank)
    stop words       stop_words=None: nothing
    n-grams          ngram_range=(1, 1): the tokens themselves

The vocabulary is sorted(tokens) in Python's str order (`_sort_features`), which on ASCII is byte order.

The corpus is one byte buffer: the strings of the valid rows, each followed by one separator byte that is no word byte
(`SEPARATOR`), and docptr[D + 1] from the string LENGTHS (a string may hold the separator byte itself): document d is
buf[docptr[d] : docptr[d + 1]], its last byte the separator, so no run crosses a document.
"""
from __future__ import annotations

import numpy as np

SEPARATOR = 0x0A

_BYTES = np.arange(256, dtype=np.uint8)
# \w on ASCII
IS_WORD = (((_BYTES >= ord("0")) & (_BYTES <= ord("9"))) | ((_BYTES >= ord("A")) & (_BYTES <= ord("Z")))
           | ((_BYTES >= ord("a")) & (_BYTES <= ord("z"))) | (_BYTES == ord("_")))
# str.lower() on ASCII
LOWER = np.where((_BYTES >= ord("A")) & (_BYTES <= ord("Z")), _BYTES + 32, _BYTES).astype(np.uint8)


def token_spans(buf):
    """(start, length) of every token of the byte buffer, in text order: the maximal runs of word bytes, length >= 2."""
    buf = np.asarray(buf, dtype=np.uint8)
    w = np.concatenate([[False], IS_WORD[buf], [False]])
    start = np.flatnonzero(w[1:-1] & ~w[:-2])     # a word byte behind a non-word byte (or at byte 0)
    end = np.flatnonzero(w[1:-1] & ~w[2:]) + 1    # one past a word byte in front of a non-word byte (or the end)
    keep = end - start >= 2
    return start[keep], (end - start)[keep]


def analyse(doc: str):
    """`TfidfVectorizer().build_analyzer()(doc)` for an ASCII string."""
    buf = np.frombuffer(doc.encode("ascii"), dtype=np.uint8)
    low = LOWER[buf].tobytes()
    return [low[s:s + n].decode("ascii") for s, n in zip(*token_spans(buf))]


def corpus_arrays(buf, docptr):
    """The buffer of D documents -> (vocabulary, rowptr[D + 1], term, cnt, pos): the CSR of mused_amd.text.TextCorpus
    over the DOCUMENTS (the valid rows), int64.

    term: rank of the token in the sorted vocabulary, ascending inside a document; cnt: its occurrences there;
    pos: the ordinal of the term's first occurrence among the document's distinct terms (0, 1, ...)."""
    buf = np.asarray(buf, dtype=np.uint8)
    docptr = np.asarray(docptr, dtype=np.int64)
    D = len(docptr) - 1
    start, length = token_spans(buf)
    low = LOWER[buf].tobytes()
    tokens = np.array([low[s:s + n] for s, n in zip(start, length)], dtype=bytes)   # no token holds a NUL
    voc, ident = np.unique(tokens, return_inverse=True) if len(tokens) else (np.zeros(0, dtype=bytes), np.zeros(0, np.int64))
    V = len(voc)
    doc = np.searchsorted(docptr, start, side="right") - 1
    # one entry per distinct (document, term): sorted by document, then term; the first token of each and its count
    pair, first, cnt = np.unique(doc * max(V, 1) + ident.reshape(-1), return_index=True, return_counts=True)
    rows, term = pair // max(V, 1), pair % max(V, 1)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=D))]).astype(np.int64)
    by_first = np.argsort(first)   # token positions ascend with the documents
    pos = np.empty(len(pair), dtype=np.int64)
    pos[by_first] = np.arange(len(pair)) - rowptr[rows[by_first]]
    return [t.decode("ascii") for t in voc.tolist()], rowptr, term.astype(np.int64), cnt.astype(np.int64), pos
