"""scikit-learn's default analyser on ASCII text as a rule on bytes, and the corpus arrays it leads to.  NumPy only.

PARITY PINNED: scikit-learn is installed, so tests/test_tokens_host.py compares `analyse` with
`TfidfVectorizer().build_analyzer()` on random ASCII strings over all 128 byte values, and `corpus_arrays` with
`mused_amd.text.tokenise` array for array.  scikit-learn stays the authority -- MUSED_TOKENISE=host keeps calling it;
this module is the statement of the rule the device kernels (csrc/tokenise.hip) follow step by step.  Text that is
not pure ASCII follows the same rule on code points: the second half of this module, pinned by
tests/test_tokens_unicode_host.py.

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


# ---- code points: the same analyser on text that is not pure ASCII --------------------------------------------------------
#
# What changes against the byte rule (all of it derived from the running interpreter, so that it matches the analyser
# of the same process; tests/test_tokens_unicode_host.py pins every statement):
#
#     preprocess   str.lower() maps one code point to one code point, but for the EXPANDING code points (CPython: U+0130
#                  alone, 'İ' -> 'i' + U+0307) and for U+03A3, which becomes 'ς' or 'σ' by the final-sigma rule.  An
#                  expanding code point is kept as ONE element: it lower-cases to the first code point of its expansion
#                  and, the rest of the expansion being no word code points, the run ends behind it ("aİb" -> ["ai"]).
#                  The final-sigma rule is not restated: `resolve_sigma` replaces every U+03A3 of the buffer by what the
#                  row's own str.lower() has in its place; lower-casing is idempotent on 'σ' and 'ς'.
#     tokenize     \w on str is chr(cp).isalnum() or '_'; lower-casing never changes the class of a code point.  The
#                  tokens are the maximal runs of word code points of length >= 2 in code points, a run also ending
#                  behind an expanding code point; a token is the sequence of its lowered code points.
#     vocabulary   Python's str order is code-point order.
#
# The corpus is one uint32 buffer of code points, laid out as the byte buffer is; `class_table()` holds one uint32 per
# code point: the lowered code point in the low 21 bits, CP_WORD, CP_END.

N_CODEPOINTS = 0x110000
CP_MASK = (1 << 21) - 1
CP_WORD = 1 << 21
CP_END = 1 << 22      # a word code point behind which the run ends
SIGMA = 0x3A3

_TABLE = None


def _build_table():
    """(table, expanding, unsupported): `expanding` maps a code point to its str.lower() of more than one code point;
    `unsupported` lists those of them the two flags cannot express (none in CPython 3.10)."""
    import re

    word = re.compile(r"\w")
    table = np.arange(N_CODEPOINTS, dtype=np.uint32)
    expanding = {}
    step = 256
    for lo in range(0, N_CODEPOINTS, step):
        chars = [chr(cp) for cp in range(lo, lo + step)]
        block = "".join(chars)
        # a block str.lower() leaves alone holds no cased code point: each of its code points lowers to itself
        if block.lower() != block:
            for cp, ch in zip(range(lo, lo + step), chars):
                low = ch.lower()
                table[cp] = ord(low[0])
                if len(low) != 1:
                    expanding[cp] = low
        if word.search(block):
            is_word = np.fromiter((ch.isalnum() for ch in chars), dtype=bool, count=step)
            table[lo:lo + step][is_word] |= CP_WORD
    table[ord("_")] |= CP_WORD
    unsupported = []
    for cp, low in expanding.items():
        rest_is_no_word = not any(table[ord(c)] & CP_WORD for c in low[1:])
        if table[cp] & CP_WORD and table[ord(low[0])] & CP_WORD and rest_is_no_word:
            table[cp] |= CP_END
        elif table[cp] & CP_WORD or any(table[ord(c)] & CP_WORD for c in low):
            unsupported.append(cp)
    return table, expanding, np.array(sorted(unsupported), dtype=np.uint32)


def _tables():
    global _TABLE
    if _TABLE is None:
        _TABLE = _build_table()
    return _TABLE


def class_table():
    """uint32[N_CODEPOINTS], built once per process from chr(cp).lower() and chr(cp).isalnum()."""
    return _tables()[0]


def expanding_codepoints():
    """code point -> its str.lower(), for the code points that lower-case to more than one."""
    return _tables()[1]


def unsupported_codepoints():
    """Sorted uint32 array of the expanding code points the table cannot express: a corpus holding one is the host's."""
    return _tables()[2]


def resolve_sigma(buf, docptr):
    """Replaces, in place, every U+03A3 of the corpus buffer by the code point the str.lower() of its document has in
    its place.  A document is lower-cased as a whole (the final-sigma rule looks at the neighbours) and only if it holds
    U+03A3; element p of a document stands at place p + (the places the expanding code points in front of it add) of the
    lowered string."""
    at = np.flatnonzero(buf == SIGMA)
    if not len(at):
        return
    docptr = np.asarray(docptr, dtype=np.int64)
    added = np.zeros(len(buf) + 1, dtype=np.int64)     # added[p]: places gained in front of element p
    for cp, low in expanding_codepoints().items():
        added[1:][buf == cp] = len(low) - 1
    np.cumsum(added, out=added)
    doc = np.searchsorted(docptr, at, side="right") - 1
    bounds = np.append(np.flatnonzero(np.concatenate([[True], doc[1:] != doc[:-1]])), len(at)).tolist()
    for a, b in zip(bounds[:-1], bounds[1:]):
        start, end = int(docptr[doc[a]]), int(docptr[doc[a] + 1]) - 1     # without the separator
        low = buf[start:end].astype("<u4").tobytes().decode("utf-32-le", "surrogatepass").lower()
        low = np.frombuffer(low.encode("utf-32-le", "surrogatepass"), dtype="<u4")
        assert len(low) == end - start + added[end] - added[start], "str.lower() expanded a code point the table does not know"
        p = at[a:b]
        buf[p] = low[p - start + added[p] - added[start]]


def codepoint_token_spans(buf):
    """(start, length) of every token of the code-point buffer (U+03A3 resolved), in text order."""
    e = class_table()[np.asarray(buf, dtype=np.uint32)]
    w = np.concatenate([[False], (e & CP_WORD) != 0, [False]])
    goes_on = np.concatenate([[False], (e & (CP_WORD | CP_END)) == CP_WORD, [False]])   # a word element the run continues behind
    # a run starts at a word element behind one the run does not continue from, and ends at a word element that ends the
    # run or stands in front of an element that is no word element
    start = np.flatnonzero(w[1:-1] & ~goes_on[:-2])
    end = np.flatnonzero(w[1:-1] & ~(goes_on[1:-1] & w[2:])) + 1
    keep = end - start >= 2
    return start[keep], (end - start)[keep]


def lowered_text(buf):
    """The lowered code points of the buffer as one str (lone surrogates, which are in no token, as U+FFFD)."""
    low = (class_table()[np.asarray(buf, dtype=np.uint32)] & CP_MASK).astype("<u4")
    low[(low >= 0xD800) & (low < 0xE000)] = 0xFFFD
    return low.tobytes().decode("utf-32-le")


def analyse_codepoints(doc: str):
    """`TfidfVectorizer().build_analyzer()(doc)` for any str."""
    buf = np.array([ord(c) for c in doc] + [SEPARATOR], dtype=np.uint32)
    resolve_sigma(buf, [0, len(buf)])
    low = lowered_text(buf)
    return [low[s:s + n] for s, n in zip(*(a.tolist() for a in codepoint_token_spans(buf)))]


def codepoint_corpus_arrays(buf, docptr):
    """`corpus_arrays` for a code-point buffer (U+03A3 resolved, as text.corpus_codepoints leaves it)."""
    buf = np.asarray(buf, dtype=np.uint32)
    docptr = np.asarray(docptr, dtype=np.int64)
    D = len(docptr) - 1
    start, length = codepoint_token_spans(buf)
    low = lowered_text(buf)
    tokens = [low[s:s + n] for s, n in zip(start.tolist(), length.tolist())]
    voc = sorted(set(tokens))                       # Python's str order, as `_sort_features`
    rank = {t: i for i, t in enumerate(voc)}
    ident = np.array([rank[t] for t in tokens], dtype=np.int64)
    V = len(voc)
    doc = np.searchsorted(docptr, start, side="right") - 1
    pair, first, cnt = np.unique(doc * max(V, 1) + ident, return_index=True, return_counts=True)
    rows, term = pair // max(V, 1), pair % max(V, 1)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=D))]).astype(np.int64)
    by_first = np.argsort(first)
    pos = np.empty(len(pair), dtype=np.int64)
    pos[by_first] = np.arange(len(pair)) - rowptr[rows[by_first]]
    return voc, rowptr, term.astype(np.int64), cnt.astype(np.int64), pos
