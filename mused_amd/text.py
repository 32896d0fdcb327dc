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

import os
from collections import defaultdict

import numpy as np

# the most distinct terms of one document the rows kernel ranks in LDS (csrc/tfidf.hip: TFIDF_MAX_ROW_TERMS)
TFIDF_MAX_ROW_TERMS = 1024
# the most tokens of one document, repeats included, `tokenise_on_device` sorts in LDS (csrc/tokenise.hip:
# TK_MAX_DOC_TOKENS; 16 bytes a token: 128 KiB of the 160 KiB at the cap).  A corpus with a longer document is
# tokenised on the host.
TOKENISE_MAX_DOC_TOKENS = 8192
_INT32_END = 2 ** 31
_MAX_DEVICE_TERMS = 2 ** 24      # the posting sort of csrc/tokenise.hip runs three 8-bit passes at the most
_TK_FLAG_DOC, _TK_FLAG_TABLE, _TK_FLAG_STATE = 1, 2, 4

# corpora `tokenise_on_device` handed to the host `tokenise`: not pure ASCII, 2^31 bytes or more, a document beyond
# max_doc_tokens, 2^24 distinct terms or more; and those `tokenise_codepoints_on_device` handed over (its docstring)
tokenise_fallbacks = 0

_LAZY_FIELDS = ("term", "cnt", "pos", "gpostptr", "gpostrow", "gpostent")

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
    document with more than TFIDF_MAX_ROW_TERMS distinct terms) and every window of it takes the host path.

    A corpus built by `tokenise_on_device` keeps term, cnt, pos, gpostptr, gpostrow and gpostent as device tensors:
    `device_arrays` of that device returns them as they are, and the host attributes of the same names are fetched on
    first access.  rowptr, vrank and vrow are host arrays from the start."""

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

    @classmethod
    def _from_device(cls, records, vocabulary, rowptr, valid, tensors, device, max_row_terms_cap):
        """The corpus `tokenise_on_device` built: `tensors` holds the six large arrays on `device`."""
        import torch

        self = cls.__new__(cls)
        self.records, self.vocabulary = records, vocabulary
        self.N, self.V = len(records), len(vocabulary)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.nnz = int(self.rowptr[-1])
        self.max_row_terms = int(np.diff(self.rowptr).max())
        self.host_only = self.max_row_terms > max_row_terms_cap
        valid = np.asarray(valid, dtype=bool)
        self.vrank = np.concatenate([[0], np.cumsum(valid)]).astype(np.int32)
        self.vrow = np.flatnonzero(valid).astype(np.int32)
        self._lazy = dict(tensors)
        dev = {name: torch.from_numpy(getattr(self, name)).to(device) for name in ("rowptr", "vrank", "vrow")}
        dev.update(tensors)
        torch.cuda.current_stream().synchronize()
        self._dev = {_device_key(device): dev}
        return self

    def __getattr__(self, name):
        # only reached when the attribute is not set: a large array of a device-built corpus, on its first host access
        lazy = self.__dict__.get("_lazy")
        if lazy is not None and name in _LAZY_FIELDS:
            a = np.ascontiguousarray(lazy[name].cpu().numpy())
            setattr(self, name, a)
            return a
        raise AttributeError(name)

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

        if self.host_only:
            raise ValueError("a host-only corpus has no device arrays")
        dev = self._dev.get(_device_key(device))
        if dev is None:
            dev = {}
            for name in _DEVICE_FIELDS:
                a = getattr(self, name)
                dev[name] = torch.from_numpy(a if len(a) else np.zeros(1, np.int32)).to(device)
            torch.cuda.current_stream().synchronize()   # resident before any other stream reads them
            self._dev[_device_key(device)] = dev
        return dev


def _device_key(device) -> str:
    """"cuda" and "cuda:<current device>" name the same arrays."""
    import torch

    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return str(d)


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


def _valid_rows(records):
    records = np.asarray(records)
    if records.ndim != 2 or records.shape[1] != 2:
        raise ValueError(f"text records must be (N, 2) title / description strings, got {records.shape}")
    valid = np.any(records != "", axis=1) if len(records) else np.zeros(0, dtype=bool)
    return records, valid


def corpus_buffer(records, valid):
    """The strings of the valid rows (matrix_operations.py:97,102: where(title != "", title, " ") + " " + where(description
    != "", description, " ")) as one byte buffer, every string followed by tokens.SEPARATOR, and docptr[D + 1] from the
    string lengths: (buf uint8, docptr int32).  None if a character is not ASCII or the buffer would hold 2^31 bytes
    or more.  Works on the code points of the fixed-width string array as a whole: no Python per row."""
    from . import tokens

    vd = records[valid]
    if vd.dtype.kind != "U":
        vd = vd.astype(str)
    D, k = len(vd), vd.dtype.itemsize // 4
    cp = np.ascontiguousarray(vd).view(np.uint32).reshape(D, 2, k)
    if vd.dtype.byteorder == ">" or int(cp.max()) > 127:
        return None
    # NumPy pads with NULs behind the string (and cannot keep a NUL at a string's end): the length ends at the last other one
    length = np.char.str_len(vd).astype(np.int32)
    blank = length == 0
    length = np.where(blank, 1, length)
    doclen = length.sum(axis=1, dtype=np.int64) + 2
    if int(doclen.sum()) >= _INT32_END:
        return None
    grid = np.empty((D, 2 * k + 2), dtype=np.uint8)
    grid[:, :k], grid[:, k + 1:2 * k + 1] = cp[:, 0], cp[:, 1]
    grid[:, k], grid[:, 2 * k + 1] = ord(" "), tokens.SEPARATOR
    grid[blank[:, 0], 0] = ord(" ")
    grid[blank[:, 1], k + 1] = ord(" ")
    keep = np.ones((D, 2 * k + 2), dtype=bool)
    col = np.arange(k, dtype=np.int32)
    keep[:, :k] = col < length[:, :1]
    keep[:, k + 1:2 * k + 1] = col < length[:, 1:]
    docptr = np.concatenate([[0], np.cumsum(doclen)]).astype(np.int32)
    return grid[keep], docptr


# the most code points of a corpus `tokenise_codepoints_on_device` takes (csrc/tokenise.hip: tk_cp_sizes_ok): below it
# every element offset and token count is an int32 and the workspace arithmetic stays far inside an int64
_MAX_CODEPOINTS = 2 ** 30


def corpus_codepoints(records, valid):
    """`corpus_buffer` for any text: the strings of the valid rows as one buffer of code points, every string followed by
    tokens.SEPARATOR, every U+03A3 replaced by what the row's str.lower() has in its place (tokens.resolve_sigma), and
    docptr[D + 1] in ELEMENTS from the string lengths: (buf uint32, docptr int32).

    None -- the corpus is the host's -- if the buffer would hold _MAX_CODEPOINTS = 2^30 elements or more (element offsets are
    int32, and the workspace of 2^30 code points is some 24 GiB), if an element is no code point (above U+10FFFF: not from
    a str) or is one of tokens.unsupported_codepoints().  The fixed-width string array is UCS-4 already, so this works on
    it as a whole: no Python per row but for the rows that hold U+03A3."""
    from . import tokens

    vd = records[valid]
    if vd.dtype.kind != "U":
        vd = vd.astype(str)
    D, k = len(vd), vd.dtype.itemsize // 4
    cp = np.ascontiguousarray(vd).view(np.uint32).reshape(D, 2, k)
    if vd.dtype.byteorder == ">" or int(cp.max()) >= tokens.N_CODEPOINTS:
        return None
    length = np.char.str_len(vd).astype(np.int32)
    blank = length == 0
    length = np.where(blank, 1, length)
    doclen = length.sum(axis=1, dtype=np.int64) + 2
    if int(doclen.sum()) >= _MAX_CODEPOINTS:
        return None
    grid = np.empty((D, 2 * k + 2), dtype=np.uint32)
    grid[:, :k], grid[:, k + 1:2 * k + 1] = cp[:, 0], cp[:, 1]
    grid[:, k], grid[:, 2 * k + 1] = ord(" "), tokens.SEPARATOR
    grid[blank[:, 0], 0] = ord(" ")
    grid[blank[:, 1], k + 1] = ord(" ")
    keep = np.ones((D, 2 * k + 2), dtype=bool)
    col = np.arange(k, dtype=np.int32)
    keep[:, :k] = col < length[:, :1]
    keep[:, k + 1:2 * k + 1] = col < length[:, 1:]
    docptr = np.concatenate([[0], np.cumsum(doclen)]).astype(np.int32)
    buf = grid[keep]
    unsupported = tokens.unsupported_codepoints()
    if len(unsupported) and np.isin(buf, unsupported).any():
        return None
    tokens.resolve_sigma(buf, docptr)
    return buf, docptr


def _fallback(records, max_row_terms):
    global tokenise_fallbacks
    tokenise_fallbacks += 1
    return tokenise(records, max_row_terms)


def tokenise_on_device(records, device=None, max_row_terms=TFIDF_MAX_ROW_TERMS, max_doc_tokens=TOKENISE_MAX_DOC_TOKENS,
                       table_slots=0) -> TextCorpus:
    """`tokenise(records)` with the tokens found, told apart, counted and posted on the device (csrc/tokenise.hip; the
    rule: mused_amd/tokens.py): equal to the host's corpus field for field, the six large arrays left on the device.

    The host joins the strings into one buffer, reads 16 bytes and the V spans of the distinct tokens after the first
    call, sorts those V strings (the vocabulary) and uploads their ranks; the D + 1 row pointers come back after the
    second.  A corpus that is not pure ASCII, holds 2^31 bytes or more, has a document of more than `max_doc_tokens`
    tokens or 2^24 distinct terms or more is tokenised by `tokenise` (counted in `tokenise_fallbacks`).
    `table_slots`: slots of the hash table, 0 = two per possible token (tests: a small table, long probe chains)."""
    import ctypes as C

    import torch

    from . import _lib

    records, valid = _valid_rows(records)
    N, D = len(records), int(valid.sum())
    if not 1 <= int(max_doc_tokens) <= TOKENISE_MAX_DOC_TOKENS:
        raise ValueError(f"max_doc_tokens={max_doc_tokens} outside [1, {TOKENISE_MAX_DOC_TOKENS}]")
    empty = np.zeros(0, dtype=np.int64)
    if D == 0:   # no string at all
        return TextCorpus(records, [], np.zeros(N + 1, dtype=np.int64), empty, empty, empty, valid, max_row_terms)
    joined = corpus_buffer(records, valid)
    if joined is None:
        return _fallback(records, max_row_terms)
    buf, docptr = joined
    B = len(buf)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    L = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=device)
    ws_bytes = int(L.mused_tokenise_ws_bytes(B, D, int(table_slots)))
    if ws_bytes < 0:
        raise ValueError(f"tokenise_on_device: {B} bytes, {D} documents, table_slots={table_slots}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    tok_cap = B // 3 + 1
    buf_d = torch.from_numpy(buf).to(device)
    voc_start, voc_len, info = i32(tok_cap), i32(tok_cap), i32(4)
    _lib.call("mused_tokenise_scan", ptr(buf_d), B, docptr.ctypes.data_as(C.c_void_p), D, int(table_slots),
              int(max_doc_tokens), ptr(voc_start), ptr(voc_len), tok_cap, ptr(info), ptr(ws), ws_bytes, stream())
    T, V, flags, doc_tokens = (int(x) for x in info.cpu().numpy())
    if flags & _TK_FLAG_TABLE:
        raise ValueError(f"tokenise_on_device: {T} tokens do not fit a table of {table_slots} slots")
    if flags & _TK_FLAG_DOC or V >= _MAX_DEVICE_TERMS:
        return _fallback(records, max_row_terms)
    if T == 0:   # documents without a token
        return TextCorpus(records, [], np.zeros(N + 1, dtype=np.int64), empty, empty, empty, valid, max_row_terms)
    # alphabetical ids: V strings sorted on the host (str order on ASCII is byte order), as scikit-learn's _sort_features
    low = buf.tobytes().lower()
    spans = zip(voc_start[:V].cpu().numpy().tolist(), voc_len[:V].cpu().numpy().tolist())
    found = [low[s:s + n] for s, n in spans]
    order = sorted(range(V), key=found.__getitem__)
    rank = np.empty(V, dtype=np.int32)
    rank[order] = np.arange(V, dtype=np.int32)
    vocabulary = [found[i].decode("ascii") for i in order]
    rank_d = torch.from_numpy(rank).to(device)
    vrow_d = torch.from_numpy(np.flatnonzero(valid).astype(np.int32)).to(device)
    doc_rowptr, gpostptr = i32(D + 1), i32(V + 1)
    big = {name: i32(T) for name in ("term", "cnt", "pos", "gpostrow", "gpostent")}
    _lib.call("mused_tokenise_build", B, D, int(table_slots), T, V, doc_tokens, ptr(rank_d), ptr(vrow_d), ptr(doc_rowptr),
              ptr(big["term"]), ptr(big["cnt"]), ptr(big["pos"]), ptr(gpostptr), ptr(big["gpostrow"]), ptr(big["gpostent"]),
              ptr(info), ptr(ws), ws_bytes, stream())
    doc_rowptr_h = doc_rowptr.cpu().numpy()
    flags = int(info.cpu().numpy()[2])
    if flags:
        raise _lib.MusedError(f"mused_tokenise_build: the workspace is not what mused_tokenise_scan left (flags {flags})")
    nnz = int(doc_rowptr_h[D])
    rowptr = doc_rowptr_h[np.concatenate([[0], np.cumsum(valid)])]   # invalid rows are empty
    tensors = {name: t[:nnz] for name, t in big.items()}
    tensors["gpostptr"] = gpostptr
    return TextCorpus._from_device(records, vocabulary, rowptr, valid, tensors, device, max_row_terms)


_CLASS_TABLES = {}   # device -> tokens.class_table() as a tensor, uploaded once per device


def _class_table_on(device):
    import torch

    from . import tokens

    key = _device_key(device)
    if key not in _CLASS_TABLES:
        _CLASS_TABLES[key] = torch.from_numpy(tokens.class_table().view(np.int32)).to(device)
    return _CLASS_TABLES[key]


def tokenise_codepoints_on_device(records, device=None, max_row_terms=TFIDF_MAX_ROW_TERMS,
                                  max_doc_tokens=TOKENISE_MAX_DOC_TOKENS, table_slots=0) -> TextCorpus:
    """`tokenise_on_device` for text of any script: the same steps on code points (the mused_tokenise_cp_* entries of
    csrc/tokenise.hip; the rule: mused_amd/tokens.py, "code points"), equal to `tokenise(records)` field for field, the six
    large arrays left on the device.

    The host joins the strings into one uint32 buffer (`corpus_codepoints`) and hands the device the class table of the
    running interpreter (built once per process, uploaded once per device).  The V distinct tokens come back as spans;
    the host gathers those spans from its own buffer through the same table, decodes them in one call, sorts the V
    strings and uploads their ranks.  A corpus of 2^30 code points or more, with a document of more than
    `max_doc_tokens` tokens, 2^24 distinct terms or more, or a code point the table cannot express is tokenised by
    `tokenise` (counted in `tokenise_fallbacks`)."""
    import ctypes as C

    import torch

    from . import _lib, tokens

    records, valid = _valid_rows(records)
    N, D = len(records), int(valid.sum())
    if not 1 <= int(max_doc_tokens) <= TOKENISE_MAX_DOC_TOKENS:
        raise ValueError(f"max_doc_tokens={max_doc_tokens} outside [1, {TOKENISE_MAX_DOC_TOKENS}]")
    empty = np.zeros(0, dtype=np.int64)
    if D == 0:   # no string at all
        return TextCorpus(records, [], np.zeros(N + 1, dtype=np.int64), empty, empty, empty, valid, max_row_terms)
    joined = corpus_codepoints(records, valid)
    if joined is None:
        return _fallback(records, max_row_terms)
    buf, docptr = joined
    B = len(buf)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    L = _lib.lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=device)
    ws_bytes = int(L.mused_tokenise_cp_ws_bytes(B, D, int(table_slots)))
    if ws_bytes < 0:
        raise ValueError(f"tokenise_codepoints_on_device: {B} code points, {D} documents, table_slots={table_slots}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    tok_cap = B // 2 + 1
    table = tokens.class_table()
    table_d = _class_table_on(device)
    buf_d = torch.from_numpy(buf.view(np.int32)).to(device)
    voc_start, voc_len, info = i32(tok_cap), i32(tok_cap), i32(4)
    _lib.call("mused_tokenise_cp_scan", ptr(buf_d), B, ptr(table_d), len(table), docptr.ctypes.data_as(C.c_void_p), D,
              int(table_slots), int(max_doc_tokens), ptr(voc_start), ptr(voc_len), tok_cap, ptr(info), ptr(ws), ws_bytes, stream())
    T, V, flags, doc_tokens = (int(x) for x in info.cpu().numpy())
    if flags & _TK_FLAG_TABLE:
        raise ValueError(f"tokenise_codepoints_on_device: {T} tokens do not fit a table of {table_slots} slots")
    if flags & _TK_FLAG_DOC or V >= _MAX_DEVICE_TERMS:
        return _fallback(records, max_row_terms)
    if T == 0:   # documents without a token
        return TextCorpus(records, [], np.zeros(N + 1, dtype=np.int64), empty, empty, empty, valid, max_row_terms)
    # alphabetical ids: the V spans gathered from the host's buffer through the table, decoded at once, sorted as str
    # (code-point order, as scikit-learn's _sort_features)
    vs, vl = voc_start[:V].cpu().numpy().astype(np.int64), voc_len[:V].cpu().numpy().astype(np.int64)
    off = np.concatenate([[0], np.cumsum(vl)])
    packed = table[buf[np.repeat(vs - off[:-1], vl) + np.arange(off[-1])]] & tokens.CP_MASK
    text_ = packed.astype("<u4").tobytes().decode("utf-32-le")
    bounds = off.tolist()
    found = [text_[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
    order = sorted(range(V), key=found.__getitem__)
    rank = np.empty(V, dtype=np.int32)
    rank[order] = np.arange(V, dtype=np.int32)
    vocabulary = [found[i] for i in order]
    rank_d = torch.from_numpy(rank).to(device)
    vrow_d = torch.from_numpy(np.flatnonzero(valid).astype(np.int32)).to(device)
    doc_rowptr, gpostptr = i32(D + 1), i32(V + 1)
    big = {name: i32(T) for name in ("term", "cnt", "pos", "gpostrow", "gpostent")}
    _lib.call("mused_tokenise_cp_build", B, D, int(table_slots), T, V, doc_tokens, ptr(rank_d), ptr(vrow_d), ptr(doc_rowptr),
              ptr(big["term"]), ptr(big["cnt"]), ptr(big["pos"]), ptr(gpostptr), ptr(big["gpostrow"]), ptr(big["gpostent"]),
              ptr(info), ptr(ws), ws_bytes, stream())
    doc_rowptr_h = doc_rowptr.cpu().numpy()
    flags = int(info.cpu().numpy()[2])
    if flags:
        raise _lib.MusedError(f"mused_tokenise_cp_build: the workspace is not what mused_tokenise_cp_scan left (flags {flags})")
    nnz = int(doc_rowptr_h[D])
    rowptr = doc_rowptr_h[np.concatenate([[0], np.cumsum(valid)])]   # invalid rows are empty
    tensors = {name: t[:nnz] for name, t in big.items()}
    tensors["gpostptr"] = gpostptr
    return TextCorpus._from_device(records, vocabulary, rowptr, valid, tensors, device, max_row_terms)


def _is_ascii(records) -> bool:
    """No code point of the (N, 2) strings is above 127 (one pass over the UCS-4 array)."""
    records = np.asarray(records)
    if records.dtype.kind != "U":
        records = records.astype(str)
    if records.size == 0 or records.dtype.itemsize == 0:
        return True
    return int(np.ascontiguousarray(records).view(np.uint32).max()) <= 127 and records.dtype.byteorder != ">"


def tokenise_for_device(records, device=None) -> TextCorpus:
    """The corpus of `records` by the tokeniser MUSED_TOKENISE names (read at every call): "host" = `tokenise`;
    "device" = `tokenise_on_device` for a pure-ASCII corpus and `tokenise_codepoints_on_device` for any other; unset:
    the device from TOKENISE_DEVICE_MIN_ROWS rows of ASCII on, from TOKENISE_CODEPOINTS_MIN_ROWS rows of other text."""
    mode = os.environ.get("MUSED_TOKENISE", "")
    if mode not in ("", "device", "host"):
        raise ValueError(f"MUSED_TOKENISE={mode!r}: device or host")
    n = len(records)
    if mode == "host" or (mode == "" and n < min(TOKENISE_DEVICE_MIN_ROWS, TOKENISE_CODEPOINTS_MIN_ROWS)):
        return tokenise(records)
    if _is_ascii(records):
        if mode == "device" or n >= TOKENISE_DEVICE_MIN_ROWS:
            return tokenise_on_device(records, device)
    elif mode == "device" or n >= TOKENISE_CODEPOINTS_MIN_ROWS:
        return tokenise_codepoints_on_device(records, device)
    return tokenise(records)


# measured: the device tokeniser was the faster one from 500 rows on, by more than the spread between
# repeated runs; at 100 rows the two are level (a call of either takes about 0.5 ms) and the host stays the default
TOKENISE_DEVICE_MIN_ROWS = 500
# the code-point path against `tokenise` on the same swapped-letter rows, a threshold of its own: 500
# rows was the smallest measured count at which it was faster on both streams by more than the spread (2.6 against 5.9 ms,
# 1.4 against 2.2 ms); at 100 rows it won on one stream and lost on the other
TOKENISE_CODEPOINTS_MIN_ROWS = 500
