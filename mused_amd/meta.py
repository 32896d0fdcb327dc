"""One encoding pass over a whole stream of a metadata modality ("location", "time", "username", "tags";
matrix_operations.py:22-89), the counterpart of mused_amd/text.py for the "text" modality.

What `matrix_operations._metadata_adjacency` works out per window on the host does not depend on the window: whether a
row is valid is a property of the row; the same-user relation compares ids for equality, so ids numbered over the whole
stream serve every window; Jaccard similarity depends on the sets only, so stream-global tag ids serve every window; and
the rows inside a tag's posting list ascend, so a window's part of a list is one contiguous range.  `encode(records,
modality_type)` therefore applies the validity and encoding expressions of `_metadata_adjacency` once to the whole column
and keeps the result as arrays (`MetaCorpus`) that are uploaded once; a window is a view (`MetaWindow`) and its adjacency
one enqueue-only launch that writes the window-coordinate bitmask (csrc/meta_window.hip; "username": mused_group_mask on
a slice of the id array).  With step_window_ratio = r a row is no longer encoded r times.
"""
from __future__ import annotations

import numpy as np

_INT32_END = 2 ** 31
_RECORD_KINDS = {"location": 0, "time": 1}
_DEVICE_FIELDS = {"location": ("rec", "vrank"), "time": ("rec", "vrank"), "username": ("uid", "vrank"),
                  "tags": ("rowptr", "tag", "gpostptr", "gpostrow", "vrank")}


class MetaCorpus:
    """Host arrays of an encoded stream of N rows of one metadata type (`kind`); all integers int32.

        every type   vrank[N + 1]                     prefix count of valid rows
        location     rec (N, 2) fp64                  data.astype(float64); valid: neither entry is NaN
        time         rec (N, 2) fp64                  valid: both stamps != 0.0
        username     uid[N]                           rank of the name in np.unique over the non-empty names, -1 for ''
        tags         rowptr[N + 1], tag[nnz]          CSR over ALL rows (invalid rows are empty) of set(tags), stream-global
                                                      ids ascending inside a row; valid: data[:, 0] != "" ([] is valid)
                     gpostptr[V + 1], gpostrow[nnz]   tag-major postings: the rows that hold a tag, ascending

    `records` holds the original host rows (the host path and every fallback read them).  `host_only`: the int32 arrays
    cannot hold the corpus (N or nnz >= 2^31); only the records are kept and every window takes the host path."""

    def __init__(self, records, kind, valid, max_entries=_INT32_END, rec=None, uid=None, rowptr=None, tag=None, n_tags=0):
        self.records, self.kind = records, kind
        self.N = len(records)
        self.V = int(n_tags)
        self.nnz = int(rowptr[-1]) if rowptr is not None else 0
        self.host_only = self.N >= max_entries or self.nnz >= max_entries
        self._dev = {}
        self.rec = self.uid = self.rowptr = self.tag = self.gpostptr = self.gpostrow = self.vrank = None
        if self.host_only:
            return
        self.vrank = np.concatenate([[0], np.cumsum(np.asarray(valid, dtype=bool))]).astype(np.int32)
        if rec is not None:
            self.rec = np.ascontiguousarray(rec, dtype=np.float64)
        if uid is not None:
            self.uid = np.ascontiguousarray(uid, dtype=np.int32)
        if rowptr is not None:
            self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
            self.tag = np.ascontiguousarray(tag, dtype=np.int32)
            order = np.argsort(self.tag, kind="stable")   # entries are row-major: rows ascend inside a tag
            rows = np.repeat(np.arange(self.N, dtype=np.int32), np.diff(self.rowptr))
            self.gpostptr = np.concatenate([[0], np.cumsum(np.bincount(self.tag, minlength=self.V))]).astype(np.int32)
            self.gpostrow = np.ascontiguousarray(rows[order], dtype=np.int32)

    def __len__(self):
        return self.N

    @property
    def shape(self):
        return (self.N,) + tuple(np.shape(self.records)[1:])

    def window(self, lo=0, hi=None) -> "MetaWindow":
        """Rows [lo, hi) of the corpus: a view, nothing is copied."""
        hi = self.N if hi is None else hi
        if not 0 <= lo <= hi <= self.N:
            raise IndexError(f"window [{lo}, {hi}) outside a corpus of {self.N} rows")
        return MetaWindow(self, int(lo), int(hi))

    def __getitem__(self, rows):
        if not isinstance(rows, slice) or rows.step not in (None, 1):
            raise TypeError("a MetaCorpus is sliced by contiguous row ranges")
        lo, hi, _ = rows.indices(self.N)
        return self.window(lo, max(lo, hi))

    def device_arrays(self, device):
        """The arrays of this type as device tensors, uploaded once per corpus and device."""
        import torch

        dev = self._dev.get(str(device))
        if dev is None:
            if self.host_only:
                raise ValueError("a host-only corpus has no device arrays")
            dev = {}
            for name in _DEVICE_FIELDS[self.kind]:
                a = getattr(self, name)
                dev[name] = torch.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)).to(device)
            torch.cuda.current_stream().synchronize()   # resident before any other stream reads them
            self._dev[str(device)] = dev
        return dev


class MetaWindow:
    """Rows [lo, hi) of a MetaCorpus, what `adjacency_on_device(x, corpus.kind, ...)` takes in place of the rows."""

    def __init__(self, corpus: MetaCorpus, lo: int, hi: int):
        self.corpus, self.lo, self.hi = corpus, lo, hi

    def __len__(self):
        return self.hi - self.lo

    @property
    def shape(self):
        return (self.hi - self.lo,) + self.corpus.shape[1:]

    @property
    def records(self):
        return self.corpus.records[self.lo:self.hi]

    def __getitem__(self, rows):
        if not isinstance(rows, slice) or rows.step not in (None, 1):
            raise TypeError("a MetaWindow is sliced by contiguous row ranges")
        lo, hi, _ = rows.indices(len(self))
        return MetaWindow(self.corpus, self.lo + lo, self.lo + max(lo, hi))


def encode(records, modality_type, max_entries=_INT32_END) -> MetaCorpus:
    """A whole stream of one metadata type -> MetaCorpus: validity and encoding are the expressions of
    `matrix_operations._metadata_adjacency`, applied once to the whole column.  records: the (N, 2) / (N, 1) array the
    reference's branch takes (a tensor is copied to the host once).  `max_entries`: the row / entry count from which
    the corpus is marked host-only (the int32 range; smaller values are for tests)."""
    if modality_type not in _DEVICE_FIELDS:
        raise ValueError(f"modality_type={modality_type!r} is not a metadata type {tuple(_DEVICE_FIELDS)}")
    if hasattr(records, "cpu") and hasattr(records, "numpy"):
        records = records.cpu().numpy()
    data = np.asarray(records)
    if data.ndim != 2:
        raise ValueError(f"{modality_type} records must be a 2-D array of rows, got shape {data.shape}")
    N = len(data)
    if modality_type in _RECORD_KINDS:
        if data.shape[1] != 2:
            raise ValueError(f"{modality_type}: need N x 2 records, got {data.shape}")
        if modality_type == "location":
            rec = data.astype(np.float64)
            valid = ~np.isnan(rec).any(axis=1)
        else:
            valid = ~((data[:, 0] == 0.0) | (data[:, 1] == 0.0))
            rec = np.ascontiguousarray(data, dtype=np.float64)
        return MetaCorpus(data, modality_type, valid, max_entries, rec=rec)
    valid = np.asarray(data[:, 0] != "", dtype=bool) if N else np.zeros(0, dtype=bool)
    if modality_type == "username":
        uid = np.full(N, -1, dtype=np.int32)
        if valid.any():
            _, uid[valid] = np.unique(data[valid, 0].astype(str), return_inverse=True)
        return MetaCorpus(data, modality_type, valid, max_entries, uid=uid)
    vocab, rowptr, ids = {}, [0], []
    for ok, tags in zip(valid, data[:, 0]):
        if ok:
            tag_set = set(tags) if tags else set()
            ids.extend(sorted(vocab.setdefault(t, len(vocab)) for t in tag_set))
        rowptr.append(len(ids))
    return MetaCorpus(data, modality_type, valid, max_entries, rowptr=np.asarray(rowptr, dtype=np.int64),
                      tag=np.asarray(ids, dtype=np.int64), n_tags=len(vocab))
