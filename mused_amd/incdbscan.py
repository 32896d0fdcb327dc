"""`IncrementalDBSCAN(eps, min_pts)` with the two calls the reference's DBSCAN_incr approach makes (main.py:87-91:
`clusterer.insert(reduced).get_cluster_labels(reduced)` per window), on the device (csrc/dbscan_incr.hip).

What the labels are: after every insert, those of sklearn.cluster.DBSCAN(eps, min_samples=min_pts).fit_predict on all rows
inserted so far, numbering included (the rule and why it is exact: mused_amd/dbscan_incr.py).  That refit is what the tests
pin the class to, bit for bit.  It is NOT pinned to the `incdbscan` package the reference imports: the package is not
available here, so its cluster numbers, its float labels and its choice for a border row between clusters are unchecked.
The labels of rows inserted earlier may change with a later insert (clusters merge, numbers shift), as a refit's would.

A SLIDING WINDOW: `delete_oldest(m)` drops the m oldest rows on the device (mused_dbscan_incr_delete), `max_rows` lets every
insert do so by itself, `delete(X)` is the package's call for rows that ARE the oldest ones.  The pin is the same: after any
sequence of inserts and deletes the labels of the rows still held are those of scikit-learn's refit of these rows in their order.

ANY ROWS: `delete_rows(idx)` drops the rows at any positions among the rows held (mused_dbscan_incr_delete_rows; the rule:
`IncrementalSpec.delete_rows`, the same pin), `find(X)` looks rows up by value (mused_rows_find; pinned to the NumPy rule of
mused_amd/rows_find.py: bit equality, duplicates handed out in order of position) and `labels_of(X)` returns their labels.
With `by_value=True`, `delete(X)` and `get_cluster_labels(X)` take any rows, as the package describes its own calls: rows not
held are skipped with a warning, or get NaN.  These two are UNPINNED against the package, like its numbering and its float labels.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np
import torch

from . import _lib
from . import matrix_operations as mo
from .dbscan import FLAG_AMBIGUOUS, FLAG_NONFINITE
from .engine import ptr
from .rows_find import rows_find

MAX_ROWS = mo.DBSCAN_MAX_ROWS   # csrc/dbscan_incr.hip: the limit of mused_dbscan
_FIRST_CAPACITY = 4096


class IncrementalDBSCAN:
    """eps, min_pts: as DBSCAN's eps, min_samples.  eps="auto": eps is chosen by `matrix_operations.select_eps_on_device` from
    the rows of the first insert (k = min_pts; the knee of their sorted k-distance curve) and then fixed for the object's life,
    in sliding and by_value modes alike; `.eps_` is the eps in use (None until chosen).  chunk: rows per staging panel of the kernels (a multiple of 128).
    stream: the kernels run on it (default: the current stream at each insert); an insert returns after they have finished.

    max_rows: None (the default: the state only grows, as the reference's use of the class has it), or the most rows to hold: an
    insert that would leave more first deletes the surplus oldest rows (deleting first keeps the insert small; the final state
    does not depend on the order).  A window of more than max_rows rows is a ValueError.

    The state tensors (rows, norms, counts, union-find, border minima) are owned here and grow by doubling up to 2^19 rows.
    The rows live in a buffer behind an offset: a delete moves no row, and when the tail of the buffer runs out the rows held
    are copied to its front once (with deletes the buffer is sized for twice the rows held, so that this happens once per that
    many rows).  With max_rows set the buffer never exceeds 2 max_rows rows, the other state tensors max_rows: a stream of any
    length runs.
    Host mode, in which every insert refits scikit-learn's DBSCAN on a host copy of all rows, is entered for good
      * by an insert whose kernel raises the ambiguity flag (some pair lies within rounding of eps: mused_amd/dbscan.py); that
        insert and every later one is counted in `matrix_operations.dbscan_incr_fallbacks`;
      * uncounted, under MUSED_DBSCAN=host (read at construction) and beyond 2^19 rows.
    A non-finite row raises scikit-learn's ValueError("Input contains NaN or infinity."); the object then refuses inserts.

    by_value: False (the default) keeps `delete(X)` to the oldest rows and `get_cluster_labels(X)` to the batch of the last
    insert, with their errors.  True: both look X up by value (`find`); `delete` skips rows that are not held, with one
    UserWarning that gives their number, and `get_cluster_labels` returns float64 labels with NaN for them.
    A delete of any rows packs the survivors into a second row buffer and the two change places.  From the first such delete
    on, with max_rows set, each of the two holds at most max_rows rows (2 max_rows in all, as before), and the rows held are
    copied to the front whenever the tail runs out."""

    def __init__(self, eps=1.0, min_pts=5, chunk=4096, stream=None, max_rows=None, by_value=False):
        self._auto = isinstance(eps, str)
        if self._auto:
            if eps != "auto":
                raise ValueError(f'eps must be a number or "auto", got {eps!r}')
            if int(min_pts) < 1:
                raise ValueError("eps must be > 0 and min_pts >= 1")
        elif not (float(eps) > 0.0) or int(min_pts) < 1:
            raise ValueError("eps must be > 0 and min_pts >= 1")
        if max_rows is not None and int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1")
        self.max_rows = None if max_rows is None else int(max_rows)
        self.by_value = bool(by_value)
        self._off = 0              # the rows held are _X[_off : _off + n]
        self._X2 = None            # the buffer a delete of any rows packs the survivors into; it then becomes _X
        self._two = False          # such a delete has happened
        self._find_ws = None
        self.last_delete_info = None   # device mode: {0, clusters, core rows, lost core status, |R|, |B|} of the last delete
        self.eps, self.min_pts, self.chunk = (None if self._auto else float(eps)), int(min_pts), int(chunk)
        self.eps_ = self.eps       # the eps in use: the number given, or the one chosen at the first insert (None before it)
        self._stream = stream
        self.n, self.d = 0, None
        self._host_mode = os.environ.get("MUSED_DBSCAN", "device") == "host" or not (self._auto or self.eps < 1e150)
        self._counted = False      # host mode entered through the flag: inserts are counted
        self._host_rows = None
        self._dead = False
        self._X = self._nrm = self._count = self._parent = self._best = self._labels = self._ws = None
        self._host_labels = None
        self._last, self._last_lo = None, 0
        self.last_info = None      # device mode: {flags, clusters, core rows, dirty rows, turned core, root moved}
        self.dirty = []            # per device insert (rows that turned core, core rows whose root moved)

    # ---- state ---------------------------------------------------------------------------------
    def _rows(self):
        return self._X[self._off:self._off + self.n]

    def _grow(self, n, dev):
        """Room for n rows in all (the n - self.n new ones behind the rows held)."""
        cap = 0 if self._nrm is None else self._nrm.shape[0]
        if n > cap:
            new = max(_FIRST_CAPACITY, cap)
            while new < n:
                new *= 2
            new = min(new, MAX_ROWS) if self.max_rows is None else min(new, MAX_ROWS, self.max_rows)
            L = _lib.lib()
            nbytes = max(int(L.mused_dbscan_incr_ws_bytes(new, self.d, self.chunk)),
                         int(L.mused_dbscan_incr_delete_ws_bytes(new, self.d, self.chunk)),
                         int(L.mused_dbscan_incr_delete_rows_ws_bytes(new, self.d, self.chunk)))
            if nbytes < 0:
                raise ValueError(f"IncrementalDBSCAN: d = {self.d} or chunk = {self.chunk} is not taken (chunk: a multiple of "
                                 "128 in [128, 65536])")

            def moved(old, dtype):
                t = torch.empty((new,), dtype=dtype, device=dev)
                if old is not None and self.n:
                    t[:self.n] = old[:self.n]
                return t

            self._nrm = moved(self._nrm, torch.float64)
            self._count, self._parent, self._best = (moved(t, torch.int32) for t in (self._count, self._parent, self._best))
            self._labels = torch.empty(new, dtype=torch.int32, device=dev)
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cap = 0 if self._X is None else self._X.shape[0]
        if self._off + n <= cap:
            return
        # the tail has run out.  A state that deletes keeps twice the rows held, so that the copy to the front is paid once
        # per that many rows; one that only grows keeps the capacity of the other tensors
        two = self._two and self.max_rows is not None   # two buffers of at most max_rows rows each
        slack = 1 if two else 2 if (self.max_rows is not None or self._off) else 1
        if slack * n <= cap:
            self._X[:self.n] = self._rows().clone()
            self._off = 0
            return
        new = max(_FIRST_CAPACITY, cap)
        while new < slack * n:
            new *= 2
        if two:
            new = min(new, self.max_rows)
        else:
            new = min(new, MAX_ROWS) if slack == 1 else (new if self.max_rows is None else min(new, 2 * self.max_rows))
        X = torch.empty((new, self.d), dtype=torch.float64, device=dev)
        if self.n:
            X[:self.n] = self._rows()
        self._X, self._off = X, 0

    def _to_host_mode(self, counted):
        self._host_mode, self._counted = True, counted
        if self._X is not None:
            self._host_rows = self._rows().cpu().numpy()
        self._X = self._nrm = self._count = self._parent = self._best = self._labels = self._ws = None
        self._X2 = self._find_ws = None

    # ---- the reference's two calls ---------------------------------------------------------------
    def insert(self, X):
        """X: (w, d) ndarray or CUDA tensor (taken as fp64).  Returns self."""
        if self._dead:
            raise ValueError("this IncrementalDBSCAN met a non-finite row and takes no further inserts")
        on_dev = isinstance(X, torch.Tensor)
        rows = X.to(torch.float64) if on_dev else np.ascontiguousarray(X, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1 or (self.d is not None and rows.shape[1] != self.d):
            raise ValueError("X must be (w, d) with w, d >= 1 and the d of the earlier inserts")
        self.d = int(rows.shape[1])
        if self.max_rows is not None:
            if rows.shape[0] > self.max_rows:
                raise ValueError(f"a window of {rows.shape[0]} rows is larger than max_rows = {self.max_rows}")
            if self.n + rows.shape[0] > self.max_rows:
                self._delete(self.n + int(rows.shape[0]) - self.max_rows, refit=False)   # (host mode: the insert below refits)
        if self.eps is None:
            # eps="auto": chosen from the rows of the FIRST insert, then fixed (a ValueError -- a flat curve, min_pts = 1 or more
            # than 64 or than the rows, a non-finite row -- leaves the object without an eps and the insert undone)
            self.eps = self.eps_ = mo.select_eps_on_device(rows, self.min_pts, self._stream)[0]
        n0, n = self.n, self.n + int(rows.shape[0])
        if not self._host_mode and n > MAX_ROWS:
            self._to_host_mode(False)
        if self._host_mode:
            self._insert_host(rows.cpu().numpy() if on_dev else rows, n)
        else:
            self._insert_device(rows, n0, n)
        self._last, self._last_lo = X, n0
        return self

    def _insert_host(self, rows, n):
        self._host_rows = rows.copy() if self._host_rows is None else np.concatenate([self._host_rows, rows])
        self.n = n
        if self._counted:
            mo._dbscan_incr_count_fallback()
        try:
            self._host_labels = np.asarray(mo.perform_dbscan_clustering(self._host_rows, self.eps, self.min_pts), dtype=np.int64)
        except ValueError:
            self._dead = True
            raise

    def _insert_device(self, rows, n0, n):
        st = mo._match_stream(self._stream)
        with torch.cuda.stream(st):
            dev = rows.device if isinstance(rows, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
            self._grow(n, dev)
            held = self._X[self._off:]
            held[n0:n] = rows if isinstance(rows, torch.Tensor) else torch.tensor(rows, device=dev)
            info = (C.c_int * 6)()
            _lib.call("mused_dbscan_incr_insert", ptr(held), held.stride(0), self.d, ptr(self._nrm), ptr(self._count),
                      ptr(self._parent), ptr(self._best), n0, n - n0, self.eps, self.min_pts, self.chunk, ptr(self._labels),
                      info, ptr(self._ws), self._ws.numel(), C.c_void_p(st.cuda_stream))
            self.n = n
            self.last_info = np.array(info[:], dtype=np.int32)
            if info[0] & FLAG_NONFINITE:
                self._dead = True
                raise ValueError("Input contains NaN or infinity.")
            if info[0] & FLAG_AMBIGUOUS:
                self.n = n0   # (the rows of this insert are appended again, on the host)
                self._to_host_mode(True)
                self._insert_host(rows.cpu().numpy() if isinstance(rows, torch.Tensor) else rows, n)
                return
            self.dirty.append((int(info[4]), int(info[5])))

    # ---- a sliding window -------------------------------------------------------------------------
    def delete_oldest(self, m):
        """Drops the m oldest rows held, 1 <= m <= n.  Returns self; `labels()` then covers the rows still held."""
        if self._dead:
            raise ValueError("this IncrementalDBSCAN met a non-finite row and takes no further calls")
        m = int(m)
        if not 1 <= m <= self.n:
            raise ValueError(f"delete_oldest: m = {m} is outside [1, {self.n}] (the rows held)")
        self._delete(m, refit=True)
        return self

    def delete(self, X):
        """The `incdbscan` package's call.  by_value=False: for the oldest rows only: X must be bit-equal to the oldest len(X)
        rows held, in their order; anything else is a ValueError.  by_value=True: the rows that `find(X)` returns are deleted,
        rows not held are skipped with one UserWarning that gives their number."""
        if self.by_value:
            pos = self.find(X)
            missing = int((pos < 0).sum())
            if missing:
                warnings.warn(f"IncrementalDBSCAN.delete: {missing} of {len(pos)} rows are not held and were skipped", UserWarning,
                              stacklevel=2)
            return self.delete_rows(pos[pos >= 0]) if missing < len(pos) else self
        on_dev = isinstance(X, torch.Tensor)
        rows = X.to(torch.float64) if on_dev else np.ascontiguousarray(X, dtype=np.float64)
        k = int(rows.shape[0]) if rows.ndim == 2 else 0
        same = rows.ndim == 2 and 1 <= k <= self.n and rows.shape[1] == self.d
        if same and self._host_mode:
            mine = self._host_rows[:k]
            same = np.array_equal(mine.view(np.int64), (rows.cpu().numpy() if on_dev else rows).view(np.int64))
        elif same:
            mine = self._X[self._off:self._off + k]
            theirs = rows if on_dev else torch.tensor(rows, device=mine.device)
            same = bool(torch.equal(mine.view(torch.int64), theirs.contiguous().view(torch.int64)))
        if not same:
            raise ValueError("delete takes the oldest rows held only, bit-equal and in their order: lookup by value is not "
                             "offered (delete_oldest(m) drops them by number)")
        return self.delete_oldest(k)

    def _delete(self, m, refit):
        n = self.n - m
        if self._last is not None:
            self._last_lo -= m
            if self._last_lo < 0:
                self._last = None
        if self._host_mode:
            self._host_rows = self._host_rows[m:]
            self.n = n
            if refit:
                if self._counted:
                    mo._dbscan_incr_count_fallback()
                self._host_labels = (np.asarray(mo.perform_dbscan_clustering(self._host_rows, self.eps, self.min_pts), dtype=np.int64)
                                     if n else np.empty(0, dtype=np.int64))
            return
        st = mo._match_stream(self._stream)
        with torch.cuda.stream(st):
            held = self._X[self._off:]
            info = (C.c_int * 6)()
            _lib.call("mused_dbscan_incr_delete", ptr(held), held.stride(0), self.d, ptr(self._nrm), ptr(self._count),
                      ptr(self._parent), ptr(self._best), self.n, m, self.eps, self.min_pts, self.chunk, ptr(self._labels),
                      info, ptr(self._ws), self._ws.numel(), C.c_void_p(st.cuda_stream))
        self.n = n
        self._off = self._off + m if n else 0
        self.last_delete_info = np.array(info[:], dtype=np.int32)

    # ---- any rows ---------------------------------------------------------------------------------
    def delete_rows(self, idx):
        """Drops the rows at the positions `idx` among the rows held: an int array or a bool mask over the rows held, NumPy
        (or a sequence) or a CUDA tensor.  Positions that repeat or lie outside [0, n) are a ValueError and leave the state
        untouched, as does an empty set.  Returns self; `labels()` then covers the rows still held, in their order."""
        if self._dead:
            raise ValueError("this IncrementalDBSCAN met a non-finite row and takes no further calls")
        n = self.n
        if isinstance(idx, torch.Tensor):
            t = idx.reshape(-1)
            if t.dtype == torch.bool:
                if t.numel() != n:
                    raise ValueError(f"delete_rows: a mask must have one entry per row held ({n})")
                t = torch.nonzero(t).reshape(-1)
            elif t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
                raise ValueError("delete_rows: positions must be integers or a bool mask")
            t = torch.sort(t.to(torch.int64)).values
            bad = t.numel() < 1 or bool((t[0] < 0) | (t[-1] >= n) | (t[1:] == t[:-1]).any())
            below = 0 if bad else int((t < self._last_lo).sum())
            last_hit = not bad and int(t[-1]) >= self._last_lo
        else:
            t = np.asarray(idx).reshape(-1)
            if t.dtype == np.bool_:
                if t.size != n:
                    raise ValueError(f"delete_rows: a mask must have one entry per row held ({n})")
                t = np.flatnonzero(t)
            elif t.size and not np.issubdtype(t.dtype, np.integer):
                raise ValueError("delete_rows: positions must be integers or a bool mask")
            t = np.sort(t.astype(np.int64))
            bad = t.size < 1 or t[0] < 0 or t[-1] >= n or bool((t[1:] == t[:-1]).any())
            below = 0 if bad else int((t < self._last_lo).sum())
            last_hit = not bad and int(t[-1]) >= self._last_lo
        if bad:
            raise ValueError(f"delete_rows: needs 1 to {n} distinct positions in [0, {n})")
        m = int(t.shape[0])
        if m == n:                                          # everything goes: the empty state
            self._delete(n, refit=True)
            return self
        if self._last is not None:
            self._last_lo -= below
            if last_hit:
                self._last = None
        if self._host_mode:
            keep = np.ones(n, dtype=bool)
            keep[t.cpu().numpy() if isinstance(t, torch.Tensor) else t] = False
            self._host_rows = self._host_rows[keep]
            self.n = n - m
            if self._counted:
                mo._dbscan_incr_count_fallback()
            self._host_labels = np.asarray(mo.perform_dbscan_clustering(self._host_rows, self.eps, self.min_pts), dtype=np.int64)
            return self
        st = mo._match_stream(self._stream)
        with torch.cuda.stream(st):
            dev = self._X.device
            dele = (t.to(dev) if isinstance(t, torch.Tensor) else torch.from_numpy(t).to(dev)).to(torch.int32).contiguous()
            if self._X2 is None or self._X2.shape[0] < n - m:
                cap = self._X.shape[0] if self.max_rows is None else min(self._X.shape[0], self.max_rows)
                self._X2 = torch.empty((cap, self.d), dtype=torch.float64, device=dev)
            held, out = self._X[self._off:], self._X2
            info = (C.c_int * 6)()
            _lib.call("mused_dbscan_incr_delete_rows", ptr(held), held.stride(0), self.d, ptr(out), out.stride(0), ptr(self._nrm),
                      ptr(self._count), ptr(self._parent), ptr(self._best), n, ptr(dele), m, self.eps, self.min_pts, self.chunk,
                      ptr(self._labels), info, ptr(self._ws), self._ws.numel(), C.c_void_p(st.cuda_stream))
        if info[0]:
            raise RuntimeError(f"mused_dbscan_incr_delete_rows refused a checked list (flags {info[0]})")
        self._X, self._X2, self._off, self.n, self._two = out, self._X, 0, n - m, True
        if self.max_rows is not None and self._X2.shape[0] > self.max_rows:
            self._X2 = None                                 # (the buffer of 2 max_rows rows of the sliding window)
        self.last_delete_info = np.array(info[:], dtype=np.int32)
        return self

    def _queries(self, X):
        on_dev = isinstance(X, torch.Tensor)
        rows = X.to(torch.float64) if on_dev else np.ascontiguousarray(X, dtype=np.float64)
        if rows.ndim != 2 or (self.d is not None and rows.shape[1] != self.d):
            raise ValueError("X must be (q, d) with the d of the inserts")
        return rows, on_dev

    def find(self, X):
        """int64 NumPy positions of the rows of X among the rows held, -1 for rows that are not held (the rule:
        mused_amd/rows_find.py: bit equality; a value held several times is handed out in order of position)."""
        rows, on_dev = self._queries(X)
        q = int(rows.shape[0])
        if q == 0 or self.n == 0:
            return np.full(q, -1, dtype=np.int64)
        if self._host_mode:
            return rows_find(self._host_rows, rows.cpu().numpy() if on_dev else rows)
        st = mo._match_stream(self._stream)
        with torch.cuda.stream(st):
            dev = self._X.device
            Q = (rows.to(dev) if on_dev else torch.tensor(rows, device=dev)).contiguous()
            nbytes = int(_lib.lib().mused_rows_find_ws_bytes(self.n, q, self.d))
            if nbytes < 0:
                raise ValueError(f"find: {self.n} rows held and {q} asked for are more than mused_rows_find takes")
            if self._find_ws is None or self._find_ws.numel() < nbytes:
                self._find_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            idx = torch.empty(q, dtype=torch.int32, device=dev)
            info = torch.empty(4, dtype=torch.int32, device=dev)
            held = self._rows()
            _lib.call("mused_rows_find", ptr(held), held.stride(0), self.n, ptr(Q), Q.stride(0), q, self.d, ptr(idx), ptr(info),
                      ptr(self._find_ws), self._find_ws.numel(), C.c_void_p(st.cuda_stream))
            return idx.cpu().numpy().astype(np.int64)

    def labels_of(self, X):
        """int64 NumPy labels of the rows of X, which must all be held (`find`); ValueError otherwise."""
        pos = self.find(X)
        if (pos < 0).any():
            raise ValueError(f"labels_of: {int((pos < 0).sum())} of {len(pos)} rows are not held")
        return self.labels()[pos] if len(pos) else np.empty(0, dtype=np.int64)

    def labels(self):
        """int64 NumPy labels of the rows held: all rows inserted so far but the deleted ones (-1 = noise)."""
        if self.n == 0:
            return np.empty(0, dtype=np.int64)
        if self._host_mode:
            return self._host_labels.copy()
        return self._labels[:self.n].cpu().numpy().astype(np.int64)

    def get_cluster_labels(self, X):
        """by_value=False: int64 NumPy labels of the batch just inserted.  X must BE that batch (the object handed to the last
        `insert`, or an ndarray equal to it).  by_value=True: float64 labels of any rows, NaN for rows that are not held."""
        if self.by_value:
            pos = self.find(X)
            out = np.full(len(pos), np.nan)
            if (pos >= 0).any():
                out[pos >= 0] = self.labels()[pos[pos >= 0]]
            return out
        last = self._last
        same = X is last
        if not same and last is not None and isinstance(X, np.ndarray) and isinstance(last, np.ndarray):
            same = X.shape == last.shape and np.array_equal(X, last)
        if not same:
            raise ValueError("get_cluster_labels takes the batch of the last insert only: lookup by value is not offered")
        if self._host_mode:
            return self._host_labels[self._last_lo:self.n].copy()
        return self._labels[self._last_lo:self.n].cpu().numpy().astype(np.int64)
