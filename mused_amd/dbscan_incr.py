"""Incremental DBSCAN under insertions, written out as a rule: the specification of csrc/dbscan_incr.hip (plain NumPy,
blocks of O(dirty x n) distances, O(n) state).

The reference's DBSCAN_incr approach (main.py:87-91) keeps one `incdbscan.IncrementalDBSCAN(eps, min_pts)` for the stream and
calls `insert(window).get_cluster_labels(window)` per window.  Incremental DBSCAN under insertions maintains the clustering
of a batch DBSCAN on everything inserted so far, and mused_amd/dbscan.py holds scikit-learn's batch DBSCAN in closed form.
So the rule here is stated against that:

    after every insert, the labels of ALL rows seen so far equal
    sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(all rows so far), numbering included.

THE PIN is scikit-learn's refit of the prefix (tests/test_dbscan_incr_host.py, after every insert, exact equality, wherever
`mused_amd.dbscan.ambiguous(prefix, eps)` is False).  It is UNPINNED AGAINST `incdbscan`: the package is not available
here, so its numbering of the clusters, its float labels (NaN for unknown rows, -1 noise) and the cluster it gives a border
row that touches several cannot be checked.

State over the n rows inserted so far (notation of mused_amd/dbscan.py: N(i) = { j : d2(i, j) <= eps^2 }, i included):

    X, nrm[i]   the rows and their squared norms
    count[i]    |N(i)|
    parent[]    union-find over the core rows, parent[x] <= x: a component's root is its smallest core index
    best[i]     for a non-core row the smallest root among its core neighbours as of the last insert, or NONE

Inserting w rows as indices n0 .. n0 + w - 1:

    1 COUNT    the new rows against all n0 + w rows: count[new] += |N(new)|, count[old] += the new rows within eps.  Both
               orientations of a new-new pair lie in the rectangle, so the row side alone counts them, once each.  A pair
               i != j with |d2 - eps^2| <= tau(i, j) raises flag 1, a non-finite row flag 2.
    2 NEWLY CORE   core_before and root_before[i] = find(i) are remembered (O(n)); dirtyA = the rows that are core now and
               were not before.  Old rows can be among them.
    3 UNION    dirtyA against all rows: every core-core edge within eps^2 is united.  Here two old clusters merge through
               an old row that has only now turned core -- the new x all rectangle alone misses those edges.  (An edge
               between two rows that were both core before was united when the later of them turned core.)
    4 RESOLVE  every non-core row with best != NONE: best = find(best) (O(n)).
    5 BORDER   dirtyB = the core rows whose root differs from root_before, every newly core row included.  For each pair
               (c in dirtyB, b non-core) within eps^2: best[b] = min(best[b], root[c]).  Each new non-core row is also taken
               against all core rows and gets the smallest root among its core neighbours.
    6 LABELS   rank[r] = number of roots below r; a core row gets rank[root], a non-core row rank[best] or -1.

Why 4 and 5 together are exact.  Roots only ever decrease (the smaller root wins every union, and core rows stay core under
insertions).  After step 4 best[b] is the current root of the old minimum, which is <= the current root of every old core
neighbour whose root did not change (that root was >= the old minimum then and is the same now), and every core neighbour
whose root did change, or which is newly core, is in dirtyB and is visited explicitly.  So best[b] is again the smallest
root among all core neighbours of b, and rank is monotone in the root index: the smallest root carries the smallest label,
which is the cluster scikit-learn's index-order search reaches b from first.

For min_samples <= 2 a non-core row has no neighbour but itself: no border row exists, steps 4-5 are empty and every
non-core row is noise.  Duplicate rows are ordinary rows at distance ~0, as for scikit-learn.

DELETING a non-empty set D of distinct positions among the n rows held; S = the rest, in their order (`_delete`, reached through
`delete_rows(idx)` and `delete_oldest(m)`; the kernels: mused_dbscan_incr_delete_rows, mused_dbscan_incr_delete).  The pin is the
same: afterwards the labels of S equal scikit-learn's refit of those rows in their order (tests/test_dbscan_incr_delete_host.py,
tests/test_dbscan_incr_delete_rows_host.py, after every operation).

    1 UNCOUNT  D against ALL rows: count[j] -= |{ i in D : d2(i, j) <= eps^2 }|.  Subtracting from a dead column is harmless: the
               column is dropped in step 6.  No rounding test and no new flag: every pair was tested against tau when the later
               of its two rows was inserted, so an unflagged state holds no pair whose side of eps^2 depends on how d2 is
               evaluated, and the counts stay exact.
    2 REMEMBER before anything moves: core_before, root_before[i] = find(i) for the core rows, find(best[i]) for the non-core
               rows that have a best (O(n)).
    3 AFFECTED gone = the core rows of D; lost = the rows of S that were core and have count < min_samples now.  A component
               (old root r) is affected iff it holds a row of gone or of lost.  An unaffected component keeps every core row
               and every edge: it stays one component with the same root.
    4 REBUILD  R = the rows of S that are still core and whose root_before is affected: parent[x] = x for x in R, then every
               pair of R within eps^2 is united (the smaller root wins).  A dead row is never core in it.  No edge joins R to a
               core row outside R: such a row was in the same component before, and a deletion adds no edge.  R against the rows
               of S, never S x S; the components the delete does not touch cost nothing.  (A lost row gets parent[x] = x: a
               non-core row is its own parent, which is what an insert that turns it core again starts from.)
    5 BORDER   (min_samples >= 3)  B = lost and the non-core rows of S whose remembered best is an affected root.  For b in B:
               best[b] = the smallest NEW root among its core neighbours in S, or NONE.  Every other non-core row keeps its
               best: the pieces of an affected component have roots >= the old root, so a minimum that came from an
               unaffected component is still the minimum, and a row without a best gains no neighbour.
    6 COMPACT  survivor i becomes pos[i] = i - |{ j in D : j < i }|: nrm, count, parent and best are packed, and parent and best
               entries are renumbered through the same map (a core row's best is not read anywhere and is reset to NONE).  The
               map keeps the order, so parent[x] <= x still holds and a root is still the smallest core index of its component.
               Labels as in 6 above.  D = everything leaves the empty state: the next insert is a first insert.

Afterwards best is a root as of this operation: with the two invariants of step 6, what an insert relies on.

THE m OLDEST ROWS are the case D = [0, m): pos[i] = i - m, and the device skips the columns of D in step 1 (they are dropped
anyway).  `delete_rows(range(m))` and `delete_oldest(m)` are one path here; that the two device entries agree is pinned on the
device (tests/test_gpu_dbscan_incr_delete_rows.py).
"""
from __future__ import annotations

import numpy as np

from .dbscan import FLAG_AMBIGUOUS, FLAG_NONFINITE, _check, eps_slack, tau_coefficient  # noqa: F401

NONE = np.iinfo(np.int32).max   # DB_NONE of the kernels
_BLOCK = 512                    # dirty rows per block of distances


def _flatten(parent):
    """parent[i] = root of i for every i (pointer jumping)."""
    while True:
        pp = parent[parent]
        if np.array_equal(pp, parent):
            return parent
        parent = pp


class IncrementalSpec:
    """`insert(X)` -> int64 labels of all rows seen so far (the rule at the head of this module).  `flags`: FLAG_AMBIGUOUS
    once some pair of an insert lay within tau of eps^2 (the labels then hang on rounding and are no longer pinned).
    `dirty`: per insert (|dirtyA|, |dirtyB|).  `delete_oldest(m)` -> int64 labels of the rows still held; `last_delete`: its
    (flags = 0, clusters, core rows, rows that lost core status, |R|, |B|), the info word of mused_dbscan_incr_delete.
    `delete_rows(idx)` -> the same for the rows at any distinct positions, with the same `last_delete`.
    max_rows: an insert that would leave more rows first deletes the surplus oldest ones."""

    def __init__(self, eps, min_samples, max_rows=None):
        if not (float(eps) > 0.0) or int(min_samples) < 1:
            raise ValueError("eps must be > 0 and min_samples >= 1")
        if max_rows is not None and int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1")
        self.eps, self.min_samples = float(eps), int(min_samples)
        self.max_rows = None if max_rows is None else int(max_rows)
        self.last_delete = None
        self.n, self.X = 0, None
        self.nrm = np.empty(0)
        self.count = np.empty(0, dtype=np.int64)
        self.parent = np.empty(0, dtype=np.int64)
        self.best = np.empty(0, dtype=np.int64)
        self.flags = 0
        self.dirty = []

    def _blocks(self, rows):
        """(rows of the block, d2 <= eps^2 of them against all rows [the pair (i, i) is in range by definition], |d2 - eps^2|,
        |x_i|^2 + |x_j|^2) for blocks of `rows`."""
        e2 = self.eps * self.eps
        for i0 in range(0, len(rows), _BLOCK):
            r = rows[i0:i0 + _BLOCK]
            s = self.nrm[r, None] + self.nrm[None, :]
            d2 = s - 2.0 * (self.X[r] @ self.X.T)     # the device's form
            k = np.arange(len(r))
            d2[k, r] = 0.0
            within = d2 <= e2
            d2 -= e2
            np.abs(d2, out=d2)
            d2[k, r] = np.inf
            yield r, within, d2, s

    def insert(self, X):
        X = _check(X, self.eps, self.min_samples)
        if not np.isfinite(X).all():
            self.flags |= FLAG_NONFINITE
            raise ValueError("Input contains NaN or infinity.")
        if self.X is not None and X.shape[1] != self.X.shape[1]:
            raise ValueError("every insert must have the same number of columns")
        if self.max_rows is not None:
            if X.shape[0] > self.max_rows:
                raise ValueError(f"a window of {X.shape[0]} rows is larger than max_rows = {self.max_rows}")
            if self.n + X.shape[0] > self.max_rows:
                self.delete_oldest(self.n + X.shape[0] - self.max_rows)
        n0, w = self.n, X.shape[0]
        n = self.n = n0 + w
        ms = self.min_samples
        self.X = X.copy() if self.X is None else np.concatenate([self.X, X])
        self.nrm = np.concatenate([self.nrm, np.einsum("ij,ij->i", X, X)])
        count = self.count = np.concatenate([self.count, np.zeros(w, dtype=np.int64)])
        parent = np.concatenate([self.parent, np.arange(n0, n)])
        best = self.best = np.concatenate([self.best, np.full(w, NONE, dtype=np.int64)])
        new, idx = np.arange(n0, n), np.arange(n)
        # 1 COUNT
        c, te = tau_coefficient(X.shape[1]) * 2.0 ** -52, eps_slack(self.eps)
        core_before = count >= ms
        core_before[n0:] = False
        for r, within, margin, s in self._blocks(new):
            count[r] += within.sum(axis=1)
            count[:n0] += within[:, :n0].sum(axis=0)
            if (margin <= c * s + te).any():
                self.flags |= FLAG_AMBIGUOUS
        # 2 NEWLY CORE
        parent = _flatten(parent)
        root_before = parent.copy()
        core = count >= ms
        dirty_a = np.flatnonzero(core & ~core_before)
        # 3 UNION (rounds as in dbscan.dbscan_labels: every root that sees a smaller root across an edge is hooked under the
        # smallest such one, then all paths are shortened)
        for r, within, _, _ in self._blocks(dirty_a):
            k, col = np.nonzero(within & core[None, :])
            ea, eb = r[k], col
            while True:
                pa, pb = parent[ea], parent[eb]
                diff = pa != pb
                if not diff.any():
                    break
                np.minimum.at(parent, np.maximum(pa, pb)[diff], np.minimum(pa, pb)[diff])
                parent = _flatten(parent)
        self.parent = parent
        # 4 RESOLVE
        stale = ~core & (best != NONE)
        best[stale] = parent[best[stale]]
        # 5 BORDER
        dirty_b = np.flatnonzero(core & ((parent != root_before) | ~core_before))
        if ms > 2:
            for r, within, _, _ in self._blocks(dirty_b):
                k, col = np.nonzero(within & ~core[None, :])
                np.minimum.at(best, col, parent[r[k]])
            for r, within, _, _ in self._blocks(new[~core[new]]):
                k, col = np.nonzero(within & core[None, :])
                np.minimum.at(best, r[k], parent[col])
        self.dirty.append((len(dirty_a), len(dirty_b)))
        return self._labels()

    def _labels(self):
        """6 LABELS (parent is flat)."""
        n, parent, best = self.n, self.parent, self.best
        core = self.count >= self.min_samples
        roots = np.flatnonzero(core & (parent == np.arange(n)))
        rank = np.full(n, -1, dtype=np.int64)
        rank[roots] = np.arange(len(roots))
        self.core, self.clusters = core, len(roots)
        border = ~core & (best != NONE)
        labels = np.full(n, -1, dtype=np.int64)
        labels[core] = rank[parent[core]]
        labels[border] = rank[best[border]]
        return labels

    def delete_oldest(self, m):
        """Deletes rows 0 .. m - 1 (the rule at the head of this module) -> int64 labels of the n - m rows still held."""
        n, m = self.n, int(m)
        if not 1 <= m <= n:
            raise ValueError(f"delete_oldest: m = {m} is outside [1, {n}]")
        return self._delete(np.arange(n) < m)

    def delete_rows(self, idx):
        """Deletes the rows at the distinct positions `idx` (any order; the rule at the head of this module) -> int64 labels of
        the rows still held.  `delete_rows(range(m))` leaves the state and `last_delete` of `delete_oldest(m)`."""
        n = self.n
        dele = np.asarray(idx, dtype=np.int64).reshape(-1)
        if len(dele) < 1 or dele.min() < 0 or dele.max() >= n or len(np.unique(dele)) != len(dele):
            raise ValueError(f"delete_rows: needs 1 to {n} distinct positions in [0, {n})")
        dead = np.zeros(n, dtype=bool)
        dead[dele] = True
        return self._delete(dead)

    def _delete(self, dead):
        """Steps 1-6 of the delete's rule for D = the rows marked in the bool mask `dead` (not empty)."""
        n, ms = self.n, self.min_samples
        if dead.all():
            self.n, self.X = 0, None
            self.nrm = np.empty(0)
            self.count, self.parent, self.best = (np.empty(0, dtype=np.int64) for _ in range(3))
            self.last_delete = (0, 0, 0, 0, 0, 0)
            return self._labels()
        count, best, idx = self.count, self.best, np.arange(n)
        surv = ~dead
        # 2 REMEMBER
        core_before = count >= ms
        parent = _flatten(self.parent)
        root_before = parent.copy()
        had_best = ~core_before & (best != NONE)
        best_before = np.full(n, NONE, dtype=np.int64)
        best_before[had_best] = parent[best[had_best]]
        # 1 UNCOUNT (D against all rows; the dead columns are dropped below)
        for r, within, _, _ in self._blocks(idx[dead]):
            count -= within.sum(axis=0)
        # 3 AFFECTED
        core = surv & (count >= ms)
        lost = surv & core_before & ~core
        affected = np.zeros(n, dtype=bool)
        affected[root_before[core_before & ~core]] = True      # gone and lost
        # 4 REBUILD
        in_r = core & affected[root_before]
        rows_r = np.flatnonzero(in_r)
        parent[rows_r] = rows_r
        parent[lost] = idx[lost]
        for r, within, _, _ in self._blocks(rows_r):
            k, col = np.nonzero(within & core[None, :])
            assert in_r[col].all()                             # no edge joins R to a core row outside R
            ea, eb = r[k], col
            while True:
                pa, pb = parent[ea], parent[eb]
                diff = pa != pb
                if not diff.any():
                    break
                np.minimum.at(parent, np.maximum(pa, pb)[diff], np.minimum(pa, pb)[diff])
                parent = _flatten(parent)
        # 5 BORDER
        rows_b = np.empty(0, dtype=np.int64)
        if ms > 2:
            stale = surv & had_best
            stale[stale] = affected[best_before[stale]]
            rows_b = np.flatnonzero(lost | stale)
            best[rows_b] = NONE
            for r, within, _, _ in self._blocks(rows_b):
                k, col = np.nonzero(within & core[None, :])
                np.minimum.at(best, r[k], parent[col])
        # 6 COMPACT: survivor i becomes pos[i] = i - |{ j in D : j < i }|, an order-preserving map
        best[core] = NONE
        pos = np.cumsum(surv) - 1
        self.n, self.X, self.nrm, self.count = int(surv.sum()), self.X[surv], self.nrm[surv], count[surv]
        self.parent = pos[parent[surv]]
        bs = best[surv]
        self.best = np.where(bs == NONE, NONE, pos[np.minimum(bs, n - 1)])
        labels = self._labels()
        self.last_delete = (0, self.clusters, int(core.sum()), int(lost.sum()), len(rows_r), len(rows_b))
        return labels
