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
    `dirty`: per insert (|dirtyA|, |dirtyB|)."""

    def __init__(self, eps, min_samples):
        if not (float(eps) > 0.0) or int(min_samples) < 1:
            raise ValueError("eps must be > 0 and min_samples >= 1")
        self.eps, self.min_samples = float(eps), int(min_samples)
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
        # 6 LABELS
        roots = np.flatnonzero(core & (parent == idx))
        rank = np.full(n, -1, dtype=np.int64)
        rank[roots] = np.arange(len(roots))
        self.core, self.clusters = core, len(roots)
        border = ~core & (best != NONE)
        labels = np.full(n, -1, dtype=np.int64)
        labels[core] = rank[parent[core]]
        labels[border] = rank[best[border]]
        return labels
