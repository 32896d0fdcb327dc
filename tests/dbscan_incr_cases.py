"""Streams shared by tests/test_dbscan_incr_host.py and tests/test_gpu_dbscan_incr.py: (name, [batch, ...], eps, min_samples).

The hand-built ones live in 5 dimensions with eps = 1.05 and min_samples = 4.  A CELL at x is a centre (x, 0, 0, 0, 0) with
three satellites at distance 1 along axes 1, 2, 3: the centre has 4 rows within eps and is core, a satellite has 2 and is
not (satellites are sqrt(2) apart).  Centres 2 apart do not see each other; a LINK row half way between two centres sees
both (3 rows within eps: a border row of both) and turns core as soon as an ACTIVATOR, the link moved by 1 along axis 4,
arrives -- the activator sees the link alone.  Every distance is 0, 1, sqrt(2) or >= 2: far from eps."""
import numpy as np

EPS, MS, D = 1.05, 4, 5


def _e(k):
    v = np.zeros(D)
    v[k] = 1.0
    return v


def cell(x):
    c = np.zeros(D)
    c[0] = x
    return [c, c + _e(1), c + _e(2), c + _e(3)]


def link(x):
    c = np.zeros(D)
    c[0] = x
    return c


def activator(x):
    return link(x) + _e(4)


def far(j):
    """Noise row j: 3 apart from every other one, far from every cell."""
    v = np.zeros(D)
    v[0] = 1000.0 + 3.0 * j
    return v


def _b(rows):
    return np.array(rows, dtype=np.float64).reshape(-1, D)


def hand_cases():
    out = []
    # (a) rows 0-3, 4-7: two cells; row 8 their link (a border row).  The insert is the link's activator: row 8, an OLD row,
    # turns core and joins the two clusters; the new row itself is not core
    out.append(("a_old_row_turns_core_and_joins", [_b(cell(0) + cell(2) + [link(1)]), _b([activator(1)])], EPS, MS))
    # (b) cell Z (root 0) at x = 4, a noise row, cell P (root 5) at 0, cell Q (root 9) at 2, row 13 the link of P and Q (best
    # = 5), row 14 the link of Q and Z.  The activator of row 14 merges Q under root 0 < 5: row 13 gains no neighbour and must
    # move from P's label to the merged cluster's
    out.append(("b_border_row_follows_a_merge",
                [_b(cell(4) + [far(0)] + cell(0) + cell(2) + [link(1), link(3)]), _b([activator(3)])], EPS, MS))
    # (c) rows 0-2: a centre with two satellites (3 within eps: noise), then two cells (clusters 0 and 1).  The third
    # satellite arrives: row 0 founds a cluster with the smallest index and every number shifts
    out.append(("c_old_row_founds_the_first_cluster", [_b(cell(-10)[:3] + cell(0) + cell(2)), _b([cell(-10)[3]])], EPS, MS))
    # (d) three cells; one insert brings both links and their activators: one cluster
    out.append(("d_three_clusters_chained", [_b(cell(0) + cell(2) + cell(4)),
                                            _b([link(1), activator(1), link(3), activator(3)])], EPS, MS))
    # (e) an insert of pure noise between two ordinary ones
    out.append(("e_noise_insert", [_b(cell(0) + [link(1)]), _b([far(j) for j in range(5)]), _b(cell(2))], EPS, MS))
    # (f) the insert repeats earlier rows: satellites turn core through their copies, the link through its own
    first = cell(0) + cell(2) + [link(1)]
    out.append(("f_duplicates", [_b(first), _b([first[1], first[8], first[5], first[1]])], EPS, MS))
    # (g) min_samples 1 and 2 (the reference's value): no border rows
    rng = np.random.default_rng(5)
    R = rng.standard_normal((90, 3))
    for ms in (1, 2):
        out.append((f"g_min_samples_{ms}", [R[:30], R[30:31], R[31:90]], 0.8, ms))
        out.append((f"g_cells_min_samples_{ms}", [_b(cell(0) + cell(2) + [link(1)]), _b([activator(1), far(0)])], EPS, ms))
    return out


def spread(batches, gap):
    """The same stream with `gap` far noise rows behind every row, so that rows that interact lie in different 128-row tiles
    (the noise rows see nothing; the order of the others is kept)."""
    out, j = [], 0
    for b in batches:
        d = b.shape[1]
        rows = []
        for r in b:
            rows.append(r)
            for _ in range(gap):
                v = np.zeros(d)
                v[0] = 1000.0 + 3.0 * j
                j += 1
                rows.append(v)
        out.append(np.array(rows).reshape(-1, d))
    return out


def random_streams():
    """Blobs plus noise in 1-5 dimensions, cut into uneven inserts."""
    out = []
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        d, ms = 1 + seed % 5, 1 + seed % 6
        n = 120
        cen = 4.0 * rng.standard_normal((4, d))
        X = cen[rng.integers(0, 4, n)] + 0.5 * rng.standard_normal((n, d))
        noise = rng.random(n) < 0.2
        X[noise] = 8.0 * rng.standard_normal((int(noise.sum()), d))
        cuts = np.sort(rng.choice(np.arange(1, n), 4, replace=False))
        out.append((f"random_s{seed}_d{d}_m{ms}", np.split(X, cuts), 0.9, ms))
    return out


def split_case(X, cuts):
    """X cut at the distinct cut points that lie inside (0, n)."""
    cuts = sorted({c for c in cuts if 0 < c < len(X)})
    return np.split(X, cuts)


def refit(prefix, eps, ms):
    from sklearn.cluster import DBSCAN

    m = DBSCAN(eps=eps, min_samples=ms, metric="euclidean").fit(prefix)
    return m.labels_.astype(np.int64), len(m.core_sample_indices_)
