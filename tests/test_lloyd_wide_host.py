"""No GPU: the cases of tests/lloyd_wide_cases.py (k * d > 8192) -- the high-precision Lloyd reference against
scikit-learn's KMeans, the margins that make the device comparison exact, no empty cluster, and what the library answers
without a device: the workspace size and the tiles of mused_kmeans_lloyd_wide."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import lloyd_cases as lc
import lloyd_wide_cases as lw

IDS = [c.name for c in lw.EXACT]


def sklearn_fit(c):
    from sklearn.cluster import KMeans
    from sklearn.exceptions import ConvergenceWarning

    X, mean, C0, _ = lc.inputs(c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)   # the max_iter cases stop before they converge
        return KMeans(n_clusters=c.k, init=C0 + mean, n_init=1, max_iter=c.max_iter, tol=lc.relative_tolerance(c)).fit(X)


def library():
    from mused_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.lib()


@pytest.mark.parametrize("c", lw.EXACT, ids=IDS)
def test_reference_is_sklearns_lloyd(c):
    r = lc.reference(c)
    km = sklearn_fit(c)
    assert r.empty == 0, "a cluster ran empty"
    assert km.n_iter_ == r.iters
    assert np.array_equal(km.labels_, r.labels)
    X, mean, _, _ = lc.inputs(c)
    # scikit-learn's centres: fp64 sums of at most n rows in its own order, shifted back by the mean
    bound = (c.n + 8) * 2.0 ** -52 * np.abs(X).max()
    assert float(np.abs((km.cluster_centers_ - mean) - r.centers).max()) <= bound


@pytest.mark.parametrize("c", lw.EXACT, ids=IDS)
def test_margins_keep_the_comparison_exact(c):
    r = lc.reference(c)
    print(f"{c.name}: iterations {r.iters} code {r.code} e_margin {r.e_margin:.3g} s_margin {r.s_margin:.3g}")
    assert r.e_margin >= lc.E_MARGIN_MIN
    assert r.s_margin >= lc.S_MARGIN_MIN


def test_table_is_past_the_old_limit_and_at_the_new_ones():
    assert all(c.k * c.d > 8192 and c.k <= lw.K_MAX and c.d <= lw.D_MAX for c in lw.EXACT)
    assert min(c.k * c.d for c in lw.TABLE) == 8194
    assert any(c.k == lw.K_MAX and c.d == lw.D_MAX for c in lw.TABLE)
    assert sum(1 for c in lw.TABLE if c.ld) == 1 and all(c.ld == c.d + 3 for c in lw.TABLE if c.ld)
    assert {c.n % 256 for c in lw.TABLE} >= {1, 44}     # a chunk of one row, a short last chunk
    iters = [lc.reference(c).iters for c in lw.TABLE]
    # the host queues four iterations between two reads of the stopping flag
    assert any(i % 4 == 1 for i in iters) and any(i % 4 == 2 for i in iters) and any(i > 8 for i in iters)
    assert all(lc.reference(c).code == 1 for c in lw.TABLE)


def test_max_iter_cases_stop_early_with_other_labels():
    free = lc.reference(lw._BASE)
    assert (free.iters, free.code) == (lw.FREE_ITERS, 1)
    for c in lw.MAX_ITER:
        r = lc.reference(c)
        assert (r.iters, r.code) == (c.max_iter, 0)
        # the final E step matters: it moves rows, and the result is not yet the converged one
        assert np.count_nonzero(r.history[-1] != r.history[-2]) > 0
        assert np.count_nonzero(r.labels != free.labels) > 0


def test_forced_tolerance_stops_on_the_shift():
    r = lc.reference(lw.FORCED_TOL)
    assert (r.iters, r.code) == (lw.FORCED_TOL_ITER, 2)
    assert np.count_nonzero(r.history[-1] != r.history[-2]) > 0, "the last E step must change labels"


def test_empty_case_raises_the_flag():
    r = lc.reference(lw.EMPTY)
    assert r.empty == 1
    assert len(np.unique(r.history[0])) < lw.EMPTY.k, "the first M step already meets a cluster without rows"


def test_every_case_has_tiles_that_fit():
    """mused_kmeans_wide_tiles needs no device.  E step: (TR + KT) rows of pitch d + 1; 256 / TR lanes share a row and take a
    centre each, so a tile that is not all of k holds a multiple of them.  M-step partials: k x DT sums and 256 labels."""
    L = library()
    shapes = {(c.d, c.k) for c in lw.EXACT + [lw.EMPTY] + lc.EXACT} | {(512, 1024), (1, 1), (512, 1), (1, 1024), (100, 150)}
    for d, k in sorted(shapes):
        out = (C.c_int * 3)(-1, -1, -1)
        assert L.mused_kmeans_wide_tiles(d, k, out) == 0, (d, k)
        tr, kt, dt = out
        assert tr in (32, 16) and 1 <= kt <= k and dt in (64, 32, 16), (d, k, tr, kt, dt)
        assert kt == k or kt % (256 // tr) == 0, (d, k, tr, kt)
        assert 8 * (tr + kt) * (d + 1) <= lw.LDS_MAX, (d, k, tr, kt)
        assert 8 * k * dt + 1040 <= lw.LDS_MAX, (d, k, dt)
    out = (C.c_int * 3)()
    assert L.mused_kmeans_wide_tiles(512, 1024, out) == 0 and out[1] < 1024, "k = 1024 goes through more than one tile"


def test_limits_are_rejected_without_a_device():
    L = library()
    out = (C.c_int * 3)(-1, -1, -1)
    for d, k in [(16, 1025), (513, 17), (0, 4), (4, 0)]:
        assert L.mused_kmeans_wide_tiles(d, k, out) == -1, (d, k)
        assert b"mused_kmeans_wide_tiles" in L.mused_last_error()
    assert list(out) == [-1, -1, -1]
    for n, d, k in [(2000, 16, 1025), (300, 513, 17), (16, 600, 17), (0, 4, 1), (4, 0, 1), (4, 4, 0)]:
        assert L.mused_kmeans_wide_ws_bytes(n, d, k) == -1, (n, d, k)
    for c in lw.EXACT + lc.EXACT:
        nchunk = (c.n + 255) // 256
        need = 8 * c.n * c.d + 8 * nchunk * c.k * c.d + 8 * c.k * c.d + 4 * nchunk * c.k + 8 * c.k + 8 * c.n
        assert need < L.mused_kmeans_wide_ws_bytes(c.n, c.d, c.k) <= need + 4096, c.name
    # the narrow entry keeps its own limit
    assert L.mused_kmeans_assign_rows(482, 17) == -1 and L.mused_kmeans_ws_bytes(300, 482, 17) > 0
