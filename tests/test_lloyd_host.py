"""No GPU: the high-precision Lloyd reference of tests/lloyd_cases.py against scikit-learn's KMeans on every case the
device test compares with it, the margins that make that comparison exact, and the coverage the case table promises."""
import os
import warnings

import numpy as np
import pytest

import lloyd_cases as lc

IDS = [c.name for c in lc.EXACT]


def sklearn_fit(c):
    from sklearn.cluster import KMeans
    from sklearn.exceptions import ConvergenceWarning

    X, mean, C0, _ = lc.inputs(c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)   # the max_iter cases stop before they converge
        return KMeans(n_clusters=c.k, init=C0 + mean, n_init=1, max_iter=c.max_iter, tol=lc.relative_tolerance(c)).fit(X)


@pytest.mark.parametrize("c", lc.EXACT, ids=IDS)
def test_reference_is_sklearns_lloyd(c):
    r = lc.reference(c)
    km = sklearn_fit(c)
    assert r.empty == 0
    assert km.n_iter_ == r.iters
    assert np.array_equal(km.labels_, r.labels)
    X, mean, _, _ = lc.inputs(c)
    # scikit-learn's centres: fp64 sums of at most n rows in its own order, shifted back by the mean
    bound = (c.n + 8) * 2.0 ** -52 * np.abs(X).max()
    assert float(np.abs((km.cluster_centers_ - mean) - r.centers).max()) <= bound


@pytest.mark.parametrize("c", lc.EXACT, ids=IDS)
def test_margins_keep_the_comparison_exact(c):
    r = lc.reference(c)
    print(f"{c.name}: iterations {r.iters} code {r.code} e_margin {r.e_margin:.3g} s_margin {r.s_margin:.3g}")
    assert r.e_margin >= lc.E_MARGIN_MIN
    assert r.s_margin >= lc.S_MARGIN_MIN


def test_table_reaches_every_kernel_and_batch_position():
    assert {c.rows for c in lc.TABLE} == {64, 32, 16, 0}
    assert sum(1 for c in lc.TABLE if c.ld) == 1 and all(c.ld == c.d + 3 for c in lc.TABLE if c.ld)
    iters = [lc.reference(c).iters for c in lc.TABLE]
    # the host queues four iterations between two reads of the stopping flag
    assert any(i % 4 == 0 for i in iters) and any(i % 4 == 1 for i in iters) and any(i > 8 for i in iters)
    assert 4 in iters and 5 in iters
    codes = {lc.reference(c).code for c in lc.TABLE}
    assert codes == {1, 2}
    for c in lc.TABLE:
        if c.name.startswith("k_is_n"):
            r = lc.reference(c)
            assert (r.iters, r.code) == (1, 2) and r.shifts[0] <= 1e-30


def test_selection_formula_names_the_tables_kernels():
    """mused_kmeans_assign_rows needs no device: the kernel each case is listed under is the one the library picks."""
    from mused_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    L = _lib.lib()
    for c in lc.EXACT + lc.EMPTY:
        assert L.mused_kmeans_assign_rows(c.d, c.k) == c.rows, c.name
    assert L.mused_kmeans_assign_rows(8193, 1) == -1 and L.mused_kmeans_assign_rows(1, 1025) == -1


def test_max_iter_cases_stop_early_with_other_labels():
    free = lc.reference(lc._BASE)
    assert (free.iters, free.code) == (8, 1)
    for c in lc.MAX_ITER:
        r = lc.reference(c)
        if c.max_iter < free.iters:
            assert (r.iters, r.code) == (c.max_iter, 0)
            if c.max_iter <= 5:   # the final E step matters: it moves rows, and the result is not yet the converged one
                assert np.count_nonzero(r.history[-1] != r.history[-2]) > 0
                assert np.count_nonzero(r.labels != free.labels) > 0
        else:
            assert (r.iters, r.code) == (free.iters, 1) and np.array_equal(r.labels, free.labels)


def test_forced_tolerance_stops_on_the_shift():
    r = lc.reference(lc.FORCED_TOL)
    assert (r.iters, r.code) == (lc.FORCED_TOL_ITER, 2)
    assert np.count_nonzero(r.history[-1] != r.history[-2]) > 0, "the last E step must change labels"


@pytest.mark.parametrize("c", lc.EMPTY, ids=[c.name for c in lc.EMPTY])
def test_empty_cases_raise_the_flag(c):
    r = lc.reference(c)
    assert r.empty == 1
    k_used = len(np.unique(r.history[0]))
    assert k_used < c.k, "the first M step already meets a cluster without rows"
