"""mused_amd/kdist.py (the NumPy rule csrc/kdist.hip implements) against scikit-learn's NearestNeighbors within kd2_bound, the
knee and the midpoint eps on the six blob-plus-noise inputs of tests/kdist_cases.py (the eps is usable by the device DBSCAN,
the curve's own value at the knee is not), the rule's properties, and the argument errors of the public side that need no
GPU."""
import numpy as np
import pytest

import kdist_cases as kc
from mused_amd import dbscan, kdist

IDX = list(range(len(kc.BLOBS)))


@pytest.mark.parametrize("i", IDX, ids=kc.BLOB_IDS)
def test_rule_against_sklearn_within_the_bound(i):
    kd2, ref, bound = kc.blob_reference(i)
    ratio = np.abs(kd2 - ref) / bound
    print(f"{kc.BLOB_IDS[i]}: largest |rule - sklearn| / bound = {ratio.max():.4f}")
    assert (kd2 >= 0).all() and (np.abs(kd2 - ref) <= bound).all()


@pytest.mark.parametrize("i", IDX, ids=kc.BLOB_IDS)
def test_knee_is_the_same_from_sklearns_distances(i):
    kd2, ref, _ = kc.blob_reference(i)
    assert kdist.knee(np.sort(np.sqrt(kd2)))[0] == kdist.knee(np.sort(np.sqrt(ref)))[0]


@pytest.mark.parametrize("i", IDX, ids=kc.BLOB_IDS)
def test_midpoint_eps_is_usable_and_the_curve_value_is_not(i):
    X, k = kc.blob_input(i)
    eps, knee, nxt, v_knee, v_nxt = kdist.select_eps(X, k)
    v = np.sort(np.sqrt(kc.blob_reference(i)[0]))
    assert (knee, nxt) == kdist.knee(v) and v_knee == v[knee] and v_nxt == v[nxt] and eps == kdist.eps_from_curve(v)
    assert v_knee < eps < v_nxt and nxt > knee
    mid = dbscan.Scan(X, eps)
    print(f"{kc.BLOB_IDS[i]}: eps {eps!r}, margin / tau {mid.margin / mid.tau:.3e}")
    assert not mid.ambiguous
    assert dbscan.Scan(X, v_knee).ambiguous     # a k-distance IS the distance of a pair: mused_dbscan would fall back


@pytest.mark.parametrize("i", IDX[:5], ids=kc.BLOB_IDS[:5])
def test_dbscan_at_that_eps_finds_the_planted_clusters(i):
    from sklearn.cluster import DBSCAN

    X, k = kc.blob_input(i)
    labels = DBSCAN(eps=kdist.select_eps(X, k)[0], min_samples=k).fit_predict(X)
    assert labels.max() + 1 == kc.PLANTED[i]
    assert np.array_equal(dbscan.dbscan_labels(X, kdist.select_eps(X, k)[0], k), labels)


def test_first_argmax_on_a_plateau():
    # g = x - y: 0, 0.25, 0.25, 0.25, 0 -- three equal maxima (exact in binary), the first one counts
    v = np.array([0.0, 0.0, 1.0, 2.0, 4.0])
    x, y = np.arange(5) / 4.0, v / 4.0
    assert list(x - y) == [0.0, 0.25, 0.25, 0.25, 0.0]
    assert kdist.knee(v) == (1, 2)
    assert kdist.eps_from_curve(v) == 0.5
    # the value at the knee repeats behind it: nxt skips the repeats
    v = np.array([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 16.0])
    i, nxt = kdist.knee(v)
    assert (i, nxt) == (7, 8)
    v = np.array([0.0, 0.0, 0.0, 0.0, 5.0, 5.0])
    assert kdist.knee(v) == (3, 4) and kdist.eps_from_curve(v) == 2.5
    assert kdist.knee(np.array([1.0, 2.0])) == (0, 1)


def test_duplicate_rows_give_zeros():
    X = kc.two_point_blobs()
    kd2 = kdist.kth_sq_distances(X, 2)
    assert (kd2 == 0.0).sum() == 150 and (kd2 == 0.015625).sum() == 150
    assert (np.abs(kd2 - kc.sklearn_kd2(X, 2)) <= kdist.kd2_bound(X, kd2)).all()
    eps, knee, nxt, a, b = kdist.select_eps(X, 2)
    assert (a, b, eps) == (0.0, 0.125, 0.0625) and (knee, nxt) == (149, 150)   # g grows along the zeros
    assert (kdist.kth_sq_distances(X, 1) == 0.0).all()


def test_k_equal_to_n():
    X = kc.gaussian(37, 4, 3)
    kd2 = kdist.kth_sq_distances(X, 37)
    far = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1).max(axis=1)
    assert (np.abs(kd2 - far) <= kdist.kd2_bound(X, kd2)).all()
    assert (np.abs(kd2 - kc.sklearn_kd2(X, 37)) <= kdist.kd2_bound(X, kd2)).all()


def test_flat_curves_raise():
    X = kc.gaussian(50, 3, 1)
    with pytest.raises(ValueError, match="flat"):
        kdist.select_eps(X, 1)                       # every row is its own nearest row: all zeros
    with pytest.raises(ValueError, match="flat"):
        kdist.select_eps(np.ones((20, 4)), 3)        # all rows equal
    with pytest.raises(ValueError, match="flat"):
        kdist.knee(np.array([2.0, 2.0, 2.0]))
    with pytest.raises(ValueError, match="flat"):
        kdist.knee(np.array([2.0]))


def test_argument_errors():
    X = kc.gaussian(10, 2, 0)
    for k in (0, 11, -1, 2.5, True):
        with pytest.raises(ValueError):
            kdist.kth_sq_distances(X, k)
    with pytest.raises(ValueError):
        kdist.kth_sq_distances(X[0], 1)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        kdist.kth_sq_distances(bad, 2)
    with pytest.raises(ValueError, match="ascending"):
        kdist.knee(np.array([0.0, 2.0, 1.0]))
    with pytest.raises(ValueError):
        kdist.knee(np.array([0.0, np.inf]))
    with pytest.raises(ValueError):
        kdist.knee(np.zeros((2, 2)))


def test_public_side_refuses_without_touching_the_device():
    """What the public functions reject before any launch."""
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    assert mo.last_chosen_eps is None or isinstance(mo.last_chosen_eps, float)
    with pytest.raises(ValueError, match="auto"):
        mo.perform_dbscan_incr_clustering(kc.gaussian(10, 2, 0), None, None, eps="auto", min_samples=2)
    with pytest.raises(ValueError, match="auto"):
        IncrementalDBSCAN(eps="knee", min_pts=3)
    with pytest.raises(ValueError):
        IncrementalDBSCAN(eps="auto", min_pts=0)
    inc = IncrementalDBSCAN(eps="auto", min_pts=3)
    assert inc.eps_ is None and inc.eps is None
    with pytest.raises(ValueError):
        inc.insert(np.empty((0, 3)))                 # an empty first insert
    assert inc.eps_ is None
    assert IncrementalDBSCAN(eps=0.5, min_pts=3).eps_ == 0.5


def test_host_switch_runs_the_numpy_rule(monkeypatch):
    """MUSED_KDIST=host needs no kernel: the rule's eps, bit for bit (the upload of the curve needs a GPU, so this part is
    checked through the module's own pieces)."""
    from mused_amd import matrix_operations as mo

    monkeypatch.setenv("MUSED_KDIST", "host")
    assert mo._kdist_host()
    monkeypatch.setenv("MUSED_KDIST", "device")
    assert not mo._kdist_host()
