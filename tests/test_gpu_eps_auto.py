"""eps="auto" on the public side: matrix_operations.select_eps_on_device / kth_neighbor_distances_on_device,
perform_dbscan_clustering_on_device(eps="auto"), IncrementalDBSCAN(eps="auto") and the two pipeline entries.  The eps that is
chosen must be one the device DBSCAN can USE: scikit-learn's labels at that eps, and no fallback to the host -- which is what
an eps taken from the curve itself (the distance of a pair) fails on every input."""
import numpy as np
import pytest

import kdist_cases as kc
from mused_amd import kdist

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IDX = list(range(len(kc.BLOBS)))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _eps_tolerance(X, k):
    """How far the device's eps may lie from the rule's when their k-distances differ in the last bits but the knee is the
    same: the sorted curves of kd2 differ rank by rank by at most B = max kd2_bound, a root v >= v_knee > 0 of them by at most
    B / v_knee (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b)), and eps is the mean of two such roots."""
    kd2 = kdist.kth_sq_distances(X, k)
    v = np.sort(np.sqrt(kd2))
    return kdist.kd2_bound(X, kd2).max() / v[kdist.knee(v)[0]]


@pytest.mark.parametrize("i", IDX, ids=kc.BLOB_IDS)
def test_dbscan_auto_gives_sklearns_labels_without_fallback(i, monkeypatch):
    from sklearn.cluster import DBSCAN

    from mused_amd import matrix_operations as mo

    X, k = kc.blob_input(i)

    def no_host(*a, **kw):
        raise AssertionError("eps='auto' sent the call to the host DBSCAN")

    monkeypatch.setattr(mo, "perform_dbscan_clustering", no_host)
    before = mo.dbscan_fallbacks
    labels = mo.perform_dbscan_clustering_on_device(np.array(X), "auto", k)
    eps = mo.last_chosen_eps
    assert mo.dbscan_fallbacks == before          # fails for an eps ON the curve: that is the distance of a pair
    assert isinstance(eps, float) and labels.dtype == np.int64
    assert np.array_equal(labels, DBSCAN(eps=eps, min_samples=k).fit_predict(X))
    if i < len(kc.PLANTED):
        assert labels.max() + 1 == kc.PLANTED[i]
    # the same from a device tensor, and the chosen eps next to the rule's
    eps_d, info = mo.select_eps_on_device(torch.tensor(X, device="cuda"), k)
    assert eps_d == eps and info["v_knee"] < eps < info["v_next"] and info["next"] > info["knee"]
    curve = info["curve"]
    assert curve.is_cuda and curve.dtype == torch.float64 and tuple(curve.shape) == (len(X),)
    v = curve.cpu().numpy()
    assert (np.diff(v) >= 0).all() and v[info["knee"]] == info["v_knee"] and v[info["next"]] == info["v_next"]
    assert (info["knee"], info["next"]) == kdist.knee(v) and eps == kdist.eps_from_curve(v)
    want, knee = kdist.select_eps(X, k)[:2]
    print(f"{kc.BLOB_IDS[i]}: device eps {eps!r}, rule {want!r}, knee {info['knee']} / {knee}")
    assert info["knee"] == knee and abs(eps - want) <= _eps_tolerance(X, k)


def test_kth_neighbor_distances_on_device():
    from mused_amd import matrix_operations as mo

    X, k = kc.blob_input(4)
    _, ref, bound = kc.blob_reference(4)
    for arg in (np.array(X), torch.tensor(X, device="cuda")):
        got = mo.kth_neighbor_distances_on_device(arg, k, stream=torch.cuda.Stream())
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (len(X),)
        assert (np.abs(got.cpu().numpy() ** 2 - ref) <= bound + 4 * np.spacing(ref)).all()   # (the root squared again: 4 ulp more)


@pytest.mark.parametrize("max_rows", [None, 1000], ids=["growing", "sliding_1000"])
def test_incremental_auto_fixes_eps_at_the_first_insert(max_rows):
    from sklearn.cluster import DBSCAN

    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    X, k = kc.blob_input(1)                        # 2,000 x 50, k = 5: 3 windows of 500 rows
    before = mo.dbscan_incr_fallbacks
    inc = IncrementalDBSCAN("auto", k, max_rows=max_rows)
    assert inc.eps_ is None
    want = mo.select_eps_on_device(np.array(X[:500]), k)[0]
    rule, knee = kdist.select_eps(X[:500], k)[:2]
    for t in range(3):
        W = X[500 * t:500 * (t + 1)]
        inc.insert(np.array(W))
        assert inc.eps_ == want == inc.eps         # chosen from window 0, then fixed
        held = X[:500 * (t + 1)] if max_rows is None else X[max(0, 500 * (t + 1) - max_rows):500 * (t + 1)]
        assert np.array_equal(inc.labels(), DBSCAN(eps=inc.eps_, min_samples=k).fit_predict(held))
    assert mo.dbscan_incr_fallbacks == before
    assert abs(want - rule) <= _eps_tolerance(X[:500], k)


def test_incremental_auto_errors_leave_no_eps():
    from mused_amd.incdbscan import IncrementalDBSCAN

    X = kc.gaussian(200, 4, 50)
    inc = IncrementalDBSCAN("auto", 1)
    with pytest.raises(ValueError, match="flat"):
        inc.insert(X)                               # min_pts = 1: the curve of zeros
    assert inc.eps_ is None and inc.n == 0
    inc = IncrementalDBSCAN("auto", 3)
    with pytest.raises(ValueError, match="flat"):
        inc.insert(np.ones((50, 4)))
    with pytest.raises(ValueError):
        IncrementalDBSCAN("auto", 65).insert(X)     # beyond the kernel's k
    with pytest.raises(ValueError):
        IncrementalDBSCAN("auto", 5).insert(X[:4])  # fewer rows than min_pts
    inc.insert(X)                                   # a failed first insert does not spoil the object
    assert inc.eps_ > 0 and inc.n == 200


def test_batch_pipeline_auto():
    from mused_amd import matrix_operations as mo
    from mused_amd import synth
    from mused_amd.pipeline import process_batch_data

    X, labels = synth.blob_stream(600, 16, 0, n_centres=4)
    mods = [X.astype(np.float64)]

    def go(eps):
        return process_batch_data({}, mods, [""], 8, 5, 4, 0, "DBSCAN_batch", labels, 0.0, "all", False, eps, 3, 3, 600)

    before = mo.dbscan_fallbacks
    auto = go("auto")
    eps = auto["chosen_eps"]
    assert isinstance(eps, float) and eps > 0 and mo.dbscan_fallbacks == before
    fixed = go(eps)
    assert "chosen_eps" not in fixed
    assert np.array_equal(auto["all_clusters"], fixed["all_clusters"])
    other = process_batch_data({}, mods, [""], 8, 5, 4, 0, "SVDMC_batch", labels, 0.0, "all", False, "auto", 3, 3, 600)
    assert "chosen_eps" not in other                # the other approaches ignore eps as before


def test_streaming_pipeline_auto():
    from mused_amd import matrix_operations as mo
    from mused_amd import synth
    from mused_amd.pipeline import process_streaming_data

    W = 256
    X, labels = synth.blob_stream(3 * W, 16, 0, n_centres=4)
    mods = [X.astype(np.float64)]

    def go(eps, approach="DBSCAN_incr"):
        return process_streaming_data({}, mods, [""], W, 8, 5, 4, 0, approach, labels, 1, 0.0, "types", False, eps, 3)

    before = mo.dbscan_incr_fallbacks
    auto = go("auto")
    eps = auto["chosen_eps"]
    assert isinstance(eps, float) and eps > 0 and mo.dbscan_incr_fallbacks == before
    fixed = go(eps)
    assert "chosen_eps" not in fixed
    assert len(auto["all_clusters"]) == 3 * W and np.array_equal(auto["all_clusters"], fixed["all_clusters"])
    assert "chosen_eps" not in go("auto", "sSVDMC")


@pytest.mark.parametrize("name", ["two_point_blobs_k2", "ramp_n1000_k8", "n300_d1_k64", "n2000_d50_k2_blobs"])
def test_host_switch_agrees_with_the_device(name, monkeypatch):
    """MUSED_KDIST=host runs the NumPy rule.  Where the device's kd2 equals the rule's (the exact inputs do) eps has the same
    bits; otherwise the knee is the same and eps agrees within the bound."""
    from mused_amd import matrix_operations as mo

    c = kc.case(name)
    X = np.array(c.X)
    eps_d, info_d = mo.select_eps_on_device(X, c.k)
    dist_d = mo.kth_neighbor_distances_on_device(X, c.k).cpu().numpy()
    monkeypatch.setenv("MUSED_KDIST", "host")
    eps_h, info_h = mo.select_eps_on_device(X, c.k)
    dist_h = mo.kth_neighbor_distances_on_device(X, c.k).cpu().numpy()
    assert eps_h == kdist.select_eps(X, c.k)[0] and info_h["curve"].is_cuda
    assert dist_h.tobytes() == np.sqrt(c.rule).tobytes()
    same = dist_d.tobytes() == dist_h.tobytes()
    print(f"{name}: device kd2 {'equals' if same else 'differs from'} the rule's; eps {eps_d!r} / {eps_h!r}")
    if name in ("two_point_blobs_k2", "ramp_n1000_k8"):
        assert same                                 # exact arithmetic: nothing to differ about
    if same:
        plain = [{k: v for k, v in info.items() if k != "curve"} for info in (info_d, info_h)]
        assert eps_d == eps_h and plain[0] == plain[1]
        assert info_d["curve"].cpu().numpy().tobytes() == info_h["curve"].cpu().numpy().tobytes()
    else:
        assert info_d["knee"] == info_h["knee"] and abs(eps_d - eps_h) <= _eps_tolerance(X, c.k)


def test_errors():
    from mused_amd import matrix_operations as mo

    X = kc.gaussian(300, 4, 51)
    with pytest.raises(ValueError, match="flat"):
        mo.perform_dbscan_clustering_on_device(X, "auto", 1)      # every row is its own nearest row
    with pytest.raises(ValueError, match="flat"):
        mo.select_eps_on_device(np.ones((100, 3)), 4)
    with pytest.raises(ValueError, match="auto"):
        mo.perform_dbscan_clustering_on_device(X, "knee", 3)
    for k in (0, 65, 301, 2.0, True):
        with pytest.raises(ValueError):
            mo.select_eps_on_device(X, k)
        with pytest.raises(ValueError):
            mo.kth_neighbor_distances_on_device(X[:40] if k == 301 else X, 41 if k == 301 else k)
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[7, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            mo.select_eps_on_device(Y, 3)
        with pytest.raises(ValueError, match="NaN or infinity"):
            mo.kth_neighbor_distances_on_device(torch.tensor(Y, device="cuda"), 3)
    with pytest.raises(ValueError):
        mo.select_eps_on_device(X[0], 1)
