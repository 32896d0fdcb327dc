"""Scoring a run on the device (csrc/score.hip): every label pair of tests/metrics_cases.py through the C entry and through
compute_all_metrics against the recorded values of the reference's own compute_all_metrics, without a host fallback.

Tolerance: as derived in tests/test_scores_host.py -- |device - reference| <= 1e-12 for f1, nmi, nmi_e, precision and
recall; accuracy and MAE equal.  The integers the kernel reports (T, P, union, event rows, agreeing rows) are exact."""
import contextlib
import io

import numpy as np
import pytest

import metrics_cases as mc
from conftest import load_golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-12
VARIABLES = (1234, 0.95, "binary", False, 10, 50, 2000)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("metrics_cases")
    assert [str(x) for x in g["names"]] == mc.CASE_NAMES
    return g


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    monkeypatch.delenv("MUSED_SCORE", raising=False)


def check_seven(got, want, what):
    got, want = [float(x) for x in got], [float(x) for x in want]
    for i, key in enumerate(mc.KEYS):
        print(f"{what} {key}: got {got[i]!r} want {want[i]!r} diff {abs(got[i] - want[i]):.3e}")
    for i, key in enumerate(mc.KEYS):
        if key in ("accuracy", "mae"):
            assert got[i] == want[i], (what, key, got[i], want[i])
        else:
            assert abs(got[i] - want[i]) <= TOL, (what, key, got[i], want[i])


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def entry(true, pred, cells_cap=1 << 22):
    from mused_amd import metrics_evaluation as me

    return me.score_labels_on_device(dev32(true), dev32(pred), cells_cap)


def quiet_metrics(me, pred, true):
    results, _ = me.get_initial_results()
    with contextlib.redirect_stdout(io.StringIO()) as log:
        me.compute_all_metrics(results, *VARIABLES, pred, true, 3_500_000_000, 1_000_000_000)
    return results, log.getvalue()


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_c_entry_matches_the_reference_fixture(golden, name):
    from mused_amd import metrics_evaluation as me
    from mused_amd import scores

    true, pred = mc.case(name)
    assert mc.digest(true, pred) == str(golden[f"{name}__digest"])
    before = me.score_fallbacks
    out, info = entry(true, pred)
    assert me.score_fallbacks == before
    assert out.shape == (1, 8) and info.shape == (1, 8)
    assert tuple(info[0, :5]) == scores.table_info(*scores.contingency(true, pred)) and not info[0, 5:].any()
    check_seven(out[0, :7], golden[f"{name}__values"], name)
    assert out[0, 7] == float(np.abs(true - pred).sum())


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_compute_all_metrics_matches_the_reference_fixture(golden, name):
    from mused_amd import metrics_evaluation as me

    true, pred = mc.case(name)
    before = me.score_fallbacks
    results, log = quiet_metrics(me, pred, true)
    assert me.score_fallbacks == before   # a host fallback cannot hide a kernel failure
    assert list(results) == [str(k) for k in golden["result_keys"]] and all(len(v) == 1 for v in results.values())
    check_seven([results[k][0] for k in mc.KEYS], golden[f"{name}__values"], name)
    assert results["processing_time"][0] == 2.5 and [results[k][0] for k in me._VARIABLES] == list(VARIABLES)
    assert log == str(golden[f"{name}__log"])   # two decimals of values within 1e-12


@pytest.mark.parametrize("order", [("all_150x150", "binary_noise95"), ("binary_noise95", "all_150x150"),
                                   ("wide_151x700", "lds_over_96x257"), ("lds_over_96x257", "wide_151x700")])
def test_a_dirty_workspace_does_not_matter(golden, order):
    from mused_amd import metrics_evaluation as me

    dev = torch.device("cuda", torch.cuda.current_device())
    key = (dev, torch.cuda.current_stream().cuda_stream)
    alone = {}
    for name in order:
        me._SCORE_WS.pop(key, None)   # a workspace of its own
        alone[name] = entry(*mc.case(name))
    me._SCORE_WS[key] = torch.full((4 << 22,), 0x5A, dtype=torch.uint8, device=dev)
    for name in order:   # one after the other on the SAME workspace, dirty from the start
        out, info = entry(*mc.case(name))
        check_seven(out[0, :7], golden[f"{name}__values"], name)
        assert out.tobytes() == alone[name][0].tobytes() and np.array_equal(info, alone[name][1])
    assert me._SCORE_WS[key].numel() == 4 << 22


@pytest.mark.parametrize("name", ["binary_noise95", "all_150x150", "wide_151x700", "dbscan_like"])
def test_two_calls_are_bit_identical(name):
    true, pred = mc.case(name)
    a, b = entry(true, pred), entry(true, pred)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("width", [500, 503])   # 503: segments that do not start on a 16-byte boundary
def test_windows_equal_the_same_window_scored_alone(width):
    from mused_amd import metrics_evaluation as me
    from mused_amd import scores

    true, pred = mc.windows(width)
    before = me.score_fallbacks
    got = me.score_windows(true, pred)
    assert got.shape == (7, 7) and got.dtype == np.float64
    for k in range(7):
        out, info = entry(true[k], pred[k], me.WINDOW_CELLS_CAP)
        assert got[k].tobytes() == out[0, :7].tobytes(), k
        assert tuple(info[0, :5]) == scores.table_info(*scores.contingency(true[k], pred[k]))
        check_seven(got[k], scores.scores(true[k], pred[k]), f"window {k}")
    assert me.score_fallbacks == before
    assert got[2, 2] == 0.0 and got[4, 2] == 0.0   # a single true class; no event rows: integer decisions
    assert me.score_windows(torch.from_numpy(true).cuda(), dev32(pred)).tobytes() == got.tobytes()


def test_segments_off_the_16_byte_boundary():
    from mused_amd import metrics_evaluation as me

    true, pred = mc.case("tail_n4097")
    want, winfo = entry(true, pred)
    t, p = dev32(np.concatenate([[9], true])), dev32(np.concatenate([[9, 9, 9], pred]))
    out, info = me.score_labels_on_device(t[1:], p[3:], 1 << 22)
    assert out.tobytes() == want.tobytes() and np.array_equal(info, winfo)


@pytest.mark.parametrize("name", ["types_4x4", "dbscan_like", "range_ends"])
def test_input_kinds_give_the_same_bits(name):
    from mused_amd import metrics_evaluation as me

    true, pred = mc.case(name)
    before = me.score_fallbacks
    kinds = [(true, pred), (true.astype(np.int32), pred.astype(np.int32)), (list(true), list(pred)),
             (torch.from_numpy(true.copy()).cuda(), torch.from_numpy(pred.copy()).cuda()), (dev32(true), dev32(pred)),
             (true, dev32(pred)), (torch.from_numpy(true.copy()), pred.astype(np.int32))]
    got = [me.seven_scores(t, p) for t, p in kinds]
    assert me.score_fallbacks == before
    for g in got[1:]:
        assert list(g) == list(mc.KEYS) and np.array(list(g.values())).tobytes() == np.array(list(got[0].values())).tobytes()


def _out_of_contract():
    rng = np.random.default_rng(5)
    base_t, base_p = (a.copy() for a in mc.case("types_4x4"))
    hi_t, hi_p = base_t.copy(), base_p.copy()
    hi_p[17] = 65535
    lo_t, lo_p = base_t.copy(), base_p.copy()
    lo_t[3] = -2
    many_t = rng.integers(0, 3, 6000)
    many_p = np.concatenate([np.arange(5000), rng.integers(0, 5000, 1000)])
    big_t = np.concatenate([np.arange(2100), rng.integers(0, 2100, 2900)])   # 2100 x 2100 > 2^22 cells
    big_p = np.concatenate([np.arange(2100)[::-1], rng.integers(0, 2100, 2900)])
    far_t, far_p = base_t.copy(), base_p.copy()
    far_p[5] = 2 ** 32   # equal to 0 once cut to 32 bits: must not be read that way
    return {"label_65535": (hi_t, hi_p, 4), "label_minus_2": (lo_t, lo_p, 4), "5000_predicted_values": (many_t, many_p, 8),
            "table_above_cells_cap": (big_t, big_p, 8), "label_2^32": (far_t, far_p, 4)}


@pytest.mark.parametrize("name", ["label_65535", "label_minus_2", "5000_predicted_values", "table_above_cells_cap", "label_2^32"])
def test_out_of_contract_raises_its_flag_and_returns_the_host_result(name, monkeypatch):
    from mused_amd import metrics_evaluation as me

    true, pred, flag = _out_of_contract()[name]
    if name != "label_2^32":
        _, info = entry(true, pred)
        assert info[0, 5] == flag
    before = me.score_fallbacks
    results, _ = quiet_metrics(me, pred, true)
    assert me.score_fallbacks == before + 1
    monkeypatch.setenv("MUSED_SCORE", "host")
    want, _ = quiet_metrics(me, pred, true)
    assert [results[k][0] for k in mc.KEYS] == [want[k][0] for k in mc.KEYS]


def test_a_flagged_window_is_scored_on_the_host():
    from mused_amd import metrics_evaluation as me
    from mused_amd import scores

    true, pred = (a.copy() for a in mc.windows())
    pred[3, 10] = 70000
    before = me.score_fallbacks
    got = me.score_windows(true, pred)
    assert me.score_fallbacks == before + 1
    clean = me.score_windows(*mc.windows())
    assert np.array_equal(np.delete(got, 3, axis=0), np.delete(clean, 3, axis=0))
    check_seven(got[3], scores.scores(true[3], pred[3]), "flagged window")


def _blob(n, d=16, seed=0):
    from mused_amd import synth

    X, labels = synth.blob_stream(n, d, seed, n_centres=4)
    return [X.astype(np.float64)], np.asarray(labels)


def _host_results(me, monkeypatch, variables, clusters, true_labels):
    monkeypatch.setenv("MUSED_SCORE", "host")
    results, _ = me.get_initial_results()
    with contextlib.redirect_stdout(io.StringIO()):
        me.compute_all_metrics(results, *variables, clusters, true_labels, 2, 1)
    monkeypatch.delenv("MUSED_SCORE")
    return results


def test_batch_pipeline_scores_its_labels(monkeypatch):
    from mused_amd import metrics_evaluation as me
    from mused_amd.pipeline import process_batch_data

    mods, labels = _blob(600)
    args = (mods, [""], 8, 10, 4, 0, "SVDMC_batch", labels, 0.0, "types", False, 1.5, 2, 3, 2000)
    plain = process_batch_data({}, *args)
    assert sorted(plain) == ["all_clusters", "processing_time"] and isinstance(plain["processing_time"], float)
    before = me.score_fallbacks
    with contextlib.redirect_stdout(io.StringIO()):
        res = process_batch_data(None, *args, score=True)
    assert me.score_fallbacks == before
    assert np.array_equal(res["all_clusters"], plain["all_clusters"])
    assert list(res) == list(me.get_initial_results()[0]) + ["all_clusters"]
    variables = (600, 0.0, "types", False, 8, 10, 2000)
    want = _host_results(me, monkeypatch, variables, res["all_clusters"], labels)
    check_seven([res[k][0] for k in mc.KEYS], [want[k][0] for k in mc.KEYS], "SVDMC_batch")
    assert [res[k] for k in me._VARIABLES] == [[v] for v in variables] and len(res["processing_time"]) == 1


@pytest.mark.parametrize("ratio", [1, 2])
def test_streaming_pipeline_scores_its_labels(ratio, monkeypatch):
    from mused_amd import metrics_evaluation as me
    from mused_amd.pipeline import process_streaming_data

    W = 200
    n = 4 * W if ratio == 1 else W + 3 * W // 2   # four windows either way
    mods, labels = _blob(n)
    args = (mods, [""], W, 8, 10, 4, 0, "sSVDMC", labels, ratio, 0.0, "types", False, 1.5, 2)
    plain = process_streaming_data({}, *args)
    assert sorted(plain) == ["all_clusters", "processing_time"] and len(plain["all_clusters"]) == 4 * W
    mine, _ = me.get_initial_results()
    mine["f1_score"].append(0.5)   # an experiment's earlier point
    before = me.score_fallbacks
    with contextlib.redirect_stdout(io.StringIO()):
        res = process_streaming_data(mine, *args, score=True)
    assert me.score_fallbacks == before
    assert np.array_equal(res["all_clusters"], plain["all_clusters"])
    assert list(res) == list(me.get_initial_results()[0]) + ["all_clusters", "window_scores"]
    true_cat = np.concatenate([labels[lo : lo + W] for lo in range(0, n - W + 1, W // ratio)])
    assert len(true_cat) == 4 * W
    variables = (n, 0.0, "types", False, 8, 10, W)
    want = _host_results(me, monkeypatch, variables, res["all_clusters"], true_cat)
    assert res["f1_score"][0] == 0.5 and len(res["f1_score"]) == 2 and len(res["nmi_score"]) == 1
    check_seven([res[k][-1] for k in mc.KEYS], [want[k][0] for k in mc.KEYS], f"sSVDMC ratio {ratio}")
    ws = res["window_scores"]
    assert ws.shape == (4, 7)
    for k in range(4):
        w = me.host_scores(true_cat[k * W : (k + 1) * W], res["all_clusters"][k * W : (k + 1) * W])
        check_seven(ws[k], [w[key] for key in mc.KEYS], f"window {k}")
