"""The partition scores on the GPU (csrc/score_partitions.hip, metrics_evaluation.compute_partition_metrics) against
scikit-learn and SciPy under the contract of tests/partition_cases.py: five values equal, the V-measure family within 1e-12,
the EMI within 16 * 2^-52 * (G * S_abs + log N), the AMI within the bound built from those."""
import ctypes as C
import math

import numpy as np
import pytest

import partition_cases as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CELLS = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def dev32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def raw(true, pred, want_emi=True, cells=CELLS):
    from mused_amd import metrics_evaluation as me

    out, ints, info, tables = me.partition_scores_on_device(dev32(true), dev32(pred), cells, want_emi=want_emi)
    return out, ints, info, tables.cpu().numpy()


def check_raw(name, out, ints, info, table_dev):
    """One segment's device outputs against the rule (integers, table: equal) and scikit-learn (the four doubles)."""
    from mused_amd import partition_scores as ps
    from mused_amd import scores

    true, pred = pc.case(name)
    tv, pv, table = scores.contingency(true, pred)
    T, P, n = len(tv), len(pv), len(true)
    assert tuple(info[:3]) == (T, P, 0)
    assert np.array_equal(table_dev[: T * P].reshape(T, P), table)
    a, b = table.sum(axis=1), table.sum(axis=0)
    terms = sum(max(0, min(int(x), int(y)) - max(1, int(x) + int(y) - n) + 1) for x in a for y in b)
    assert tuple(int(v) for v in ints[:7]) == (*ps.pair_sums(table), int(table.max(axis=0).sum()), int(table.max(axis=1).sum()),
                                               terms, n)
    mi, ht, hp, e, s_abs, G, _, _ = pc.rule_parts(name)
    emi_sk = pc.reference(name)[1]
    for what, got, want in (("MI", out[0], mi), ("H_true", out[1], ht), ("H_pred", out[2], hp)):
        print(f"{name} {what}: device {got!r} rule {want!r} diff {abs(got - want):.3e}")
        assert abs(got - want) <= pc.TOL
    tol = pc.emi_tolerance(s_abs, G, n)
    ratio = abs(out[3] - emi_sk) / (pc.EPS * G * s_abs) if s_abs else 0.0
    print(f"{name} EMI: device {out[3]!r} sklearn {emi_sk!r} diff {abs(out[3] - emi_sk):.3e} tolerance {tol:.3e} "
          f"EMI_RATIO {ratio:.4f}")
    if min(T, P) == 1:
        assert out[3] == 0.0 == emi_sk
    else:
        assert abs(out[3] - emi_sk) <= tol


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_device_outputs_and_the_nine_values(name):
    """Every input of the host test (segment tails n = 1, 2, 3, 5, 257; both placements of the table; both orientations of
    the solver; labels -1 and 65534) through the kernels and through compute_partition_metrics, with no host fallback."""
    from mused_amd import metrics_evaluation as me

    true, pred = pc.case(name)
    out, ints, info, tables = raw(true, pred)
    check_raw(name, out[0], ints[0], info[0], tables[0])
    before = me.partition_fallbacks
    got = me.compute_partition_metrics(true, pred)
    assert me.partition_fallbacks == before, "the device path fell back to the host"
    assert list(got) == list(pc.KEYS) and all(type(v) is float for v in got.values())
    pc.check_nine([got[k] for k in pc.KEYS], name, "device")


def test_table_placement_cases_are_what_they_claim():
    for name, cells, in_lds in (("rand_3000_150x150", 22500, True), ("rand_3000_160x160", 25600, False)):
        T, P = (len(np.unique(x)) for x in pc.case(name))
        assert T * P == cells and (cells <= 24576) == in_lds


def test_input_kinds_and_stream():
    """Lists, int64 / int32 CUDA tensors and a caller's stream give the values of the NumPy call."""
    from mused_amd import metrics_evaluation as me

    true, pred = pc.case("rand_2000_40x37")
    want = me.compute_partition_metrics(true, pred)
    assert me.compute_partition_metrics(list(true), list(pred)) == want
    assert me.compute_partition_metrics(torch.from_numpy(true.copy()).cuda(), dev32(pred)) == want
    assert me.compute_partition_metrics(dev32(true), pred, stream=torch.cuda.Stream()) == want


def test_windows_equal_single_calls():
    from mused_amd import metrics_evaluation as me

    rng = np.random.default_rng(21)
    true, pred = rng.integers(0, 5, (3, 257)), rng.integers(-1, 6, (3, 257))
    pred[1] = true[1]
    before = me.partition_fallbacks
    got = me.partition_windows(true, pred)
    assert got.shape == (3, 9) and got.dtype == np.float64
    for k in range(3):
        single = me.compute_partition_metrics(true[k], pred[k])
        assert tuple(got[k]) == tuple(single[key] for key in pc.KEYS), k
    assert np.array_equal(me.partition_windows(dev32(true), dev32(pred)), got)
    assert me.partition_fallbacks == before


@pytest.mark.parametrize("name", ["rand_400_5x9", "rand_400_9x5"])
def test_matched_accuracy_both_orientations(name):
    """P < N and P > N of the solver: the table summed over the assigned cells is SciPy's optimum."""
    from scipy.optimize import linear_sum_assignment

    from mused_amd import metrics_evaluation as me
    from mused_amd import scores

    true, pred = pc.case(name)
    table = scores.contingency(true, pred)[2]
    rows, cols = linear_sum_assignment(table, maximize=True)
    before = me.partition_fallbacks
    total = me._matched_total(dev32(true), dev32(pred), dev32(table.ravel()), *table.shape, torch.cuda.current_stream())
    assert me.partition_fallbacks == before
    assert total == int(table[rows, cols].sum())
    assert me.compute_partition_metrics(true, pred)["matched_accuracy"] == total / len(true)


@pytest.mark.parametrize("kind", ["range", "size"])
def test_flagged_inputs_take_the_host(kind):
    from mused_amd import metrics_evaluation as me

    rng = np.random.default_rng(31)
    if kind == "range":   # a label of 70,000: flag 4
        true, pred = rng.integers(0, 4, 500), rng.integers(0, 3, 500)
        pred[17] = 70000
        flag = me.SCORE_FLAG_RANGE
    else:                 # 4,097 distinct values at n = 5,000: flag 8
        true, pred = rng.integers(0, 3, 5000), np.arange(5000) % 4097
        flag = me.SCORE_FLAG_SIZE
    _, ints, info, _ = raw(np.clip(true, -2, 65535), np.clip(pred, -2, 65535), cells=1 << 22)
    assert info[0, 2] == flag and ints[0, 6] == len(true)
    before = me.partition_fallbacks
    got = me.compute_partition_metrics(true, pred)
    assert me.partition_fallbacks == before + 1
    assert tuple(got[k] for k in pc.KEYS) == pc.sklearn_values(true, pred)[0]


def test_c_abi_without_emi():
    """want_emi = 0: the EMI slot is NaN and flag 64 is set; every other output is what the full call gives.  The Python
    finish then takes only `ami_score` from scikit-learn."""
    from mused_amd import metrics_evaluation as me

    name = "rand_2000_40x37"
    true, pred = pc.case(name)
    out1, ints1, info1, tab1 = raw(true, pred)
    out0, ints0, info0, tab0 = raw(true, pred, want_emi=False)
    assert math.isnan(out0[0, 3]) and info0[0, 2] == me.PARTITION_FLAG_NO_EMI and info1[0, 2] == 0
    assert np.array_equal(ints0, ints1) and np.array_equal(tab0[0, : 40 * 37], tab1[0, : 40 * 37])
    assert np.array_equal(out0[0, :3].view(np.int64), out1[0, :3].view(np.int64)) and tuple(info0[0, :2]) == tuple(info1[0, :2])
    labels = (dev32(true), dev32(pred))
    before = me.partition_fallbacks
    vals = me._partition_segment(0, labels, out0, ints0, info0, torch.from_numpy(tab0).cuda(), torch.cuda.current_stream(),
                                 lambda: (true, pred))
    assert me.partition_fallbacks == before + 1
    want = pc.reference(name)[0]
    assert vals["ami_score"] == want[1]
    pc.check_nine([vals[k] for k in pc.KEYS], name, "no-emi")


def test_short_workspace_is_an_error():
    from mused_amd import _lib
    from mused_amd import engine as eng

    t = dev32(np.zeros(8))
    res = torch.zeros(160, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    need = _lib.lib().mused_score_partitions_ws_bytes(1, 8, 64)
    assert need > 1024
    with pytest.raises(_lib.MusedError):
        _lib.call("mused_score_partitions", eng.ptr(t), eng.ptr(t), 1, 8, 64, 1, eng.ptr(res[:64]), eng.ptr(res[64:128]),
                  eng.ptr(res[128:]), None, eng.ptr(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name", ["rand_5000_150x150", "rand_3000_160x160", "skew_4096_2x2"])
def test_two_runs_and_both_lgamma_paths_give_the_same_bits(name, monkeypatch):
    true, pred = pc.case(name)
    first = raw(true, pred)
    second = raw(true, pred)
    monkeypatch.setenv("MUSED_PARTITION_LGAMMA", "direct")   # no table: lgamma evaluated where it is used
    direct = raw(true, pred)
    for other in (second, direct):
        assert np.array_equal(first[0].view(np.int64), other[0].view(np.int64))
        assert np.array_equal(first[1], other[1]) and np.array_equal(first[2], other[2])


STREAM = (900, 20, 4, 3, 300)   # rows, d, seed, centres, W: the smallest stream of tests/test_gpu_pipeline.py


def test_pipeline_stream():
    from mused_amd import metrics_evaluation as me
    from mused_amd import synth
    from mused_amd.pipeline import process_streaming_data

    n, d, seed, centres, W = STREAM
    X, labels = synth.blob_stream(n, d, seed, n_centres=centres)
    args = ({}, [X.astype(np.float64)], [""], W, 6, 15, 3, 0, "sSVDMC", labels, 1, 0.0, "types", False, 1.5, 2)
    plain = process_streaming_data(*args, score=True)
    res = process_streaming_data(*args, score=True, partition_scores=True)
    assert set(res) == set(plain) | {"partition_scores", "window_partition_scores"}
    assert np.array_equal(res["all_clusters"], plain["all_clusters"])
    assert res["partition_scores"] == me.compute_partition_metrics(labels, res["all_clusters"])
    assert res["window_partition_scores"].shape == (n // W, 9)
    assert tuple(res["window_partition_scores"][1]) == tuple(
        me.compute_partition_metrics(labels[W : 2 * W], res["all_clusters"][W : 2 * W]).values())
    unscored = process_streaming_data(*args, partition_scores=True)
    assert set(unscored) == {"all_clusters", "processing_time", "partition_scores", "window_partition_scores"}
    assert set(process_streaming_data(*args, partition_scores=False)) == {"all_clusters", "processing_time"}
    with pytest.raises(ValueError):
        process_streaming_data(*args[:9], None, *args[10:], partition_scores=True)


def test_pipeline_batch():
    from mused_amd import metrics_evaluation as me
    from mused_amd import synth
    from mused_amd.pipeline import process_batch_data

    n, d, seed, centres, _ = STREAM
    X, labels = synth.blob_stream(n, d, seed, n_centres=centres)
    args = ({}, [X.astype(np.float64)], [""], 6, 15, 3, 0, "SVDMC_batch", labels, 0.0, "all", False, 1.5, 2, 3, 2000)
    plain = process_batch_data(*args, score=True)
    res = process_batch_data(*args, score=True, partition_scores=True)
    assert set(res) == set(plain) | {"partition_scores"}
    assert res["partition_scores"] == me.compute_partition_metrics(labels, res["all_clusters"])
    assert set(process_batch_data(*args)) == {"all_clusters", "processing_time"}
    with pytest.raises(ValueError):
        process_batch_data(*args[:8], None, *args[9:], partition_scores=True)


def test_batch_size_once():
    """(150,000, 150 x 150), the batch approaches' own size, once and under the same bounds."""
    from mused_amd import metrics_evaluation as me
    from mused_amd import partition_scores as ps
    from mused_amd import scores

    rng = np.random.default_rng(41)
    n = 150_000
    true, pred = rng.integers(0, 150, n), rng.integers(0, 150, n)
    want, emi_sk = pc.sklearn_values(true, pred)
    table = scores.contingency(true, pred)[2]
    mi, ht, hp, e, s_abs, G, num, den = ps.ami_parts(table)
    out, ints, info, tables = raw(true, pred)
    assert np.array_equal(tables[0, : 150 * 150].reshape(150, 150), table) and info[0, 2] == 0
    tol = pc.emi_tolerance(s_abs, G, n)
    print(f"batch EMI: device {out[0, 3]!r} sklearn {emi_sk!r} diff {abs(out[0, 3] - emi_sk):.3e} tolerance {tol:.3e} "
          f"EMI_RATIO {abs(out[0, 3] - emi_sk) / (pc.EPS * G * s_abs):.4f} terms {ints[0, 5]}")
    assert abs(out[0, 3] - emi_sk) <= tol
    before = me.partition_fallbacks
    got = me.compute_partition_metrics(dev32(true), dev32(pred))
    assert me.partition_fallbacks == before
    assert abs(den) >= 1e-3
    for i, key in enumerate(pc.KEYS):
        print(f"batch {key}: got {got[key]!r} want {want[i]!r} diff {abs(got[key] - want[i]):.3e}")
        if key in pc.EXACT:
            assert got[key] == want[i], key
        elif key == "ami_score":
            assert abs(got[key] - want[i]) <= pc.ami_tolerance((mi, ht, hp, e, s_abs, G, num, den), n), key
        else:
            assert abs(got[key] - want[i]) <= pc.TOL, key
