"""Host side of the partition scores: mused_amd/partition_scores.py (the rule csrc/score_partitions.hip and the host finish
follow) against live scikit-learn and SciPy calls under the contract of tests/partition_cases.py, and the host path of the
drop-in metrics_evaluation module (get_initial_results, compute_all_metrics)."""
import numpy as np
import pytest

import partition_cases as pc

VARIABLES = (1234, 0.95, "binary", False, 10, 50, 2000)


def test_keys():
    from mused_amd import partition_scores as ps

    assert ps.KEYS == pc.KEYS


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_rule_equals_scikit_learn_and_scipy(name):
    from mused_amd import partition_scores as ps
    from mused_amd import scores

    tv, pv, table = scores.contingency(*pc.case(name))
    pc.check_nine(ps.scores_from_table(tv, pv, table), name, "rule")
    assert ps.scores(*pc.case(name)) == ps.scores_from_table(tv, pv, table)


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_rule_emi_within_its_bound(name):
    """The rule's EMI (the C library's lgamma, one table) against scikit-learn's (SciPy's gammaln and the same lgamma)."""
    from mused_amd import partition_scores as ps
    from mused_amd import scores

    table = scores.contingency(*pc.case(name))[2]
    e, s_abs, G = ps.emi(table)
    want = pc.reference(name)[1]
    n = int(table.sum())
    tol = pc.emi_tolerance(s_abs, G, n)
    print(f"{name}: emi {e!r} sklearn {want!r} diff {abs(e - want):.3e} tolerance {tol:.3e} S_abs {s_abs:.6g} G {G:.6g}")
    if min(table.shape) == 1:
        assert e == 0.0 == want and s_abs == 0.0
    else:
        assert abs(e - want) <= tol
        assert s_abs >= abs(e) * (1 - 1e-9)   # the two sums run in different orders


def test_term_range_starts_above_one():
    """The 2 x 2 input with a_0 + b_0 > N: the terms of cell (0, 0) start at a + b - N = 7, and the term count follows."""
    from mused_amd import scores

    table = scores.contingency(*pc.case("high_overlap_2x2"))[2]
    a, b, N = table.sum(axis=1), table.sum(axis=0), int(table.sum())
    assert (a[0], b[0], N) == (9, 8, 10) and max(1, a[0] + b[0] - N) == 7


def test_pair_sums_are_python_ints_beyond_int64():
    from mused_amd import partition_scores as ps

    sq, sa, sb = ps.pair_sums(np.array([[3_000_000_000, 1], [2, 3_000_000_000]], dtype=np.int64))
    assert (sq, sa, sb) == (2 * 3_000_000_000 ** 2 + 5, 3_000_000_001 ** 2 + 3_000_000_002 ** 2,
                            3_000_000_002 ** 2 + 3_000_000_001 ** 2)
    assert all(type(v) is int for v in (sq, sa, sb))


def test_get_initial_results_unchanged_without_the_argument():
    from mused_amd import metrics_evaluation as me
    from mused_amd import scores

    results, variables = me.get_initial_results()
    assert list(results) == list(scores.KEYS) + ["processing_time"] + variables and all(v == [] for v in results.values())
    assert variables == ["subset_size", "noise_rate", "label_mode", "sorting", "reduced_dim", "k_basis", "window_size"]
    with_nine, variables2 = me.get_initial_results(partition=True)
    assert list(with_nine) == list(results) + list(pc.KEYS) and variables2 == variables
    assert all(v == [] for v in with_nine.values())


def test_compute_all_metrics_host_path(monkeypatch, capsys):
    """MUSED_SCORE=host: with the nine lists compute_all_metrics appends nine more values (scikit-learn's and SciPy's) and
    extends the log line; with the default results it prints the line it printed before."""
    from mused_amd import metrics_evaluation as me

    monkeypatch.setenv("MUSED_SCORE", "host")
    true, pred = pc.case("rand_2000_4x4")
    before = me.partition_fallbacks
    plain, _ = me.get_initial_results()
    me.compute_all_metrics(plain, *VARIABLES, pred, true, 3_500_000_000, 1_000_000_000)
    line_plain = capsys.readouterr().out
    assert me.partition_fallbacks == before
    seven = me.host_scores(true, pred)
    want_plain = ("processing_time=2.5\n" + "".join(f"{short}={seven[key]:.2f}, " for key, short in me._LOGGED)
                  + "processing_time=2.50\n")
    assert line_plain == want_plain
    assert not any(k in plain for k in pc.KEYS)

    nine, _ = me.get_initial_results(partition=True)
    me.compute_all_metrics(nine, *VARIABLES, pred, true, 3_500_000_000, 1_000_000_000)
    line_nine = capsys.readouterr().out
    assert me.partition_fallbacks == before + 1
    want = pc.reference("rand_2000_4x4")[0]
    for i, key in enumerate(pc.KEYS):
        assert nine[key] == [want[i]], key
    for key in plain:
        assert nine[key] == plain[key], key
    shorts = dict(me._PARTITION_LOGGED)
    extra = "".join(f"{shorts[key]}={want[i]:.2f}, " for i, key in enumerate(pc.KEYS))
    assert line_nine == want_plain.replace("processing_time=2.50\n", extra + "processing_time=2.50\n")


def test_host_path_takes_what_the_device_cannot(monkeypatch):
    from mused_amd import metrics_evaluation as me

    monkeypatch.setenv("MUSED_SCORE", "host")
    true, pred = pc.case("rand_300_3x5")
    got = me.compute_partition_metrics(list(true), list(pred))
    assert list(got) == list(pc.KEYS)
    assert tuple(got[k] for k in pc.KEYS) == pc.reference("rand_300_3x5")[0]
    assert all(type(v) is float for v in got.values())
    with pytest.raises(ValueError):
        me.compute_partition_metrics([0, 1, 2], [0, 1])
    res = me.partition_windows(np.stack([true[:100], true[100:200]]), np.stack([pred[:100], pred[100:200]]))
    assert res.shape == (2, 9)
    assert tuple(res[1]) == pc.sklearn_values(true[100:200], pred[100:200])[0]


def test_compat_module_re_exports_the_new_names():
    from mused_amd import metrics_evaluation as me
    from mused_amd.compat import metrics_evaluation as cme

    assert cme.compute_partition_metrics is me.compute_partition_metrics and cme.partition_windows is me.partition_windows
