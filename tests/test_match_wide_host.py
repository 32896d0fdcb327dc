"""The host specification of the wide Hungarian label chain, `hungarian.match_labels`, against `match_clusters(...,
"hungarian", 3)` on small inputs (any int32 label value, -1 first) and against SciPy's linear_sum_assignment on the generator
table that the device tests (tests/test_gpu_match_wide.py) use beyond the narrow chain's limits, where the host's P x N
overlap loop takes seconds.  Also: the built library exports the wide entry and the header declares it.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from mused_amd import _lib
from mused_amd import hungarian as hg
from mused_amd import matrix_operations as mo
from test_match_hung_host import TUPLES, host_pair, pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_OVERLAP = 3
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

# (k, per, g) -> seeds; W = k * per.  Seeds 0-3, noise 0.05 on the odd ones.  SciPy solves all of them but (1040, 24, 4) seed 3,
# which passes the feasibility test and has no complete assignment: the large flag-16 case of the device tests.
TABLE = {(264, 40, 8): (0, 1, 2, 3), (304, 24, 4): (0, 1, 2, 3), (1040, 24, 4): (0, 1, 2, 3), (1040, 40, 8): (0, 1, 2, 3)}
RAISES = {(3, 1040, 24, 4)}


def noise_of(seed):
    return 0.05 if seed % 2 else 0.0


def wide_pair(seed, k, per, g, noise):
    """test_gpu_match_hung.table_chain's rule at k labels in blocks of g: a new label stays in the block of its previous
    label or, for 15 % of the rows, moves to the next block; the blocks mix, so the solver has to augment.  noise > 0: first
    `cur`, then `new` get -1 on that share of the rows."""
    rng = np.random.default_rng(seed)
    W = k * per
    cur = rng.integers(0, k, W)
    base = (cur // g) * g + np.where(rng.random(W) < 0.15, g, 0)
    new = (base + rng.integers(0, g, W)) % k
    if noise > 0:
        cur = np.where(rng.random(W) < noise, -1, cur)
        new = np.where(rng.random(W) < noise, -1, new)
    return cur, new


def wide_chain(seed=0, k=264, per=40, g=8, windows=6):
    """The generator applied to its own output: every window drifts from the one before (264 labels: every window is beyond
    the narrow chain; SciPy solves all six for seeds 0-5)."""
    rng = np.random.default_rng(seed)
    W = k * per
    cur, out = rng.integers(0, k, W), []
    for _ in range(windows):
        out.append(cur)
        base = (cur // g) * g + np.where(rng.random(W) < 0.15, g, 0)
        cur = (base + rng.integers(0, g, W)) % k
    return np.array(out)


def spec_chain(raw, prev=None, min_overlap=MIN_OVERLAP):
    """match_labels applied in sequence -> (K * W labels, [(P, N, steps, feasible)])."""
    out, info = [], []
    for r in raw:
        prev, *rest = hg.match_labels(prev, r, min_overlap)
        out.extend(np.asarray(prev).tolist())
        info.append(tuple(rest))
    return np.array(out), info


@functools.lru_cache(maxsize=None)
def spec_pair(seed, k, per, g):
    """dict(prev, new, P, N, cost, and -- unless lsap raises, then raises=True -- labels, steps, feasible and SciPy's (rows,
    cols)): the specification on one generator pair, computed once and shared with the device tests."""
    prev, new = wide_pair(seed, k, per, g, noise_of(seed))
    up, un, _, cnt = hg.overlap_counts(prev, new)
    d = dict(prev=prev, new=new, P=len(up), N=len(un), cost=hg.costs_of(cnt, MIN_OVERLAP), raises=False)
    try:
        d["labels"], P, N, d["steps"], d["feasible"] = hg.match_labels(prev, new, MIN_OVERLAP)
        assert (P, N) == (d["P"], d["N"])
        d["rows"], d["cols"] = linear_sum_assignment(d["cost"]) if d["feasible"] else (None, None)
    except ValueError:
        d["raises"] = True
        d["feasible"] = hg.is_feasible(d["cost"])
    return d


def dbscan_like(seed=0, clusters=400, noise=0.30):
    """An infeasible pair as DBSCAN_incr produces them: 400 clusters of 2-6 rows and 30 % noise on either side, W about
    2,000; most clusters overlap no cluster of the other side in 3 rows."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 7, clusters)
    body = np.repeat(np.arange(clusters), sizes)
    W = int(round(len(body) / (1 - noise)))
    prev = np.concatenate([body, np.full(W - len(body), -1)])
    new = np.concatenate([np.full(W - len(body), -1), np.repeat(np.arange(clusters), sizes[::-1])])
    return prev[rng.permutation(W)], new


def same_as_match_clusters(prev, new):
    ref = mo.match_clusters(prev, new, "hungarian", MIN_OVERLAP)
    out, P, N, steps, feasible = hg.match_labels(prev, new, MIN_OVERLAP)
    assert (out is new) == (ref is new)
    assert np.array_equal(np.asarray(out), np.asarray(ref))
    if prev is not None and len(prev):
        up, un, cost = mo._overlap_costs(np.asarray(prev), np.asarray(new), MIN_OVERLAP)
        assert (P, N, feasible) == (len(up), len(un), mo._feasible(cost))
        assert (steps > 0) == feasible
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_equals_match_clusters_on_the_narrow_table(seed):
    for t in TUPLES:
        h = host_pair(seed, *t)   # match_clusters on this pair, computed once for test_match_hung_host.py's tests as well
        out, P, N, steps, feasible = hg.match_labels(h["prev"], h["new"], MIN_OVERLAP)
        assert (P, N, feasible) == (h["P"], h["N"], h["feasible"]) and np.array_equal(np.asarray(out), h["labels"])
        assert (out is h["new"]) == (not feasible) and steps == (h["spec"][2] if feasible else 0)


def test_equals_match_clusters_on_any_label_value():
    rng = np.random.default_rng(5)
    base_p, base_n = pair(2, 300, 8, 8)
    cases = [
        (np.where(rng.random(300) < 0.2, -1, base_p), base_n),                     # -1 on one side
        (base_p, np.where(rng.random(300) < 0.2, -1, base_n)),
        (np.where(rng.random(300) < 0.2, -1, base_p), np.where(rng.random(300) < 0.2, -1, base_n)),   # on both
        (np.array([-7, 5000, I32_MIN, I32_MAX])[base_p % 4], np.array([I32_MAX, -7, 5000, I32_MIN, 12])[base_n % 5]),
        (np.full(60, 6), np.array([3] * 20 + [4] * 20 + [8] * 20)),                # P = 1
        (np.array([3] * 20 + [4] * 20 + [8] * 20), np.full(60, 2)),                # N = 1
        (np.full(60, -1), np.full(60, -1)),
        (np.array([4]), np.array([-1])),                                           # W = 1
        (np.array([0, 0, 0, 1, 1, 1]), np.array([0, 1, 2, 0, 1, 2])),              # infeasible: passes through
    ]
    for prev, new in cases:
        same_as_match_clusters(prev, new)
    out = same_as_match_clusters(cases[3][0], cases[3][1])
    assert out.dtype == np.int64 and {I32_MIN, I32_MAX} & set(out.tolist())
    new = np.array([3, 4, 8])
    assert hg.match_labels(None, new, 3)[0] is new and hg.match_labels([], new, 3)[0] is new
    assert mo.match_clusters(None, new, "hungarian", 3) is new


def test_raises_where_scipy_raises():
    prev = np.array([0] * 9 + [1] * 3 + [2] * 3)   # tests/test_gpu_match_hung.py::test_scipy_raises_case_sets_the_assign_flag
    new = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2] + [0] * 3 + [0] * 3)
    with pytest.raises(ValueError):
        mo.match_clusters(prev, new, "hungarian", 3)
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        hg.match_labels(prev, new, 3)


@pytest.mark.parametrize("shape", list(TABLE), ids=lambda s: "-".join(str(x) for x in s))
def test_generator_table_against_scipy(shape):
    k = shape[0]
    for seed in TABLE[shape]:
        h = spec_pair(seed, *shape)
        assert h["prev"].shape == (shape[0] * shape[1],)
        assert h["P"] == h["N"] == k + (1 if seed % 2 else 0) and h["feasible"]
        if (seed,) + shape in RAISES:
            assert h["raises"]
            with pytest.raises(ValueError):
                linear_sum_assignment(h["cost"])
            continue
        assert not h["raises"]
        rows, cols = h["rows"], h["cols"]   # SciPy's, on the same costs
        print(f"{shape} seed {seed}: P x N {h['P']} x {h['N']}, steps {h['steps']}")
        assert min(h["P"], h["N"]) < h["steps"] <= 2.1 * min(h["P"], h["N"])   # augmenting paths, far inside the budget
        # match_labels' assignment is SciPy's: a matched new label takes the previous value of its row, and with distinct
        # values on either side the labels determine the assignment
        up, un = np.unique(h["prev"]), np.unique(h["new"])
        table = dict(zip(un[cols].tolist(), up[rows].tolist()))
        assert np.array_equal(h["labels"], [table.get(c, c) for c in h["new"].tolist()])


def test_wide_is_for_the_hungarian_method_only():
    pytest.importorskip("torch")
    raw = np.zeros((1, 4), dtype=np.int64)
    with pytest.raises(ValueError, match="hungarian"):
        mo.match_chain_on_device(raw, method="pot", wide=True)
    with pytest.raises(ValueError, match="hungarian"):
        mo.match_clusters_on_device(raw[0], raw[0], method="pot", wide=True)


def test_dbscan_like_pair_is_infeasible():
    prev, new = dbscan_like()
    out, P, N, steps, feasible = hg.match_labels(prev, new, MIN_OVERLAP)
    assert 1800 <= len(new) <= 2500 and P == N == 401 and out is new and steps == 0 and not feasible


def test_library_exports_and_header_declares_the_wide_entry():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "mused_hip.h")).read()
    for name in ("mused_match_hung_wide_ws_bytes", "mused_match_hung_wide_chain"):
        assert hasattr(L, name) and name in _lib.EXPORTED
        assert re.search(r"\b(long|int)\s+" + name + r"\s*\(", header)
    # the workspace as the header states it, and the limits on W
    ws = L.mused_match_hung_wide_ws_bytes
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    for W in (1, 1025, 4096, 41600, 1 << 20):
        assert ws(W) == 256 + 8 * 2 * 16384 + 4 * 6 * 4096 + al(4 * W) + al(4 * min(W, 4096) ** 2)
    assert ws(0) == -1 and ws((1 << 20) + 1) == -1
    assert mo.MATCH_WIDE_MAXC == 4096 and callable(mo.match_wide_launch)
