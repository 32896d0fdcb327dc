"""The host specification of the Hungarian label matching (mused_amd/hungarian.py) against SciPy's
linear_sum_assignment: random small matrices with many ties and infeasible patterns, and the table of label pairs the device
tests (tests/test_gpu_match_hung.py) use as well.  Also: the built library exports the device entry.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from mused_amd import _lib
from mused_amd import hungarian as hg
from mused_amd import matrix_operations as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (W, kp, kn) of the label pairs; the device tests import TUPLES, SEEDS, pair and host_pair
TUPLES = [(96, 4, 4), (300, 8, 8), (300, 7, 9), (300, 9, 7), (1200, 16, 16), (2000, 50, 50), (2500, 64, 65), (2500, 65, 64),
          (6000, 150, 150), (6000, 150, 140), (10000, 256, 256), (10000, 250, 256)]
SEEDS = (0, 1, 2)
MIN_OVERLAP = 3


def pair(seed, W, kp, kn):
    """Labels in groups of 8 (4 at (96, 4, 4)): a new label stays in the group of its previous label or, for 15 % of the rows,
    moves to the next group.  Overlap counts tie often and the greedy choice of a row is often taken: augmenting paths."""
    g = 4 if (W, kp, kn) == (96, 4, 4) else 8
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, kp, W)
    base = (prev // g) * g + np.where(rng.random(W) < 0.15, g, 0)
    new = (base + rng.integers(0, g, W)) % kn
    return prev, new


# (P, N) of the two-valued cost tables: the narrow chain's (lane boundary, counts read from the workspace beyond 24,576
# entries, capacity in both orientations) and the ones beyond it (a position's owner wraps at 256 and 512 threads)
TIE_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (64, 64), (65, 64), (64, 65), (160, 160), (256, 256), (256, 255)]
TIE_SEEDS = (0, 1)
TIE_WIDE_SHAPES = [(257, 257), (300, 290), (513, 513), (512, 520)]
TIE_STEPS = {(64, 64): 110, (65, 64): 103, (64, 65): 136, (160, 160): 280, (256, 256): 476, (256, 255): 482, (257, 257): 510,
             (300, 290): 504, (513, 513): 1070}   # Dijkstra steps of the specification at seed 0


def tie_pair(seed, P, N):
    """Labels whose P x N overlap counts take two values only, 6 on about two entries a row and 3 elsewhere (every entry
    is finite at min_overlap = 3): almost every selection of the solver is decided by its tie rule."""
    C = np.where(np.random.default_rng(seed).random((P, N)) < 2 / max(P, N), 6, 3)
    i, j = np.nonzero(C)
    return np.repeat(i, C[i, j]), np.repeat(j, C[i, j])


@functools.lru_cache(maxsize=None)
def host_tie(seed, P, N):
    """host_pair's dict for tie_pair(seed, P, N), from one contingency pass (hungarian.match_labels is held to match_clusters
    by tests/test_match_wide_host.py; the host's own P x N loop would take minutes at 256 x 256 and W = 200,000)."""
    prev, new = tie_pair(seed, P, N)
    up, un, _, cnt = hg.overlap_counts(prev, new)
    cost = hg.costs_of(cnt, MIN_OVERLAP)
    return dict(prev=prev, new=new, P=len(up), N=len(un), cost=cost, feasible=hg.is_feasible(cost),
                scipy=linear_sum_assignment(cost), spec=hg.lsap(cost),
                labels=np.asarray(hg.match_labels(prev, new, MIN_OVERLAP)[0]))


@functools.lru_cache(maxsize=None)
def host_pair(seed, W, kp, kn):
    """dict(prev, new, P, N, cost, feasible (match_clusters' own test), scipy (rows, cols), spec (rows, cols, steps),
    labels (the host match_clusters))."""
    prev, new = pair(seed, W, kp, kn)
    up, un, cost = mo._overlap_costs(prev, new, MIN_OVERLAP)
    return dict(prev=prev, new=new, P=len(up), N=len(un), cost=cost, feasible=mo._feasible(cost),
                scipy=linear_sum_assignment(cost), spec=hg.lsap(cost),
                labels=np.asarray(mo.match_clusters(prev, new, "hungarian", MIN_OVERLAP)))


def test_specification_equals_scipy_on_random_costs():
    rng = np.random.default_rng(0)
    infeasible = 0
    for n in range(4000):
        P, N = (int(x) for x in rng.integers(1, 14, 2))
        hi = int(rng.choice([2, 3, 5, 50]))
        min_overlap = int(rng.choice([1, 3]))
        ov = rng.integers(0, hi, (P, N))
        cost = np.where(ov >= min_overlap, -ov.astype(np.float64), np.inf)
        try:
            ref = linear_sum_assignment(cost)
        except ValueError as e:
            assert "infeasible" in str(e)
            infeasible += 1
            with pytest.raises(ValueError, match="cost matrix is infeasible"):
                hg.lsap(cost)
            continue
        rows, cols, steps = hg.lsap(cost)
        assert np.array_equal(rows, ref[0]) and np.array_equal(cols, ref[1]), (n, cost)
        assert steps >= min(P, N)
    # both outcomes are well represented; with these draws (P and N in one call, then hi, min_overlap, the counts) SciPy
    # raises on 1,057 of the 4,000
    assert infeasible == 1057


def test_label_pair_table():
    """SciPy solves all 36 pairs, the specification returns its assignment on each, and most of them walk augmenting paths
    (more Dijkstra steps than rows)."""
    hs = [host_pair(s, *t) for t in TUPLES for s in SEEDS]   # host_pair calls SciPy: a pair it cannot solve raises here
    assert len(hs) == 36 and all(len(h["scipy"][0]) == min(h["P"], h["N"]) for h in hs)
    # match_clusters' own test (every row AND column keeps a finite entry) is stricter than SciPy's on rectangular
    # matrices: 7 of the pairs with P < N pass through unmatched, the device tests expect no solve for them
    assert sum(h["feasible"] for h in hs) == 29
    assert all(h["P"] < h["N"] and np.array_equal(h["labels"], h["new"]) for h in hs if not h["feasible"])
    for h in hs:
        rows, cols, _ = h["spec"]
        assert np.array_equal(rows, h["scipy"][0]) and np.array_equal(cols, h["scipy"][1])
    walked = sum(h["spec"][2] > min(h["P"], h["N"]) for h in hs)
    print("pairs with augmenting paths:", walked, "largest step count:", max(h["spec"][2] for h in hs))
    assert walked >= 30
    # the device solves only the 29 feasible pairs (the 7 others pass through before the solver): 27 of those walk paths,
    # the two that do not are 4 x 4
    on_device = [h for h in hs if h["feasible"]]
    assert sum(h["spec"][2] > min(h["P"], h["N"]) for h in on_device) == 27
    # sizes on both sides of the kernel's limits and orientations: P < N, P > N, 256 x 256
    shapes = {(h["P"], h["N"]) for h in hs}
    assert (256, 256) in shapes and any(p < n for p, n in shapes) and any(p > n for p, n in shapes)


def test_two_valued_tables_against_scipy():
    """The specification returns SciPy's assignment where ties decide nearly every step, every pair is feasible, paths are
    walked (the step counts of seed 0 are pinned: the device tests compare with them), and W stays below the wide chain's 2^20."""
    for P, N in TIE_SHAPES + TIE_WIDE_SHAPES:
        for seed in TIE_SEEDS if (P, N) in TIE_SHAPES else (0,):
            h = host_tie(seed, P, N)
            assert (h["P"], h["N"]) == (P, N) and h["feasible"] and set(np.unique(-h["cost"])) <= {3.0, 6.0}
            rows, cols, steps = h["spec"]
            assert np.array_equal(rows, h["scipy"][0]) and np.array_equal(cols, h["scipy"][1])
            assert min(P, N) <= steps <= 32 * min(P, N)   # the wide chain's default budget
            if seed == 0 and (P, N) in TIE_STEPS:
                assert steps == TIE_STEPS[(P, N)] > min(P, N)
            up, un = np.unique(h["prev"]), np.unique(h["new"])
            table = dict(zip(un[cols].tolist(), up[rows].tolist()))
            assert np.array_equal(h["labels"], [table.get(c, c) for c in h["new"].tolist()])
    assert max(len(host_tie(0, P, N)["new"]) for P, N in TIE_WIDE_SHAPES) == 801801 < 1 << 20


def test_transposed_output_is_sorted_by_row():
    cost = np.array([[-3.0, -9.0], [-8.0, -4.0], [-7.0, -7.0]])   # more rows than columns
    rows, cols, _ = hg.lsap(cost)
    ref = linear_sum_assignment(cost)
    assert np.array_equal(rows, ref[0]) and np.array_equal(cols, ref[1]) and list(rows) == sorted(rows)


def test_scipy_raises_where_rows_share_their_only_column():
    prev = np.array([0] * 9 + [1] * 3 + [2] * 3)
    new = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2] + [0] * 3 + [0] * 3)
    _, _, cost = mo._overlap_costs(prev, new, 3)
    assert np.array_equal(np.isfinite(cost), np.array([[1, 1, 1], [1, 0, 0], [1, 0, 0]], dtype=bool))
    assert mo._feasible(cost)
    with pytest.raises(ValueError):
        linear_sum_assignment(cost)
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        hg.lsap(cost)
    with pytest.raises(ValueError):
        mo.match_clusters(prev, new, "hungarian", 3)


def test_library_exports_and_header_declares_the_entry():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "mused_hip.h")).read()
    for name in ("mused_match_hung_ws_bytes", "mused_match_hung_chain"):
        assert hasattr(L, name) and name in _lib.EXPORTED
        assert re.search(r"\b(long|int)\s+" + name + r"\s*\(", header)
    assert mo.MATCH_FLAG_ASSIGN == 16
