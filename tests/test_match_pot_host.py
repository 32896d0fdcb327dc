"""match_clusters(method="pot") on the host: the Sinkhorn-Knopp specification (mused_amd/sinkhorn.py) against a second
statement of the same arithmetic written here with plain loops, the selection rule, the degenerate shapes, the chain replay
and the unchanged Hungarian path.  No GPU, no POT."""
import functools
import math

import numpy as np
import pytest

from conftest import load_golden
from mused_amd import distributed as mdist
from mused_amd import matrix_operations as mo
from mused_amd import sinkhorn as sk

# (W, kp, kn, noise) of the label pairs the device tests use as well
TUPLES = [(500, 4, 4, 0), (500, 4, 4, .05), (2000, 8, 8, .02), (2000, 8, 6, .3), (10000, 150, 150, .02),
          (10000, 150, 150, .5), (2000, 50, 50, .1), (64, 3, 5, .5), (2000, 2, 2, .2), (4000, 256, 256, .3),
          (4000, 200, 256, .6), (300, 1, 3, 0), (300, 3, 1, 0)]
SEEDS = (0, 1, 2)
PLAN_FACTOR = 64   # a different summation tree over at most 256 terms and an exp within an ulp or two


def case(seed, W, kp, kn, noise):
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, kp, W)
    perm = rng.permutation(max(kp, kn))
    new = perm[prev] % kn
    new = np.where(rng.random(W) < noise, rng.integers(0, kn, W), new)
    return prev, new


@functools.lru_cache(maxsize=None)
def host_case(seed, W, kp, kn, noise, min_overlap=3):
    """What the specification gives for a case: dict(prev, new, P, N, feasible, plan, iters, labels, margin)."""
    prev, new = case(seed, W, kp, kn, noise)
    up, un, cost = mo._overlap_costs(prev, new, min_overlap)
    out = dict(prev=prev, new=new, P=len(up), N=len(un), feasible=mo._feasible(cost), cost=cost,
               labels=np.asarray(mo.match_clusters(prev, new, "pot", min_overlap)))
    if out["feasible"]:
        plan, iters = sk.pot_plan(cost)
        thr = plan.max() * 0.5
        out.update(plan=plan, iters=iters, margin=float(np.min(np.abs(plan - thr) / thr)))
    return out


@functools.lru_cache(maxsize=None)
def plan_spread():
    """The yardstick of the plan tolerance: the largest relative difference between the specification in float64 and in
    np.longdouble over the cases where both stop at the same iteration."""
    worst = 0.0
    for tup in TUPLES:
        for seed in SEEDS:
            h = host_case(seed, *tup)
            if not h["feasible"]:
                continue
            wide, iters = sk.pot_plan(h["cost"], np.longdouble)
            if iters == h["iters"]:
                worst = max(worst, float(np.max(np.abs(h["plan"] - wide) / wide)))
    assert 0.0 < worst < 1e-10
    return worst


def loops_sinkhorn(M, reg=0.1, itermax=1000, stop=1e-9):
    """The iteration once more, scalar by scalar."""
    P, N = len(M), len(M[0])
    a, b = [1.0 / P] * P, [1.0 / N] * N
    u, v = list(a), list(b)
    K = [[math.exp(M[i][j] / (-reg)) for j in range(N)] for i in range(P)]
    Kp = [[(1.0 / a[i]) * K[i][j] for j in range(N)] for i in range(P)]
    it = 0
    for ii in range(itermax):
        it = ii + 1
        ktu = [0.0] * N
        for j in range(N):
            s = 0.0
            for i in range(P):
                s += K[i][j] * u[i]
            ktu[j] = s
        v = [b[j] / ktu[j] for j in range(N)]
        for i in range(P):
            s = 0.0
            for j in range(N):
                s += Kp[i][j] * v[j]
            u[i] = 1.0 / s
        if ii % 10 == 0:
            e = 0.0
            for j in range(N):
                s = 0.0
                for i in range(P):
                    s += u[i] * K[i][j] * v[j]
                e += (s - b[j]) ** 2
            if math.sqrt(e) < stop:
                break
    return np.array([[u[i] * K[i][j] * v[j] for j in range(N)] for i in range(P)]), it


def loops_match(prev, new, min_overlap):
    up, un = sorted(set(prev.tolist())), sorted(set(new.tolist()))
    ov = [[sum(1 for p, q in zip(prev.tolist(), new.tolist()) if p == a and q == b) for b in un] for a in up]
    big = [[float(o) if o >= min_overlap else 1e9 for o in row] for row in ov]
    if any(all(x == 1e9 for x in row) for row in big) or any(all(row[j] == 1e9 for row in big) for j in range(len(un))):
        return None, None, new
    cmax = max(max(row) for row in big)
    plan, it = loops_sinkhorn([[x / cmax for x in row] for row in big])
    thr = plan.max() * 0.5
    mapping = {}
    for i in range(len(up)):
        for j in range(len(un)):
            if plan[i, j] > thr:
                mapping[un[j]] = up[i]
    return plan, it, np.array([mapping.get(c, c) for c in new.tolist()])


# the loop statement costs P N W Python steps for the counts: the small shapes, every path of the iteration
LOOP_CASES = [(s,) + t for t in TUPLES if t[1] <= 8 and t[2] <= 8 for s in SEEDS]


@pytest.mark.parametrize("c", LOOP_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_pot_matches_the_loop_statement(c):
    h = host_case(*c)
    plan, it, labels = loops_match(h["prev"], h["new"], 3)
    assert np.array_equal(h["labels"], labels)
    if not h["feasible"]:
        assert plan is None and h["labels"] is not None and np.array_equal(h["labels"], h["new"])
        return
    assert it == h["iters"]
    assert np.max(np.abs(plan - h["plan"]) / h["plan"]) <= PLAN_FACTOR * plan_spread()


def test_counts_of_the_case_table():
    """The table's make-up: infeasible pairs, pairs that run all 1000 iterations, several selections in a row / column."""
    hs = [host_case(s, *t) for t in TUPLES for s in SEEDS]
    assert len(hs) == 39
    assert sum(not h["feasible"] for h in hs) == 6
    feas = [h for h in hs if h["feasible"]]
    assert sum(h["iters"] == 1000 for h in feas) >= 5 and sum(1 < h["iters"] < 1000 for h in feas) >= 5
    multi = 0
    for h in feas:
        sel = h["plan"] > h["plan"].max() * 0.5
        multi += bool((sel.sum(axis=0) > 1).any() or (sel.sum(axis=1) > 1).any())
    assert multi >= 1
    assert sorted(h["margin"] for h in feas)[1] > 1e-2   # one pair sits near the threshold, the next is far from it


def test_larger_row_wins_a_shared_column():
    """Two previous labels select one new label: np.where runs row-major, the dict keeps the last, i.e. the larger row."""
    prev = np.array([5] * 40 + [9] * 40 + [2] * 30)
    new = np.array([7] * 80 + [1] * 30)
    up, un, cost = mo._overlap_costs(prev, new, 3)
    plan, _ = sk.pot_plan(cost)
    sel = plan > plan.max() * 0.5
    j7 = list(un).index(7)
    assert sel[:, j7].sum() == 2   # the rows of 5 and 9
    top = int(np.max(np.where(sel[:, j7])[0]))
    out = mo.match_clusters(prev, new, "pot", 3)
    assert set(out[:80]) == {up[top]} and up[top] == 9
    assert sk.select(plan)[j7] == top


def test_degenerate_shapes_and_arguments():
    new = np.array([3] * 20 + [4] * 20 + [8] * 20)
    one_prev = mo.match_clusters(np.zeros(60, dtype=int) + 6, new, "pot", 3)   # P = 1: every column selects row 0
    assert np.array_equal(one_prev, np.full(60, 6))
    one_new = mo.match_clusters(new, np.zeros(60, dtype=int) + 2, "pot", 3)    # N = 1: the largest row wins
    assert np.array_equal(one_new, np.full(60, 8))
    prev = np.array([0, 0, 0, 1, 1, 1])
    inf_new = np.array([0, 1, 2, 0, 1, 2])                                     # no overlap reaches 3
    assert mo.match_clusters(prev, inf_new, "pot", 3) is inf_new
    assert mo.match_clusters(None, new, "pot", 3) is new
    assert mo.match_clusters([], new, "pot", 3) is new
    with pytest.raises(ValueError):
        mo.match_clusters(new, new, "nope", 3)


def test_sinkhorn_numerical_error_branch_keeps_previous_scalings():
    """A cost so large that K underflows to 0: the specification returns the plan of the scalings before the failure."""
    M = np.array([[0.0, 1e6], [1e6, 1e6]])
    with np.errstate(divide="ignore", invalid="ignore"):
        plan, it = sk.sinkhorn_knopp(np.full(2, .5), np.full(2, .5), M, 0.1)
    assert it == 1 and np.all(np.isfinite(plan))
    assert np.array_equal(plan, np.outer(np.full(2, .5), np.full(2, .5)) * np.exp(M / -0.1))


def drift_chain(seed=0, W=500, ks=(4, 5, 3, 4, 5, 3)):
    """Windows whose labels drift: `case`'s rule applied to the previous window's labels, k going 4 -> 5 -> 3."""
    rng = np.random.default_rng(seed)
    cur = rng.integers(0, ks[0], W)
    out = [cur]
    for k in ks[1:]:
        kp = int(cur.max()) + 1
        perm = rng.permutation(max(kp, k))
        nxt = perm[cur] % k
        nxt = np.where(rng.random(W) < 0.3, rng.integers(0, k, W), nxt)
        if len(out) == 3:
            nxt[:2] = 7   # a label with two rows: no overlap of its column reaches 3, the window passes through unmatched
        out.append(nxt)
        cur = nxt
    return np.array(out)


def host_chain(raw, prev=None, min_overlap=3):
    out = []
    for r in raw:
        m = mo.match_clusters(prev, r, "pot", min_overlap)
        if m is None or len(m) == 0:
            m = np.full(len(r), 0)
        prev = m
        out.extend(m)
    return np.array(out)


def test_replay_label_chain_passes_the_method_on():
    raw = drift_chain()
    chain = host_chain(raw).reshape(raw.shape)
    feas = [mo._feasible(mo._overlap_costs(a, b, 3)[2]) for a, b in zip(chain[:-1], raw[1:])]
    # window 3 carries a label with two rows: it passes through unmatched, and as the previous window it leaves window 4
    # a row without an overlap of 3
    assert feas == [True, True, False, False, True]
    assert np.array_equal(chain[3], raw[3]) and not np.array_equal(chain[2], raw[2])
    assert np.array_equal(mdist.replay_label_chain(raw, mo.match_clusters, method="pot"), host_chain(raw))
    hung = mdist.replay_label_chain(raw, mo.match_clusters)
    prev, ref = None, []
    for r in raw:
        prev = mo.match_clusters(prev, r, "hungarian", 3)
        ref.extend(prev)
    assert np.array_equal(hung, np.array(ref))


def test_hungarian_labels_unchanged():
    g = load_golden("edges")
    assert np.array_equal(mo.match_clusters(g["match_prev"], g["match_new"], "hungarian", 3), g["match_out"])
    assert np.array_equal(mo.match_clusters(g["match_prev"], g["match_new_inf"], "hungarian", 3), g["match_out_inf"])
