"""tests/knn_fused_cases.py on the CPU: every case reaches the path of knn_fused_t it is named for (by the schedule model),
the integer rows make the l2 reference exact, the narrow rows tie across the k-th boundary often enough to decide the tie
rule, and the cosine rows leave a gap that fp64 cannot bridge (no GPU)."""
import numpy as np
import pytest

import knn_fused_cases as kc


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_reaches_the_path_it_is_named_for(name):
    c = kc.case(name)
    s = kc.schedule(c.n, c.k, c.cap)
    assert 1 <= c.k <= c.n and c.k <= c.cap <= 1024
    for field, want in c.reaches.items():
        assert getattr(s, field) == want, (name, field, s)
    # a DIRECT first phase needs its fixed slots in the list and no column tile reached from both sides
    if s.direct:
        assert (2 * s.a + 1) * kc.TILE <= c.cap and s.tiles >= 2 * s.a + 2
    # the phases cover every cyclic distance once
    flat = [d for lo, hi in s.phases for d in range(lo, hi + 1)]
    assert flat == list(range(s.tiles // 2 + 1))


def test_the_table_covers_every_branch_of_the_schedule():
    S = {c.name: kc.schedule(c.n, c.k, c.cap) for c in kc.CASES}
    assert {s.pl for s in S.values()} == {4, 8, 16}
    assert {s.a for s in S.values() if s.direct} == {0, 1, 2}
    assert any(not s.direct and s.tiles in (4, 5) and s.a == 2 for s in S.values())          # 385..640 rows, large cap
    assert any(len(s.phases) == 3 for s in S.values()) and any(len(s.phases) == 1 for s in S.values())
    assert any(s.first_select_early for s in S.values())
    assert any(s.tiles % 2 == 0 and s.tiles > 1 for s in S.values()) and any(s.tiles % 2 == 1 for s in S.values())
    assert any(c.n % kc.TILE == 1 for c in kc.CASES) and any(c.n % kc.TILE == 0 for c in kc.CASES)
    assert any(c.n == c.k == c.cap for c in kc.CASES) and any(c.k == 1 for c in kc.CASES)
    assert any(c.cap == 704 for c in kc.CASES) and any(4 * c.k + 128 == c.cap == 1024 for c in kc.CASES)
    # what the older primitive-level test reaches (cap = 1024): two band launches in every case, a = 2
    for n, k in [(100, 7), (128, 128), (300, 20), (1024, 50), (1500, 50), (2000, 200), (2900, 31)]:
        s = kc.schedule(n, k, 1024)
        assert len(s.phases) <= 2 and s.pl == 16 and (s.a == 2 or not s.direct)
    # the engine's own window (W = 10,000, k = 50, cap = 704) is where the tripling branch ran so far
    assert kc.schedule(10000, 51, 704).tripled >= 1


def test_schedule_model_in_ring_mode():
    for q in kc.FRIENDLY:
        s = kc.schedule(q.W, q.k, q.cap, ring=True)
        assert s.kthr == 2 * q.k and s.direct
        assert s.a == (2 if q.cap == 1024 else 1)
    s = kc.schedule(kc.GROWTH.W, kc.GROWTH.k, kc.GROWTH.cap, ring=True)                        # 5 tiles: pushes only
    assert not s.direct and s.phases == ((0, 1), (2, 2)) and s.kthr == 2 * kc.GROWTH.k
    # the distribution shift needs a select BETWEEN two phases (only that lowers a threshold); at three tiles there is none
    s = kc.schedule(kc.SHIFT_W, kc.SHIFT_K, 1024, ring=True)
    assert not s.direct and s.phases == ((0, 1), (2, 2)) and s.kthr == 2 * kc.SHIFT_K
    assert kc.schedule(kc.SINGLE_W, kc.SHIFT_K, 1024, ring=True).phases == ((0, 1),)
    assert kc.schedule(300, 200, 512, ring=True).kthr == 200                                   # cap / 4 < k: kthr = k


@pytest.mark.parametrize("name", kc.NAMES)
def test_integer_rows_make_the_l2_reference_exact(name):
    c = kc.case(name)
    for vname in ("l2_f32_narrow", "l2_f64_wide", "l2_f32_wide"):
        X = kc.rows_as(name, vname)
        S = kc.scores(name, vname)
        assert np.array_equal(X.astype(np.float64), kc.rows(name, kc.variant(vname)[3]))       # the cast lost nothing
        X64 = X.astype(np.float64)
        G = X64 @ X64.T
        nrm = (X64 * X64).sum(axis=1)
        S64 = nrm[:, None] - 2.0 * G + nrm[None, :]
        assert np.array_equal(S64, S.astype(np.float64)) and np.abs(S).max() < 2 ** 40 and (S >= 0).all()
        assert len(np.unique(X, axis=0)) == c.n, "duplicate rows"
        assert (np.diag(S) == 0).all()
        L = kc.reference_lists(name, vname)
        assert L.shape == (c.n, c.k) and (np.diff(L, axis=1) > 0).all()
        # the own column ranks first (distance 0, no duplicate rows)
        assert (L == np.arange(c.n)[:, None]).any(axis=1).all()


@pytest.mark.parametrize("name", kc.NAMES)
def test_narrow_rows_tie_across_the_boundary(name):
    c = kc.case(name)
    tied, run = kc.boundary_ties(kc.scores(name, "l2_f32_narrow"), c.k)
    print(f"{name}: {tied} rows with a tie across the k-th boundary, longest run of equal scores {run}")
    assert run <= kc.MAX_EQUAL_RUN
    if c.n >= 1000 and c.k <= 55:
        assert tied >= kc.MIN_BOUNDARY_TIES
    # the tie rule decides a list: the (k+1)-th in (score, column) order has the k-th's score and a larger column
    if tied:
        S = kc.scores(name, "l2_f32_narrow")
        order = np.argsort(S, axis=1, kind="stable")
        r = np.flatnonzero(S[np.arange(c.n), order[:, c.k - 1]] == S[np.arange(c.n), order[:, c.k]])
        assert (order[r, c.k - 1] < order[r, c.k]).all()


def test_ties_are_decided_somewhere_in_every_select_size():
    sizes = set()
    for c in kc.CASES:
        if kc.boundary_ties(kc.scores(c.name, "l2_f32_narrow"), c.k)[0] >= kc.MIN_BOUNDARY_TIES:
            sizes.add(kc.schedule(c.n, c.k, c.cap).pl)
    assert sizes == {4, 8, 16}


@pytest.mark.parametrize("name", kc.NAMES)
def test_cosine_rows_leave_a_gap(name):
    assert np.finfo(kc.LD).eps <= 2.0 ** -63, "np.longdouble is no wider than fp64 here"
    c = kc.case(name)
    for vname in ("cos_f64_gauss", "cos_f32_gauss"):
        S = kc.scores(name, vname)
        gap = kc.smallest_gap(S, c.k)
        print(f"{name} {vname}: smallest gap between the k-th and the (k+1)-th score {gap:.2e}")
        assert gap >= kc.COS_GAP
        assert not np.isnan(S.astype(np.float64)).any()


def test_reference_is_a_stable_lexsort():
    S = np.array([[3, 1, 1, 0, 1], [0, 0, 0, 0, 0]])
    assert kc.topk(S, 3).tolist() == [[1, 2, 3], [0, 1, 2]] and kc.topk(S, 5).tolist() == [[0, 1, 2, 3, 4]] * 2
    assert kc.mask_of(kc.topk(S, 3)[:1], 1, 2).tolist() == [[0b1110, 0]]
    assert kc.mask_of(kc.topk(S, 3), 2, 1).tolist() == [[0b1110], [0b101]]
    assert kc.boundary_ties(S, 2) == (2, 5) and kc.boundary_ties(S, 1) == (1, 5)
    assert kc.smallest_gap(np.array([[0.0, 1.0, 3.0]]), 2) == 2.0


def test_padded_pitches_select_both_load_variants():
    d = kc.rows(kc.PADDED, "wide").shape[1]
    assert [(kc.loads_vector(t, d + e), v) for t, e, v in kc.PITCHES] == [(False, "scalar"), (True, "vector"), (True, "vector")]
    assert kc.loads_vector(np.float32, d) and kc.loads_vector(np.float64, d)


def test_hop_streams_are_what_the_tests_assume():
    # positions: the last window of the shifted sequence ends below 2^30
    for q in kc.FRIENDLY:
        lo0 = kc.POSITION_LIMIT - q.W - 8 * q.hop
        assert lo0 + (q.windows - 1) * q.hop + q.W < kc.POSITION_LIMIT and len(kc.friendly_stream(q.hop)) >= q.W + (q.windows - 1) * q.hop
    assert any(q.hop % kc.TILE for q in kc.FRIENDLY) and any((kc.POSITION_LIMIT - q.W - 8 * q.hop) % q.W for q in kc.FRIENDLY)
    # the distribution shift: consecutive calls overlap as their n_new says, and at the flagged call 10 near rows stay
    X, W = kc.shift_stream(), kc.SHIFT_W
    for calls, width, stream in ((kc.SHIFT_CALLS, W, X), (kc.SINGLE_CALLS, kc.SINGLE_W, kc.single_phase_stream())):
        prev = None
        for lo, n_new in calls:
            assert lo + width <= len(stream) and (n_new == 0 or lo - prev == n_new)
            prev = lo
    lo, n_new = kc.SHIFT_CALLS[kc.SHIFT_FLAGGED_AT]
    assert W - n_new == kc.SHIFT_NEAR - lo == 10 < kc.SHIFT_K
    # no far column can lie below a near row's threshold: the far block is farther from every near row than any near row is
    near, far = X[:kc.SHIFT_NEAR], X[kc.SHIFT_NEAR:]
    d_near = ((near[:, None, :] - near[None, :, :]) ** 2).sum(axis=2).max()
    d_far = ((near[:, None, :] - far[None, :, :]) ** 2).sum(axis=2).min()
    assert d_far > 10 * d_near
