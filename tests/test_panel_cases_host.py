"""No GPU: the plain fp64 restatements of the LU and Householder panel factorisations (tests/panel_cases.py) satisfy every
assertion tests/test_gpu_panel.py makes on the device's outputs, every named wrong variant breaks one, the exact cases are
exact in rational arithmetic, the pivot order of every case that asserts it is decided by a gap and not by rounding, and the
case tables reach the branches of csrc/panel.hip they promise."""
import os

import numpy as np
import pytest
import scipy.linalg

import panel_cases as pc


# ---- LU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.LU_TABLE, ids=pc.LU_IDS)
def test_lu_restatement_satisfies_every_assertion(c):
    PL, ps = pc.lu_restated(c)
    assert PL.shape == (c.n, c.k)
    ratios, bad = pc.lu_verdict(c, PL, ps)
    print(f"{c.name}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert not bad, bad


@pytest.mark.parametrize("c", [c for c in pc.LU_TABLE if c.data in ("gauss", "adj")],
                         ids=[c.name for c in pc.LU_TABLE if c.data in ("gauss", "adj")])
def test_lu_restatement_is_scipys_on_tie_free_panels(c):
    ref = scipy.linalg.lu(pc.panel(c), permute_l=True)[0]
    np.testing.assert_allclose(pc.lu_restated(c)[0], ref, rtol=0, atol=1e-11)


@pytest.mark.parametrize("c", [c for c in pc.LU_TABLE if c.exact], ids=[c.name for c in pc.LU_TABLE if c.exact])
def test_exact_cases_are_exact(c):
    """the fp64 elimination equals the one in fractions.Fraction: no step rounds, so any correct kernel gives these bits"""
    PL, ps = pc.lu_restated(c)
    PLx, psx = pc.exact_lu(pc.panel(c))
    assert np.array_equal(ps, psx)
    assert np.all(PL == PLx.astype(np.float64)) and all(float(x) == x for x in PLx.ravel())
    ties = pc.step_ties(pc.panel(c))
    assert all(len(losers) for _, losers in ties[: min(c.k, c.n - 1)]) or c.data == "zero_col", "every step is a tie"
    if c.data == "zeros":
        assert list(pc.pivot_rows(ps, c.k)) == list(range(c.k)) and np.all(np.tril(PL, -1) == 0)
    if c.data == "zero_col":
        z = (2 * c.r) // 3
        win = pc.pivot_rows(ps, c.k)[z]
        assert z < c.k and not pc.panel(c)[:, z].any() and win == min(set(range(c.n)) - set(pc.pivot_rows(ps, c.k)[:z]))
        assert z + 1 < c.k and np.any(PL[:, z + 1:] != 0), "the steps behind the zero column go on"
        assert any(len(losers) for _, losers in ties) and not all(len(losers) == c.n - 1 - j for j, (_, losers) in enumerate(ties))


@pytest.mark.parametrize("c", [c for c in pc.LU_TABLE if c.order and not c.exact],
                         ids=[c.name for c in pc.LU_TABLE if c.order and not c.exact])
def test_pivot_order_is_decided_by_a_gap(c):
    g = pc.gap(pc.panel(c))
    print(f"{c.name}: seed {c.seed}, largest runner-up / winner = 1 - {1 - g:.3g}")
    assert g <= 1.0 - pc.GAP
    # the longdouble elimination and the fp64 one pick the same rows
    assert np.array_equal(pc.lu_restate(pc.panel(c), dtype=pc.LD)[1], pc.lu_restated(c)[1])


def test_only_the_rank_deficient_twin_panel_leaves_its_order_open():
    """order=False: adj_dup with more columns than distinct rows, and nothing else.  Past the rank the winner is a rounding
    residue: the gap condition fails there for every seed."""
    loose = [c for c in pc.LU_TABLE if not c.order]
    assert [c.name for c in loose] == ["lu_adj_dup_n300_r139"]
    for c in loose:
        Y = pc.panel(c)
        assert c.data == "adj_dup" and c.k > pc.DISTINCT and len(np.unique(Y, axis=0)) == pc.DISTINCT
        assert np.linalg.matrix_rank(Y) == pc.DISTINCT and pc.gap(Y) > 1.0 - pc.GAP
    for c in pc.LU_TABLE:
        if c.data == "adj_dup":
            assert len(np.unique(pc.panel(c), axis=0)) == pc.DISTINCT
            assert c.order == (c.k <= pc.DISTINCT)


@pytest.mark.parametrize("variant", pc.LU_VARIANTS)
def test_wrong_lu_variant_breaks_an_assertion(variant):
    caught = {}
    for c in pc.LU_TABLE:
        PL, ps = pc.lu_restate(pc.panel(c), variant)
        _, bad = pc.lu_verdict(c, PL, ps)
        if bad:
            caught[c.name] = bad
    print(f"{variant}: caught on {len(caught)} cases: " + "; ".join(f"{k} {v}" for k, v in caught.items()))
    assert caught, f"{variant}: no case notices it -- a case is missing"
    kinds = {a for bad in caught.values() for a in bad}
    want = {"tie_last": "order", "tie_position": "order", "skip_last_update": "backward", "panel_tail": "backward"}[variant]
    assert want in kinds


def _placements(c):
    """which pairs (tied winner, loser) the steps of an exact case hold, by the places the five implementations of the tie
    rule keep them in"""
    found = set()
    for win, losers in pc.step_ties(pc.panel(c)):
        if not len(losers):
            continue
        w, l = win, np.asarray(losers)
        if np.any(l // 16 == w // 16):
            found.add("same 16 rows")                       # lu_partial_colmax, luc_candidates: the serial scan
        if np.any(l // 16 == w // 16 + 1):
            found.add("next 16 rows")
        if np.any(l // 32 == w // 32 + 1):
            found.add("next 32 rows")                       # two workgroups of luc_step_kernel
        if np.any((l // 16 % 1024) // 64 != (w // 16 % 1024) // 64):
            found.add("waves of lu_pivot_kernel")
        if np.any((l // 32 % 256) // 64 != (w // 32 % 256) // 64):
            found.add("waves of luc_step_kernel")
        if np.any((l % 1024) // 64 != (w % 1024) // 64):
            found.add("waves of lu_panel_kernel")
        if np.any((l // 16 % 1024 == w // 16 % 1024) & (l // 16 != w // 16)):
            found.add("one thread of lu_pivot_kernel")      # partials i and i + 1024
        if np.any(l == w + 1024):
            found.add("rows t and t + 1024")                # one thread of lu_panel_kernel
        if pc.lu_route(c) == "panel10" and w >= pc.PANEL3_MAX:
            found.add("winner beyond row 3072")
        if w > 0 and np.any(l > w):
            found.add("winner is not row 0")
    return found


def test_ties_fall_where_the_tie_rule_is_implemented():
    found = set()
    for c in pc.LU_TABLE:
        if c.exact:
            found |= _placements(c)
    print(sorted(found))
    assert found >= {"same 16 rows", "next 16 rows", "next 32 rows", "waves of lu_pivot_kernel", "waves of luc_step_kernel",
                     "waves of lu_panel_kernel", "rows t and t + 1024", "winner beyond row 3072", "winner is not row 0"}
    # one thread of lu_pivot_kernel holds two partials only from n = 16,385 on: outside the table (the chain stops at
    # n_max windows of about 10^4 rows), noted here so that nobody reads the table as covering it
    assert "one thread of lu_pivot_kernel" not in found


def test_lu_table_reaches_every_branch():
    T = pc.LU_TABLE
    assert len({c.name for c in T}) == len(T)
    assert {c.n for c in T if c.data == "gauss"} >= {1, 3, 15, 16, 17, 33, 1023, 1024, 1025, 2049, 3072, 3073, 10240, 10241}
    assert {c.r for c in T if c.data == "gauss"} >= {1, 2, 3, 4, 5, 7, 8, 9}
    for route in ("panel3", "panel10"):
        tails = {t for c in T if pc.lu_route(c) == route for t in pc.lu_tails(c)}
        assert tails == {1, 2, 3, 4}, (route, tails)
        assert any(len(pc.lu_tails(c)) > 1 for c in T if pc.lu_route(c) == route), "a panel behind a finished one"
        assert {c.data for c in T if pc.lu_route(c) == route} >= {"gauss", "hadamard", "zeros", "zero_col"}
    assert {c.data for c in T if pc.lu_route(c) == "column"} >= {"gauss", "hadamard", "zero_col"}
    assert any(c.n == pc.PANEL3_MAX for c in T) and any(c.n == pc.PANEL3_MAX + 1 for c in T)
    assert any(c.n == pc.PANEL10_MAX for c in T) and any(c.n == pc.PANEL10_MAX + 1 for c in T)
    # rows t and t + 1024 in one thread of the panel kernel; the last of the 3 / 10 row slots of a thread in use
    assert any(1024 < c.n <= pc.PANEL3_MAX for c in T) and any(c.n > 2048 and pc.lu_route(c) == "panel3" for c in T)
    assert any(c.n > 9 * 1024 and pc.lu_route(c) == "panel10" for c in T)
    # r > n (k = n: the columns behind k are U and are not returned), r > 1024, the chain's own shape
    assert {(3, 7), (8, 12), (40, 1030), (300, 139)} <= {(c.n, c.r) for c in T}
    assert any(c.r > 1024 for c in T) and any(c.r > c.n for c in T if c.exact)
    assert {c.data for c in T} == {"gauss", "adj", "adj_dup", "hadamard", "zeros", "zero_col"}
    assert all(c in T for c in pc.LU_SCALED) and len(pc.LU_SCALED) == 7
    assert {pc.lu_route(c) for c in pc.LU_SCALED} == {"panel3", "panel10", "column"}


def test_library_names_the_same_routes():
    """mused_lu_path needs no device: the kernels each case is listed under are the ones the library picks by default."""
    from mused_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    L = _lib.lib()
    mode = L.mused_lu_mode()   # 1 unless MUSED_LU_MODE / MUSED_LU_BLOCKED are set in this environment
    assert mode in (0, 1, 2)
    for c in pc.LU_TABLE:
        assert L.mused_lu_path(c.n, c.r) == (mode if mode != 1 else 0 if pc.lu_route(c) == "column" else 1), c.name
    assert L.mused_lu_path(0, 1) == -1 and L.mused_lu_path(1, 0) == -1


# ---- QR --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", pc.QR_TABLE, ids=pc.QR_IDS)
def test_qr_restatement_satisfies_every_assertion(c):
    Q, tau, alpha, beta = pc.qr_restated(c)
    ratios, bad = pc.qr_verdict(c, Q)
    print(f"{c.name}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert not bad, bad
    if c.data == "zeros":
        assert not tau.any() and np.array_equal(Q, np.eye(c.n, c.r))
    if c.data == "zero_col":
        assert tau[(2 * c.r) // 3] == 0.0 and np.count_nonzero(tau == 0.0) == 1 + (c.n == c.r)
    if c.data == "zero_sub":
        m = min(2, c.r)
        assert not tau[:m].any() and list(alpha[:m]) == [-2.5, 1.5][:m] and (c.r <= 2 or tau[2:c.r - (c.n == c.r)].all())


@pytest.mark.parametrize("variant", pc.QR_VARIANTS)
def test_wrong_qr_variant_breaks_an_assertion(variant):
    caught = {}
    for c in pc.QR_TABLE:
        if c.n * c.r > 1030 * 138:
            continue   # (the largest panel adds nothing here)
        Q = pc.qr_restate(pc.panel(c), variant)[0]
        _, bad = pc.qr_verdict(c, Q)
        if bad:
            caught[c.name] = bad
    print(f"{variant}: caught on {len(caught)} cases: " + "; ".join(f"{k} {v}" for k, v in caught.items()))
    assert caught, f"{variant}: no case notices it -- a case is missing"
    if variant == "chunk_dropped":
        assert all(name in caught for name in pc.QR_IDS if "_n513_" in name and "zeros" not in name)
        assert not any("_n511_" in name or "_n512_" in name for name in caught)
    if variant == "tau0_not_skipped":
        assert {"qr_zero_sub_n17_r15", "qr_zero_col_n513_r17", "qr_zeros_n17_r16"} <= set(caught)


def test_qr_table_reaches_every_branch():
    T = pc.QR_TABLE
    assert len({c.name for c in T}) == len(T) and all(1 <= c.r <= c.n for c in T)
    assert {c.n for c in T} >= {1, 2, 16, 17, 511, 512, 513, 1024, 1025, 1030}
    assert {c.r for c in T} >= {1, 2, 15, 16, 17, 63, 64, 65}
    assert {(40, 40), (1030, 138), (520, 515)} <= {(c.n, c.r) for c in T}
    # qr_dot_kernel: one chunk, a full one, a second of one row, two full, a third; qr_house_kernel: a second stride
    assert {-(-c.n // pc.QR_CHUNK) for c in T} == {1, 2, 3}
    assert any(c.n > 1024 for c in T) and any(c.n == 1024 for c in T)
    # first_chunk > 0: a column j >= 512
    assert any(c.r > pc.QR_CHUNK for c in T)
    # the 16 lanes of a row in qr_update_kernel and the 64 columns of a qr_dot_kernel block, on either side
    for edge in (16, 64):
        assert {edge - 1, edge, edge + 1} <= {c.r for c in T if c.n > 2 * pc.QR_CHUNK}
    assert any(c.n == c.r for c in T) and any(c.n == 1 for c in T)
    assert {c.data for c in T} == {"gauss", "orth", "graded", "adj", "adj_dup", "zeros", "zero_col", "zero_sub"}
    assert all(c in T for c in pc.QR_SCALED) and len(pc.QR_SCALED) == 6


@pytest.mark.parametrize("c", pc.LU_SCALED + pc.QR_SCALED, ids=[c.name for c in pc.LU_SCALED + pc.QR_SCALED])
def test_restatements_are_scale_invariant(c):
    """2^200 and 2^-200 change exponents only: neither restatement rounds differently, so a kernel has no reason to"""
    Y = pc.panel(c)
    for s in pc.SCALES:
        if c.name.startswith("lu_"):
            PL, ps = pc.lu_restate(Y * s)
            assert np.array_equal(ps, pc.lu_restated(c)[1]) and np.array_equal(pc.bits(PL), pc.bits(pc.lu_restated(c)[0]))
        else:
            assert np.array_equal(pc.bits(pc.qr_restate(Y * s)[0]), pc.bits(pc.qr_restated(c)[0]))
