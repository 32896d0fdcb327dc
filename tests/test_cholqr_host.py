"""No GPU: a plain fp64 restatement of the eigenstep's Cholesky-QR satisfies every bound tests/test_gpu_cholqr.py asserts on
the device's outputs, named wrong variants break them, every case keeps its distance from the weak-pivot line, and the case
table reaches the branches it promises."""
import numpy as np
import pytest

import cholqr_cases as cc


@pytest.mark.parametrize("c", cc.TABLE, ids=cc.IDS)
def test_restatement_satisfies_every_bound(c):
    Y = cc.panel(c)
    Q, G, L, weak = cc.restate(Y)
    assert np.array_equal(G, G.T)
    assert np.isfinite(Q).all() and np.isfinite(G).all() and np.isfinite(L).all()
    assert weak == int(c.weak)
    ratios = cc.pass_ratios(Y, Q, G, L)
    print(f"{c.name}: " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("c", cc.SOUND, ids=[c.name for c in cc.SOUND])
def test_two_restated_passes_are_orthonormal(c):
    orth = cc.restated_orthogonality(c)
    print(f"{c.name}: max |Q^T Q - I| = {orth:.3g}, bound {cc.yamamoto(c.n, c.r):.3g}")
    assert orth <= cc.yamamoto(c.n, c.r)
    # the shift alone leaves about delta / pivot = 16 r_block eps on the diagonal: the x 4 of the device test compares
    # with a number of this size, never with an accidental zero
    assert orth >= 8 * max(c.blocks) * cc.EPS


@pytest.mark.parametrize("c", cc.TABLE, ids=cc.IDS)
def test_no_case_is_decided_by_rounding(c):
    p = cc.smallest_pivot(c)
    print(f"{c.name}: smallest pivot / max diag G = {p:.3g}")
    assert (p < cc.PIVOT_LOW) if c.weak else (p > cc.PIVOT_HIGH)


@pytest.mark.parametrize("variant", cc.VARIANTS)
def test_wrong_variant_breaks_a_bound(variant):
    broken = []
    for c in cc.SINGLE:
        if c.weak:
            continue
        Y = cc.panel(c)
        Q, G, L, _ = cc.restate(Y, variant)
        worst = max(cc.single_block_ratios(Y, Q, G, L).values())
        applies = {"tail_unsolved": c.r % 4 != 0, "last_rows_zeroed": c.n % 64 != 0}.get(variant, True)
        assert (worst > 1.0) == applies, (variant, c.name, worst)
        if worst > 1.0:
            broken.append(c.name)
    print(f"{variant}: breaks a bound on {len(broken)} cases")
    assert broken


def test_no_delta_shows_on_the_largest_diagonal_entry():
    """A factor without the shift misses G + delta I by delta = 16 r eps max diag G there: 16 r / (r + 2) >= 5.3 times
    (r + 2) eps |L| |L|^T, against the 2 the bound allows."""
    for c in cc.SINGLE:
        if c.weak:
            continue
        _, G, L, _ = cc.restate(cc.panel(c), "no_delta")
        j = int(np.argmax(np.diag(G)))
        miss = abs(float(L[j] @ L[j]) - (G[j, j] + cc.shift_of(G, c.r)))
        assert miss > 5 * (c.r + 2) * cc.EPS * float(np.abs(L[j]) @ np.abs(L[j])), c.name


def test_table_reaches_every_branch():
    blocks = {b for c in cc.TABLE for b in c.blocks}
    rs = {c.r for c in cc.TABLE}
    ns = {c.n for c in cc.TABLE}
    assert {1, 2, 3, 4, 5, 15, 16, 17, 60, 138, 143} <= {c.r for c in cc.SINGLE}
    assert {144, 145, 266, 286} == {c.r for c in cc.TWO_BLOCK}
    # chol_kernel: a last 16-wide register block that is full, one short, one over; the largest order it is given
    # (16 CH_NB - 1: r = 144 itself goes to the two-block path as 72 + 72)
    assert {0, 1, 15} <= {b % 16 for b in blocks} and max(blocks) == cc.MAX_R == 16 * cc.CH_NB - 1
    # trsm_rows_kernel: fewer columns than a 4-column pass, every r % 4, a tail column with and without the 16-step inner loop
    assert {1, 2, 3} <= blocks and {b % 4 for b in blocks} == {0, 1, 2, 3}
    assert any(b % 4 and b > 16 for b in blocks) and any(b % 4 and 4 < b < 13 for b in blocks)
    # rows: n % 64 and n % 128 on either side of a full block, a square panel, more than two blocks of the split-K Gram
    assert {63, 64, 65, 127, 129} <= ns and (333 in ns or 1000 in ns)
    assert any(c.n == c.r for c in cc.SINGLE) and any(c.n == c.r for c in cc.TWO_BLOCK)
    # the in-place second block with r1 != r2 and with both halves at the largest order
    assert any(c.blocks[0] != c.blocks[1] for c in cc.TWO_BLOCK) and (cc.MAX_R, cc.MAX_R) in {c.blocks for c in cc.TWO_BLOCK}
    assert {"gauss", "orth", "graded", "adj", "zero_col", "dup_col", "low_rank"} == {c.data for c in cc.TABLE}
    assert any(c.weak for c in cc.TWO_BLOCK) and any(c.weak for c in cc.SINGLE)
    assert rs and len({c.name for c in cc.TABLE}) == len(cc.TABLE)
    for c in cc.TABLE:
        assert 1 <= c.r <= min(c.n, 2 * cc.MAX_R)


def test_graded_and_orthonormal_panels_have_the_condition_they_claim():
    for c in cc.TABLE:
        if c.data in ("orth", "graded") and c.r > 1:
            s = np.linalg.svd(cc.panel(c), compute_uv=False)
            want = 1.0 if c.data == "orth" else 1e3
            assert abs(s[0] / s[-1] / want - 1.0) < 1e-10
