"""The case table of the valued SpMM and of the edge values can tell the rule from its near misses: every named wrong variant
(tests/spmm_valued_cases.py) changes at least one case that the GPU tests compare bit for bit.  No GPU here."""
import numpy as np
import pytest

import spmm_valued_cases as sc


def case(n, r):
    lists = sc.make_lists(n)
    return lists, sc.make_values(lists, 50 + n), sc.make_q(n, r, 7 * r + n)


def test_table_holds_what_the_rules_need():
    lists = sc.make_lists(257)
    vals = sc.make_values(lists, 50 + 257)
    assert {len(nb) for nb in lists} == set(sc.DEGREES)
    flat = np.concatenate(vals)
    assert (flat < 0).any() and (flat == 0.3).any()
    assert ((flat == 0) & ~np.signbit(flat)).any() and ((flat == 0) & np.signbit(flat)).any()
    assert ((flat != 0) & (np.abs(flat) < 2.3e-308)).any()                      # subnormal
    big = np.abs(flat[(np.abs(flat) > 1e-300) & (flat != 0.3)])
    assert big.max() / big.min() > 2.0 ** 50
    Q = sc.make_q(29, 14, 1)
    assert ((Q == 0) & np.signbit(Q)).any()


def test_all_ones_is_the_binary_sum():
    lists, _, Q = case(29, 14)
    ones = [np.ones(len(nb)) for nb in lists]
    want = np.zeros((29, 14))
    for i, nb in enumerate(lists):
        for j in nb:
            want[i] = want[i] + Q[j]
    assert sc.same_bits(sc.restate(lists, ones, Q), want)


@pytest.mark.parametrize("variant", ["wrong_reversed", "wrong_pairwise", "wrong_value_after_sum"])
def test_order_variants_change_a_case(variant):
    changed = 0
    for n in sc.NS:
        lists, vals, Q = case(n, 14)
        changed += not sc.same_bits(getattr(sc, variant)(lists, vals, Q), sc.restate(lists, vals, Q))
    assert changed >= 1


def test_fused_multiply_add_changes_a_case():
    """One rounding per step instead of two, emulated exactly; on all-ones values it changes nothing (the product is exact)."""
    changed = 0
    for n, r in sc.SMALL:
        lists, vals, Q = case(n, r)
        changed += not sc.same_bits(sc.wrong_fma(lists, vals, Q), sc.restate(lists, vals, Q))
        ones = [np.ones(len(nb)) for nb in lists]
        Qp = np.where(Q == 0, 0.0, Q)   # (exact arithmetic has no signed zero)
        assert np.array_equal(sc.wrong_fma(lists, ones, Qp), sc.restate(lists, ones, Qp))
    assert changed >= 1


@pytest.mark.parametrize("M", [2, 3, 5])
def test_value_variants_change_a_case(M):
    masks = sc.make_masks(65, M, 300 + M)
    pattern = np.logical_or.reduce(masks)
    assert not np.array_equal(pattern, pattern.T)
    weights = [0.3, 0.7, 1.9, 1.0, 0.5][:M]
    rowptr, col = sc.lists_of(pattern.T)
    want = sc.values_from_masks(masks, weights, rowptr, col, True)
    assert (want > 0).all()
    assert not sc.same_bits(sc.wrong_values_untransposed(masks, weights, rowptr, col, True), want)


@pytest.mark.parametrize("weights", sc.ORDER_WEIGHTS)
def test_modality_order_decides_the_last_bit(weights):
    masks = sc.make_masks(65, 3, 303)
    pattern = np.logical_or.reduce(masks)
    rowptr, col = sc.lists_of(pattern)
    want = sc.values_from_masks(masks, weights, rowptr, col, False)
    assert not sc.same_bits(sc.wrong_values_reversed_order(masks, weights, rowptr, col, False), want)
    assert want.max() == (2.0 ** 53 if weights[0] > 1 else 2.0 ** 53 + 2.0)


def test_pack_mask_bit_layout():
    A = np.zeros((65, 65), dtype=bool)
    A[0, 0] = A[1, 63] = A[2, 64] = True
    W = sc.pack_mask(A).view(np.uint64)
    assert W.shape == (65, 2) and W[0, 0] == 1 and W[1, 0] == 1 << 63 and W[2, 1] == 1 and W.sum() == 2 + (1 << 63)
