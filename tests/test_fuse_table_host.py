"""The host side of the fusion by agreement threshold (mused_amd/fusion.py), no GPU: `threshold_table` against a scalar-loop
restatement, `fuse_table_numpy` against direct NumPy, every bad argument of the rule, and the named wrong variants, each of
which changes at least one case (so the cases can tell them from the rule)."""
import numpy as np
import pytest

import fuse_table_cases as fc
from mused_amd import fusion


def outcome(fn, *args):
    """The table as a tuple, or "ValueError"."""
    try:
        return tuple(int(x) for x in fn(*args))
    except ValueError:
        return "ValueError"


@pytest.mark.parametrize("weights,tau", fc.threshold_cases())
def test_threshold_table_is_the_scalar_loop(weights, tau):
    assert outcome(fusion.threshold_table, weights, tau) == outcome(fc.scalar_table, weights, tau)


def test_named_tables():
    for M in range(1, 9):
        ones = (1.0,) * M
        assert np.array_equal(fusion.threshold_table(ones, 1.0), fc.or_table(M))
        assert np.array_equal(fusion.threshold_table(ones, float(M)), fc.and_table(M))
        for t in range(1, M + 1):
            assert np.array_equal(fusion.threshold_table(ones, float(t)), fc.at_least_table(M, t))
    assert np.array_equal(fusion.threshold_table((1.0, 0.5, 0.75), 1.25), fc.majority_table(3))
    drops = fusion.table_bits(fusion.threshold_table((1.0, 0.5, 0.75), 1.5))
    assert [s for s in range(8) if drops[s]] == [0b011, 0b101, 0b111]   # {1, 2} = 0b110 scores 1.25


def test_order_of_the_additions_decides():
    assert fusion.subset_score((0.1, 0.2, 0.3), 7) == 0.6000000000000001 and fusion.subset_score((0.3, 0.2, 0.1), 7) == 0.6
    t = fusion.threshold_table((0.1, 0.2, 0.3), 0.6000000000000001)
    assert [s for s in range(256) if fusion.table_bits(t)[s]] == [7]
    with pytest.raises(ValueError, match="above the score of all 3"):
        fusion.threshold_table((0.3, 0.2, 0.1), 0.6000000000000001)
    big = 2.0 ** 53
    assert fusion.subset_score((big, 1.0, 1.0), 7) == big and fusion.subset_score((1.0, 1.0, big), 7) == big + 2.0
    with pytest.raises(ValueError):
        fusion.threshold_table((big, 1.0, 1.0), big + 2.0)
    assert np.array_equal(fusion.threshold_table((1.0, 1.0, big), big + 2.0), fc.and_table(3))


@pytest.mark.parametrize("name", list(fc.WRONG_VARIANTS))
def test_wrong_variant_changes_a_case(name):
    wrong = fc.WRONG_VARIANTS[name]
    changed = [c for c in fc.threshold_cases() if outcome(wrong, *c) != outcome(fusion.threshold_table, *c)]
    assert changed, f"no case tells '{name}' from the rule"


@pytest.mark.parametrize("M", range(1, 9))
def test_fuse_table_numpy(M):
    n = 24
    mats = fc.make_masks(n, M, 40 + M)
    assert fc.subsets_present(mats) == set(range(1 << M)), "a subset pattern is missing from the inputs"
    count = sum(a.astype(np.int64) for a in mats)
    for t in range(1, M + 1):
        got = fusion.fuse_table_numpy(mats, fusion.threshold_table((1.0,) * M, float(t)))
        assert got.dtype == np.int64 and np.array_equal(got, (count >= t).astype(np.int64))
    assert np.array_equal(fusion.fuse_table_numpy(mats, fc.or_table(M)), np.logical_or.reduce(mats).astype(np.int64))
    assert np.array_equal(fusion.fuse_table_numpy(mats, fc.and_table(M)), np.logical_and.reduce(mats).astype(np.int64))
    # any nonzero is an edge; a wrong table bit shows: every table that differs from T in one bit changes the output
    T = fc.random_tables(M, 1, M)[0]
    ref = fusion.fuse_table_numpy([a * 2.5 for a in mats], T)
    assert np.array_equal(ref, fusion.fuse_table_numpy(mats, T))
    for s in range(1, 1 << M):
        flipped = T.copy()
        flipped[s >> 6] ^= np.uint64(1 << (s & 63))
        assert not np.array_equal(fusion.fuse_table_numpy(mats, flipped), ref)


def test_weighted_fusion_on_matrices():
    mats = fc.make_masks(24, 3, 5)
    w = (1.0, 0.5, 0.75)
    score = sum(wm * a for wm, a in zip(w, mats))   # exact in fp64 whatever the order: multiples of 0.25 below 4
    for tau in (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.25):
        got = fusion.fuse_table_numpy(mats, fusion.threshold_table(w, tau))
        assert np.array_equal(got, (score >= tau).astype(np.int64))


def test_bad_arguments_raise():
    for bad_w in ((1.0, 0.0), (1.0, -2.0), (1.0, np.nan), (np.inf, 1.0), (), (1.0,) * 9, ("a", 1.0), None, 3.0):
        with pytest.raises(ValueError):
            fusion.threshold_table(bad_w, 1.0)
    for bad_tau in (0.0, -1.0, np.nan, np.inf, -np.inf, 2.5, "x", None):
        with pytest.raises(ValueError):
            fusion.threshold_table((1.0, 1.0), bad_tau)
    assert np.array_equal(fusion.threshold_table((1.0, 1.0), 2.0), fc.and_table(2))   # tau = the total is the AND
    mats = fc.make_masks(8, 2, 0)
    with pytest.raises(ValueError, match="bit 0"):
        fusion.fuse_table_numpy(mats, fc.table_of_bits([1, 1, 1, 1]))
    with pytest.raises(ValueError, match="at or above"):
        fusion.fuse_table_numpy(mats, fc.table_of_bits([0, 1, 1, 1, 1]))
    with pytest.raises(ValueError):
        fusion.fuse_table_numpy(mats, np.zeros(3, dtype=np.uint64))
    with pytest.raises(ValueError):
        fusion.fuse_table_numpy(mats * 5, fc.or_table(8))          # 10 matrices
    with pytest.raises(ValueError):
        fusion.fuse_table_numpy([mats[0], mats[1][:4, :4]], fc.or_table(2))


def test_fusion_module_needs_no_torch():
    import subprocess
    import sys

    code = "import sys; import mused_amd.fusion; assert 'torch' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], cwd=str(__import__("pathlib").Path(__file__).parents[1])).returncode == 0


def test_pack_and_unpack_are_inverse():
    for n, words in ((1, 1), (65, 2), (65, 5), (130, 3)):
        A = fc.make_masks(n, 1, n)[0]
        m = fc.pack_mask(A, words)
        assert m.shape == (n, words) and m.dtype == np.int64
        bits = fc.unpack_mask(m, n)
        assert np.array_equal(bits[:, :n], A) and not bits[:, n:].any()
        j = n - 1
        assert ((int(m.view(np.uint64)[0, j >> 6]) >> (j & 63)) & 1) == int(A[0, j])
