"""tests/adjacency_cases.py against direct boolean NumPy, and every named wrong variant against the case table: each must
break a case, at the sizes the table holds for that edge (no GPU)."""
import numpy as np
import pytest

import adjacency_cases as ac


def test_table_holds_the_sizes_it_claims():
    assert {n for n in ac.NS if n % 64 == 0} >= {64, 128, 1024, 4160} and 1 in ac.NS
    assert {1023, 1024, 1025, 2049} <= set(ac.NS)                        # around one and two scan blocks
    assert [n for n in ac.NS if ac.words_for(n) > ac.CSR_GROUP] == [4097, 4160]   # a second group of words
    assert all(ac.words_for(n) == 65 for n in (4097, 4160))
    for n in ac.NS:
        assert ac.pattern(n, "full").sum(1).tolist() == [n - 1] * n
        assert ac.pattern(n, "corner").sum() == 1 and ac.pattern(n, "corner")[n - 1, n - 1]
        assert ac.pattern(n, "top_right").sum() == 1 and ac.pattern(n, "top_right")[0, n - 1]
        hubs = ac.pattern(n, "hubs").sum(1)
        assert set(hubs.tolist()) <= {0, n - 1} and hubs[0] == hubs[n - 1] == n - 1
        if n > 2:
            asym = ac.pattern(n, "asym")
            assert asym.any() and not (asym & asym.T).any()
    assert abs(ac.pattern(4160, "random").mean() - 0.07) < 0.005


@pytest.mark.parametrize("n", ac.NS)
def test_restatements_equal_direct_numpy(n):
    for name in ac.PATTERNS:
        A = ac.pattern(n, name)
        for pad in ac.PADS:
            w = ac.words_for(n) + pad
            m = ac.pack(A, w)
            packed = np.packbits(A, axis=1, bitorder="little")       # little-endian words on a little-endian host
            direct = np.zeros((n, w * 8), dtype=np.uint8)
            direct[:, :packed.shape[1]] = packed
            assert np.array_equal(m.view(np.uint8), direct), (name, pad)
            assert ac.tail_is_clean(m, n)
            assert np.array_equal(ac.unpack(m, n), A)
            assert np.array_equal(ac.popcount(m), A.sum(1))
        deg, rowptr, stats = ac.degrees(A)
        assert np.array_equal(deg, A.sum(1))
        assert np.array_equal(rowptr, np.concatenate([[0], np.cumsum(A.sum(1))]))
        assert stats.tolist() == [int(A.sum(1).max()), int(A.sum())]
        col = ac.csr(A, rowptr)
        assert np.array_equal(col[:-1], np.nonzero(A)[1]) and col[-1] == -1
        assert np.array_equal(ac.transpose(A), A.T)
    R, F = ac.pattern(n, "random"), ac.pattern(n, "asym")
    assert np.array_equal(ac.fuse([R]), R) and np.array_equal(ac.fuse([R, F, ac.pattern(n, "hubs")]), R | F | ac.pattern(n, "hubs"))


def test_unpack_ignores_what_lies_past_n():
    A = ac.pattern(65, "random")
    m = ac.pack(A, 5)
    m[:, 1] |= ~np.uint64(0) << np.uint64(1)
    m[:, 2:] = ~np.uint64(0)
    assert not ac.tail_is_clean(m, 65) and np.array_equal(ac.unpack(m, 65), A)
    assert (ac.popcount(m) > A.sum(1)).all()          # ... and the degree kernel's count does not


def test_from_dense_rule():
    D = np.array([[0.0, 1.0, -0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    A, flag = ac.from_dense(D)
    assert flag == 0 and np.array_equal(A, D.astype(bool)) and not A[0, 2]
    for v in ac.DENSE_EDGES:
        E = D.copy()
        E[1, 2] = v
        A, flag = ac.from_dense(E)
        assert flag == 1 and A[1, 2]
    Ai, flag = ac.from_dense(np.array([[0, 1], [2, 0]], dtype=np.int64))
    assert flag == 1 and Ai.tolist() == [[False, True], [True, False]]


@pytest.mark.parametrize("n", ac.GROUP_NS)
def test_group_mask_equals_direct_numpy(n):
    for kind in ac.GROUP_KINDS:
        ids = ac.group_ids(n, kind)
        want = (ids[:, None] == ids[None, :]) & (ids[:, None] >= 0) & ~np.eye(n, dtype=bool)
        assert np.array_equal(ac.group_mask(ids), want), kind
    assert ac.group_mask(ac.group_ids(n, "equal")).sum() == n * (n - 1) and not ac.group_mask(ac.group_ids(n, "distinct")).any()
    if n > 1:
        assert (ac.group_ids(n, "mixed") < 0).any() and ac.group_mask(ac.group_ids(n, "mixed")).any()


@pytest.mark.parametrize("n,k,n_rows", [(65, 0, None), (65, 5, None), (333, 9, None), (333, 9, 100), (129, 4, 0), (1025, 7, 1000)])
def test_lists_to_mask_equals_direct_numpy(n, k, n_rows):
    idx, rmap = ac.list_case(n, k, n_rows)
    m = n if n_rows is None else n_rows
    assert idx.shape == (m, k) and (m == 0 or k == 0 or (idx.min() >= 0 and idx.max() < m))
    assert rmap is None or (len(rmap) == n_rows and len(set(rmap.tolist())) == n_rows and (n_rows == 0 or (rmap.min() >= 0 and rmap.max() < n)))
    want = np.zeros((n, n), dtype=bool)
    if m and k:
        rows = np.repeat(np.arange(m), k)
        r, c = (rows, idx.ravel()) if rmap is None else (rmap[rows], rmap[idx.ravel()])
        want[r, c] = True
        np.fill_diagonal(want, False)
    got = ac.lists_to_mask(idx, n, rmap)
    assert np.array_equal(got, want)
    if k > 2 and m:
        assert (got.sum(1)[rmap if rmap is not None else slice(None)] <= k - 2).all()    # self dropped, one column repeated
    if rmap is not None:
        assert not got[np.setdiff1d(np.arange(n), rmap)].any()


# ---- every wrong variant breaks a case, where the table says it should ------------------------------------------------
def _detecting_sizes(differs):
    return [n for n in ac.NS if any(differs(n, ac.pattern(n, name)) for name in ("random", "hubs", "corner"))]


def test_variant_big_endian():
    hit = _detecting_sizes(lambda n, A: not np.array_equal(ac.pack(A, variant="big_endian"), ac.pack(A)))
    assert hit == list(ac.NS)


def test_variant_tail_bits_set():
    def differs(n, A):
        m = ac.pack(A, variant="tail_bits_set")
        return not ac.tail_is_clean(m, n) and not np.array_equal(ac.popcount(m), A.sum(1))
    assert _detecting_sizes(differs) == [n for n in ac.NS if n % 64]


def test_variant_scan_carry_dropped():
    def differs(n, A):
        return not np.array_equal(ac.degrees(A, "scan_carry_dropped")[1], ac.degrees(A)[1])
    assert _detecting_sizes(differs) == [n for n in ac.NS if n > ac.SCAN_BLOCK]
    # row 1024 itself holds the first wrong entry, and n = 1025 sees it only through that row
    A = ac.pattern(1025, "random")
    bad, good = ac.degrees(A, "scan_carry_dropped")[1], ac.degrees(A)[1]
    assert np.array_equal(bad[:1024], good[:1024]) and bad[1024] == 0 != good[1024]


def test_variant_csr_carry_dropped():
    def differs(n, A):
        rp = ac.degrees(A)[1]
        return not np.array_equal(ac.csr(A, rp, "csr_carry_dropped"), ac.csr(A, rp))
    assert _detecting_sizes(differs) == [4097, 4160]
    # a single bit in the second group has nothing before it to carry: only rows with bits in both groups show it
    for n in (4097, 4160):
        T = ac.pattern(n, "top_right")
        assert not differs(n, T) and differs(n, ac.pattern(n, "full"))


def test_variant_partial_tile_skipped():
    def differs(n, A):
        return not np.array_equal(ac.transpose(A, "partial_tile_skipped"), A.T)
    assert _detecting_sizes(differs) == [n for n in ac.NS if n % 64]


def test_variant_self_kept():
    for n in ac.GROUP_NS:
        ids = ac.group_ids(n, "equal")
        assert not np.array_equal(ac.group_mask(ids, "self_kept"), ac.group_mask(ids))
    idx, rmap = ac.list_case(333, 9, 100)
    assert not np.array_equal(ac.lists_to_mask(idx, 333, rmap, "self_kept"), ac.lists_to_mask(idx, 333, rmap))
    idx, _ = ac.list_case(65, 5)
    assert not np.array_equal(ac.lists_to_mask(idx, 65, None, "self_kept"), ac.lists_to_mask(idx, 65))


def test_every_variant_has_a_check():
    assert set(ac.VARIANTS) == {name[len("test_variant_"):] for name in globals() if name.startswith("test_variant_")}
