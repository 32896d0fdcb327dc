"""tests/select_cases.py on the CPU: every case reaches the branch of the selection kernels its table entry names (computed
from the order-preserving keys), the location inputs make the answer unique, the chunk-by-chunk restatement of the
running-list merge gives the reference lists for every chunk size, and each emulated defect E1 to E7 changes a list of the
table, so tests/test_gpu_select_meta.py would catch a device that had it (no GPU)."""
import functools

import numpy as np
import pytest

import select_cases as sc


def _keys(name):
    return sc.f64_key(np.asarray(sc.scores(name), dtype=np.float64))


@functools.lru_cache(maxsize=None)
def _traces(name):
    """{k: [radix_trace of every probed row]} for every k < n of the case (every 8th row of the cases above 1,000 rows)."""
    c, K = sc.case(name), _keys(name)
    rows = range(0, c.n, 8 if c.n > 1000 else 1)
    return {k: [sc.radix_trace(K[i], k) for i in rows] for k in sc.ks(name, False) if k < c.n}


def _any(name, pred):
    return any(pred(t) for tr in _traces(name).values() for t in tr)


def _tie_cut_across_chunks(name, chunk_sizes=(7, 64, 256)):
    """(row, k, chunk) where k cuts a tie and the last column taken and the first one left out lie in different chunks."""
    c, S = sc.case(name), np.asarray(sc.scores(name), dtype=np.float64)
    found = []
    for k in sc.ks(name, True):
        if k == c.n:
            continue
        lists = sc.reference_lists(name, k)
        for i in range(c.n):
            thr = np.sort(S[i])[k - 1]
            tie = np.flatnonzero(S[i] == thr)
            taken = np.intersect1d(tie, lists[i])
            if len(taken) < len(tie):
                left = np.setdiff1d(tie, taken)
                assert taken.max() < left.min()                     # ties go to the smaller column
                found += [(i, k, ch) for ch in chunk_sizes if taken.max() // ch != left.min() // ch]
        if found:
            break
    return found


def _posting_bounds(c):
    ends = [(c.postrow[c.postptr[t]], c.postrow[c.postptr[t + 1] - 1] + 1) for t in range(c.n_cols)
            if c.postptr[t + 1] > c.postptr[t]]
    return np.array(ends).reshape(-1, 2)


def _decided_by_column(name):
    """A planted pair (a, b) whose columns tie in every row (but their own two, where tag sets score +1 against
    themselves), with a row and k where a is taken and b is not."""
    c, S = sc.case(name), sc.scores(name)
    for a, b in sc.loc_pairs(c.n):
        others = np.setdiff1d(np.arange(c.n), [a, b])
        assert np.array_equal(S[others, a], S[others, b]), (a, b)
        for k in sc.ks(name, True):
            L = sc.reference_lists(name, k)
            if ((L == a).any(axis=1) & ~(L == b).any(axis=1)).any():
                return True
    return False


def _order_probe(name):
    c, S = sc.case(name), sc.scores(name)
    asc = sc.sparse_cosine(c, ascending=True)
    i, p, q = sc.ENTRY, sc.PROBE_P, sc.PROBE_Q
    assert c.cols[c.rowptr[i]:c.rowptr[i + 1]].tolist() == [2, 3, 1, 0]          # stored order: not ascending
    assert S[i, p] == S[i, q] == -0.6000000000000001 and asc[i, p] == -0.6 and asc[i, q] == S[i, q]
    assert S[i, i] == -4.0 and (np.delete(S[i], [i, p, q]) == 0).all()
    assert sc.topk(S, 2)[i].tolist() == [i, p] and sc.topk(asc, 2)[i].tolist() == [i, q]
    return p < q and p // 64 != q // 64


def _fma_probe(name):
    c, S = sc.case(name), sc.scores(name)
    F = sc.sparse_cosine(c, fused=True)
    a, a2, a1, b, b1, b2 = sc.FMA_A, sc.FMA_A_TWO, sc.FMA_A_ONE, sc.FMA_B, sc.FMA_B_ONE, sc.FMA_B_TWO
    assert a2 < a1 and b1 < b2
    assert S[a, a2] == S[a, a1] == F[a, a1] and F[a, a2] > S[a, a2]            # fused: the two-term column is less similar
    assert S[b, b2] == S[b, b1] == F[b, b1] and F[b, b2] < S[b, b2]            # fused: the two-term column is more similar
    for i, cols in ((a, (a2, a1)), (b, (b1, b2))):
        assert S[i, i] < S[i, cols[0]] < 0 and (np.delete(S[i], (i,) + cols) == 0).all()
    T, TF = sc.topk(S, 2), sc.topk(F, 2)
    assert T[a].tolist() == [a, a2] and TF[a].tolist() == [a, a1] and T[b].tolist() == [b, b1] and TF[b].tolist() == [b, b2]
    assert sc.fma(0.1, 0.1, 0.0) == 0.1 * 0.1 and sc.fma(2.0 ** -30, 2.0 ** -30, 1.0) == 1.0 and sc.fma(3.0, 5.0, 7.0) == 22.0
    assert sc.fma(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, -1.0) == -(2.0 ** -104)    # what two roundings lose
    return True


def _underflow(name):
    c = sc.case(name)
    prods = [c.vals[t] * c.postval[c.postptr[c.cols[t]]:c.postptr[c.cols[t] + 1]] for t in range(len(c.cols))]
    prods = np.concatenate(prods)
    tiny = np.finfo(np.float64).tiny
    S = sc.scores(name)
    return ((prods == 0).any() and np.signbit(prods[prods == 0]).any() and ((prods != 0) & (np.abs(prods) < tiny)).any()
            and (S < 0).any() and (S > 0).any())


# what a word of the table's last column promises
CLAIMS = {
    "cand_rank": lambda nm: _any(nm, lambda t: t["done"] and t["ncand"] > 1),
    "cand_rank_tie_cut": lambda nm: _any(nm, lambda t: t["done"] and t["need_eq"] < t["equal"]),
    "cand_full": lambda nm: _any(nm, lambda t: t["done"] and t["ncand"] == 256),
    "ballot_fast_path": lambda nm: _any(nm, lambda t: t["eq_known"] and t["need_eq"] == t["equal"]),
    "diff0": lambda nm: _any(nm, lambda t: t["top"] == -1),
    "sign_bit": lambda nm: _any(nm, lambda t: t["top"] == 64),
    "narrow_first_digit": lambda nm: _any(nm, lambda t: 0 < t["first_width"] < 8 and not t["eq_known"]),
    "radix_to_bit0": lambda nm: _any(nm, lambda t: t["top"] > 0 and not t["done"] and t["equal"] > 256 and not t["eq_known"]),
    "tie_cut_count_unknown": lambda nm: _any(nm, lambda t: t["top"] > 0 and not t["eq_known"] and t["need_eq"] < t["equal"]),
    "k_max": lambda nm: sc.CS_MAX_K in sc.ks(nm, True) and sc.case(nm).n > sc.CS_MAX_K,
    "single_row": lambda nm: sc.case(nm).n == 1 and sc.ks(nm, True) == [1],
    "duplicate_ties": _decided_by_column,
    "tie_straddles_boundary": lambda nm: len(_tie_cut_across_chunks(nm)) > 0,
    "empty_rows": lambda nm: (np.diff(sc.case(nm).rowptr) == 0).any(),
    "empty_postings": lambda nm: (np.diff(sc.case(nm).postptr) == 0).any(),
    "postings_on_boundary": lambda nm: ((_posting_bounds(sc.case(nm)) % 64 == 0).all(axis=1)).sum() >= 3,
    "postings_behind_boundary": lambda nm: ((_posting_bounds(sc.case(nm)) % 64 == 1).all(axis=1)).sum() >= 3,
    "stored_order_matters": lambda nm: not np.array_equal(sc.scores(nm), sc.sparse_cosine(sc.case(nm), ascending=True)),
    "order_probe": _order_probe,
    "fma_probe": _fma_probe,
    "underflow": _underflow,
}


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_reaches_what_its_entry_names(name):
    c, S = sc.case(name), sc.scores(name)
    assert S.shape == (c.n, c.n) and not np.isnan(S).any()
    assert not (np.signbit(S) & (S == 0)).any(), "a score of -0.0: the order of the keys is not the order of the values"
    assert c.reaches and set(c.reaches) <= set(CLAIMS)
    for word in c.reaches:
        assert CLAIMS[word](name), word
    if c.source not in sc.RECORDS:
        rows = np.repeat(np.arange(c.n), np.diff(c.rowptr))
        assert all(len(set(c.cols[c.rowptr[i]:c.rowptr[i + 1]].tolist())) == c.rowptr[i + 1] - c.rowptr[i] for i in range(c.n))
        for t in range(c.n_cols):                                   # rows ascend inside a posting list, and it is the CSR
            lst = c.postrow[c.postptr[t]:c.postptr[t + 1]]
            assert (np.diff(lst) > 0).all() and np.array_equal(lst, rows[c.cols == t])
        assert c.postptr[-1] == len(c.cols) and len(c.postptr) == max(c.n_cols, 1) + 1


def test_every_edge_of_the_issue_has_a_case():
    reached = {w for nm in sc.NAMES for w in sc.case(nm).reaches}
    assert reached == set(CLAIMS)
    # the two paths of a mask-only run of the LDS-row kernels, for records and for tag sets
    for names in (sc.NAMES_OF["location"] + sc.NAMES_OF["time"], sc.NAMES_OF["tags"]):
        assert any(_any(nm, lambda t: t["eq_known"] and t["need_eq"] == t["equal"]) for nm in names)      # ballots
        assert any(_any(nm, lambda t: t["eq_known"] and t["need_eq"] < t["equal"]) for nm in names)       # tie cut
        assert any(_any(nm, lambda t: not t["eq_known"]) for nm in names)                                 # count unknown
    # small_tie: ties of 2 to 40 columns, cut
    sizes = {t["equal"] for tr in _traces("time_small_tie").values() for t in tr if t["need_eq"] < t["equal"]}
    assert min(sizes) == 2 and 40 in sizes
    # big_tie: 400 equal keys, k inside, and at chunk 64 the tie is cut across a boundary
    assert _any("time_big_tie", lambda t: t["equal"] >= sc.TIE_ROWS and 0 < t["need_eq"] < t["equal"] and not t["done"])
    assert any(ch == 64 for _, _, ch in _tie_cut_across_chunks("time_big_tie"))
    # low_bits as the issue words it: row 0's own column keeps the first digit wide; the bin of the k-th key is full
    t = sc.radix_trace(_keys("time_low_bits")[0], 2)
    assert (t["top"], t["first_width"], t["passes"], t["ncand"]) == (62, 8, 1, 256)
    # all_empty: one key above 256 equal ones, not the sign bit
    assert {t["top"] for tr in _traces("tags_all_empty").values() for t in tr} == {62}


def test_parameters_cover_the_chunk_edges():
    for name in sc.NAMES:
        n = sc.case(name).n
        ch = sc.chunks(n)
        assert 0 in ch and n in ch and n + 1 in ch and (n < 2 or n - 1 in ch) and (1 in ch) == (n < 1025)
        assert all(sc.effective_chunk(k, 0) >= n for k in sc.ks(name, True))                 # chunk 0: one chunk
        assert all(1 <= k <= min(n, sc.CS_MAX_K) for k in sc.ks(name, True)) and n in sc.ks(name, False)
        if n == sc.N:
            assert {1, 2, 50, 51, 151, n - 1, n} == set(sc.ks(name, True))
            assert any(n % c == 0 and n // c > 1 for c in ch if c)                          # n a multiple of the chunk
            assert sum(n % c == 1 and c > 1 for c in ch if c) >= 2                          # a last chunk of one column
            assert any(0 < c < k for c in ch for k in sc.ks(name, True))                    # the list still fills at a chunk's end
        words = sc.mask_words(n, True)
        assert words[:2] == [sc.words_for(n), sc.words_for(n) + 3] and words[:2] == sc.mask_words(n, False)
        first_free = -(-n // 1024) * 16
        if n in (100, 1025):
            assert min(words) < first_free and first_free in words + [w - 1 for w in words] and max(words) > first_free
    assert sc.mask_words(100, True) == [2, 5, 16, 17, 20] and sc.mask_words(1025, True) == [17, 20, 33]
    assert sc.CS_MAX_K in sc.ks("time_1100", True) and sc.CS_MAX_K in sc.ks("loc_1025", True) and 1100 in sc.ks("time_1100", False)


# ---- location: the answer is unique ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES_OF["location"])
def test_location_inputs_decide_every_list(name):
    assert np.finfo(sc.LD).eps <= 2.0 ** -63, "np.longdouble is no wider than fp64 here"
    c, S = sc.case(name), sc.scores(name)
    same = (c.rec[:, None, :] == c.rec[None, :, :]).all(axis=2)
    assert (S[same] == 0).all() and (S[~same] > 0).all()
    for a, b in sc.loc_pairs(c.n):
        assert same[a, b]
    if c.name != "loc_all_equal" and c.n > 1:
        assert same.sum() == c.n + 2 * len(sc.loc_pairs(c.n))
        # (a) no two distinct geotags closer than MIN_SEPARATION_DEG (central angle)
        angle = np.degrees(np.asarray(S, dtype=np.float64) / 6371.0)
        assert angle[~same].min() >= sc.MIN_SEPARATION_DEG
        # (b) no column but exact duplicates of the k-th one within REL_GAP of the k-th score
        worst = np.inf
        for k in sc.ks(name, False):
            if k == c.n:
                continue
            order = sc._order(name)
            kth = order[:, k - 1]
            t = S[np.arange(c.n), kth]
            near = np.abs(S - t[:, None]) <= sc.REL_GAP * t[:, None]
            assert not (near & ~same[kth]).any(), k
            gap = np.where(same[kth], np.inf, np.abs(S - t[:, None]) / np.where(t > 0, t, 1)[:, None])
            worst = min(worst, float(gap.min()))
        print(f"{name}: smallest nonzero distance {float(S[~same].min()):.1f} km, smallest relative gap at a tested k {worst:.2e}")
    # fp64 NumPy gives the same lists, and lies far inside the band the device is held to
    S64 = sc.haversine_km(c.rec, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(S > 0, np.abs(S64 - S) / np.where(S > 0, S, 1), np.abs(S64))
    assert rel.max() <= 1e-13
    for k in sc.ks(name, False):
        assert np.array_equal(sc.topk(S64, k), sc.reference_lists(name, k)), k


# ---- the merge, chunk by chunk ----------------------------------------------------------------------------------------------------
def _probe_rows(n, chunk):
    """All rows; every 16th of the cases above 1,000 rows and every 8th where the chunk is 1 or 7 (the merge runs n / chunk
    times): the rows are independent of each other."""
    if n > 1000:
        return np.arange(0, n, 16)
    return np.arange(0, n, 8) if 0 < chunk < 64 and n > 64 else np.arange(n)


@pytest.mark.parametrize("name", sc.NAMES)
def test_running_list_merge_gives_the_reference(name):
    c, K = sc.case(name), _keys(name)
    for k in sc.ks(name, True):
        for chunk in sc.chunks(c.n):
            rows = _probe_rows(c.n, chunk)
            assert np.array_equal(sc.merge_select(K[rows], k, chunk), sc.reference_lists(name, k)[rows]), (k, chunk)


def test_reference_is_a_stable_lexsort():
    S = np.array([[3.0, 1.0, 1.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    assert sc.topk(S, 3).tolist() == [[1, 2, 3], [0, 1, 2]] and sc.topk(S, 5).tolist() == [[0, 1, 2, 3, 4]] * 2
    assert sc.mask_of(sc.topk(S, 3)[:1], 1, 2).tolist() == [[0b1110, 0]]
    key = sc.f64_key(np.array([-np.inf, -1.0, -5e-324, 0.0, 5e-324, 1.0, np.inf]))
    assert (np.diff(key.astype(object)) > 0).all() and key[3] == 1 << 63


# ---- each emulated defect is caught ----------------------------------------------------------------------------------------------
def _changed(defect, name, k, chunk):
    ref = sc.reference_lists(name, k)
    return not np.array_equal(sc.emulate(defect, name, k, chunk), ref)


@pytest.mark.parametrize("defect,name,k,chunk", [
    ("E1", "time_small_tie", 50, 0), ("E1", "loc_random", 50, 0), ("E1", "tags_random", 51, 0), ("E1", "text_random", 151, 0),
    ("E2", "time_big_tie", 50, 64), ("E2", "tags_block", 51, 64), ("E2", "text_order_probe", 2, 64),
    ("E3a", "tags_block", 151, 64), ("E3b", "tags_block", 151, 64), ("E3a", "text_random", 2, 7), ("E3b", "text_random", 2, 7),
    ("E3a", "tags_random", 2, 256), ("E3b", "tags_random", 2, 256),
    ("E4", "text_order_probe", 2, 0), ("E4", "text_order_probe", 2, 64),
    ("E5", "tags_random", 1, 0), ("E5", "tags_block", 256, 64),
    ("E7", "text_fma_probe", 2, 0), ("E7", "text_fma_probe", 2, 7),
    ("E6", "time_random", 50, 64), ("E6", "tags_random", 257, 256), ("E6", "text_signed", 2, 256), ("E6", "time_random", 1, 1),
])
def test_defect_changes_a_list_of_the_table(defect, name, k, chunk):
    assert defect in sc.DEFECTS and k in sc.ks(name, True) and chunk in sc.chunks(sc.case(name).n)
    assert _changed(defect, name, k, chunk)


def test_defects_that_need_a_boundary_hide_without_one():
    """E2, E3 and E6 are defects of the chunk walk: with one chunk (chunk 0) the lists are right, so only the runs with
    several chunks can catch them.  E3 with one chunk loses column 0 (E3b) or n - 1 (E3a) only."""
    assert not _changed("E2", "time_big_tie", 50, 0) and not _changed("E6", "time_random", 50, 0)
    assert not _changed("E2", "time_random", 50, 64)                # no ties: nothing for E2 to reorder
    assert not _changed("E6", "time_random", 50, 7)                 # 257 = 36 * 7 + 5: the last chunk holds five columns
    # E4 moves last bits of many scores of the random rows and not one of their lists: text_order_probe is there for it
    assert not np.array_equal(sc.scores("text_random"), sc.sparse_cosine(sc.case("text_random"), ascending=True))
    assert not any(_changed("E4", nm, k, 0) for nm in ("text_random", "text_signed") for k in sc.ks(nm, True))
