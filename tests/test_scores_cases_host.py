"""tests/scores_cases.py on the CPU: the layouts hold the same values at the offsets they claim, the longdouble reference
agrees with plain fp64 NumPy, the band decides no comparison but the planted ties, and a device whose row norms depend on
the row's address would fail the duplicate assertions of tests/test_gpu_scores_layout.py on these cases (no GPU)."""
import numpy as np
import pytest

import scores_cases as sc


@pytest.mark.parametrize("dtype,d", sc.CASES, ids=sc.IDS)
def test_rows_and_layouts(dtype, d):
    X = sc.rows(dtype, d)
    assert X.shape == (sc.N, d) and X.dtype == dtype and not X[sc.ZERO_ROW].any()
    in_pairs = [i for p in sc.PAIRS for i in p]
    assert len(set(in_pairs)) == 16 and sc.ZERO_ROW not in in_pairs
    for a, b in sc.PAIRS:
        assert a < b and np.array_equal(X[a], X[b])
    assert sum((b - a) % 2 for a, b in sc.PAIRS) == 7
    assert sum(1 for a, b in sc.PAIRS if a < 128 <= b) == 3          # pairs across the two GEMM tiles, rows in between
    rest = np.setdiff1d(np.arange(sc.N), in_pairs + [sc.ZERO_ROW])
    assert len(np.unique(X[rest], axis=0)) == len(rest)              # no other duplicates
    V = 16 // np.dtype(dtype).itemsize
    for name in sc.LAYOUTS:
        buf, off, ld = sc.layout(X, name)
        assert ld >= d and len(buf) == off + sc.N * ld
        view = buf[off:].reshape(sc.N, ld)
        assert np.array_equal(view[:, :d], X) and np.isnan(view[:, d:]).all() and np.isnan(buf[:off]).all()
    assert (sc.line_offsets(dtype, d, "offset1") != 0).all()
    assert (sc.line_offsets(dtype, d, "aligned") == 0).all()
    assert sc.layout(X, "pad3")[2] == d + 3 and sc.layout(X, "tight")[2] == d
    # wherever the pitch is no multiple of a line, the rows of some pair start at different offsets inside their lines
    for name in ("tight", "pad3"):
        o = sc.line_offsets(dtype, d, name)
        if sc.layout(X, name)[2] % V:
            assert any(o[a] != o[b] for a, b in sc.PAIRS), name
            assert any((o[a] == 0) != (o[b] == 0) for a, b in sc.PAIRS), name
    # ... and one layout at least has rows on a line and rows off it, unless every pitch of the case is a multiple
    mixed = [name for name in sc.LAYOUTS if len(set((sc.line_offsets(dtype, d, name) == 0).tolist())) == 2]
    assert mixed or all(sc.layout(X, name)[2] % V == 0 for name in ("tight", "pad3"))


@pytest.mark.parametrize("dtype,d", sc.CASES, ids=sc.IDS)
def test_reference_agrees_with_fp64_numpy(dtype, d):
    X = np.asarray(sc.rows(dtype, d), dtype=np.float64)
    nrm, l2, cos = sc.reference(dtype, d)
    bn, bl, bc = sc.bands(dtype, d)
    sq = np.einsum("ij,ij->i", X, X)
    assert (np.abs(sq - nrm) <= bn).all()
    assert (np.abs(np.maximum(sq[:, None] - 2.0 * (X @ X.T) + sq[None, :], 0.0) - l2) <= bl).all()
    root = np.sqrt(sq)
    inv = np.where(root == 0, 1.0, 1.0 / np.where(root == 0, 1.0, root))
    assert (np.abs(-(X @ X.T) * inv[:, None] * inv[None, :] - cos) <= bc).all()
    assert nrm[sc.ZERO_ROW] == 0 and not cos[sc.ZERO_ROW].any() and not cos[:, sc.ZERO_ROW].any()
    for a, b in sc.PAIRS:
        assert nrm[a] == nrm[b]
        assert np.array_equal(l2[:, a], l2[:, b]) and np.array_equal(cos[a], cos[b])


@pytest.mark.parametrize("metric", sc.METRICS)
@pytest.mark.parametrize("dtype,d", sc.CASES, ids=sc.IDS)
def test_band_decides_nothing_but_the_planted_ties(dtype, d, metric):
    for k in sc.KS:
        assert sc.ambiguity(dtype, d, metric, k) == [], (k,)


def test_degenerate_rows_are_ties_in_exact_arithmetic():
    """What `degenerate` leaves out of the statement above really is undecidable by any band: all scores of those rows are
    equal (to -1, 0 or +1) within a few longdouble roundings."""
    tiny = 64 * float(np.finfo(sc.LD).eps)
    for dtype in sc.DTYPES:
        cos1 = sc.reference(dtype, 1)[2]
        assert (np.abs(np.abs(cos1) - 1)[np.abs(cos1) > 0.5] <= tiny).all() and (np.abs(cos1)[np.abs(cos1) <= 0.5] == 0).all()
        for d in sc.DS:
            assert not sc.reference(dtype, d)[2][sc.ZERO_ROW].any()
            assert all(sc.degenerate(dtype, d, 1, i) == (d == 1 or i == sc.ZERO_ROW) for i in range(sc.N))
            assert not any(sc.degenerate(dtype, d, 0, i) for i in range(sc.N))


@pytest.mark.parametrize("dtype,d", sc.CASES, ids=sc.IDS)
def test_reference_lists_pass_their_own_check(dtype, d):
    """The stable top-k of the reference (ties to the smaller column) passes check_topk; a list with a planted pair's larger
    column in place of the smaller one, and a list one column off, do not."""
    for metric in sc.METRICS:
        S = sc.reference_scores(dtype, d, metric)
        for k in sc.KS:
            idx = np.sort(np.argsort(S, axis=1, kind="stable")[:, :k], axis=1)
            sc.check_topk(dtype, d, metric, k, idx)
        k = 7
        order = np.argsort(S, axis=1, kind="stable")
        idx = np.sort(order[:, :k], axis=1)
        if not sc.degenerate(dtype, d, metric, 0):
            wrong = idx.copy()
            wrong[0] = np.sort(np.concatenate([order[0, :k - 1], order[0, -1:]]))      # the farthest column instead of the k-th
            with pytest.raises(AssertionError):
                sc.check_topk(dtype, d, metric, k, wrong)
        a, b = sc.PAIRS[0]
        r = next(i for i in range(sc.N) if a in idx[i] and b not in idx[i]) if any(a in idx[i] and b not in idx[i] for i in range(sc.N)) else None
        if r is not None:
            swapped = idx.copy()
            swapped[r] = np.sort(np.where(idx[r] == a, b, idx[r]))
            with pytest.raises(AssertionError):
                sc.check_topk(dtype, d, metric, k, swapped)


def test_emulated_orders_sum_the_same_terms():
    rng = np.random.default_rng(3)
    for dtype in sc.DTYPES:
        for d in (1, 2, 3, 4, 5, 63, 64, 65, 130, 257, 515):
            x = rng.standard_normal(d).astype(dtype)
            exact = float((x.astype(sc.LD) ** 2).sum())
            for f in (sc.norm_line_order, sc.norm_column_order):
                assert abs(f(x) - exact) <= sc.coefficient(d) * exact
    # whole numbers: no rounding, every order gives the same sum
    x = np.arange(1, 131, dtype=np.float64)
    assert sc.norm_line_order(x) == sc.norm_column_order(x) == float((x ** 2).sum())
    assert sc.norm_line_order(x[:1]) == 1.0 and sc.norm_column_order(x[:1]) == 1.0


def test_an_address_dependent_norm_breaks_the_duplicate_assertions():
    """The defect the device test is there for, emulated: rows on a 16-byte line summed in line order, the others in column
    order.  On these cases that gives a planted pair two different norms, and one row's values two different norms in two
    layouts, for at least one case of each dtype.  (Where a row fills no more than one 16-byte line per lane pair the two
    orders add the same numbers and no case can tell them apart; the share of rows they differ on is printed.)"""
    seen_pair, seen_layout = set(), set()
    for dtype, d in sc.CASES:
        X = sc.rows(dtype, d)
        norms = {name: sc.address_dependent_norms(dtype, d, name) for name in sc.LAYOUTS}
        if any(norms[name][a] != norms[name][b] for name in sc.LAYOUTS for a, b in sc.PAIRS):
            seen_pair.add((np.dtype(dtype).name, d))
        if any(not np.array_equal(norms[name], norms["aligned"]) for name in sc.LAYOUTS):
            seen_layout.add((np.dtype(dtype).name, d))
        line = np.array([sc.norm_line_order(x) for x in X])
        col = np.array([sc.norm_column_order(x) for x in X])
        print(f"{np.dtype(dtype).name} d={d}: orders differ on {np.mean(line != col):.0%} of the rows")
    print("pair assertion violated for", sorted(seen_pair), "layout assertion violated for", sorted(seen_layout))
    assert {t for t, _ in seen_pair} == {"float32", "float64"}
    assert {t for t, _ in seen_layout} == {"float32", "float64"}
    assert ("float64", 33) in seen_pair and ("float64", 9) in seen_pair
