"""The adjacency bitmask layer at its edges, through the C ABI: the six mused_adj_* entry points, mused_group_mask and
mused_lists_to_mask against the NumPy restatements of tests/adjacency_cases.py on its whole case table (n = 1, multiples of
64, the 1024-row scan blocks, a 65th word), padded pitches, every output pre-filled with -1 and compared exactly; and the
tail invariant of every producer of a mask: no bit at a column >= n, no bit in a padding word, whatever the buffer held."""
import ctypes as C

import numpy as np
import pytest

import adjacency_cases as ac

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    torch.cuda.synchronize()


def minus_ones(*shape, dtype=torch.int64):
    return torch.full(shape, -1, dtype=dtype, device="cuda")


def words_of(t):
    return t.cpu().numpy().view(np.uint64)


def fresh_mask(n, words):
    """(n + 1) x words of ones: the last row is a guard that must stay as it is."""
    return minus_ones(n + 1, words)


def read_mask(t, n):
    m = words_of(t)
    assert (m[n] == ~np.uint64(0)).all(), "written past the last row"
    return m[:n]


# ---- from_dense / to_dense ----------------------------------------------------------------------------------------------
DENSE_NS = (1, 63, 64, 65, 333, 1025)
NP_OF = {"F32": np.float32, "F64": np.float64, "I64": np.int64}


def _import(L, D, dtype, n, ld, words):
    mask = fresh_mask(n, words)
    flag = torch.zeros(2, dtype=torch.int32, device="cuda")
    flag[1] = -1
    dD = dev(D)
    L.call("mused_adj_from_dense", P(dD), getattr(L, dtype), n, ld, words, P(mask), P(flag), S())
    sync()
    f = flag.cpu().tolist()
    assert f[1] == -1
    return read_mask(mask, n), f[0]


@pytest.mark.parametrize("dtype", ["F32", "F64", "I64"])
@pytest.mark.parametrize("n", DENSE_NS)
def test_from_dense(L, n, dtype):
    A = ac.pattern(n, "random") | ac.pattern(n, "corner") | ac.pattern(n, "top_right")
    npdt = NP_OF[dtype]
    for ld in (n, n + 5):
        for pad in ac.PADS:
            w = ac.words_for(n) + pad
            D = np.full((n, ld), 7, dtype=npdt)              # the padding columns: neither a bit nor the flag
            D[:, :n] = A
            if dtype != "I64":
                D[:, :n][~A & (np.arange(n)[None, :] % 3 == 0)] = -0.0     # -0.0 is a zero, not an edge
            got, flag = _import(L, D, dtype, n, ld, w)
            assert flag == 0, (ld, pad)
            assert np.array_equal(got, ac.pack(A, w)), (ld, pad)           # exact words: tail bits and padding words zero
            want, wflag = ac.from_dense(D[:, :n])
            assert wflag == 0 and np.array_equal(want, A)
    # every value that is neither 0 nor 1 is an edge and raises the flag
    ld, w = n + 5, ac.words_for(n) + 3
    for v in ac.DENSE_EDGES:
        if dtype == "I64" and not float(v).is_integer():
            continue
        D = np.full((n, ld), 7, dtype=npdt)
        D[:, :n] = A
        D[n - 1, 0] = v
        want, wflag = ac.from_dense(D[:, :n])
        got, flag = _import(L, D, dtype, n, ld, w)
        assert wflag == 1 and flag == 1, v
        assert np.array_equal(got, ac.pack(want, w)), v


@pytest.mark.parametrize("n", DENSE_NS)
def test_to_dense_and_round_trip(L, n):
    A = ac.pattern(n, "random") | ac.pattern(n, "corner") | ac.pattern(n, "top_right")
    w = ac.words_for(n) + 3
    m = ac.pack(A, w)
    m[:, ac.words_for(n):] = np.uint64(0xDEADBEEFCAFEF00D)           # garbage in the padding words ...
    if n % 64:
        m[:, ac.words_for(n) - 1] |= ~np.uint64(0) << np.uint64(n % 64)   # ... and past column n of the last word
    dm = dev(m)
    for dtype, tdt in (("F64", torch.float64), ("I64", torch.int64)):
        out = torch.full((n * n + 1,), -1, dtype=tdt, device="cuda")
        L.call("mused_adj_to_dense", P(dm), n, w, getattr(L, dtype), P(out), S())
        sync()
        o = out.cpu().numpy()
        assert o[n * n] == -1, "written past the output"
        assert np.array_equal(o[:n * n].reshape(n, n), A.astype(NP_OF[dtype])), dtype
        # and back
        got, flag = _import(L, o[:n * n].reshape(n, n), dtype, n, n, ac.words_for(n))
        assert flag == 0 and np.array_equal(got, ac.pack(A)), dtype


# ---- fuse -----------------------------------------------------------------------------------------------------------------
def _fuse(L, tensors, out, n, w):
    arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    L.call("mused_adj_fuse", arr, len(tensors), n, w, P(out), S())
    sync()


@pytest.mark.parametrize("pad", ac.PADS)
@pytest.mark.parametrize("n", [1, 64, 333, 1025])
def test_fuse(L, n, pad):
    w = ac.words_for(n) + pad
    mats = [ac.pattern(n, "random"), ac.pattern(n, "asym"), ac.pattern(n, "hubs"), ac.pattern(n, "corner"),
            ac.pattern(n, "top_right")]
    packed = [ac.pack(A, w) for A in mats]

    def upload(i):
        t = fresh_mask(n, w)
        t[:n] = dev(packed[i])
        return t

    # M = 1 into a distinct buffer, and onto itself
    src, out = upload(0), fresh_mask(n, w)
    _fuse(L, [src], out, n, w)
    assert np.array_equal(read_mask(out, n), packed[0]) and np.array_equal(read_mask(src, n), packed[0])
    _fuse(L, [src], src, n, w)
    assert np.array_equal(read_mask(src, n), packed[0])
    # M = 2 with out == masks[0]: WindowEngine.fuse_into
    dst, other = upload(0), upload(1)
    _fuse(L, [dst, other], dst, n, w)
    assert np.array_equal(read_mask(dst, n), ac.pack(ac.fuse(mats[:2]), w))
    assert np.array_equal(read_mask(other, n), packed[1])
    # M = 3 and M = 5: the ones the output held must not leak into the accumulation
    for M in (3, 5):
        ins, out = [upload(i) for i in range(M)], fresh_mask(n, w)
        _fuse(L, ins, out, n, w)
        assert np.array_equal(read_mask(out, n), ac.pack(ac.fuse(mats[:M]), w)), M
        for i in range(M):
            assert np.array_equal(read_mask(ins[i], n), packed[i]), (M, i)


# ---- degrees + csr_fill ---------------------------------------------------------------------------------------------------
def _degrees(L, dm, n, w):
    deg, rowptr, stats = minus_ones(n + 1, dtype=torch.int32), minus_ones(n + 2, dtype=torch.int32), minus_ones(3, dtype=torch.int32)
    L.call("mused_adj_degrees", P(dm), n, w, P(deg), P(rowptr), P(stats), S())
    sync()
    deg, rowptr_h, stats = deg.cpu().numpy(), rowptr.cpu().numpy(), stats.cpu().numpy()
    assert deg[n] == -1 and rowptr_h[n + 1] == -1 and stats[2] == -1, "written past an output"
    return deg[:n], rowptr, rowptr_h[:n + 1], stats[:2]


@pytest.mark.parametrize("n", ac.NS)
def test_degrees_and_csr(L, n):
    for name in ac.PATTERNS:
        A = ac.pattern(n, name)
        wdeg, wrowptr, wstats = ac.degrees(A)
        wcol = ac.csr(A, wrowptr)
        for pad in ac.PADS:
            w = ac.words_for(n) + pad
            dm = dev(ac.pack(A, w))
            deg, rowptr_d, rowptr, stats = _degrees(L, dm, n, w)
            assert np.array_equal(deg, wdeg), (name, pad)
            assert np.array_equal(rowptr, wrowptr), (name, pad)
            assert np.array_equal(stats, wstats), (name, pad)
            nnz = int(wstats[1])
            col = minus_ones(nnz + 1, dtype=torch.int32)             # one guard element past nnz
            L.call("mused_adj_csr_fill", P(dm), n, w, P(rowptr_d), P(col), S())
            sync()
            assert np.array_equal(col.cpu().numpy(), wcol), (name, pad)


# ---- transpose --------------------------------------------------------------------------------------------------------------
def _transpose(L, dm, n, w):
    out = fresh_mask(n, w)
    L.call("mused_adj_transpose", P(dm), n, w, P(out), S())
    sync()
    return out


@pytest.mark.parametrize("n", ac.NS)
def test_transpose(L, n):
    w = ac.words_for(n)
    rows64 = w * 64
    for name in ac.PATTERNS:
        A = ac.pattern(n, name)
        # rows n .. 64 w - 1 of the last tile exist in the buffer and are full of ones: they are no part of the matrix
        src = minus_ones(rows64 + 1, w)
        src[:n] = dev(ac.pack(A, w))
        t = _transpose(L, src, n, w)
        got = read_mask(t, n)
        assert np.array_equal(got, ac.pack(ac.transpose(A), w)), name        # exact words: nothing at a column >= n
        assert np.array_equal(ac.unpack(got, n), A.T), name
        src[:n] = t[:n]
        back = read_mask(_transpose(L, src, n, w), n)
        assert np.array_equal(back, ac.pack(A, w)), name


def test_transpose_rejects_a_padded_pitch(L):
    n = 65
    for pad in (1, 3):
        w = ac.words_for(n) + pad
        dm, out = dev(ac.pack(ac.pattern(n, "random"), w)), fresh_mask(n, w)
        with pytest.raises(L.MusedError):
            L.call("mused_adj_transpose", P(dm), n, w, P(out), S())
        sync()
        assert (words_of(out) == ~np.uint64(0)).all()
    with pytest.raises(L.MusedError):                               # in place
        dm = dev(ac.pack(ac.pattern(n, "random")))
        L.call("mused_adj_transpose", P(dm), n, ac.words_for(n), P(dm), S())


# ---- group_mask / lists_to_mask against NumPy -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ac.GROUP_NS)
def test_group_mask(L, n):
    for kind in ac.GROUP_KINDS:
        ids = ac.group_ids(n, kind)
        for pad in ac.PADS:
            w = ac.words_for(n) + pad
            out = fresh_mask(n, w)
            d_ids = dev(ids)
            L.call("mused_group_mask", P(d_ids), n, P(out), w, S())
            sync()
            assert np.array_equal(read_mask(out, n), ac.pack(ac.group_mask(ids), w)), (kind, pad)


def _lists_to_mask(L, idx, n, rmap, w):
    out = fresh_mask(n, w)
    n_rows, k = idx.shape
    d_idx = dev(idx) if idx.size else None
    d_map = dev(rmap) if rmap is not None else None
    L.call("mused_lists_to_mask", P(d_idx), n_rows, k, P(d_map), n, P(out), w, S())
    sync()
    return read_mask(out, n)


@pytest.mark.parametrize("n,k,n_rows", [(65, 0, None), (1, 1, None), (64, 3, None), (65, 5, None), (333, 9, None), (1025, 7, None),
                                        (333, 9, 100), (129, 4, 0), (65, 5, 64), (1025, 7, 1000), (64, 0, 10)])
def test_lists_to_mask(L, n, k, n_rows):
    idx, rmap = ac.list_case(n, k, n_rows)       # n_rows = 0: an empty map (the call gets a pointer it may not read)
    want = ac.lists_to_mask(idx, n, rmap)
    for pad in ac.PADS:
        w = ac.words_for(n) + pad
        got = _lists_to_mask(L, idx, n, rmap, w)
        assert np.array_equal(got, ac.pack(want, w)), pad
        if n_rows is not None:                   # rows no list maps to are empty although the buffer held ones
            rest = np.setdiff1d(np.arange(n), rmap)
            assert len(rest) == n - n_rows and not got[rest].any()


# ---- the tail invariant of every producer of a mask --------------------------------------------------------------------------
TAIL_NS = (64, 65, 127, 1023, 1025)
TAIL_PAD = 2


def _check_tail(L, out, n, w, what, idx=None):
    m = read_mask(out, n)
    assert ac.tail_is_clean(m, n), f"{what}: a bit at a column >= {n} or in a padding word"
    _, _, _, stats = _degrees(L, out, n, w)
    assert 0 < stats[0] <= n - 1, what
    assert not np.diag(ac.unpack(m, n)).any(), f"{what}: a self bit"
    if idx is not None:
        sel = np.zeros((n, n), dtype=bool)
        np.put_along_axis(sel, np.asarray(idx, dtype=np.int64), True, axis=1)
        np.fill_diagonal(sel, False)
        assert np.array_equal(m, ac.pack(sel, w)), f"{what}: the mask is not the list minus the row itself"
    return m


def _tag_sets(n, rng, n_tags=20):
    sets = [np.sort(rng.choice(n_tags, rng.integers(0, 5), replace=False)) for _ in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    tags = np.concatenate(sets).astype(np.int32)
    return rowptr, tags, n_tags


def _postings(rowptr, cols, n_cols, vals=None):
    from mused_amd.engine import WindowEngine

    return WindowEngine._postings(rowptr, cols, n_cols, vals)


@pytest.mark.parametrize("n", TAIL_NS)
def test_tail_invariant_of_every_producer(L, n):
    rng = np.random.default_rng(n)
    w = ac.words_for(n) + TAIL_PAD
    k = 10
    idx = lambda: minus_ones(n, k, dtype=torch.int32)

    # mused_select_k_smallest: the mask alone (the engine's call) and the lists with the mask
    Sm = dev(rng.standard_normal((n, n)))
    out = fresh_mask(n, w)
    L.call("mused_select_k_smallest", P(Sm), n, n, k, None, P(out), w, S())
    alone = _check_tail(L, out, n, w, "select_k_smallest, mask only")
    out, i1 = fresh_mask(n, w), idx()
    L.call("mused_select_k_smallest", P(Sm), n, n, k, P(i1), P(out), w, S())
    sync()
    assert np.array_equal(_check_tail(L, out, n, w, "select_k_smallest, lists and mask", i1.cpu().numpy()), alone)

    # mused_knn_topk
    X = dev(rng.standard_normal((n, 8)))
    ws, nr = torch.empty(n * n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    out, i1 = fresh_mask(n, w), idx()
    L.call("mused_knn_topk", P(X), L.F64, n, 8, 8, k, L.METRIC_L2, P(ws), P(nr), P(i1), P(out), w, S())
    sync()
    _check_tail(L, out, n, w, "knn_topk", i1.cpu().numpy())

    # mused_record_knn and mused_record_knn_chunked, both kinds
    recs = (np.column_stack([rng.uniform(-60, 60, n), rng.uniform(-180, 180, n)]), rng.uniform(0, 1e6, (n, 2)).round())
    for kind, rec in enumerate(recs):
        d_rec = dev(rec)
        out = fresh_mask(n, w)
        L.call("mused_record_knn", P(d_rec), n, kind, k, None, P(out), w, S())
        alone = _check_tail(L, out, n, w, f"record_knn kind {kind}, mask only")
        out, i1 = fresh_mask(n, w), idx()
        L.call("mused_record_knn", P(d_rec), n, kind, k, P(i1), P(out), w, S())
        sync()
        assert np.array_equal(_check_tail(L, out, n, w, f"record_knn kind {kind}", i1.cpu().numpy()), alone)
        out, i2 = fresh_mask(n, w), idx()
        L.call("mused_record_knn_chunked", P(d_rec), n, kind, k, 0, P(i2), P(out), w, S())
        sync()
        assert np.array_equal(_check_tail(L, out, n, w, f"record_knn_chunked kind {kind}", i2.cpu().numpy()), alone)

    # mused_jaccard_knn and mused_jaccard_knn_chunked
    rowptr, tags, n_tags = _tag_sets(n, rng)
    postptr, postrow, _ = _postings(rowptr, tags, n_tags)
    d_tag = [dev(a) for a in (rowptr, tags, postptr, postrow)]
    out, i1 = fresh_mask(n, w), idx()
    L.call("mused_jaccard_knn", *[P(t) for t in d_tag], n, n_tags, k, P(i1), P(out), w, S())
    sync()
    both = _check_tail(L, out, n, w, "jaccard_knn", i1.cpu().numpy())
    out = fresh_mask(n, w)
    L.call("mused_jaccard_knn", *[P(t) for t in d_tag], n, n_tags, k, None, P(out), w, S())
    assert np.array_equal(_check_tail(L, out, n, w, "jaccard_knn, mask only"), both)
    out, i2 = fresh_mask(n, w), idx()
    L.call("mused_jaccard_knn_chunked", *[P(t) for t in d_tag], n, n_tags, k, 0, P(i2), P(out), w, S())
    sync()
    assert np.array_equal(_check_tail(L, out, n, w, "jaccard_knn_chunked", i2.cpu().numpy()), both)

    # mused_sparse_cosine_knn: L2-normalised sparse rows in stored (unsorted) order
    n_terms = 30
    sets = [rng.permutation(n_terms)[:rng.integers(1, 5)] for _ in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    terms = np.concatenate(sets).astype(np.int32)
    vals = np.concatenate([(lambda v: v / np.sqrt((v * v).sum()))(rng.uniform(0.1, 1.0, len(s))) for s in sets])
    postptr, postrow, postval = _postings(rowptr, terms, n_terms, vals)
    d_sp = [dev(a) for a in (rowptr, terms, vals, postptr, postrow, postval)]
    out, i2 = fresh_mask(n, w), idx()
    L.call("mused_sparse_cosine_knn", *[P(t) for t in d_sp], n, n_terms, k, 0, P(i2), P(out), w, S())
    sync()
    _check_tail(L, out, n, w, "sparse_cosine_knn", i2.cpu().numpy())

    # mused_group_mask and mused_lists_to_mask (with and without a row map)
    ids = ac.group_ids(n, "mixed")
    out, d_ids = fresh_mask(n, w), dev(ids)
    L.call("mused_group_mask", P(d_ids), n, P(out), w, S())
    _check_tail(L, out, n, w, "group_mask")
    for n_rows in (None, n - 3):
        lists, rmap = ac.list_case(n, k, n_rows)
        out = fresh_mask(n, w)
        d_l, d_m = dev(lists), (dev(rmap) if rmap is not None else None)
        L.call("mused_lists_to_mask", P(d_l), lists.shape[0], k, P(d_m), n, P(out), w, S())
        assert np.array_equal(_check_tail(L, out, n, w, f"lists_to_mask, n_rows {n_rows}"), ac.pack(ac.lists_to_mask(lists, n, rmap), w))
