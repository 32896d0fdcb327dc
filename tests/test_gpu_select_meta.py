"""The metadata and sparse-text neighbour selection at its edges, through the C ABI: mused_record_knn_chunked,
mused_jaccard_knn_chunked and mused_sparse_cosine_knn (chunk_select_kernel) for every case x k x chunk of
tests/select_cases.py, mused_record_knn and mused_jaccard_knn (select_k_kernel on a row of scores in LDS) for every case x k
with the lists alone, the mask alone and both, at every listed mask pitch, against the NumPy reference of that table: not
against another kernel.  Every output is pre-filled with -1, has one guard row behind it and is compared exactly.

Measured on the MI355X: mused_record_scores (haversine) against the np.longdouble reference, largest relative difference on
the nonzero entries 1.24e-14 (loc_random) and 3.89e-14 (loc_1025), that is 3.9e-4 of the 1e-10 allowed; exactly +0 on
duplicates and the diagonal.

What failed before the fixes that came with this file:
  * haversine_km and the sparse-cosine accumulation went through __dmul_rn / __dsub_rn / __dadd_rn, which the compiler fused
    into multiply-adds once inlined.  test_device_haversine_is_within_the_band failed for all four location cases (1.26e-13 km
    instead of 0 between equal geotags: the rounding error of latitude * pi / 180), and test_chunked_lists_equal_the_reference
    and test_chunked_mask_is_the_lists_without_the_row_itself failed for text_fma_probe (rows 5 and 7 took the other column
    of their tie).  No list of any other case moved.
  * mused_record_knn and mused_jaccard_knn accepted a mask pitch one word short, and two null outputs:
    test_bad_arguments_are_rejected_and_nothing_is_written failed for loc_random, time_1100 and tags_1025."""
import ctypes as C

import numpy as np
import pytest

import select_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MUSED_ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


def dev(a):
    a = np.array(a, order="C")                                       # a copy: the cases are read-only
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    torch.cuda.synchronize()


def filled(value, *shape, dtype=torch.int64):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def fresh_idx(n, k, value=-1):
    """(n + 1) x k: the last row is a guard that must stay as it is."""
    return filled(value, n + 1, k, dtype=torch.int32)


def fresh_mask(n, words, value=-1):
    return filled(value, n + 1, words)


def read_idx(t, n, value=-1):
    a = t.cpu().numpy()
    assert (a[n] == value).all(), "lists written past the last row"
    return a[:n]


def read_mask(t, n, value=-1):
    m = t.cpu().numpy().view(np.uint64)
    assert (m[n] == np.int64(value).astype(np.uint64)).all(), "mask written past the last row"
    return m[:n]


_ON_DEVICE = {}


def on_device(name):
    """The arrays of a case in the order its entry points take them."""
    if name not in _ON_DEVICE:
        c = sc.case(name)
        if c.source in sc.RECORDS:
            arrays = (c.rec,)
        elif c.source == "tags":
            arrays = (c.rowptr, c.cols, c.postptr, c.postrow)
        else:
            arrays = (c.rowptr, c.cols, c.vals, c.postptr, c.postrow, c.postval)
        _ON_DEVICE[name] = [dev(a) for a in arrays]
    return _ON_DEVICE[name]


def chunked(L, name, k, chunk, words=0, fill=-1):
    """(lists, mask or None) of the chunked entry of the case's source."""
    c, d = sc.case(name), on_device(name)
    idx, mask = fresh_idx(c.n, k, fill), (fresh_mask(c.n, words, fill) if words else None)
    if c.source in sc.RECORDS:
        L.call("mused_record_knn_chunked", P(d[0]), c.n, sc.RECORDS.index(c.source), k, chunk, P(idx), P(mask), words, S())
    elif c.source == "tags":
        L.call("mused_jaccard_knn_chunked", *[P(t) for t in d], c.n, c.n_cols, k, chunk, P(idx), P(mask), words, S())
    else:
        L.call("mused_sparse_cosine_knn", *[P(t) for t in d], c.n, c.n_cols, k, chunk, P(idx), P(mask), words, S())
    sync()
    return read_idx(idx, c.n, fill), (read_mask(mask, c.n, fill) if words else None)


def lds_row(L, name, k, lists, words=0, fill=-1):
    """(lists or None, mask or None) of mused_record_knn / mused_jaccard_knn."""
    c, d = sc.case(name), on_device(name)
    idx, mask = (fresh_idx(c.n, k, fill) if lists else None), (fresh_mask(c.n, words, fill) if words else None)
    if c.source in sc.RECORDS:
        L.call("mused_record_knn", P(d[0]), c.n, sc.RECORDS.index(c.source), k, P(idx), P(mask), words, S())
    else:
        L.call("mused_jaccard_knn", *[P(t) for t in d], c.n, c.n_cols, k, P(idx), P(mask), words, S())
    sync()
    return (read_idx(idx, c.n, fill) if lists else None), (read_mask(mask, c.n, fill) if words else None)


def device_scores(L, name):
    c = sc.case(name)
    out = torch.full((c.n * c.n + 1,), np.nan, dtype=torch.float64, device="cuda")
    L.call("mused_record_scores", P(on_device(name)[0]), c.n, sc.RECORDS.index(c.source), P(out), S())
    sync()
    o = out.cpu().numpy()
    assert np.isnan(o[-1]), "scores written past the matrix"
    return o[:-1].reshape(c.n, c.n)


def test_posting_lists_are_the_engines():
    from mused_amd.engine import WindowEngine

    for name in sc.NAMES_OF["tags"] + sc.NAMES_OF["text"]:
        c = sc.case(name)
        postptr, postrow, postval = WindowEngine._postings(c.rowptr, c.cols, c.n_cols, getattr(c, "vals", None))
        assert np.array_equal(postptr, c.postptr) and np.array_equal(postrow, c.postrow)
        assert (postval is None and c.postval is None) or np.array_equal(postval, c.postval)


# ---- the chunked entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_chunked_lists_equal_the_reference(L, name):
    c = sc.case(name)
    own = device_scores(L, name) if c.source == "location" else None
    for k in sc.ks(name, True):
        want = sc.reference_lists(name, k)
        if own is not None:          # the device's own matrix decides as the longdouble reference does
            assert np.array_equal(sc.topk(own, k), want), k
        for chunk in sc.chunks(c.n):
            got, _ = chunked(L, name, k, chunk)
            assert np.array_equal(got, want), (k, chunk, np.flatnonzero((got != want).any(axis=1))[:8])


@pytest.mark.parametrize("name", sc.NAMES)
def test_chunked_mask_is_the_lists_without_the_row_itself(L, name):
    c = sc.case(name)
    for k in sc.ks(name, True):
        want = sc.reference_lists(name, k)
        for words in sc.mask_words(c.n, False):
            got, mask = chunked(L, name, k, sc.MASK_CHUNK, words)
            assert np.array_equal(got, want), (k, words)
            assert np.array_equal(mask, sc.mask_of(want, c.n, words)), (k, words)


# ---- the LDS-row entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.LDS_ROW_NAMES)
def test_lds_row_lists_and_masks_equal_the_reference(L, name):
    c = sc.case(name)
    for k in sc.ks(name, False):
        want = sc.reference_lists(name, k)
        got, _ = lds_row(L, name, k, True)
        assert np.array_equal(got, want), (k, "lists alone", np.flatnonzero((got != want).any(axis=1))[:8])
        for words in sc.mask_words(c.n, True):
            want_mask = sc.mask_of(want, c.n, words)
            _, mask = lds_row(L, name, k, False, words)              # ballots where no tie is cut, the general emit elsewhere
            assert np.array_equal(mask, want_mask), (k, words, "mask alone")
            got, mask = lds_row(L, name, k, True, words)
            assert np.array_equal(got, want), (k, words, "lists with the mask")
            assert np.array_equal(mask, want_mask), (k, words, "mask with the lists")


# ---- the device's scores ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES_OF["location"])
def test_device_haversine_is_within_the_band(L, name):
    c, ref = sc.case(name), sc.scores(name)
    got = device_scores(L, name)
    same = (c.rec[:, None, :] == c.rec[None, :, :]).all(axis=2)
    assert (got[same] == 0).all() and not np.signbit(got[same]).any(), "duplicates and the diagonal are exactly +0"
    if (~same).any():
        rel = np.abs(got.astype(sc.LD) - ref)[~same] / ref[~same]
        print(f"{name}: largest |device - reference| / reference = {float(rel.max()):.3e} = "
              f"{float(rel.max()) / sc.SCORE_RTOL:.2e} of the {sc.SCORE_RTOL:g} allowed")
        assert rel.max() <= sc.SCORE_RTOL


@pytest.mark.parametrize("name", sc.NAMES_OF["time"])
def test_device_time_scores_are_the_reference_bit_for_bit(L, name):
    got, ref = device_scores(L, name), sc.scores(name)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))


# ---- determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["loc_random", "time_big_tie", "tags_random", "text_random"])
def test_two_runs_on_dirty_buffers_give_equal_bits(L, name):
    c, k = sc.case(name), 51
    words = sc.words_for(c.n) + 3
    a = chunked(L, name, k, 64, words, fill=-1)
    b = chunked(L, name, k, 64, words, fill=0x5A5A5A5A)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if name in sc.LDS_ROW_NAMES:
        for lists in (True, False):
            a = lds_row(L, name, k, lists, words, fill=-1)
            b = lds_row(L, name, k, lists, words, fill=0x5A5A5A5A)
            assert (a[0] is None and b[0] is None) or np.array_equal(a[0], b[0])
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], sc.mask_of(sc.reference_lists(name, k), c.n, words))


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def _rejected(L, rc, entry, *outputs):
    msg = L.lib().mused_last_error()
    assert rc == MUSED_ERR_ARG, (entry, rc)
    assert msg and entry.encode() in msg, (entry, msg)
    sync()
    for t in outputs:
        assert (t.cpu().numpy() == -1).all(), (entry, "an output was written")


def _entry_args(name):
    """(entry, the arrays before n, the arguments between n and k) of the chunked entry of a case, and of its LDS-row entry
    (None for text)."""
    c, d = sc.case(name), [P(t) for t in on_device(name)]
    if c.source in sc.RECORDS:
        kind = sc.RECORDS.index(c.source)
        return ("mused_record_knn_chunked", d, (kind,)), ("mused_record_knn", d, (kind,))
    if c.source == "tags":
        return ("mused_jaccard_knn_chunked", d, (c.n_cols,)), ("mused_jaccard_knn", d, (c.n_cols,))
    return ("mused_sparse_cosine_knn", d, (c.n_cols,)), None


@pytest.mark.parametrize("name", ["loc_random", "time_1100", "tags_1025", "text_random"])
def test_bad_arguments_are_rejected_and_nothing_is_written(L, name):
    c = sc.case(name)
    n, w = c.n, sc.words_for(c.n)
    lib = L.lib()
    idx, mask = fresh_idx(n, 8), fresh_mask(n, w)
    chunked_entry, lds_entry = _entry_args(name)
    entry, lead, mid = chunked_entry
    fn = getattr(lib, entry)

    def call_chunked(n_, k, chunk, out_idx, out_mask, words):
        return fn(*lead, n_, *mid, k, chunk, P(out_idx), P(out_mask), words, S())

    bad = [(n, 0, 0, idx, None, 0), (n, n + 1, 0, idx, None, 0), (n, 1, -1, idx, None, 0), (0, 1, 0, idx, None, 0),
           (n, 8, 0, None, None, 0), (n, 8, 0, None, mask, w), (n, 8, 0, idx, mask, w - 1)]
    if n > sc.CS_MAX_K:
        bad.append((n, sc.CS_MAX_K + 1, 0, idx, None, 0))
    for args in bad:
        _rejected(L, call_chunked(*args), entry, idx, mask)
    if name == "tags_1025":          # k = 1025 for the text entry too: rejected before an array is read
        d = on_device(name)
        vals = filled(0, 8, dtype=torch.float64)
        rc = lib.mused_sparse_cosine_knn(P(d[0]), P(d[1]), P(vals), P(d[2]), P(d[3]), P(vals), n, c.n_cols, sc.CS_MAX_K + 1, 0,
                                         P(idx), None, 0, S())
        _rejected(L, rc, "mused_sparse_cosine_knn", idx)
    if lds_entry is None:
        return
    entry, lead, mid = lds_entry
    fn = getattr(lib, entry)
    for n_, k, out_idx, out_mask, words in [(n, 0, idx, None, 0), (n, n + 1, idx, None, 0), (0, 1, idx, None, 0),
                                            (n, 8, idx, mask, w - 1), (n, 8, None, mask, w - 1), (n, 8, None, None, 0)]:
        _rejected(L, fn(*lead, n_, *mid, k, P(out_idx), P(out_mask), words, S()), entry, idx, mask)
