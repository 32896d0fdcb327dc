"""mused_adj_fuse_table / mused_adj_fuse_threshold (csrc/adj_fuse_table.hip) through the C ABI.  Outputs are pre-filled and
compared exactly with `mused_amd.fusion.fuse_table_numpy`.

  * n = 1, 63, 64, 65, 257, 1025 at the pitches ceil(n/64) and ceil(n/64) + 3: n * words is odd for some (one word per thread)
    and even for the others (a 16-byte pair per thread, M <= 6); a buffer that starts 8 bytes off a 16-byte boundary turns the
    pair kernel off at an even size too.
  * M = 1 .. 8.  M <= 3: every table with bit 0 clear (1, 7, 127); M = 5 and 8: OR, AND, majority, the two weighted tables
    of (1, 0.5, 0.75, ...) at tau = 1.25 and 1.5, and 16 seeded random tables; M = 4, 6, 7: OR, AND, majority and 4 random.
  * out aliased to each input in turn; the OR table against mused_adj_fuse; no bit at a column >= n or in a padding word;
    the guard words in front of and behind the output untouched.
  * The arguments both entries refuse: MUSED_ERR_ARG, a message, the output untouched."""
import ctypes as C

import numpy as np
import pytest

import fuse_table_cases as fc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64                      # words in front of and behind every output (512 bytes: the alignment of the output is kept)
SENTINEL = 0x5A5A5A5A5A5A5A5A   # (positive as int64)
ERR_ARG = -1
SIZES = [1, 63, 64, 65, 257, 1025]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def table_arg(table):
    return (C.c_uint64 * 4)(*[int(x) for x in table])


def pointers(d_masks):
    return (C.c_void_p * len(d_masks))(*[m.data_ptr() for m in d_masks])


def guarded(n, words, shift=0):
    """(buffer, the (n, words) output inside it `shift` words further on), both filled with the sentinel."""
    buf = torch.full((n * words + 2 * GUARD + shift,), SENTINEL, dtype=torch.int64, device="cuda")
    return buf, buf[GUARD + shift:GUARD + shift + n * words].view(n, words)


def check_guards(buf, n, words, shift=0):
    b = buf.cpu().numpy()
    assert (b[:GUARD + shift] == SENTINEL).all() and (b[GUARD + shift + n * words:] == SENTINEL).all(), "guard words written"


def fuse_table(L, d_masks, table, n, words, shift=0):
    buf, out = guarded(n, words, shift)
    L.call("mused_adj_fuse_table", pointers(d_masks), len(d_masks), table_arg(table), n, words, P(out), S())
    torch.cuda.synchronize()
    check_guards(buf, n, words, shift)
    return out.cpu().numpy()


def weighted_tables(M):
    from mused_amd import fusion

    w = ((1.0, 0.5, 0.75) * 3)[:M]
    return [fusion.threshold_table(w, 1.25), fusion.threshold_table(w, 1.5)]


def tables_for(M):
    if M <= 3:
        return fc.all_tables(M)
    named = [fc.or_table(M), fc.and_table(M), fc.majority_table(M)]
    if M in (5, 8):
        return named + weighted_tables(M) + fc.random_tables(M, 16, 1000 + M)
    return named + fc.random_tables(M, 4, 1000 + M)


_INPUTS = {}


def inputs(n, M):
    """M boolean matrices and their subset index, computed once per (n, M)."""
    if (n, M) not in _INPUTS:
        mats = fc.make_masks(n, M, 17 * n + M)
        _INPUTS[(n, M)] = (mats, fc.subset_index(mats))
    return _INPUTS[(n, M)]


@pytest.mark.parametrize("M", range(1, 9))
@pytest.mark.parametrize("n", SIZES)
def test_tables(L, n, M):
    from mused_amd import fusion

    mats, s = inputs(n, M)
    if n * n >= (1 << M):
        assert fc.subsets_present(mats) == set(range(1 << M))
    tables = tables_for(M)
    assert len(tables) == {1: 1, 2: 7, 3: 127, 5: 21, 8: 21}.get(M, 7)
    for words in ((n + 63) // 64, (n + 63) // 64 + 3):
        d_masks = [dev(fc.pack_mask(A, words)) for A in mats]
        for i, T in enumerate(tables):
            ref = fc.fuse_by_index(s, T)
            if i == 0:
                assert np.array_equal(ref, fusion.fuse_table_numpy(mats, T))
            got = fuse_table(L, d_masks, T, n, words)
            assert np.array_equal(got, fc.pack_mask(ref, words)), (n, words, M, i)
            bits = fc.unpack_mask(got, n)
            assert not bits[:, n:].any(), "a bit at a column >= n or in a padding word"


@pytest.mark.parametrize("M", [2, 5, 8])
def test_buffers_off_the_16_byte_boundary(L, M):
    """n * words even, but the output (then an input) starts 8 bytes off: one word per thread, the same mask."""
    n, words = 64, 4
    mats, s = inputs(n, M)
    T = fc.random_tables(M, 1, 7)[0]
    want = fc.pack_mask(fc.fuse_by_index(s, T), words)
    d_masks = [dev(fc.pack_mask(A, words)) for A in mats]
    assert all(m.data_ptr() % 16 == 0 for m in d_masks)
    assert np.array_equal(fuse_table(L, d_masks, T, n, words, shift=1), want)
    odd = torch.zeros(n * words + 1, dtype=torch.int64, device="cuda")
    odd[1:] = d_masks[0].view(-1)
    shifted = [odd[1:].view(n, words)] + d_masks[1:]
    assert shifted[0].data_ptr() % 16 == 8
    assert np.array_equal(fuse_table(L, shifted, T, n, words), want)


@pytest.mark.parametrize("n,words", [(65, 2), (65, 5), (257, 8)])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 8])
def test_in_place(L, n, words, M):
    """out aliased to each input in turn: the mask of a fresh output."""
    mats, s = inputs(n, M)
    for T in tables_for(M)[-3:]:
        want = fc.pack_mask(fc.fuse_by_index(s, T), words)
        for alias in range(M):
            d_masks = [dev(fc.pack_mask(A, words)) for A in mats]
            L.call("mused_adj_fuse_table", pointers(d_masks), M, table_arg(T), n, words, P(d_masks[alias]), S())
            torch.cuda.synchronize()
            assert np.array_equal(d_masks[alias].cpu().numpy(), want)
            for m in range(M):
                if m != alias:
                    assert np.array_equal(d_masks[m].cpu().numpy(), fc.pack_mask(mats[m], words)), "an input changed"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("M", [1, 2, 3, 5, 8])
def test_or_table_is_adj_fuse(L, n, M):
    mats, _ = inputs(n, M)
    for words in ((n + 63) // 64, (n + 63) // 64 + 3):
        d_masks = [dev(fc.pack_mask(A, words)) for A in mats]
        ref = torch.full((n, words), SENTINEL, dtype=torch.int64, device="cuda")
        L.call("mused_adj_fuse", pointers(d_masks), M, n, words, P(ref), S())
        assert np.array_equal(fuse_table(L, d_masks, fc.or_table(M), n, words), ref.cpu().numpy())


def test_edgeless_results(L):
    """An AND of modalities that never agree, and empty inputs: the all-zero mask (the kernel only produces it)."""
    n, words = 65, 2
    A = fc.make_masks(n, 1, 3)[0]
    d_masks = [dev(fc.pack_mask(A, words)), dev(fc.pack_mask(~A, words))]
    assert not fuse_table(L, d_masks, fc.and_table(2), n, words).any()
    zeros = [dev(np.zeros((n, words), dtype=np.int64))] * 3
    assert not fuse_table(L, zeros, fc.or_table(3), n, words).any()
    assert not fuse_table(L, d_masks, np.zeros(4, dtype=np.uint64), n, words).any()   # the table that accepts nothing


def fuse_threshold(L, d_masks, weights, tau, n, words):
    buf, out = guarded(n, words)
    w = None if weights is None else (C.c_double * len(weights))(*weights)
    rc = L.lib().mused_adj_fuse_threshold(pointers(d_masks), w, len(d_masks), tau, n, words, P(out), S())
    torch.cuda.synchronize()
    check_guards(buf, n, words)
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("weights,tau", fc.threshold_cases())
def test_threshold_entry_is_the_table_of_threshold_table(L, weights, tau):
    from mused_amd import fusion

    n, words, M = 65, 2, len(weights)
    mats, _ = inputs(n, M)
    d_masks = [dev(fc.pack_mask(A, words)) for A in mats]
    try:
        T = fusion.threshold_table(weights, tau)
    except ValueError:
        T = None
    rc, got = fuse_threshold(L, d_masks, list(weights), tau, n, words)
    if T is None:
        assert rc == ERR_ARG and (got == SENTINEL).all() and L.lib().mused_last_error()
        return
    assert rc == 0 and np.array_equal(got, fuse_table(L, d_masks, T, n, words))
    assert np.array_equal(got, fc.pack_mask(fusion.fuse_table_numpy(mats, T), words))
    if all(w == 1.0 for w in weights):   # weights NULL = all 1.0
        rc, unweighted = fuse_threshold(L, d_masks, None, tau, n, words)
        assert rc == 0 and np.array_equal(unweighted, got)


def test_bad_arguments(L):
    n, words, M = 65, 2, 2
    mats, _ = inputs(n, M)
    d_masks = [dev(fc.pack_mask(A, words)) for A in mats]
    out = torch.full((n, words), SENTINEL, dtype=torch.int64, device="cuda")
    lib = L.lib()

    def table(M=M, T=None, ptrs=None, n=n, words=words, o=out, null_masks=False, null_table=False):
        ptrs = [m.data_ptr() for m in d_masks] if ptrs is None else ptrs
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        T = fc.or_table(min(max(M, 1), 8)) if T is None else T
        return lib.mused_adj_fuse_table(None if null_masks else arr, M, None if null_table else table_arg(T), n, words,
                                        P(o) if o is not None else None, S())

    def threshold(M=M, w=(1.0, 1.0), tau=1.0, ptrs=None, words=words, null_masks=False):
        ptrs = [m.data_ptr() for m in d_masks] if ptrs is None else ptrs
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        wa = None if w is None else (C.c_double * max(len(w), 1))(*w)
        return lib.mused_adj_fuse_threshold(None if null_masks else arr, wa, M, tau, n, words, P(out), S())

    def refused(rc):
        torch.cuda.synchronize()
        msg = lib.mused_last_error()
        return rc == ERR_ARG and bool(msg) and b"mused_adj_fuse" in msg and bool((out == SENTINEL).all().item())

    nine = [d_masks[0].data_ptr()] * 9
    assert refused(table(M=0)) and refused(table(M=9, ptrs=nine))
    assert refused(table(null_masks=True)) and refused(table(null_table=True)) and refused(table(o=None))
    assert refused(table(ptrs=[d_masks[0].data_ptr(), None]))
    assert refused(table(T=fc.table_of_bits([1, 1, 1, 1])))              # bit 0
    assert refused(table(T=fc.table_of_bits([0, 1, 1, 1, 1])))           # bit 4 = 2^M
    assert refused(table(T=fc.table_of_bits([0, 1] + [0] * 253 + [1])))  # bit 255
    assert refused(table(words=1)) and refused(table(n=0))               # a pitch below ceil(n/64)
    assert refused(threshold(M=0)) and refused(threshold(M=9, w=(1.0,) * 9, ptrs=nine))
    assert refused(threshold(null_masks=True)) and refused(threshold(ptrs=[None, d_masks[1].data_ptr()]))
    assert refused(threshold(words=1))
    for tau in (0.0, -1.0, float("nan"), float("inf"), 2.5, np.nextafter(2.0, 3.0)):
        assert refused(threshold(tau=tau))
    for w in (0.0, -1.0, float("nan"), float("inf")):
        assert refused(threshold(w=(1.0, w)))
    assert table() == 0 and threshold(tau=2.0) == 0 and threshold(w=None, tau=2.0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), fc.pack_mask(mats[0] & mats[1], words))
