"""On the GPU: the batched fp64 GEMM with a K bound per batch entry and with a compacted list of the entries to compute
(csrc/gemm_f64.h: `kact`, `list`), at the shape of the FD rotate product T_s = Wc_s buf_s (M = 128, N = 64, K = 256).  Both
operands are exact zeros from the bound on, so the bounded product must equal the full one bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

M, N, K, BATCH = 128, 64, 256, 4
KACT = [128, 144, 200, 256]
SENT = -1.2345678912345e300


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def launch(A, B, lst=None, kact=None):
    """C[z] = A[z] (M x K, K contiguous) B[z] (K x N, N contiguous) through the library's batched launch; C pre-filled with a
    sentinel.  lst: the entries to compute (the library's layout {count, entries} is built here)."""
    from mused_amd import _lib

    fn = _lib.lib().mused_debug_gemm_f64_batched_active
    fn.restype = C.c_int
    fn.argtypes = ([C.c_int, C.c_int] + [C.c_void_p, C.c_long, C.c_long] * 3 + [C.c_int] * 4 + [C.c_double]
                   + [C.c_void_p] * 3)
    out = torch.full((BATCH, M, N), SENT, dtype=torch.float64, device="cuda")
    dl = None if lst is None else torch.tensor([len(lst)] + list(lst) + [0] * (BATCH - len(lst)), dtype=torch.int32, device="cuda")
    dk = None if kact is None else torch.tensor(kact, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(fn(1, 0, p(A), K, M * K, p(B), N, K * N, p(out), N, M * N, M, N, K, BATCH, 1.0, p(dl), p(dk),
                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def operands():
    """Wc-like A (columns >= the bound zero) and buf-like B (rows >= the bound zero), and the full-K product of the kernel."""
    rng = np.random.default_rng(12)
    A = rng.standard_normal((BATCH, M, K))
    B = rng.standard_normal((BATCH, K, N))
    for z, kb in enumerate(KACT):
        A[z, :, kb:] = 0.0
        B[z, kb:, :] = 0.0
    At, Bt = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    full = launch(At, Bt)
    return A, B, At, Bt, full


def test_the_k_loop_stops_at_the_bound(operands):
    """Operands that are NOT zero beyond the bound: the bounded launch must leave those terms out, i.e. give the bits of the
    full product of the operands cut off at the bound (a launch that ignored kact would add them)."""
    A, B, _, _, full = operands
    rng = np.random.default_rng(13)
    A2, B2 = A.copy(), B.copy()
    for z, kb in enumerate(KACT):
        A2[z, :, kb:] = rng.standard_normal((M, K - kb))
        B2[z, kb:, :] = rng.standard_normal((K - kb, N))
    got = launch(torch.from_numpy(A2).cuda(), torch.from_numpy(B2).cuda(), kact=KACT)
    assert np.array_equal(got.view(np.int64), full.view(np.int64))
    unbounded = launch(torch.from_numpy(A2).cuda(), torch.from_numpy(B2).cuda())
    for z, kb in enumerate(KACT):
        assert (kb == K) == np.array_equal(unbounded[z], full[z]), z     # (the tail terms do matter where there are any)


def test_full_product_is_the_product(operands):
    A, B, _, _, full = operands
    ref = A @ B
    tol = (K + 2) * np.finfo(np.float64).eps * (np.abs(A) @ np.abs(B))
    assert (np.abs(full - ref) <= tol).all()


def test_bounded_k_loop_is_bit_identical(operands):
    _, _, At, Bt, full = operands
    got = launch(At, Bt, kact=KACT)
    assert np.array_equal(got.view(np.int64), full.view(np.int64))


def test_list_skips_an_entry_and_leaves_its_output(operands):
    _, _, At, Bt, full = operands
    lst = [3, 0, 2]                       # entry 1 is not listed; the order of the list is not the order of the batch
    got = launch(At, Bt, lst=lst, kact=KACT)
    for z in lst:
        assert np.array_equal(got[z].view(np.int64), full[z].view(np.int64)), z
    assert (got[1] == SENT).all()
