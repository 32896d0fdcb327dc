"""On the GPU: the launch modes of the fp64 MFMA GEMM (csrc/gemm_f64.h, csrc/gemm_f64.hip) that the library reaches only
from inside -- symmetric launches (A == B: upper tiles + mirrored stores), split-K with its fixed-order sum, batched split-K
and plain batched launches that skip duplicate entries (rep) -- against a NumPy fp64 reference.

Bound: |C - C_ref| <= (K + c) eps |alpha| (|A| |B|) elementwise (the rounding of two length-K sums, the kernel's and the
reference's).  Every output buffer is larger than the result and pre-filled with a sentinel that must survive outside it;
operand padding holds NaN, so a load outside the operands poisons the result."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = np.finfo(np.float64).eps
SENT = -1.2345678912345e300
MUSED_ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def sentinel(count):
    return torch.full((count,), SENT, dtype=torch.float64, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_bitwise(a, b, what):
    bad = bits(a) != bits(b)
    assert not bad.any(), f"{what}: {np.count_nonzero(bad)} of {bad.size} entries differ in their bits"


def assert_within(Cm, ref, absprod, K, alpha=1.0, extra=2, what=""):
    tol = (K + extra) * EPS * abs(alpha) * absprod
    err = np.abs(Cm - ref)
    bad = ~(err <= tol)  # NaN / sentinel fail too
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} entries outside the bound, first {tuple(i)}: "
                             f"got {Cm[tuple(i)]!r}, want {ref[tuple(i)]!r} +- {tol[tuple(i)]!r}")


def padded(mat, ld, rows=None):
    """mat (r x c) in a row-major buffer of pitch ld >= c (at least `rows` rows); padding NaN."""
    r, c = mat.shape
    rows = max(r, rows or 0, 1)
    buf = np.full((rows, max(ld, 1)), np.nan)
    buf[:r, :c] = mat
    return buf


def stored(op, kc, pad):
    """Storage of an operand the kernel reads as `op` (rows = M or N, cols = K): kc -> op itself, else op.T (K rows)."""
    m = op if kc else op.T
    return m, m.shape[1] + pad


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).ravel()).cuda()


def tile_mirror_mask(n, tile=128):
    i = np.arange(n)
    return (i[:, None] // tile) != (i[None, :] // tile)


# ------------------------------------------------------------------ symmetric launches --------------------------------------
@pytest.mark.parametrize("K", [0, 1, 7, 16, 250, 1024])
@pytest.mark.parametrize("n", [1, 15, 16, 127, 128, 129, 255, 257, 513, 1100])
def test_symmetric_gemm(L, n, K):
    """C = alpha A A^T through mused_gemm_f64 with the same buffer for both operands: both layouts, odd (scalar loads) and
    even (16-byte loads) leading dimensions.  Pairs (i, j) / (j, i) in different 128-tiles are written by the mirror
    store of one accumulator: bitwise equal."""
    rng = np.random.default_rng(1000 * n + K)
    X = rng.standard_normal((n, K))
    ref = X @ X.T
    absprod = np.abs(X) @ np.abs(X).T
    off = tile_mirror_mask(n)
    ldc = n + 3
    for kc in (1, 0):
        for odd in (0, 1):
            m, _ = stored(X, kc, 0)
            lda = m.shape[1] + (1 if (m.shape[1] + 1) % 2 == odd else 2)
            assert lda % 2 == odd
            alpha = -0.75 if odd else 1.0
            A = dev(padded(m, lda))
            Cd = sentinel((n + 2) * ldc)
            L.call("mused_gemm_f64", kc, kc, P(A), lda, P(A), lda, P(Cd), ldc, n, n, K, alpha, S())
            out = host(Cd).reshape(n + 2, ldc)
            what = f"n={n} K={K} kc={kc} lda={lda}"
            assert (out[:n, n:] == SENT).all() and (out[n:] == SENT).all(), what + ": wrote outside C"
            Cm = out[:n, :n]
            if K == 0:
                assert (Cm == 0).all(), what
            assert_within(Cm, alpha * ref, absprod, K, alpha, what=what)
            assert_bitwise(Cm[off], Cm.T[off], what + " mirrored pairs")


@pytest.mark.parametrize("kc", [1, 0])
@pytest.mark.parametrize("n,K", [(129, 250), (300, 1000)])
def test_symmetric_gemm_batched_strided(L, n, K, kc):
    """mused_gemm_f64_batched with A == B: batch 3 with padded strides, ldc > N, strideC > M ldc, a spare batch slot."""
    rng = np.random.default_rng(n + K + kc)
    batch, alpha = 3, 2.5
    Xs = [rng.standard_normal((n, K)) for _ in range(batch)]
    m0, lda = stored(Xs[0], kc, 2)
    rows = m0.shape[0]
    strideA = rows * lda + 6
    A = np.full(batch * strideA, np.nan)
    for z, X in enumerate(Xs):
        A[z * strideA : z * strideA + rows * lda] = padded(stored(X, kc, 2)[0], lda).ravel()
    ldc = n + 1
    strideC = (n + 2) * ldc
    Ad, Cd = dev(A), sentinel((batch + 1) * strideC)
    L.call("mused_gemm_f64_batched", kc, kc, P(Ad), lda, strideA, P(Ad), lda, strideA, P(Cd), ldc, strideC, n, n, K, batch,
           alpha, S())
    out = host(Cd)
    assert (out[batch * strideC :] == SENT).all()
    off = tile_mirror_mask(n)
    for z, X in enumerate(Xs):
        blk = out[z * strideC : (z + 1) * strideC].reshape(n + 2, ldc)
        assert (blk[:n, n:] == SENT).all() and (blk[n:] == SENT).all(), f"entry {z}: wrote outside C"
        Cm = blk[:n, :n]
        assert_within(Cm, alpha * (X @ X.T), np.abs(X) @ np.abs(X).T, K, alpha, what=f"entry {z}")
        assert_bitwise(Cm[off], Cm.T[off], f"entry {z} mirrored pairs")


# ------------------------------------------------------------------ split-K -------------------------------------------------
def _ordered_sum(parts):
    s = np.zeros_like(parts[0])
    for p in parts:
        s = s + p
    return s


def _operands(rng, M, N, K, a_kc, b_kc, same):
    Aop = rng.standard_normal((M, K))
    Bop = Aop.T.copy() if same else rng.standard_normal((K, N))
    am, lda = stored(Aop, a_kc, 1)
    bm, ldb = stored(Bop.T, b_kc, 3)
    return Aop, Bop, padded(am, lda), lda, padded(bm, ldb), ldb


@pytest.mark.parametrize("a_kc,b_kc,same", [(1, 1, False), (1, 0, False), (0, 1, False), (0, 0, False), (0, 0, True)])
def test_splitk_fixed_order_and_empty_splits(L, a_kc, b_kc, same):
    """mused_gemm_f64_splitk with K = 1000 (not a multiple of 16) over 12 chunks of 128: splits 8 .. 11 are empty and must
    store exact zeros; C is the split partials summed in split order, bit for bit.  (0, 0, same) is the rSVD Gram."""
    M, K, kchunk, nsplit = 150, 1000, 128, 12
    N = M if same else 133
    rng = np.random.default_rng(7 + 2 * a_kc + b_kc + 10 * same)
    Aop, Bop, Ab, lda, Bb, ldb = _operands(rng, M, N, K, a_kc, b_kc, same)
    Ad = dev(Ab)
    Bd = Ad if same else dev(Bb)
    if same:
        ldb = lda
    part, Cd = sentinel(nsplit * M * N + 77), sentinel(M * N + 77)
    L.call("mused_gemm_f64_splitk", a_kc, b_kc, P(Ad), lda, P(Bd), ldb, P(part), P(Cd), M, N, K, kchunk, nsplit, S())
    parts, out = host(part), host(Cd)
    assert (parts[nsplit * M * N :] == SENT).all() and (out[M * N :] == SENT).all()
    parts = parts[: nsplit * M * N].reshape(nsplit, M, N)
    full = -(-K // kchunk)
    assert full == 8
    assert (bits(parts[full:]) == 0).all(), "empty splits must store +0.0"
    for s in range(full):
        lo, hi = s * kchunk, min(K, (s + 1) * kchunk)
        a, b = Aop[:, lo:hi], Bop[lo:hi]
        assert_within(parts[s], a @ b, np.abs(a) @ np.abs(b), hi - lo, what=f"split {s}")
    Cm = out[: M * N].reshape(M, N)
    assert_bitwise(Cm, _ordered_sum(parts), "C vs partials summed in split order")
    assert_within(Cm, Aop @ Bop, np.abs(Aop) @ np.abs(Bop), K, extra=nsplit + 2, what="C")


@pytest.mark.parametrize("kchunk,nsplit", [(0, 8), (24, 8), (-16, -100), (16, 0), (128, 7)])
def test_splitk_rejects_bad_chunks(L, kchunk, nsplit):
    """Bad kchunk / nsplit (K = 1000): MUSED_ERR_ARG, nothing launched (partials and C keep the sentinel)."""
    M = N = 40
    K, batch = 1000, 2
    A = dev(np.ones(batch * M * K))
    part, Cd = sentinel(batch * 16 * M * N), sentinel(batch * M * N)
    lib = L.lib()
    rc = lib.mused_gemm_f64_splitk(1, 1, P(A), K, P(A), K, P(part), P(Cd), M, N, K, kchunk, nsplit, S())
    assert rc == MUSED_ERR_ARG and b"bad kchunk" in lib.mused_last_error()
    rc = lib.mused_gemm_f64_batched_splitk(1, 1, P(A), K, M * K, P(A), K, M * K, P(part), P(Cd), M, N, K, batch, kchunk, nsplit,
                                           None, S())
    assert rc == MUSED_ERR_ARG and b"bad kchunk" in lib.mused_last_error()
    assert (host(part) == SENT).all() and (host(Cd) == SENT).all()


# ------------------------------------------------------------------ batched split-K + rep -----------------------------------
REP = [3, 1, 1, 3, 4, 3]  # self-representatives 1, 3, 4; entries 0, 2, 5 are duplicates (skipped), in mixed order


def _batched_operands(rng, batch, M, N, K, same):
    """Per-entry K-contiguous operands (the sketch Gram's layout), strides padded by 4 doubles."""
    lda = K + 2
    strideA = M * lda + 4
    Aops = [rng.standard_normal((M, K)) for _ in range(batch)]
    A = np.full(batch * strideA, np.nan)
    for z, a in enumerate(Aops):
        A[z * strideA : z * strideA + M * lda] = padded(a, lda).ravel()
    if same:
        return Aops, [a.T for a in Aops], A, lda, strideA, None, lda, strideA
    ldb = K + 4
    strideB = N * ldb + 2
    Bops = [rng.standard_normal((K, N)) for _ in range(batch)]
    B = np.full(batch * strideB, np.nan)
    for z, b in enumerate(Bops):
        B[z * strideB : z * strideB + N * ldb] = padded(b.T, ldb).ravel()
    return Aops, Bops, A, lda, strideA, B, ldb, strideB


def _run_batched_splitk(L, Ad, lda, strideA, Bd, ldb, strideB, M, N, K, batch, kchunk, nsplit, rep):
    part, Cd = sentinel(batch * nsplit * M * N + 33), sentinel((batch + 1) * M * N)
    L.call("mused_gemm_f64_batched_splitk", 1, 1, P(Ad), lda, strideA, P(Bd), ldb, strideB, P(part), P(Cd), M, N, K, batch,
           kchunk, nsplit, P(rep), S())
    parts, out = host(part), host(Cd)
    assert (parts[batch * nsplit * M * N :] == SENT).all(), "partials written past the end"
    assert (out[batch * M * N :] == SENT).all(), "C written past the last entry"
    return parts[: batch * nsplit * M * N].reshape(batch, nsplit, M, N), out[: batch * M * N].reshape(batch, M, N)


@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("kchunk,nsplit", [(128, 8), (256, 8)])
def test_batched_splitk_rep(L, same, kchunk, nsplit):
    """Duplicates are skipped in both steps (their partials and C keep the sentinel); every computed entry is its partials
    summed in split order and is bitwise the entry computed alone (batch 1), the property the lanes tests rely on.
    K = 1000: with kchunk = 256, splits 4 .. 7 are empty."""
    batch, K = len(REP), 1000
    M = 130
    N = M if same else 77
    rng = np.random.default_rng(11 + same + kchunk)
    Aops, Bops, A, lda, strideA, B, ldb, strideB = _batched_operands(rng, batch, M, N, K, same)
    Ad = dev(A)
    Bd = Ad if same else dev(B)
    rep = torch.tensor(REP, dtype=torch.int32, device="cuda")
    parts, Cm = _run_batched_splitk(L, Ad, lda, strideA, Bd, ldb, strideB, M, N, K, batch, kchunk, nsplit, rep)
    full = -(-K // kchunk)
    for z in range(batch):
        if REP[z] != z:
            assert (parts[z] == SENT).all() and (Cm[z] == SENT).all(), f"skipped entry {z} was written"
            continue
        assert (bits(parts[z, full:]) == 0).all(), f"entry {z}: empty splits must store +0.0"
        assert_bitwise(Cm[z], _ordered_sum(parts[z]), f"entry {z} vs its partials summed in split order")
        a, b = Aops[z], Bops[z]
        assert_within(Cm[z], a @ b, np.abs(a) @ np.abs(b), K, extra=nsplit + 2, what=f"entry {z}")
        if same:
            off = tile_mirror_mask(M)
            assert_bitwise(Cm[z][off], Cm[z].T[off], f"entry {z} mirrored pairs")
        # the same entry alone
        Az = Ad[z * strideA :]
        Bz = Az if same else Bd[z * strideB :]
        p1, c1 = _run_batched_splitk(L, Az, lda, strideA, Bz, ldb, strideB, M, N, K, 1, kchunk, nsplit, None)
        assert_bitwise(p1[0], parts[z], f"entry {z} partials alone vs in the batch")
        assert_bitwise(c1[0], Cm[z], f"entry {z} alone vs in the batch")


@pytest.mark.parametrize("n2", [64, 300])
@pytest.mark.parametrize("K", [8192, 10000])
def test_batched_splitk_sketch_gram(L, K, n2):
    """The SWFDMC sketch Gram at d >= 8192: A == B, eight K-slices of the sketch's chunk, orders 2 l = 64 and 300."""
    nsplit, batch = 8, 2
    kchunk = ((K + nsplit - 1) // nsplit + 15) // 16 * 16
    rng = np.random.default_rng(K + n2)
    Aops, Bops, A, lda, strideA, _, _, _ = _batched_operands(rng, batch, n2, n2, K, True)
    Ad = dev(A)
    parts, Cm = _run_batched_splitk(L, Ad, lda, strideA, Ad, lda, strideA, n2, n2, K, batch, kchunk, nsplit, None)
    off = tile_mirror_mask(n2)
    for z in range(batch):
        assert_bitwise(Cm[z], _ordered_sum(parts[z]), f"entry {z} vs its partials summed in split order")
        a = Aops[z]
        assert_within(Cm[z], a @ a.T, np.abs(a) @ np.abs(a).T, K, extra=nsplit + 2, what=f"entry {z}")
        assert_bitwise(Cm[z][off], Cm[z].T[off], f"entry {z} mirrored pairs")
    p1, c1 = _run_batched_splitk(L, Ad[strideA:], lda, strideA, Ad[strideA:], lda, strideA, n2, n2, K, 1, kchunk, nsplit, None)
    assert_bitwise(c1[0], Cm[1], "entry 1 alone vs in the batch")


# ------------------------------------------------------------------ plain batched + rep -------------------------------------
@pytest.mark.parametrize("same", [True, False])
def test_batched_rep_skips_duplicates(L, same):
    """mused_gemm_f64_batched_rep (the SWFD Gram below d = 8192): skipped entries leave their C untouched; computed entries
    meet the bound and equal the entry computed alone through mused_gemm_f64."""
    batch, K, alpha = len(REP), 333, -1.5
    M = 257
    N = M if same else 140
    rng = np.random.default_rng(21 + same)
    Aops, Bops, A, lda, strideA, B, ldb, strideB = _batched_operands(rng, batch, M, N, K, same)
    Ad = dev(A)
    Bd = Ad if same else dev(B)
    ldc = N + 3
    strideC = (M + 1) * ldc
    rep = torch.tensor(REP, dtype=torch.int32, device="cuda")
    Cd = sentinel((batch + 1) * strideC)
    L.call("mused_gemm_f64_batched_rep", 1, 1, P(Ad), lda, strideA, P(Bd), ldb, strideB, P(Cd), ldc, strideC, M, N, K, batch,
           alpha, P(rep), S())
    out = host(Cd)
    assert (out[batch * strideC :] == SENT).all()
    for z in range(batch):
        blk = out[z * strideC : (z + 1) * strideC].reshape(M + 1, ldc)
        if REP[z] != z:
            assert (blk == SENT).all(), f"skipped entry {z} was written"
            continue
        assert (blk[:M, N:] == SENT).all() and (blk[M:] == SENT).all(), f"entry {z}: wrote outside C"
        a, b = Aops[z], Bops[z]
        assert_within(blk[:M, :N], alpha * (a @ b), np.abs(a) @ np.abs(b), K, alpha, what=f"entry {z}")
        C1 = sentinel(M * ldc)
        Az = Ad[z * strideA :]
        Bz = Az if same else Bd[z * strideB :]
        L.call("mused_gemm_f64", 1, 1, P(Az), lda, P(Bz), ldb, P(C1), ldc, M, N, K, alpha, S())
        assert_bitwise(host(C1).reshape(M, ldc)[:, :N], blk[:M, :N], f"entry {z} alone vs in the batch")
