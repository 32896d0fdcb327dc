"""On the GPU: the diagonal tiles of a symmetric launch of the fp64 MFMA GEMM (csrc/gemm_f64.h).  Such a tile computes
only 36 of its 64 blocks of 16 x 16 (the diagonal ones and one of every pair (i, j) / (j, i)), both MFMA operands from the
one staged panel, and writes the other 28 as mirrors.  The yardstick is the FULL launch of the same product -- the second operand a copy in
another buffer, so the launch is not symmetric and every entry is computed directly by the ordinary main loop: the
symmetric launch must give its bits at every entry, for both layouts, scalar and 16-byte loads, batched, with a list, split
over K, and through the fp32 score epilogues.  (v_mfma_f64_16x16x4_f64 gives (r, c) and (c, r) of A A^T the same bits:
measured on the MI355X before the kernel was written, symmetric against full launch at n = 300, K = 250, both layouts.)

Sentinel and padding idiom of tests/test_gpu_gemm_modes.py: outputs are larger than the result and pre-filled with a
sentinel that must survive outside it; operand padding is NaN."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = np.finfo(np.float64).eps
SENT = -1.2345678912345e300
NS = [1, 15, 16, 17, 48, 127, 128, 129, 144, 255, 256, 257, 384]
KS = [0, 1, 7, 16, 17, 250]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(bad)} of {bad.size} entries differ in their bits, first {i}: "
                             f"{np.asarray(a)[i]!r} against {np.asarray(b)[i]!r}")


def padded(mat, ld, rows=None):
    """mat (r x c) in a row-major buffer of pitch ld >= c (at least `rows` rows); padding NaN."""
    r, c = mat.shape
    rows = max(r, rows or 0, 1)
    buf = np.full((rows, max(ld, 1)), np.nan)
    buf[:r, :c] = mat
    return buf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).ravel()).cuda()


# ------------------------------------------------------------------ one product, both launches ------------------------------
@functools.lru_cache(maxsize=None)
def products(n, K):
    """{(kc, odd): (symmetric, full)}: alpha X X^T of one X (n x K) by the symmetric launch (one buffer for both operands)
    and by the full launch (second operand a copy), as whole output buffers (n + 2) x ldc.  odd: the parity of lda -- odd
    pitches take the scalar loads, even ones the 16-byte loads; alpha = -0.75 with the odd pitch, 1.0 with the even one."""
    from mused_amd import _lib

    rng = np.random.default_rng(1000 * n + K)
    X = rng.standard_normal((n, K))
    ldc = n + 3
    res = {}
    for kc in (1, 0):
        m = X if kc else X.T
        for odd in (0, 1):
            lda = m.shape[1] + (1 if (m.shape[1] + 1) % 2 == odd else 2)
            assert lda % 2 == odd
            alpha = -0.75 if odd else 1.0
            A = dev(padded(m, lda))
            B = A.clone()
            assert B.data_ptr() != A.data_ptr()
            outs = []
            for other in (A, B):
                Cd = sentinel((n + 2) * ldc)
                _lib.call("mused_gemm_f64", kc, kc, P(A), lda, P(other), lda, P(Cd), ldc, n, n, K, alpha, S())
                outs.append(host(Cd).reshape(n + 2, ldc))
            for o in outs:
                o.setflags(write=False)
            res[kc, odd] = (outs[0], outs[1], alpha, X)
    return res


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", NS)
def test_symmetric_equals_full_bitwise(L, n, K):
    """The symmetric launch against the full launch of the same product: the same bits at every entry; nothing written
    outside C (ldc = n + 3, two spare rows); the full launch itself within the rounding bound of the NumPy product."""
    for (kc, odd), (sym, full, alpha, X) in products(n, K).items():
        what = f"n={n} K={K} kc={kc} odd lda={odd} alpha={alpha}"
        for name, out in (("symmetric", sym), ("full", full)):
            assert (out[:n, n:] == SENT).all() and (out[n:] == SENT).all(), f"{what}: the {name} launch wrote outside C"
        tol = (K + 2) * EPS * abs(alpha) * (np.abs(X) @ np.abs(X).T)
        assert (np.abs(full[:n, :n] - alpha * (X @ X.T)) <= tol).all(), what + ": the full launch is off the product"
        assert_bitwise(sym[:n, :n], full[:n, :n], what + ": symmetric against full launch")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", NS)
def test_symmetric_result_is_exactly_symmetric(L, n, K):
    """C == C^T in every bit, inside the diagonal tiles too (tests/test_gpu_gemm_modes.py asserts it across tiles)."""
    for (kc, odd), (sym, _, alpha, _) in products(n, K).items():
        Cm = sym[:n, :n]
        assert_bitwise(Cm, Cm.T, f"n={n} K={K} kc={kc} odd lda={odd}: C against its transpose")


# ------------------------------------------------------------------ batched, with a list -----------------------------------
def _active(L):
    fn = L.lib().mused_debug_gemm_f64_batched_active
    fn.restype = C.c_int
    fn.argtypes = ([C.c_int, C.c_int] + [C.c_void_p, C.c_long, C.c_long] * 3 + [C.c_int] * 4 + [C.c_double]
                   + [C.c_void_p] * 3)
    return fn


@pytest.mark.parametrize("kc", [1, 0])
@pytest.mark.parametrize("n,K", [(129, 33), (256, 250)])
def test_batched_and_listed(L, n, K, kc):
    """Three entries with padded strides (ldc > n, strideC > n ldc): mused_gemm_f64_batched computes all of them, the
    launch with the list {2, 0} leaves entry 1's output alone; every computed entry has the bits of its full product."""
    rng = np.random.default_rng(5 * n + K + kc)
    batch, alpha = 3, 2.5
    Xs = [rng.standard_normal((n, K)) for _ in range(batch)]
    ms = [X if kc else X.T for X in Xs]
    rows, lda = ms[0].shape[0], ms[0].shape[1] + 2
    strideA = rows * lda + 6
    A = np.full(batch * strideA, np.nan)
    for z, m in enumerate(ms):
        A[z * strideA : z * strideA + rows * lda] = padded(m, lda).ravel()
    ldc = n + 1
    strideC = (n + 2) * ldc
    Ad = dev(A)
    Bd = Ad.clone()
    full = sentinel((batch + 1) * strideC)
    L.call("mused_gemm_f64_batched", kc, kc, P(Ad), lda, strideA, P(Bd), lda, strideA, P(full), ldc, strideC, n, n, K, batch,
           alpha, S())
    full = host(full)
    every = sentinel((batch + 1) * strideC)
    L.call("mused_gemm_f64_batched", kc, kc, P(Ad), lda, strideA, P(Ad), lda, strideA, P(every), ldc, strideC, n, n, K, batch,
           alpha, S())
    listed = sentinel((batch + 1) * strideC)
    lst = torch.tensor([2, 2, 0, 0], dtype=torch.int32, device="cuda")  # {count, entries}: entry 1 is not listed
    L.check(_active(L)(kc, kc, P(Ad), lda, strideA, P(Ad), lda, strideA, P(listed), ldc, strideC, n, n, K, batch, alpha, P(lst),
                       None, S()))
    every, listed = host(every), host(listed)
    for name, out, skipped in (("batched", every, ()), ("listed", listed, (1,))):
        assert (out[batch * strideC :] == SENT).all(), name + ": wrote past the last entry"
        for z, X in enumerate(Xs):
            blk = out[z * strideC : (z + 1) * strideC].reshape(n + 2, ldc)
            if z in skipped:
                assert (blk == SENT).all(), f"{name}: skipped entry {z} was written"
                continue
            assert (blk[:n, n:] == SENT).all() and (blk[n:] == SENT).all(), f"{name} entry {z}: wrote outside C"
            ref = full[z * strideC : (z + 1) * strideC].reshape(n + 2, ldc)[:n, :n]
            tol = (K + 2) * EPS * abs(alpha) * (np.abs(X) @ np.abs(X).T)
            assert (np.abs(ref - alpha * (X @ X.T)) <= tol).all(), f"entry {z}: the full launch is off the product"
            assert_bitwise(blk[:n, :n], ref, f"{name} entry {z} against its full product")


# ------------------------------------------------------------------ batched split-K ----------------------------------------
def test_batched_splitk_short_last_split(L):
    """mused_gemm_f64_batched_splitk at n2 = 256, K = 100, three splits of 48 (the last one covers 4 columns), A == B: every
    partial has the bits of the full product of its K range (mused_gemm_f64 on the column range, second operand a copy),
    and the reduced sum those of the partials added in split order."""
    n2, K, kchunk, nsplit, batch = 256, 100, 48, 3, 2
    rng = np.random.default_rng(77)
    lda = K + 2
    strideA = n2 * lda + 4
    Xs = [rng.standard_normal((n2, K)) for _ in range(batch)]
    A = np.full(batch * strideA, np.nan)
    for z, X in enumerate(Xs):
        A[z * strideA : z * strideA + n2 * lda] = padded(X, lda).ravel()
    Ad = dev(A)
    Bd = Ad.clone()
    count = n2 * n2
    part, Cd = sentinel(batch * nsplit * count + 33), sentinel((batch + 1) * count)
    L.call("mused_gemm_f64_batched_splitk", 1, 1, P(Ad), lda, strideA, P(Ad), lda, strideA, P(part), P(Cd), n2, n2, K, batch,
           kchunk, nsplit, None, S())
    part, out = host(part), host(Cd)
    assert (part[batch * nsplit * count :] == SENT).all(), "partials written past the end"
    assert (out[batch * count :] == SENT).all(), "C written past the last entry"
    part = part[: batch * nsplit * count].reshape(batch, nsplit, n2, n2)
    out = out[: batch * count].reshape(batch, n2, n2)
    for z, X in enumerate(Xs):
        s = np.zeros((n2, n2))
        for sp in range(nsplit):
            lo, hi = sp * kchunk, min(K, (sp + 1) * kchunk)
            one = sentinel(count)
            L.call("mused_gemm_f64", 1, 1, P(Ad[z * strideA + lo :]), lda, P(Bd[z * strideA + lo :]), lda, P(one), n2, n2, n2,
                   hi - lo, 1.0, S())
            one = host(one).reshape(n2, n2)
            x = X[:, lo:hi]
            assert (np.abs(one - x @ x.T) <= (hi - lo + 2) * EPS * (np.abs(x) @ np.abs(x).T)).all(), (z, sp)
            assert_bitwise(part[z, sp], one, f"entry {z} split {sp} against the full product of its K range")
            s = s + one
        assert_bitwise(out[z], s, f"entry {z}: reduced sum against the full per-split products added in split order")


# ------------------------------------------------------------------ fp32 rows, score epilogues ------------------------------
_CHILD = """
import ctypes as C, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from mused_amd import _lib
X = np.load(sys.argv[2])
n, d = X.shape
Xd = torch.from_numpy(X).cuda()
outs = []
for metric in (0, 1):
    ws = torch.zeros(n, dtype=torch.float64, device="cuda")
    out = torch.zeros(n * n, dtype=torch.float64, device="cuda")
    _lib.call("mused_pairwise_scores", C.c_void_p(Xd.data_ptr()), _lib.F32, n, d, d, metric, C.c_void_p(ws.data_ptr()),
              C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    outs.append(out.cpu().numpy().reshape(n, n))
np.save(sys.argv[3], np.stack(outs))
"""


def test_fp32_scores_against_the_unsymmetric_launch(L, tmp_path):
    """mused_pairwise_scores on float rows, n = 257, d = 40 (EpiSqL2 and EpiNegCos, neither commutative in rounding): within
    the band of tests/test_gpu_scores_layout.py -- (d + 8) eps (|x|^2 + |y|^2) and (d + 8) eps -- of the float64 NumPy
    formula, and the bits of the same call in a fresh child process with MUSED_SCORES_SYM=0, where every tile runs the
    ordinary main loop and nothing is mirrored."""
    n, d = 257, 40
    rng = np.random.default_rng(4057)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Xd = torch.from_numpy(X).cuda()
    got = []
    for metric in (L.METRIC_L2, L.METRIC_COSINE):
        ws = torch.full((n + 1,), np.nan, dtype=torch.float64, device="cuda")
        out = torch.full((n * n + 1,), np.nan, dtype=torch.float64, device="cuda")
        L.call("mused_pairwise_scores", P(Xd), L.F32, n, d, d, metric, P(ws), P(out), S())
        out = host(out)
        assert np.isnan(out[n * n]), "written past the output"
        got.append(out[: n * n].reshape(n, n))
    X64 = X.astype(np.float64)
    nrm = (X64 * X64).sum(axis=1)
    dot = X64 @ X64.T
    coef = (d + 8) * EPS
    l2 = np.maximum(nrm[:, None] - 2 * dot + nrm[None, :], 0.0)
    inv = 1 / np.sqrt(nrm)
    cos = 0.0 - dot * inv[:, None] * inv[None, :]
    e_l2 = float(np.max(np.abs(got[0] - l2) / (coef * (nrm[:, None] + nrm[None, :]))))
    e_cos = float(np.max(np.abs(got[1] - cos) / coef))
    print(f"|device - float64 formula| / band: l2 {e_l2:.3f}  cosine {e_cos:.3f}")
    assert e_l2 <= 1 and e_cos <= 1, (e_l2, e_cos)
    # (no S == S^T here: |x|^2 - 2 x.y + |y|^2 rounds differently in the two orientations, which is why a mirrored entry is
    # evaluated in its own)

    src, dst = tmp_path / "rows.npy", tmp_path / "scores.npy"
    np.save(src, X)
    env = dict(os.environ, MUSED_SCORES_SYM="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _CHILD, ROOT, str(src), str(dst)]
    subprocess.run(cmd, env=env, check=True, timeout=300)
    plain = np.load(dst)
    assert_bitwise(got[0], plain[0], "squared L2: symmetric launch against MUSED_SCORES_SYM=0")
    assert_bitwise(got[1], plain[1], "cosine: symmetric launch against MUSED_SCORES_SYM=0")
