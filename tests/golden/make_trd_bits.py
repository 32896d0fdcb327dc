"""Generator of tests/golden/trd_bits.npz: the bits the direct eigensolver (csrc/trd.hip) produced on a fixed set of
matrices -- d, e of the tridiagonal matrix, the eigenvalues, the certificate's verdict and a SHA-256 of the returned matrix
-- recorded on the GPU at the commit BEFORE a change that must not move them.  tests/test_gpu_trd_bits.py replays the same
cases and asserts equality on the bit patterns.

    python tests/golden/make_trd_bits.py [PATH]     # (on the GPU, library built) writes tests/golden/trd_bits.npz or PATH

The inputs are G = B B^T of small integer matrices (entries in [-8, 8]): exact in fp64 whatever the BLAS does, so every host
builds the same bits.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "trd_bits.npz")


def int_gram(rng, n, m):
    B = rng.integers(-8, 9, size=(n, m)).astype(np.float64)
    return B @ B.T


def block_diagonal(rng):
    """100 x 100 Gram | 56 distinct integers on the diagonal | 100 x 100 Gram: the reflectors of steps 99 .. 155 are identities."""
    G = np.zeros((256, 256))
    G[:100, :100] = int_gram(rng, 100, 120)
    G[100:156, 100:156] = np.diag(rng.permutation(np.arange(1000.0, 1056.0)))
    G[156:, 156:] = int_gram(rng, 100, 120)
    return G


def cases():
    """name -> (list of matrices, n, need): one launch per entry."""
    rng = np.random.default_rng(20260)
    full = int_gram(rng, 256, 300)
    blockdiag = block_diagonal(rng)
    diagonal = np.diag(rng.permutation(np.arange(1.0, 257.0)))
    rank40 = int_gram(rng, 256, 40)
    out = {
        "full256": ([full], 256, 128),
        "blockdiag": ([blockdiag], 256, 128),
        "diagonal": ([diagonal], 256, 128),
        "rank40": ([rank40], 256, 128),
        "n200": ([int_gram(rng, 200, 230), int_gram(rng, 200, 60)], 200, 100),   # off = 56
        "n129": ([int_gram(rng, 129, 150)], 129, 64),                             # off = 127: first step closes a K block
        "n33": ([int_gram(rng, 33, 40)], 33, 32),
        "n2": ([int_gram(rng, 2, 3)], 2, 1),
        "batch3": ([block_diagonal(rng), int_gram(rng, 256, 40), int_gram(rng, 256, 300)], 256, 128),
    }
    return out


def solve(Gs, n, need):
    """mused_debug_trd (order 256) / mused_debug_trd_n (embedded orders) on one batch: returned matrices, d, e, lam, done."""
    import torch

    from mused_amd import _lib
    from mused_amd.engine import ptr, stream_ptr

    L = _lib.lib()
    B = len(Gs)
    G = torch.from_numpy(np.ascontiguousarray(np.stack(Gs))).cuda()
    d = torch.zeros(B, 256, dtype=torch.float64, device="cuda")
    e = torch.zeros(B, 256, dtype=torch.float64, device="cuda")
    lam = torch.zeros(B, 128, dtype=torch.float64, device="cuda")
    res = torch.zeros(B, 128, dtype=torch.float64, device="cuda")
    done = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    if n == 256 and need == 128:
        fn = L.mused_debug_trd
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _lib.check(fn(ptr(G), B, ptr(d), ptr(e), ptr(lam), ptr(res), ptr(done), stream_ptr()))
    else:
        fn = L.mused_debug_trd_n
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
        _lib.check(fn(ptr(G), n, need, 0, B, ptr(d), ptr(e), ptr(lam), ptr(res), ptr(done), stream_ptr()))
    torch.cuda.synchronize()
    nvec = 32 * ((need + 31) // 32)   # eigenvalues formed (the entries of lam behind them are not written)
    return G.cpu().numpy(), d.cpu().numpy(), e.cpu().numpy(), lam.cpu().numpy()[:, :nvec], done.cpu().numpy()


def record(name, Gs, n, need):
    """The arrays of one case as the fixture holds them (int64 views: NaN-safe, bit-exact comparisons)."""
    out, d, e, lam, done = solve(Gs, n, need)
    sha = np.array([hashlib.sha256(np.ascontiguousarray(out[b]).tobytes()).hexdigest() for b in range(len(Gs))])
    return {f"{name}/d": d.view(np.int64), f"{name}/e": e.view(np.int64), f"{name}/lam": lam.view(np.int64),
            f"{name}/done": done.astype(np.int32), f"{name}/sha": sha}, out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    arrays = {}
    for name, (Gs, n, need) in cases().items():
        rec, out = record(name, Gs, n, need)
        done = rec[f"{name}/done"]
        for b, G in enumerate(Gs):
            assert done[b] in (0, 1), (name, b, done[b])
            if done[b] == 0:  # rejected by the certificate: the input must come back untouched
                assert np.array_equal(out[b], G), (name, b)
        print(f"{name}: done = {done.tolist()}", flush=True)
        arrays.update(rec)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
