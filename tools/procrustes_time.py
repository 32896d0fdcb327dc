#!/usr/bin/env python3
"""What aligning one window costs: matrix_operations.align_embedding_on_device on device tensors (median of 12 calls, each
ending with its 40-byte read) beside SciPy's route for the same tensors -- copy both windows to the host,
scipy.linalg.orthogonal_procrustes on the shared rows, E @ R, at 16 threads (median of 3).

    python tools/procrustes_time.py            # prints a Markdown table

Shapes (m shared rows, r columns, W rows a window)."""
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")
os.environ.setdefault("MKL_NUM_THREADS", "16")

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from mused_amd import matrix_operations as mo  # noqa: E402

SHAPES = [(1000, 50, 2000), (5000, 50, 10000), (7500, 100, 10000), (5000, 128, 10000)]


def windows(m, r, W, seed=0):
    """Two windows that share m rows up to a rotation and 1e-3 of noise, columns orthonormal like an embedding's."""
    rng = np.random.default_rng(seed)
    ref = np.linalg.qr(rng.standard_normal((W, r)))[0]
    Q = np.linalg.qr(rng.standard_normal((r, r)))[0]
    new = np.vstack([ref[W - m:] @ Q, np.linalg.qr(rng.standard_normal((W, r)))[0][:W - m]])
    return new + 1e-3 * rng.standard_normal(new.shape) / np.sqrt(W), ref


def main():
    from scipy.linalg import orthogonal_procrustes

    print("| m | r | W | device (ms) | SciPy with its copies (ms) | of which copies (ms) | sweeps |")
    print("|---|---|---|---|---|---|---|")
    for m, r, W in SHAPES:
        new, ref = windows(m, r, W)
        En, Er = torch.from_numpy(new).cuda(), torch.from_numpy(ref).cuda()
        shift = W - m
        before = mo.procrustes_fallbacks
        mo.align_embedding_on_device(En, Er, shift)          # workspace, LDS opt-in
        torch.cuda.synchronize()
        dev = []
        for _ in range(12):
            t0 = time.perf_counter()
            mo.align_embedding_on_device(En, Er, shift)      # (returns after its read)
            dev.append(1e3 * (time.perf_counter() - t0))
        assert mo.procrustes_fallbacks == before, "a timed call fell back to the host"
        sweeps = int(mo.procrustes_launch(En[:m], Er[shift:], torch.cuda.current_stream())[2].cpu()[1])
        host, copies = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            a, b = En.cpu().numpy(), Er.cpu().numpy()
            t1 = time.perf_counter()
            R = orthogonal_procrustes(a[:m], b[shift:])[0]
            out = a @ R
            host.append(1e3 * (time.perf_counter() - t0))
            copies.append(1e3 * (t1 - t0))
        del out
        print(f"| {m:,} | {r} | {W:,} | {statistics.median(dev):.3f} | {statistics.median(host):.3f} | "
              f"{statistics.median(copies):.3f} | {sweeps} |", flush=True)


if __name__ == "__main__":
    main()
