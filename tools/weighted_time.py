"""Times the valued eigenstep products (csrc/spmm_valued.hip) against the binary ones of the same build (csrc/spmm.hip), and
the eigenstep per window valued against binary:

    python tools/weighted_time.py [--json FILE]

On the kNN adjacency of one window of the benchmark stream and on its transpose, at (n, r) = (10,000, 138) and (2,000, 60):
binary and valued, `rows` and `wide`, alternating inside one process; a timing is one HIP-event bracket around LAUNCHES
launches and the figure the median of REPS brackets per launch, in microseconds.  The values are those of a weighted fusion
of the mask with itself shifted by one row (two modalities, weights 1 and 0.5), so that they are not all equal.  Then
`WindowEngine.svd_reduce` on the mask (binary) and on the same mask as a one-modality weighted fusion (valued, the same
pattern), alternating, median of REPS calls in milliseconds, under the default dispatch."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mused_amd import _lib, synth
from mused_amd.engine import Adjacency, WindowEngine, ptr, stream_ptr

PATHS = ("rows", "wide")
KINDS = ("binary", "valued")
REPS, LAUNCHES = 25, 4


def lists_and_values(adj, other):
    """A and A^T lists of `adj`, each with the values of the fusion 1.0 * adj + 0.5 * other restricted to adj's pattern."""
    mT = torch.empty_like(adj.mask)
    _lib.call("mused_adj_transpose", ptr(adj.mask), adj.n, adj.words, ptr(mT), stream_ptr())
    out = {}
    masks = (C.c_void_p * 2)(adj.mask.data_ptr(), other.mask.data_ptr())
    weights = (C.c_double * 2)(1.0, 0.5)
    for which, a, transposed in (("A", adj, 0), ("At", Adjacency(mT, adj.n), 1)):
        rowptr, col = a.neighbour_lists()
        vals = torch.empty(max(int(col.numel()), 1), dtype=torch.float64, device="cuda")
        _lib.call("mused_adj_csr_values", masks, weights, 2, adj.n, adj.words, ptr(rowptr), ptr(col), transposed, ptr(vals),
                  stream_ptr())
        out[which] = (rowptr, col, vals)
    return out


def bracket(fn, count):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    spmm_rows, step_rows = [], []
    for n, d, k, r, ell in ((10000, 1024, 50, 138, 128), (2000, 256, 50, 60, 50)):
        X, _ = synth.stream_window("blob", 0, n, d, 0)
        eng = WindowEngine(n)
        rows = torch.from_numpy(X).cuda()
        adj = eng.knn_adjacency(rows, k)
        other = Adjacency(torch.roll(adj.mask, 1, 0), n)
        Q = torch.randn(n, r, dtype=torch.float64, device="cuda")
        Y = torch.empty(n, r, dtype=torch.float64, device="cuda")
        for which, (rowptr, col, vals) in lists_and_values(adj, other).items():
            nnz = int(col.numel())

            def launch(kind):
                if kind == "binary":
                    _lib.call("mused_spmm_binary", ptr(rowptr), ptr(col), n, ptr(Q), r, r, ptr(Y), r, stream_ptr())
                else:
                    _lib.call("mused_spmm_valued", ptr(rowptr), ptr(col), ptr(vals), n, ptr(Q), r, r, ptr(Y), r, stream_ptr())

            got, times = {}, {(kind, p): [] for kind in KINDS for p in PATHS}
            for p_i, p in enumerate(PATHS):
                _lib.call("mused_spmm_force_path", p_i)
                assert _lib.lib().mused_spmm_binary_path(n, r, r, r, Q.data_ptr() % 16, Y.data_ptr() % 16) == p_i, (p, r)
                launch("valued")
                got[p] = Y.clone()
            assert torch.equal(got["rows"], got["wide"])
            for _ in range(REPS):
                for kind in KINDS:
                    for p_i, p in enumerate(PATHS):
                        _lib.call("mused_spmm_force_path", p_i)
                        times[(kind, p)].append(1e3 * bracket(lambda: launch(kind), LAUNCHES))
            row = {"n": n, "r": r, "lists": which, "nnz": nnz}
            for (kind, p), t in times.items():
                row[f"{kind}_{p}_us"] = float(np.median(t))
                row[f"{kind}_{p}_min_us"] = float(np.min(t))
            spmm_rows.append(row)
            print(f"n {n:6d} r {r:4d} {which:2s} nnz {nnz:7d}: " + "  ".join(
                f"{kind}/{p} {row[f'{kind}_{p}_us']:7.1f} us" for kind in KINDS for p in PATHS), flush=True)
        _lib.call("mused_spmm_force_path", -1)
        # the eigenstep per window under the default dispatch: one engine (one handle, one recorded graph) per kind
        engines = {"binary": eng, "valued": WindowEngine(n)}
        fused = {"binary": eng.fuse([adj]), "valued": engines["valued"].fuse_weighted([adj], [1.0])}
        step = {kind: [] for kind in KINDS}
        for kind in KINDS:   # record the graphs
            engines[kind].svd_reduce(fused[kind], ell, 0, nnz_cap=n * k)
        torch.cuda.synchronize()
        for _ in range(REPS):
            for kind in KINDS:
                step[kind].append(bracket(lambda: engines[kind].svd_reduce(fused[kind], ell, 0, nnz_cap=n * k), 1))
        row = {"n": n, "ell": ell, "r": ell + 10, "k": k}
        for kind in KINDS:
            row[f"{kind}_ms"] = float(np.median(step[kind]))
            row[f"{kind}_min_ms"] = float(np.min(step[kind]))
        step_rows.append(row)
        print(f"n {n:6d} l {ell:4d} eigenstep per window: " + "  ".join(f"{kind} {row[kind + '_ms']:7.3f} ms" for kind in KINDS),
              flush=True)
        for e in engines.values():
            e.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"what": "tools/weighted_time.py: median (and min) per launch / per call, kinds and kernels alternating in "
                               "one process", "reps": REPS, "launches_per_bracket": LAUNCHES, "spmm": spmm_rows,
                       "eigenstep": step_rows}, f, indent=1)


if __name__ == "__main__":
    main()
