"""Times the kernels behind mused_spmm_binary alone (rows, wide; csrc/spmm.hip) on the kNN adjacency of one window of
the benchmark stream and on its transpose, at the panel widths the eigenstep uses:

    python tools/spmm_time.py [--json FILE]

n = 10,000, k = 50 (c2 / c3 / c4): r = 138 and 128 (power iteration and last product of c2), 266 and 256 (c3);
n = 2,000 (refdef): r = 60 and 50.  The kernels alternate inside one process; a timing is one HIP-event bracket around
LAUNCHES launches, and the figure is the median of REPS brackets per launch, in microseconds."""
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
REPS, LAUNCHES = 25, 4


def lists_of(eng, rows, k):
    adj = eng.knn_adjacency(rows, k)
    mT = torch.empty_like(adj.mask)
    _lib.call("mused_adj_transpose", ptr(adj.mask), adj.n, adj.words, ptr(mT), stream_ptr())
    return {"A": adj.neighbour_lists(), "At": Adjacency(mT, adj.n).neighbour_lists()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = []
    for n, d, k, rs in ((10000, 1024, 50, (138, 128, 266, 256)), (2000, 256, 50, (60, 50))):
        X, _ = synth.stream_window("blob", 0, n, d, 0)
        eng = WindowEngine(n)
        lists = lists_of(eng, torch.from_numpy(X).cuda(), k)
        for r in rs:
            Q = torch.randn(n, r, dtype=torch.float64, device="cuda")
            Y = torch.empty(n, r, dtype=torch.float64, device="cuda")
            for which, (rowptr, col) in lists.items():
                nnz = int(col.numel())

                def launch():
                    _lib.call("mused_spmm_binary", ptr(rowptr), ptr(col), n, ptr(Q), r, r, ptr(Y), r, stream_ptr())

                got, times = {}, {p: [] for p in PATHS}
                for p_i, p in enumerate(PATHS):
                    _lib.call("mused_spmm_force_path", p_i)
                    assert _lib.lib().mused_spmm_binary_path(n, r, r, r, Q.data_ptr() % 16, Y.data_ptr() % 16) == p_i, (p, r)
                    launch()
                    got[p] = Y.clone()
                assert all(torch.equal(got["rows"], got[p]) for p in PATHS)
                for _ in range(REPS):
                    for p_i, p in enumerate(PATHS):
                        _lib.call("mused_spmm_force_path", p_i)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(LAUNCHES):
                            launch()
                        e1.record()
                        e1.synchronize()
                        times[p].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
                row = {"n": n, "r": r, "lists": which, "nnz": nnz, "gathered_GB": nnz * r * 8 / 1e9}
                for p in PATHS:
                    row[p + "_us"] = float(np.median(times[p]))
                    row[p + "_min_us"] = float(np.min(times[p]))
                out.append(row)
                print(f"n {n:6d} r {r:4d} {which:2s} nnz {nnz:7d}: " + "  ".join(
                    f"{p} {row[p + '_us']:7.1f} us ({row['gathered_GB'] / row[p + '_us'] * 1e3:5.2f} TB/s)" for p in PATHS), flush=True)
        eng.close()
    _lib.call("mused_spmm_force_path", -1)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"what": "tools/spmm_time.py: median (and min) microseconds per launch, kernels alternating in one process",
                       "reps": REPS, "launches_per_bracket": LAUNCHES, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
