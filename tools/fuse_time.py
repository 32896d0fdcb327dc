"""Times the fusion of M modality masks: the OR chain of mused_adj_fuse (M - 1 launches, each reading two masks and writing
one: 3 (M - 1) passes over a mask) against the one launch of mused_adj_fuse_table with the OR table (M + 1 passes):

    python tools/fuse_time.py [--json FILE] [--small]

The masks are the k = 50 kNN adjacencies of M windows of the benchmark blob stream (one window per modality), at n = 10,000
(d = 1024) for M = 2, 3, 5, 8 and at n = 150,000 (d = 64; 2.8 GB per mask, the batch shape) for M = 2 and 5 (`--small`: the
first shape only).  The two alternate inside one process; a timing is one HIP-event bracket around LAUNCHES calls and the
figure the median of REPS brackets per call, in microseconds, with the GB/s that (M + 1) * n * words * 8 bytes make of it (the
bytes the single pass moves, for both, so that the two columns compare).  Both outputs are compared once."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mused_amd import _lib, fusion, synth
from mused_amd import matrix_operations as mo
from mused_amd.engine import WindowEngine, ptr, stream_ptr

REPS, LAUNCHES, K = 25, 4, 50
SHAPES = ((10000, 1024, (2, 3, 5, 8)), (150000, 64, (2, 5)))


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
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    rows = []
    for n, d, Ms in SHAPES[:1] if args.small else SHAPES:
        eng = WindowEngine(n)
        masks = []
        for m in range(max(Ms)):
            X, _ = synth.stream_window("blob", m, n, d, 0)
            masks.append(mo.adjacency_on_device(torch.from_numpy(X).cuda(), "", K, engine=eng).mask)
        words = masks[0].shape[1]
        out = {kind: torch.empty_like(masks[0]) for kind in ("chain", "table")}
        for M in Ms:
            arr = (C.c_void_p * M)(*[t.data_ptr() for t in masks[:M]])
            words4 = fusion.threshold_table([1.0] * M, 1.0)   # the OR table
            table = words4.ctypes.data_as(C.POINTER(C.c_uint64))
            launch = {
                "chain": lambda: _lib.call("mused_adj_fuse", arr, M, n, words, ptr(out["chain"]), stream_ptr()),
                "table": lambda: _lib.call("mused_adj_fuse_table", arr, M, table, n, words, ptr(out["table"]), stream_ptr()),
            }
            for fn in launch.values():
                fn()
            torch.cuda.synchronize()
            assert torch.equal(out["chain"], out["table"])
            times = {kind: [] for kind in launch}
            for _ in range(REPS):
                for kind, fn in launch.items():
                    times[kind].append(1e3 * bracket(fn, LAUNCHES))
            nbytes = (M + 1) * n * words * 8
            row = {"n": n, "words": words, "M": M, "bytes_single_pass": nbytes}
            for kind, t in times.items():
                row[f"{kind}_us"] = float(np.median(t))
                row[f"{kind}_min_us"] = float(np.min(t))
                row[f"{kind}_GBps"] = nbytes / (1e3 * row[f"{kind}_us"])
            row["ratio"] = row["chain_us"] / row["table_us"]
            row["ratio_from_bytes"] = 3 * (M - 1) / (M + 1)
            rows.append(row)
            print(f"n {n:6d} M {M}: chain {row['chain_us']:9.1f} us ({row['chain_GBps']:7.1f} GB/s)  table {row['table_us']:9.1f} us "
                  f"({row['table_GBps']:7.1f} GB/s)  ratio {row['ratio']:.2f} (bytes: {row['ratio_from_bytes']:.2f})", flush=True)
        del masks, out
        eng.close()
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"what": "tools/fuse_time.py: median (and min) per call, the OR chain and the table kernel alternating in one "
                               "process; GB/s on (M + 1) * n * words * 8 bytes for both", "reps": REPS,
                       "launches_per_bracket": LAUNCHES, "k": K, "fuse": rows}, f, indent=1)


if __name__ == "__main__":
    main()
