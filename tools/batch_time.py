#!/usr/bin/env python3
"""Per-phase wall time and peak device memory of the reference's batch approach "SVDMC_batch" (process_batch_data,
main.py:132-167) on the device: kNN adjacency per modality, fusion, eigenstep, k-means.

Synthetic SED2012-style columns (mused_amd.synth.metadata_stream + text_stream: location, time, username, tags, text) at
the reference's default subset of 150,000 rows, l = k = 50.  Phases are timed with a device synchronisation at their
ends; "peak_bytes" is the most device memory in use (beyond what was in use before the call) at the end of any phase.

    python tools/batch_time.py [--n 150000] [--types location,time,username,tags,text] [--clusters 4] [--repeat 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=150000)
    ap.add_argument("--types", default="location,time,username,tags,text")
    ap.add_argument("--ell", type=int, default=50)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--clusters", type=int, default=4)
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()

    import torch

    from mused_amd import synth
    from mused_amd.pipeline import process_batch_data

    t = time.perf_counter()
    cols, labels = synth.metadata_stream(a.n, a.seed, users=a.users)
    types_ = a.types.split(",")
    mods = [synth.text_stream(a.n, a.seed)[0] if ty == "text" else cols[ty] for ty in types_]
    gen_s = time.perf_counter() - t
    torch.cuda.init()
    for rep in range(a.repeat):
        timings = {}
        res = process_batch_data({}, mods, types_, a.ell, a.k, a.clusters, a.seed, "SVDMC_batch", labels, 0.0, "all",
                                 False, 1.5, 2, 3, 2000, timings=timings)
        out = {"n": a.n, "types": types_, "ell": a.ell, "k": a.k, "clusters": a.clusters, "repeat": rep,
               "total_s": round(res["processing_time"], 3), "input_generation_s": round(gen_s, 3),
               "peak_GB": round(timings.pop("peak_bytes") / 1e9, 2), "nxn_fp64_GB": round(a.n * a.n * 8 / 1e9, 1),
               "edges": timings.pop("edges"),
               "phases_s": {key: round(v, 3) for key, v in timings.items()}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
