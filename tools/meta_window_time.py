"""Time per window of the metadata modalities ("location", "time", "username", "tags"): MUSED_META=host -- the rows of
every window handled on the host, as StreamPipeline hands them over (numeric columns as slices of a device tensor,
strings as they are) -- against MUSED_META=device -- a window of a stream that was encoded once, one launch on its
resident arrays (mused_amd/meta.py, csrc/meta_window.hip).

One process, the two modes alternating window by window (which one goes first alternates too); per leg the median over
`--windows` windows after `--warmup`, for every type and for the four together.  Every time is a host clock around the
calls and a device synchronisation.  Legs: W = 2,000 and 10,000 at k = 50, a share of 0.05 and 0.6 of rows without a
value, and one leg with step_window_ratio 4.  The legs with --peak-w rows per window and the larger share also report the
peak device memory of two windows in either mode (torch.cuda.max_memory_allocated above what was allocated before).
The encoding pass itself (once per stream) is reported per leg as encode_ms, and masks_equal says whether the two paths
gave the same masks in the last window.

    python tools/meta_window_time.py [--windows 12] [--warmup 2] [--legs 2000:0.05:1,...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mused_amd import matrix_operations as mo
from mused_amd import meta, synth
from mused_amd.engine import WindowEngine

TYPES = ("location", "time", "username", "tags")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def leg(W, missing, ratio, k, windows, warmup, seed, peak):
    step = W // ratio
    n = W + (windows + warmup - 1) * step
    cols, _ = synth.metadata_stream(n, seed, events=8, users=400, vocab=300, missing=missing)
    cols["tags"][np.random.default_rng(seed).random(n) < missing, 0] = ""   # photos without a tag field: invalid rows
    eng = WindowEngine(W)
    t0 = time.perf_counter()
    corpora = {t: meta.encode(cols[t], t) for t in TYPES}
    for c in corpora.values():
        c.device_arrays(eng.device)
    encode_ms = 1e3 * (time.perf_counter() - t0)
    # what StreamPipeline.run keeps under MUSED_META=host: numeric columns on the device, string records on the host
    held = {t: torch.from_numpy(np.ascontiguousarray(cols[t])).cuda() if t in ("location", "time") else cols[t] for t in TYPES}

    def run(mode, types, lo):
        os.environ["MUSED_META"] = mode
        for t in types:
            src = held[t][lo:lo + W] if mode == "host" else corpora[t].window(lo, lo + W)
            mo.adjacency_on_device(src, t, k, engine=eng)

    ms = {(mode, what): [] for mode in ("host", "device") for what in TYPES + ("all",)}
    for i in range(windows + warmup):
        lo = i * step
        for what in TYPES + ("all",):
            for mode in (("host", "device") if i % 2 == 0 else ("device", "host")):
                dt = timed(lambda: run(mode, TYPES if what == "all" else (what,), lo))
                if i >= warmup:
                    ms[(mode, what)].append(dt)
    out = dict(W=W, k=k, missing=missing, ratio=ratio, windows=windows, rows=n, encode_ms=round(encode_ms, 1))
    # outside the timing: the two paths give the same mask (last window; raw rows take the host path in either mode)
    os.environ["MUSED_META"] = "device"
    out["masks_equal"] = all(torch.equal(mo.adjacency_on_device(held[t][lo:lo + W], t, k, engine=eng).mask,
                                         mo.adjacency_on_device(corpora[t].window(lo, lo + W), t, k, engine=eng).mask)
                             for t in TYPES)
    for what in TYPES + ("all",):
        out[what] = {mode: round(float(np.median(ms[(mode, what)])), 3) for mode in ("host", "device")}
    if peak:
        for mode in ("host", "device"):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            for lo in (0, step):
                run(mode, TYPES, lo)
            torch.cuda.synchronize()
            out[f"peak_mb_{mode}"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--legs", default="2000:0.05:1,2000:0.6:1,10000:0.05:1,10000:0.6:1,10000:0.6:4",
                    help="comma-separated W:missing:step_window_ratio")
    ap.add_argument("--peak-w", type=int, default=10000, help="legs of this W and missing >= 0.5 also report peak memory")
    a = ap.parse_args()
    before = os.environ.get("MUSED_META")
    rows = []
    for spec in a.legs.split(","):
        W, missing, ratio = spec.split(":")
        W, missing, ratio = int(W), float(missing), int(ratio)
        r = leg(W, missing, ratio, a.k, a.windows, a.warmup, a.seed, peak=(W == a.peak_w and missing >= 0.5 and ratio == 1))
        rows.append(r)
        print(json.dumps(r), flush=True)
    if before is None:
        os.environ.pop("MUSED_META", None)
    else:
        os.environ["MUSED_META"] = before
    print("\n| W | missing | ratio | " + " | ".join(f"{t} host / device (ms)" for t in TYPES + ("all four",)) + " |")
    print("|---|---|---|" + "---|" * (len(TYPES) + 1))
    for r in rows:
        print(f"| {r['W']} | {r['missing']} | {r['ratio']} | "
              + " | ".join(f"{r[t]['host']:.2f} / {r[t]['device']:.2f}" for t in TYPES + ("all",)) + " |")


if __name__ == "__main__":
    main()
