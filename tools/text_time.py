#!/usr/bin/env python3
"""Time of the "text" adjacency (adjacency_on_device(x, "text", k)) per window on the device path -- TF-IDF of a window
of a corpus tokenised once, csrc/tfidf.hip -- and under MUSED_TEXT=host, the per-window TfidfVectorizer call (the former
path as a whole: the yardstick).  Both in one process, alternating window by window; every call ends in a device
synchronisation.  The one-off tokenisation of the corpus is reported separately ("tokenise_s").

--tokenise: the two tokenisers (text.tokenise on the host, text.tokenise_on_device: host preparation, both calls of
csrc/tokenise.hip, the host's sort of the vocabulary) on the same rows in one process, alternating, each call ended by a
device synchronisation; median of --tok-repeat (>= 5) after one warm-up each.  Shapes: --tok-rows rows of text_stream
and of sparse_text_stream, the --batch rows of text_stream, one window of --tok-window rows of each.  The corpora are
compared field for field once per shape.  No window is timed in this mode (kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/text_time.py --tokenise ...`).  --non-ascii SHARE: the share SHARE
of the streams' letters is swapped for letters that are not ASCII (synth.swap_letters, seeded: both cases of several
scripts, U+0130 and U+03A3 among them) and the device side is text.tokenise_codepoints_on_device.

Stream shapes: 12 hopping windows (step W / 4) of synth.text_stream / synth.sparse_text_stream, median of the 12; the
sparse stream also with text_sparse=True.  Batch shape: the whole text_stream subset as one window (best of --repeat).

    python tools/text_time.py [--shapes 2000,10000] [--k 50] [--batch 150000] [--repeat 2] [--out FILE]
    python tools/text_time.py --tokenise [--tok-rows 37500] [--tok-window 2000] [--batch 150000] [--tok-repeat 7]
                                         [--non-ascii 0.3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def one(mode, x, k, eng, sparse):
    from mused_amd import matrix_operations as mo

    os.environ["MUSED_TEXT"] = mode
    return timed(lambda: mo.adjacency_on_device(x, "text", k, engine=eng, text_sparse=sparse).mask)


def tokenise_times(a, emit):
    import numpy as np

    from mused_amd import synth, text

    shapes = [("text_stream", a.tok_rows), ("sparse_text_stream", a.tok_rows), ("text_stream", a.tok_window),
              ("sparse_text_stream", a.tok_window)] + ([("text_stream", a.batch)] if a.batch > 0 else [])
    for stream, n in shapes:
        rec = getattr(synth, stream)(n, 0)[0]
        on_device = text.tokenise_on_device
        if a.non_ascii > 0:
            rec = synth.swap_letters(rec, a.non_ascii, 0)
            on_device = text.tokenise_codepoints_on_device
        fallbacks = text.tokenise_fallbacks
        s = {"device": [], "host": []}
        same = None
        for r in range(a.tok_repeat + 1):   # round 0 warms both up (code objects, the allocator's blocks)
            dev, td = timed(lambda: on_device(rec))
            host, th = timed(lambda: text.tokenise(rec))
            if r == 0:
                same = (dev.vocabulary == host.vocabulary and
                        all(np.array_equal(getattr(dev, f), getattr(host, f)) for f in text._DEVICE_FIELDS))
            else:
                s["device"].append(td)
                s["host"].append(th)
            del dev, host
        joined = (text.corpus_codepoints if a.non_ascii > 0 else text.corpus_buffer)(*text._valid_rows(rec))
        emit({"tokenise": stream, "rows": n, "non_ascii": a.non_ascii, "bytes": int(joined[1][-1]) * joined[0].itemsize,
              "repeat": a.tok_repeat, "device_s_median": round(statistics.median(s["device"]), 4),
              "host_s_median": round(statistics.median(s["host"]), 4),
              "device_s": [round(x, 4) for x in s["device"]], "host_s": [round(x, 4) for x in s["host"]],
              "fallbacks": text.tokenise_fallbacks - fallbacks, "corpora_equal": same})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000,10000")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--batch", type=int, default=150000)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--tokenise", action="store_true")
    ap.add_argument("--tok-rows", type=int, default=37500)
    ap.add_argument("--tok-window", type=int, default=2000)
    ap.add_argument("--tok-repeat", type=int, default=7)
    ap.add_argument("--non-ascii", type=float, default=0.0)
    a = ap.parse_args()

    import torch

    from mused_amd import synth, text
    from mused_amd.engine import WindowEngine

    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(json.dumps(r) for r in lines) + "\n")

    torch.cuda.init()
    if a.tokenise:
        if a.tok_repeat < 5:
            ap.error("--tok-repeat: at least 5")
        return tokenise_times(a, emit)
    for W in (int(x) for x in a.shapes.split(",") if x):
        step = W // 4
        N = W + step * (a.windows - 1)
        eng = WindowEngine(W)
        for stream, gen in (("text_stream", synth.text_stream), ("sparse_text_stream", synth.sparse_text_stream)):
            rec = gen(N, 0)[0]
            corpus, tok_s = timed(lambda: text.tokenise(rec))
            for sparse in ((None,) if stream == "text_stream" else (None, True)):
                ms = {"device": [], "host": []}
                same = True
                for rounds in range(2):   # round 0 warms both paths up (code objects, workspaces, the corpus upload)
                    for w in range(a.windows if rounds else 1):
                        lo = w * step
                        got, td = one("device", corpus.window(lo, lo + W), a.k, eng, sparse)
                        want, th = one("host", rec[lo:lo + W], a.k, eng, sparse)
                        same = same and bool(torch.equal(got, want))
                        if rounds:
                            ms["device"].append(1e3 * td)
                            ms["host"].append(1e3 * th)
                emit({"stream": stream, "W": W, "k": a.k, "text_sparse": sparse, "windows": a.windows, "rows": N,
                      "vocabulary": corpus.V, "tokenise_s": round(tok_s, 3),
                      "device_ms_median": round(statistics.median(ms["device"]), 2),
                      "host_ms_median": round(statistics.median(ms["host"]), 2),
                      "device_ms_min": round(min(ms["device"]), 2), "host_ms_min": round(min(ms["host"]), 2),
                      "masks_equal": same})
        eng.close()
    if a.batch > 0:
        n = a.batch
        rec = synth.text_stream(n, 0)[0]
        eng = WindowEngine(n)
        corpus, tok_s = timed(lambda: text.tokenise(rec))
        dev_s, host_s, same = [], [], True
        for _ in range(a.repeat):
            got, td = one("device", corpus.window(), a.k, eng, None)
            want, th = one("host", rec, a.k, eng, None)
            same = same and bool(torch.equal(got, want))
            dev_s.append(td)
            host_s.append(th)
        emit({"stream": "text_stream", "batch_rows": n, "k": a.k, "vocabulary": corpus.V, "tokenise_s": round(tok_s, 3),
              "device_s": [round(x, 3) for x in dev_s], "host_s": [round(x, 3) for x in host_s], "masks_equal": same})
        eng.close()


if __name__ == "__main__":
    main()
