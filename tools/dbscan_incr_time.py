"""Cost of the DBSCAN_incr chain (mused_amd.incdbscan.IncrementalDBSCAN, csrc/dbscan_incr.hip) on a stream of n = 150,000 rows,
d = 50, W = 2,000 (75 inserts): blobs plus 20 % uniform noise, permuted, as in tools/hdbscan_time.py; eps = 4.0 (about half
of the pairs of one blob lie within it), min_samples 2 and 5.

Per window: the insert's time (HIP events around the call, the median over `--repeats` passes of the whole stream behind one
warm-up pass of 3 windows), the dirty row counts, and the time of ONE `mused_dbscan` refit of the same prefix (the median of
`--refits` calls behind one warm call) -- the only way to those labels without the incremental kernels, the baseline.
Totals of both, whether the labels of the last window's refit equal the chain's, the fallbacks, and the peak device memory
of a pass beyond the rows themselves.

    python tools/dbscan_incr_time.py                       # JSON on stdout, progress on stderr
    python tools/dbscan_incr_time.py --min-samples 5
    python tools/dbscan_incr_time.py --rows 40000          # a shorter stream
    python tools/dbscan_incr_time.py --no-refit --repeats 1   # ONE pass of the chain alone (for a kernel trace of its own)
    python tools/dbscan_incr_time.py --match --rows 40000  # the label matching of every window (what the pipeline records as
                                                           # host_ms["match"]): the wide chain (csrc/match_wide.hip) against the
                                                           # former host route (MUSED_MATCH_WIDE=host), same raw labels
"""
import argparse, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, W, EPS = 50, 2000, 4.0


def rows(n, centres=10):
    rng = np.random.default_rng(0)
    m = n - n // 5
    cen = 4.0 * rng.standard_normal((centres, D))
    X = cen[rng.integers(0, centres, m)] + 0.4 * rng.standard_normal((m, D))
    noise = rng.uniform(X.min(axis=0), X.max(axis=0), (n - m, D))
    return np.concatenate([X, noise])[rng.permutation(n)]


def one_pass(Xd, n, ms, timed=True):
    """One pass of the stream -> (per-window insert ms, per-window dirty counts, the object, peak bytes beyond the rows)."""
    import torch
    from mused_amd.incdbscan import IncrementalDBSCAN

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    c = IncrementalDBSCAN(EPS, ms)
    t_ms = []
    for lo in range(0, n - W + 1, W):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        c.insert(Xd[lo:lo + W])
        e1.record()
        e1.synchronize()
        t_ms.append(e0.elapsed_time(e1))
    cap_rows = 0 if c._X is None else c._X.numel() * 8
    return t_ms, list(c.dirty), c, torch.cuda.max_memory_allocated() - base - cap_rows


def measure(n, ms, repeats, refits):
    import torch
    from mused_amd import matrix_operations as mo

    Xd = torch.from_numpy(rows(n)).cuda()
    before = mo.dbscan_incr_fallbacks
    one_pass(Xd, 3 * W, ms)   # warm-up: every kernel of the chain has run once
    passes, dirty, chain, peak = [], None, None, 0
    for _ in range(repeats):
        t_ms, dirty, chain, peak = one_pass(Xd, n, ms)
        passes.append(t_ms)
        print(f"  pass: {sum(t_ms):.1f} ms", file=sys.stderr, flush=True)
    insert_ms = np.median(np.array(passes), axis=0)
    labels = chain.labels()
    windows = []
    for k, lo in enumerate(range(0, n - W + 1, W)):
        rec = dict(rows=lo + W, insert_ms=float(insert_ms[k]))
        if k < len(dirty):
            rec.update(turned_core=dirty[k][0], root_moved=dirty[k][1])
        windows.append(rec)
    out = dict(n=n, d=D, W=W, eps=EPS, min_samples=ms, repeats=repeats, windows=windows, insert_ms_total=float(insert_ms.sum()),
               clusters=int(labels.max()) + 1, noise=int((labels < 0).sum()), fallbacks=mo.dbscan_incr_fallbacks - before,
               peak_bytes_beyond_rows=int(peak))
    del chain
    if refits:
        total, lab = 0.0, None
        for rec in windows:
            p = rec["rows"]
            ts = []
            for i in range(1 + refits):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                lab, info = mo.dbscan_launch(Xd[:p], EPS, ms)
                e1.record()
                e1.synchronize()
                if i:
                    ts.append(e0.elapsed_time(e1))
            rec["refit_ms"] = float(np.median(ts))
            total += rec["refit_ms"]
        out.update(refit_ms_total=total, refit_flags=int(info[0]),
                   same_labels_as_last_refit=bool(np.array_equal(lab.cpu().numpy(), labels)))
    return out


def measure_match(n, ms):
    """The pipeline's matching step (StreamPipeline._chain: match_clusters_on_device(prev, labels, 3, "hungarian",
    wide="only")) on the raw labels of every window of one pass, by both routes: wall ms per window as host_ms["match"]."""
    import time

    import torch
    from mused_amd import hungarian as hg
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    Xd = torch.from_numpy(rows(n)).cuda()
    c, raws = IncrementalDBSCAN(EPS, ms), []
    for lo in range(0, n - W + 1, W):
        c.insert(Xd[lo:lo + W])
        raws.append(c.labels()[-W:])
    out = dict(n=n, W=W, eps=EPS, min_samples=ms, windows=len(raws), labels_a_side=[int(len(np.unique(r))) for r in raws])
    chains = {}
    for route in ("host", "device"):
        os.environ["MUSED_MATCH_WIDE"] = route
        for timed in (False, True):   # one warm pass
            prev, t_ms, chain = None, [], []
            before = mo.match_fallbacks
            for r in raws:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                prev = mo.match_clusters_on_device(prev, r, 3, method="hungarian", wide="only")
                t_ms.append(1e3 * (time.perf_counter() - t0))
                chain.extend(np.asarray(prev).tolist())
        chains[route] = chain
        out[route] = dict(match_ms=t_ms, match_ms_total=float(sum(t_ms)), match_ms_median=float(np.median(t_ms[1:])),
                          fallbacks=mo.match_fallbacks - before)
    os.environ.pop("MUSED_MATCH_WIDE")
    prev, spec = None, []
    for r in raws:
        prev = hg.match_labels(prev, r, 3)[0]
        spec.extend(np.asarray(prev).tolist())
    out["same_labels"] = chains["host"] == chains["device"] == spec
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=150000)
    ap.add_argument("--min-samples", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--refits", type=int, default=3)
    ap.add_argument("--no-refit", action="store_true")
    ap.add_argument("--match", action="store_true")
    a = ap.parse_args()
    if a.match:
        print(json.dumps(measure_match(a.rows, a.min_samples), indent=1))
        sys.exit(0)
    print(json.dumps(measure(a.rows, a.min_samples, a.repeats, 0 if a.no_refit else a.refits), indent=1))
