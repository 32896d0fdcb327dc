"""Cost of DBSCAN_incr over a sliding window (IncrementalDBSCAN(max_rows=...): mused_dbscan_incr_delete + mused_dbscan_incr_insert,
csrc/dbscan_incr.hip) on the stream of tools/dbscan_incr_time.py: n = 150,000 rows, d = 50, W = 2,000 (75 windows), blobs plus
20 % uniform noise, eps = 4.0, at most 20,000 rows held.  From the 11th window on every insert first deletes the 2,000 oldest
rows: a SLIDE.

Two row orders:
    permuted   the rows of tools/dbscan_incr_time.py: every cluster has rows in every window, so every delete touches every
               cluster and rebuilds it (the worst case)
    by_cluster the same rows in arrival order by cluster (a noise row arrives with a cluster drawn at random): time-local events

Per slide: the time of `insert` (the delete and the insert; HIP events around the call, the median over `--repeats` passes of
the whole stream behind one warm-up pass of 13 windows), the rows that lost core status, |R| and |B| of the delete.  Against
it: ONE `mused_dbscan` refit of the same last 20,000 rows (the median of `--refits` calls behind one warm call at every
`--refit-every`-th slide) -- the only way to those labels without the delete kernels.  Whether the labels at the end equal
that refit's, and the fallbacks.

    python tools/dbscan_window_time.py                       # JSON on stdout, progress on stderr
    python tools/dbscan_window_time.py --min-samples 5 --order by_cluster
"""
import argparse, json, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, W, EPS, MAX_ROWS = 50, 2000, 4.0, 20000


def rows(n, order, centres=10):
    """The rows of tools/dbscan_incr_time.py (the same draws), permuted as there or ordered by cluster."""
    rng = np.random.default_rng(0)
    m = n - n // 5
    cen = 4.0 * rng.standard_normal((centres, D))
    ids = rng.integers(0, centres, m)
    X = cen[ids] + 0.4 * rng.standard_normal((m, D))
    noise = rng.uniform(X.min(axis=0), X.max(axis=0), (n - m, D))
    X = np.concatenate([X, noise])
    perm = rng.permutation(n)
    if order == "permuted":
        return X[perm]
    ids = np.concatenate([ids, np.random.default_rng(1).integers(0, centres, n - m)])
    X, ids = X[perm], ids[perm]
    return X[np.argsort(ids, kind="stable")]


def one_pass(Xd, n, ms, max_rows):
    import torch
    from mused_amd.incdbscan import IncrementalDBSCAN

    c = IncrementalDBSCAN(EPS, ms, max_rows=max_rows)
    t_ms, infos = [], []
    for lo in range(0, n - W + 1, W):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c.last_delete_info = None
        e0.record()
        c.insert(Xd[lo:lo + W])
        e1.record()
        e1.synchronize()
        t_ms.append(e0.elapsed_time(e1))
        infos.append(None if c.last_delete_info is None else [int(v) for v in c.last_delete_info])
    return t_ms, infos, c


def measure(n, ms, order, repeats, refits, refit_every, max_rows):
    import torch
    from mused_amd import matrix_operations as mo

    Xd = torch.from_numpy(rows(n, order)).cuda()
    before = mo.dbscan_incr_fallbacks
    one_pass(Xd, min(n, max_rows + 3 * W), ms, max_rows)   # warm-up: every kernel of a slide has run
    passes, infos, chain = [], None, None
    for _ in range(repeats):
        t_ms, infos, chain = one_pass(Xd, n, ms, max_rows)
        passes.append(t_ms)
        print(f"  pass: {sum(t_ms):.1f} ms", file=sys.stderr, flush=True)
    passes = np.array(passes)
    med = np.median(passes, axis=0)
    labels = chain.labels()
    windows = []
    for k, lo in enumerate(range(0, n - W + 1, W)):
        rec = dict(rows_seen=lo + W, held=min(lo + W, max_rows), slide_ms=float(med[k]),
                   slide_ms_passes=[float(v) for v in passes[:, k]])
        if infos[k] is not None:
            rec.update(lost_core=infos[k][3], R=infos[k][4], B=infos[k][5], core=infos[k][2], clusters=infos[k][1])
        windows.append(rec)
    slides = [w for w in windows if "R" in w]
    out = dict(n=n, d=D, W=W, eps=EPS, min_samples=ms, order=order, max_rows=max_rows, repeats=repeats, windows=windows,
               slides=len(slides), slide_ms_median=float(np.median([w["slide_ms"] for w in slides])) if slides else None,
               slide_ms_min=min(w["slide_ms"] for w in slides) if slides else None,
               slide_ms_max=max(w["slide_ms"] for w in slides) if slides else None,
               R_median=float(np.median([w["R"] for w in slides])) if slides else None,
               fallbacks=mo.dbscan_incr_fallbacks - before, host_mode=bool(chain._host_mode),
               row_buffer_rows=0 if chain._X is None else int(chain._X.shape[0]))
    del chain
    if refits and slides:
        lab, info, all_ts = None, None, []
        for k, rec in enumerate(windows):
            if "R" not in rec or (k % refit_every and k != len(windows) - 1):
                continue
            hi = rec["rows_seen"]
            ts = []
            for i in range(1 + refits):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                lab, info = mo.dbscan_launch(Xd[hi - rec["held"]:hi], EPS, ms)
                e1.record()
                e1.synchronize()
                if i:
                    ts.append(e0.elapsed_time(e1))
            rec["refit_ms"], rec["refit_ms_calls"] = float(np.median(ts)), [float(t) for t in ts]
            all_ts.append(rec["refit_ms"])
        out.update(refit_ms_median=float(np.median(all_ts)), refit_flags=int(info[0]),
                   same_labels_as_last_refit=bool(np.array_equal(lab.cpu().numpy(), labels)))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=150000)
    ap.add_argument("--min-samples", type=int, default=2)
    ap.add_argument("--order", choices=["permuted", "by_cluster"], default="permuted")
    ap.add_argument("--max-rows", type=int, default=MAX_ROWS)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--refits", type=int, default=3)
    ap.add_argument("--refit-every", type=int, default=8)
    ap.add_argument("--brief", action="store_true", help="leave the per-window records out of the JSON")
    a = ap.parse_args()
    res = measure(a.rows, a.min_samples, a.order, a.repeats, a.refits, a.refit_every, a.max_rows)
    if a.brief:
        res["windows"] = [w for w in res["windows"] if "refit_ms" in w]
    print(json.dumps(res, indent=1))
