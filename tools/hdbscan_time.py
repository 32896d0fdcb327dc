"""Cost of `perform_hdbscan_clustering_on_device` (csrc/emst.hip + the host stage of mused_amd/hdbscan.py) on a device tensor at
(n, 50), n = 20,000 / 40,000 / 150,000, blobs plus 20 % uniform noise, min_cluster_size = 5, min_samples = 2: the median of
12 calls, split into the `mused_emst` bracket (events around the C call) and the host stage (host copy of the rows, weights,
Prim's order, scikit-learn's tree routines), with the rounds each shape needed and the fallbacks counted.

The host estimator (sklearn.cluster.HDBSCAN on a host copy) is timed ONCE at 20,000 and 40,000 rows only: its Prim loop is
O(n^2 d) on one thread, so 150,000 rows are an extrapolation by (n / 40,000)^2 in the record, not a measurement.

    python tools/hdbscan_time.py                    # JSON on stdout
    python tools/hdbscan_time.py --shapes 20000     # a subset of the row counts
    python tools/hdbscan_time.py --no-host          # device legs only
    python tools/hdbscan_time.py --once 150000      # ONE device call (for a kernel trace of its own)
"""
import argparse, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = (20000, 40000, 150000)
HOST_SHAPES = (20000, 40000)
D, MIN_CLUSTER_SIZE, MIN_SAMPLES, CALLS, WARM = 50, 5, 2, 12, 1


def rows(n, centres=10):
    rng = np.random.default_rng(0)
    m = n - n // 5
    cen = 4.0 * rng.standard_normal((centres, D))
    X = cen[rng.integers(0, centres, m)] + 0.4 * rng.standard_normal((m, D))
    noise = rng.uniform(X.min(axis=0), X.max(axis=0), (n - m, D))
    return np.concatenate([X, noise])[rng.permutation(n)]


def measure(shapes, host=True):
    import torch
    from mused_amd import _lib
    from mused_amd import matrix_operations as mo

    out = []
    for n in shapes:
        X = rows(n)
        Xd = torch.from_numpy(X).cuda()
        before = mo.hdbscan_fallbacks
        total, emst, stage, rounds, lab = [], [], [], None, None
        for i in range(WARM + CALLS):
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lab = mo.perform_hdbscan_clustering_on_device(Xd, MIN_CLUSTER_SIZE, MIN_SAMPLES, timings=tm)
            ms = 1e3 * (time.perf_counter() - t0)
            if i >= WARM:
                total.append(ms), emst.append(tm.get("emst_ms", float("nan"))), stage.append(tm.get("host_ms", float("nan")))
                rounds = tm.get("rounds")
        rec = dict(n=n, d=D, clusters=int(lab.max()) + 1, noise=int((lab < 0).sum()), rounds=rounds,
                   call_ms_median=float(np.median(total)), emst_ms_median=float(np.median(emst)),
                   host_stage_ms_median=float(np.median(stage)), fallbacks=mo.hdbscan_fallbacks - before,
                   mused_emst_ws_bytes=int(_lib.lib().mused_emst_ws_bytes(n)))
        if host and n in HOST_SHAPES:
            print(f"  host estimator at n = {n} ...", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            want = mo.perform_hdbscan_clustering_sklearn(Xd.cpu().numpy(), MIN_CLUSTER_SIZE, MIN_SAMPLES)
            rec.update(host_estimator_ms_once=1e3 * (time.perf_counter() - t0), same_labels=bool(np.array_equal(lab, want)))
        elif host and out and out[-1].get("host_estimator_ms_once"):
            prev = out[-1]
            rec.update(host_estimator_ms_extrapolated=prev["host_estimator_ms_once"] * (n / prev["n"]) ** 2,
                       host_estimator_note=f"NOT measured: (n / {prev['n']})^2 times the time at {prev['n']} rows")
        out.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del Xd
    return out


def once(n):
    import torch
    from mused_amd import matrix_operations as mo

    Xd = torch.from_numpy(rows(n)).cuda()
    tm = {}
    mo.perform_hdbscan_clustering_on_device(Xd, MIN_CLUSTER_SIZE, MIN_SAMPLES, timings=tm)
    torch.cuda.synchronize()
    return dict(n=n, **tm)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(str(s) for s in SHAPES))
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--once", type=int, default=0)
    a = ap.parse_args()
    if a.once:
        print(json.dumps(once(a.once)))
    else:
        res = {"min_cluster_size": MIN_CLUSTER_SIZE, "min_samples": MIN_SAMPLES, "calls": CALLS,
               "shapes": measure([int(s) for s in a.shapes.split(",")], not a.no_host)}
        print(json.dumps(res, indent=1))
