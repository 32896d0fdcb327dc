"""Cost of `metrics_evaluation.compute_internal_metrics` (csrc/silhouette.hip: silhouette, Davies-Bouldin, Calinski-Harabasz)
on a device tensor at (n, d, clusters) = (2000, 50, 4), (10000, 128, 8), (20000, 50, 150), (150000, 50, 4): the median of 12
calls, against scikit-learn's three calls on the same rows on the host with 16 threads (median of 3; n <= 20,000 only -- the
150,000-row host run takes minutes), and one `matrix_operations.select_n_clusters_on_device` call at (10000, 128) with the
candidates 2 .. 8.  Every step is a child process of its own under a time limit; after a step that fails or runs out of
time no further step is started.

    python tools/silhouette_time.py              # JSON on stdout
"""
import json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((2000, 50, 4), (10000, 128, 8), (20000, 50, 150), (150000, 50, 4))
HOST_MAX_ROWS = 20000
CALLS, HOST_CALLS, WARM, HOST_THREADS = 12, 3, 2, 16
STEP_LIMIT_S = 240


def rows(n, d, k):
    rng = np.random.default_rng(0)
    mu = rng.normal(scale=3.0, size=(k, d))
    lab = rng.integers(0, k, n)
    return mu[lab] + rng.normal(size=(n, d)), lab.astype(np.int32)


def shape_step(i):
    import torch
    from mused_amd import metrics_evaluation as me

    n, d, k = SHAPES[i]
    X, lab = rows(n, d, k)
    Xd, ld = torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda()
    ms, got = [], None
    for c in range(WARM + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = me.compute_internal_metrics(Xd, ld)
        if c >= WARM:
            ms.append(1e3 * (time.perf_counter() - t0))
    sil = []
    for c in range(WARM + CALLS):   # the silhouette alone (the O(n^2 d) part)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        me.internal_metrics_raw(Xd, ld, indices=False)
        if c >= WARM:
            sil.append(1e3 * (time.perf_counter() - t0))
    rec = dict(n=n, d=d, clusters=k, device_ms_median=float(np.median(ms)), device_ms_min=float(np.min(ms)),
               silhouette_only_ms_median=float(np.median(sil)), device=got)
    if n <= HOST_MAX_ROWS:
        from sklearn import metrics as skm
        from threadpoolctl import threadpool_limits

        hs, ref = [], None
        with threadpool_limits(limits=HOST_THREADS):
            for c in range(HOST_CALLS):
                t0 = time.perf_counter()
                ref = {"silhouette": float(skm.silhouette_score(X, lab)), "davies_bouldin": float(skm.davies_bouldin_score(X, lab)),
                       "calinski_harabasz": float(skm.calinski_harabasz_score(X, lab))}
                hs.append(1e3 * (time.perf_counter() - t0))
        rec.update(host_ms_median=float(np.median(hs)), host_threads=HOST_THREADS, host=ref,
                   speedup=float(np.median(hs) / np.median(ms)),
                   largest_difference=max(abs(got[key] - ref[key]) / max(1.0, abs(ref[key])) for key in ref))
    return rec


def selector_step():
    import torch
    from mused_amd import matrix_operations as mo

    n, d, k = 10000, 128, 8
    Xd = torch.from_numpy(rows(n, d, k)[0]).cuda()
    mo.select_n_clusters_on_device(Xd, range(2, 9), 0)   # warm: workspaces, the kernels' first launch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    best, _, scores = mo.select_n_clusters_on_device(Xd, range(2, 9), 0)
    return dict(n=n, d=d, candidates=[2, 8], ms=1e3 * (time.perf_counter() - t0), best_k=best,
                scores={str(q): s for q, s in scores.items()}, km_fallbacks=mo.km_fallbacks)


def child(step):
    """One step in a fresh process under its own time limit: its JSON record, or None (and the reason on stderr)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f"step {step}: no result within {STEP_LIMIT_S} s", file=sys.stderr)
        return None
    if r.returncode != 0:
        print(f"step {step}: exit status {r.returncode}", file=sys.stderr)
        return None
    print(f"step {step}: done", file=sys.stderr, flush=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


if __name__ == "__main__":
    if "--step" in sys.argv:
        step = sys.argv[sys.argv.index("--step") + 1]
        print(json.dumps(selector_step() if step == "selector" else shape_step(int(step))))
    else:
        res = {"calls_timed": CALLS, "host_calls_timed": HOST_CALLS, "shapes": [], "selector": None}
        for i in range(len(SHAPES)):
            rec = child(str(i))
            if rec is None:
                break
            res["shapes"].append(rec)
        else:
            res["selector"] = child("selector")
        print(json.dumps(res, indent=1))
