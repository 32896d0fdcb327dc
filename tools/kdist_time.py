"""Cost of `matrix_operations.select_eps_on_device` (csrc/kdist.hip: the k-th neighbour distances of every row, the sort of
the curve and its knee) on a device tensor at (n, d, k) = (2000, 50, 2), (10000, 128, 5), (20000, 50, 2), (150000, 50, 2),
(10000, 50, 64): the median of 12 calls (wall clock around the call, which ends in the read of its 64 result bytes), against
scikit-learn's `NearestNeighbors(n_neighbors=k, n_jobs=16).kneighbors(X)` on the same rows on the host (median of 3; one call
beyond 20,000 rows).  For k <= 8 the shape is also timed with MUSED_KDIST_WIDE=1, i.e. on the 64-long lists, which is what the
split of the tile kernel into two instances is judged by.  Every step is a child process of its own under a time limit;
after a step that fails or runs out of time no further step is started.

    python tools/kdist_time.py                   # JSON on stdout
    python tools/kdist_time.py --trace DIR       # per shape, one run under `rocprofv3 --kernel-trace --stats` writing into
                                                 # DIR: the share of the tile kernel, the merge, the sort and the rest
"""
import csv, glob, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((2000, 50, 2), (10000, 128, 5), (20000, 50, 2), (150000, 50, 2), (10000, 50, 64))
HOST_REPEAT_MAX_ROWS = 20000
CALLS, HOST_CALLS, WARM, HOST_THREADS = 12, 3, 2, 16
STEP_LIMIT_S = 240


def rows(n, d):
    """Blobs plus uniform noise, the kind of input the rule is for: 8 centres in [-10, 10]^d, 10 % noise."""
    rng = np.random.default_rng(0)
    mu = rng.uniform(-10, 10, size=(8, d))
    X = mu[rng.integers(0, 8, n)] + 0.5 * rng.normal(size=(n, d))
    m = n // 10
    X[:m] = rng.uniform(-10, 10, size=(m, d))
    return X[rng.permutation(n)]


def timed(fn):
    import torch

    ms, got = [], None
    for c in range(WARM + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        if c >= WARM:
            ms.append(1e3 * (time.perf_counter() - t0))
    return ms, got


def device_step(i, wide):
    import torch
    from mused_amd import matrix_operations as mo

    if wide:
        os.environ["MUSED_KDIST_WIDE"] = "1"
    n, d, k = SHAPES[i]
    Xd = torch.from_numpy(rows(n, d)).cuda()
    ms, (eps, info) = timed(lambda: mo.select_eps_on_device(Xd, k))
    st = torch.cuda.current_stream()
    kth, _ = timed(lambda: mo.kth_distance_launch(Xd, k, st))       # the pair pass alone, no read
    return dict(n=n, d=d, k=k, lists=64 if (wide or k > 8) else 8, device_ms_median=float(np.median(ms)),
                device_ms_min=float(np.min(ms)), kth_distance_only_ms_median=float(np.median(kth)), eps=eps,
                knee=info["knee"])


def host_step(i):
    from sklearn.neighbors import NearestNeighbors

    n, d, k = SHAPES[i]
    X = rows(n, d)
    hs = []
    for c in range(HOST_CALLS if n <= HOST_REPEAT_MAX_ROWS else 1):
        t0 = time.perf_counter()
        NearestNeighbors(n_neighbors=k, n_jobs=HOST_THREADS).fit(X).kneighbors(X)
        hs.append(1e3 * (time.perf_counter() - t0))
    return dict(host_ms_median=float(np.median(hs)), host_calls=len(hs), host_threads=HOST_THREADS)


def trace_step(i):
    import torch
    from mused_amd import matrix_operations as mo

    n, d, k = SHAPES[i]
    Xd = torch.from_numpy(rows(n, d)).cuda()
    for _ in range(4):
        mo.select_eps_on_device(Xd, k)
    torch.cuda.synchronize()
    return dict(n=n, d=d, k=k, calls=4)


GROUPS = (("tile", ("kd_tile_kernel",)), ("merge", ("kd_merge_kernel",)),
          ("sort", ("radix_hist_kernel", "radix_scatter_kernel", "blockscan_kernel")),
          ("knee", ("knee_root_kernel", "knee_gather_kernel", "knee_rule_kernel")))


def trace_shares(directory):
    """Summed kernel time by group from the kernel-stats table of one traced run (ns), and each group's share."""
    tot = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name, ns = row["Name"], float(row["TotalDurationNs"])
                group = next((g for g, keys in GROUPS if any(key in name for key in keys)), "other")
                tot[group] = tot.get(group, 0.0) + ns
    whole = sum(tot.values())
    return {g: dict(ns=v, share=v / whole) for g, v in sorted(tot.items())} if whole else None


def child(step, prefix=()):
    """One step in a fresh process under its own time limit: its JSON record, or None (and the reason on stderr)."""
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", step]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(f"step {step}: no result within {STEP_LIMIT_S} s", file=sys.stderr)
        return None
    if r.returncode != 0:
        print(f"step {step}: exit status {r.returncode}", file=sys.stderr)
        return None
    print(f"step {step}: done", file=sys.stderr, flush=True)
    lines = [ln for ln in r.stdout.decode().strip().splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def main():
    if "--step" in sys.argv:
        kind, i = sys.argv[sys.argv.index("--step") + 1].split(":")
        rec = {"device": lambda: device_step(int(i), False), "wide": lambda: device_step(int(i), True),
               "host": lambda: host_step(int(i)), "trace": lambda: trace_step(int(i))}[kind]()
        print(json.dumps(rec))
        return 0
    if "--trace" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--trace") + 1])
        res = []
        for i in range(len(SHAPES)):
            d = os.path.join(out, f"shape{i}")
            os.makedirs(d, exist_ok=True)
            rec = child(f"trace:{i}", ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kd", "--"))
            if rec is None:
                break
            rec["kernel_time"] = trace_shares(d)
            res.append(rec)
        print(json.dumps({"traced": res}, indent=1))
        return 0 if len(res) == len(SHAPES) else 1
    res = {"calls_timed": CALLS, "shapes": []}
    for i, (n, d, k) in enumerate(SHAPES):
        rec = child(f"device:{i}")
        if rec is None:
            break
        if k <= 8:
            wide = child(f"wide:{i}")
            if wide is None:
                break
            rec["with_64_long_lists"] = {key: wide[key] for key in ("device_ms_median", "device_ms_min",
                                                                    "kth_distance_only_ms_median", "eps")}
        host = child(f"host:{i}")
        if host is None:
            break
        rec.update(host, speedup=host["host_ms_median"] / rec["device_ms_median"])
        res["shapes"].append(rec)
    print(json.dumps(res, indent=1))
    return 0 if len(res["shapes"]) == len(SHAPES) else 1


if __name__ == "__main__":
    sys.exit(main())
