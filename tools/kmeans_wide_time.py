"""Per-call cost of `perform_clustering_on_device` where k * d > 8192 -- mused_kmeans_lloyd_wide (csrc/kmeans.hip) behind the
device seeding -- against MUSED_KMEANS_WIDE=host (what ran before the wide entry existed: a host copy of the embedding and
scikit-learn's KMeans) on blob rows at (n, d, k) = (2000, 100, 150), (2000, 60, 140), (10000, 256, 40), (150000, 100, 150):
the median of 12 calls of each leg after one warm-up, the two legs alternating call by call in one process on the same
device tensor, labels compared on every call, Lloyd iterations and workspace bytes reported.

    python tools/kmeans_wide_time.py              # JSON on stdout
    python tools/kmeans_wide_time.py --kernels    # + per shape, one line per kernel from a child that makes ONE device call
                                                  #   under rocprofv3 --kernel-trace --stats
    python tools/kmeans_wide_time.py --one I      # that child: one device call of shape I
"""
import csv, glob, json, os, subprocess, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((2000, 100, 150), (2000, 60, 140), (10000, 256, 40), (150000, 100, 150))
CALLS, WARM = 12, 1


def rows(n, d, k):
    rng = np.random.default_rng(0)
    mu = rng.normal(scale=3.0, size=(k, d))
    return mu[rng.integers(0, k, n)] + rng.normal(size=(n, d))


def one_call(mo, torch, Xd, k, mode):
    os.environ["MUSED_KMEANS_WIDE"] = mode
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab = mo.perform_clustering_on_device(Xd, k, 0)
    return 1e3 * (time.perf_counter() - t0), lab


def measure(shapes=SHAPES, calls=CALLS):
    import torch
    from mused_amd import _lib
    from mused_amd import matrix_operations as mo

    iters = []
    real_call = _lib.call

    def call(name, *args):
        real_call(name, *args)
        if name == "mused_kmeans_lloyd_wide":
            iters.append(int(args[10][0]))

    _lib.call = call
    out = []
    for n, d, k in shapes:
        Xd = torch.from_numpy(rows(n, d, k)).cuda()
        del iters[:]
        before = mo.km_fallbacks
        ms = {"device": [], "host": []}
        same = True
        for i in range(WARM + calls):
            t_dev, lab_dev = one_call(mo, torch, Xd, k, "device")
            t_host, lab_host = one_call(mo, torch, Xd, k, "host")
            same = same and bool(np.array_equal(lab_dev, lab_host))
            if i >= WARM:
                ms["device"].append(t_dev)
                ms["host"].append(t_host)
        out.append(dict(n=n, d=d, k=k, device_ms_median=float(np.median(ms["device"])),
                        host_ms_median=float(np.median(ms["host"])), same_labels_every_call=same,
                        lloyd_iterations=sorted(set(iters)), device_calls=len(iters),
                        host_fallbacks_counted=mo.km_fallbacks - before,
                        lloyd_ws_bytes=int(_lib.lib().mused_kmeans_wide_ws_bytes(n, d, k)),
                        seed_ws_bytes=int(_lib.lib().mused_kmeans_seed_ws_bytes(n, d, k))))
    _lib.call = real_call
    return out


def one(i):
    import torch
    from mused_amd import matrix_operations as mo

    n, d, k = SHAPES[i]
    Xd = torch.from_numpy(rows(n, d, k)).cuda()
    one_call(mo, torch, Xd, k, "device")
    torch.cuda.synchronize()


def kernel_lines(i):
    """A fresh child under rocprofv3 (the program directly behind `--`): the kernel statistics of one device call."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--one", str(i)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, env=dict(os.environ, TMPDIR=tmp), timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        lines = []
        for r in csv.DictReader(open(files[0])):
            name = r["Name"].split("(")[0].split("::")[-1]
            if name.startswith(("km_", "kmw_", "kpp_")):
                lines.append(f"{name}: calls {r['Calls']}, total {float(r['TotalDurationNs']) / 1e6:.3f} ms, "
                             f"average {float(r['AverageNs']) / 1e3:.1f} us, {float(r['Percentage']):.1f} % of kernel time")
        return lines


if __name__ == "__main__":
    if "--one" in sys.argv:
        one(int(sys.argv[sys.argv.index("--one") + 1]))
    else:
        res = {"calls_timed": CALLS, "shapes": measure()}
        if "--kernels" in sys.argv:
            res["kernels"] = {"x".join(map(str, s)): kernel_lines(i) for i, s in enumerate(SHAPES)}
        print(json.dumps(res, indent=1))
