"""Per-window cost of `perform_clustering_on_device` with the k-means++ seeding on the device (csrc/kmeanspp.hip) against
the host-seeded path (MUSED_KMEANS_SEED=host: host copy of the embedding, NumPy moments, scikit-learn's kmeans_plusplus,
upload) at (W, d, k) = (10000, 128, 8), (10000, 128, 20), (2000, 50, 150), (150000, 50, 4): the median of 12 calls of each
leg on the same device tensor, labels compared.  The embedding starts on the device in both legs, as it does in the
pipeline.

    python tools/kmeans_seed_time.py              # JSON on stdout
    python tools/kmeans_seed_time.py --kernels    # + one line per kernel of csrc/kmeanspp.hip from a child run under
                                                  #   rocprofv3 --kernel-trace --stats (device leg only, 3 calls per shape)
"""
import csv, glob, json, os, subprocess, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((10000, 128, 8), (10000, 128, 20), (2000, 50, 150), (150000, 50, 4))
CALLS, WARM = 12, 2


def rows(W, d, k):
    rng = np.random.default_rng(0)
    mu = rng.normal(scale=3.0, size=(max(k, 3), d))
    return mu[rng.integers(0, len(mu), W)] + rng.normal(size=(W, d))


def leg(mo, torch, Xd, k, mode, calls):
    os.environ["MUSED_KMEANS_SEED"] = mode
    ms, lab = [], None
    for i in range(WARM + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lab = mo.perform_clustering_on_device(Xd, k, 0)
        if i >= WARM:
            ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), lab


def measure(device_only=False, calls=CALLS):
    import torch
    from mused_amd import matrix_operations as mo

    out = []
    for W, d, k in SHAPES:
        Xd = torch.from_numpy(rows(W, d, k)).cuda()
        before = mo.km_fallbacks
        dev_ms, lab_dev = leg(mo, torch, Xd, k, "device", calls)
        rec = dict(W=W, d=d, k=k, device_seed_ms_median=dev_ms, fallbacks=mo.km_fallbacks - before)
        if not device_only:
            host_ms, lab_host = leg(mo, torch, Xd, k, "host", calls)
            rec.update(host_seed_ms_median=host_ms, same_labels=bool(np.array_equal(lab_dev, lab_host)))
        out.append(rec)
    return out


def kernel_lines():
    """Child process under rocprofv3 (the profiler wraps a fresh program); the kpp_* rows of its kernel statistics."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
               sys.executable, os.path.abspath(__file__), "--device-only"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, env=dict(os.environ, TMPDIR=tmp))
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        lines = []
        for r in csv.DictReader(open(files[0])):
            if "kpp_" in r["Name"]:
                name = r["Name"].split("(")[0].split("::")[-1]
                lines.append(f"{name}: calls {r['Calls']}, total {float(r['TotalDurationNs']) / 1e6:.3f} ms, "
                             f"average {float(r['AverageNs']) / 1e3:.1f} us, {float(r['Percentage']):.1f} % of kernel time")
        return lines


if __name__ == "__main__":
    if "--device-only" in sys.argv:
        measure(device_only=True, calls=3)
    else:
        res = {"calls_timed": CALLS, "shapes": measure()}
        if "--kernels" in sys.argv:
            res["kernels"] = kernel_lines()
        print(json.dumps(res, indent=1))
