"""Cost of `perform_dbscan_clustering_on_device` (csrc/dbscan.hip) against MUSED_DBSCAN=host -- the former path: host copy of
the embedding, sklearn.cluster.DBSCAN -- on the same device tensor, at (n, d) = (10000, 50), (40000, 50), (150000, 50) with
eps = 1.5, min_samples = 2: the median of several calls of each leg, labels compared, device fallbacks counted.

Two inputs per shape, tight blobs (sigma 0.1, centres 3 N(0, 1) apart per coordinate) that eps = 1.5 joins blob by blob:

    sparse   n / 250 blobs: a mean neighbourhood of ~250 rows, which scikit-learn's index lists hold at any of the shapes
    dense    4 blobs: a mean neighbourhood of n / 4 rows.  scikit-learn materialises n * (n / 4) * 8 bytes of neighbour
             indices; where that estimate exceeds --host-bytes (default 8 GiB) the host leg is NOT run and the record
             says so.

    python tools/dbscan_time.py                    # JSON on stdout
    python tools/dbscan_time.py --shapes 10000     # a subset of the row counts
    python tools/dbscan_time.py --kernels          # device time per kernel of one call instead (torch.profiler), no host leg

Two sizes per record: `mused_dbscan_ws_bytes`, the workspace of the C entry (the O(n) claim), and `device_peak_extra_bytes`,
the peak of the allocator over the device leg above what was held before it: workspace + labels + flags.
"""
import argparse, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = (10000, 40000, 150000)
D, EPS, MIN_SAMPLES = 50, 1.5, 2
DEVICE_CALLS, HOST_CALLS, WARM = 7, 3, 1


def rows(n, blobs):
    rng = np.random.default_rng(0)
    cen = 3.0 * rng.standard_normal((blobs, D))
    return cen[rng.integers(0, blobs, n)] + 0.1 * rng.standard_normal((n, D))


def leg(mo, torch, Xd, mode, calls, warm):
    os.environ["MUSED_DBSCAN"] = mode
    ms, lab = [], None
    for i in range(warm + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lab = mo.perform_dbscan_clustering_on_device(Xd, EPS, MIN_SAMPLES)
        if i >= warm:
            ms.append(1e3 * (time.perf_counter() - t0))
            if mode == "host":   # minutes per call at the largest shape: show that the run is alive
                print(f"  host call {len(ms)}/{calls}: {ms[-1]:.0f} ms", file=sys.stderr, flush=True)
    os.environ.pop("MUSED_DBSCAN")
    return float(np.median(ms)), lab


def kernel_ms(mo, torch, Xd):
    """Device time of every kernel of ONE device call, by name, in launch order of first appearance."""
    from torch.profiler import ProfilerActivity, profile

    mo.perform_dbscan_clustering_on_device(Xd, EPS, MIN_SAMPLES)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        mo.perform_dbscan_clustering_on_device(Xd, EPS, MIN_SAMPLES)
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if ev.device_time_total > 0:
            out[ev.name] = out.get(ev.name, 0.0) + ev.device_time_total / 1e3
    return out


def measure(shapes, host_bytes, kernels=False):
    import torch
    from mused_amd import _lib
    from mused_amd import matrix_operations as mo

    out = []
    for n in shapes:
        for kind, blobs in (("sparse", max(n // 250, 1)), ("dense", 4)):
            Xd = torch.from_numpy(rows(n, blobs)).cuda()
            if kernels:
                rec = dict(n=n, d=D, input=kind, kernel_ms=kernel_ms(mo, torch, Xd))
                out.append(rec)
                print(json.dumps(rec), file=sys.stderr, flush=True)
                continue
            before = mo.dbscan_fallbacks
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            dev_ms, lab_dev = leg(mo, torch, Xd, "device", DEVICE_CALLS, WARM)
            rec = dict(n=n, d=D, input=kind, mean_neighbourhood=n // blobs, clusters=int(lab_dev.max()) + 1,
                       noise=int((lab_dev < 0).sum()), device_ms_median=dev_ms, fallbacks=mo.dbscan_fallbacks - before,
                       mused_dbscan_ws_bytes=int(_lib.lib().mused_dbscan_ws_bytes(n)),
                       device_peak_extra_bytes=int(torch.cuda.max_memory_allocated() - base))
            est = n * (n // blobs) * 8
            if est > host_bytes:
                rec.update(host_ms_median=None, host_skipped=f"neighbour lists estimated at {est / 2 ** 30:.1f} GiB")
            else:
                host_ms, lab_host = leg(mo, torch, Xd, "host", HOST_CALLS, 0)
                rec.update(host_ms_median=host_ms, same_labels=bool(np.array_equal(lab_dev, lab_host)))
            out.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
            del Xd
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(str(s) for s in SHAPES))
    ap.add_argument("--host-bytes", type=float, default=8 * 2 ** 30)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    res = {"eps": EPS, "min_samples": MIN_SAMPLES, "device_calls": DEVICE_CALLS, "host_calls": HOST_CALLS,
           "shapes": measure([int(s) for s in a.shapes.split(",")], a.host_bytes, a.kernels)}
    print(json.dumps(res, indent=1))
