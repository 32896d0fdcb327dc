"""Cost of `metrics_evaluation.compute_partition_metrics` on device tensors (int32 labels resident): the median of 12 calls
after one warm-up call -- every call ends in its reads, so the host clock around it is the call's time -- beside
scikit-learn's and SciPy's nine calls on host copies on the same machine (16 threads, the median of 3), and `kernel_us`,
HIP events around the launch group of csrc/score_partitions.hip alone.  Random labels, shapes (n, T, P):
(2,000, 4, 4), (20,000, 150, 150), (150,000, 150, 150), (150,000, 2, 2) and (150,000, 150, 1,040).

    python tools/partition_time.py            # JSON on stdout, one record per line on stderr as it goes
"""
import json, os, platform, sys, time

os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS, WARM, HOST_CALLS = 12, 1, 3
SHAPES = ((2000, 4, 4), (20000, 150, 150), (150000, 150, 150), (150000, 2, 2), (150000, 150, 1040))


def kernel_us(me, torch, t, p):
    """Median device time of the launch group alone (table, log-gamma table, EMI, merge)."""
    import ctypes as C

    from mused_amd import _lib
    from mused_amd import engine as eng

    n = t.shape[0]
    cells = min(me.RUN_CELLS_CAP, n * n)
    ws = torch.empty(int(_lib.lib().mused_score_partitions_ws_bytes(1, n, cells)), dtype=torch.uint8, device=t.device)
    res = torch.empty(160, dtype=torch.uint8, device=t.device)
    st = torch.cuda.current_stream()
    us = []
    for i in range(WARM + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call("mused_score_partitions", eng.ptr(t), eng.ptr(p), 1, n, cells, 1, eng.ptr(res[:64]), eng.ptr(res[64:128]),
                  eng.ptr(res[128:]), None, eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
        b.record()
        b.synchronize()
        if i >= WARM:
            us.append(1e3 * a.elapsed_time(b))
    assert int(res[128:].cpu().numpy().view(np.int32)[2]) == 0
    return float(np.median(us))


def measure():
    import scipy
    import sklearn
    import torch

    from mused_amd import metrics_evaluation as me

    rng = np.random.default_rng(0)
    out = {"calls": CALLS, "host_calls": HOST_CALLS, "machine": platform.node(), "cpu": platform.processor() or platform.machine(),
           "gpu": torch.cuda.get_device_name(0), "scikit_learn": sklearn.__version__, "scipy": scipy.__version__,
           "threads": os.environ["OMP_NUM_THREADS"], "runs": []}
    for n, T, P in SHAPES:
        true, pred = rng.integers(0, T, n), rng.integers(0, P, n)
        t, p = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (true, pred))
        before = me.partition_fallbacks
        ms, dev = [], None
        for i in range(WARM + CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev = me.compute_partition_metrics(t, p)
            if i >= WARM:
                ms.append(1e3 * (time.perf_counter() - t0))
        fallbacks = me.partition_fallbacks - before
        hs, host = [], None
        for _ in range(HOST_CALLS):
            t0 = time.perf_counter()
            host = me.host_partition_scores(true, pred)
            hs.append(1e3 * (time.perf_counter() - t0))
        dev_ms, host_ms = float(np.median(ms)), float(np.median(hs))
        rec = dict(n=n, T=T, P=P, device_ms_median=dev_ms, host_ms_median=host_ms, host_over_device=host_ms / dev_ms,
                   kernel_us_median=kernel_us(me, torch, t, p), fallbacks=fallbacks,
                   max_abs_diff=max(abs(dev[k] - host[k]) for k in me.PARTITION_KEYS))
        out["runs"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    return out


if __name__ == "__main__":
    print(json.dumps(measure(), indent=1))
