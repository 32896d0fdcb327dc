"""Cost of `metrics_evaluation.compute_all_metrics` on host NumPy labels: the device path (one upload, one launch of
csrc/score.hip, one read) against MUSED_SCORE=host (the reference's scikit-learn calls) on the same machine -- the median
of 12 calls of each leg after one warm-up call, values compared, fallbacks counted.

Label sets: n = 2,000 / 10,000 / 150,000 rows with binary labels at noise rate 0.95, 4 classes and 150 classes; at
n = 150,000 also binary labels drawn uniformly, whose rows spread over the four cells where the 0.95-noise rows pile
19 of 20 onto one: `kernel_us` (HIP events around the launch alone, labels resident) of the two shows what combining equal
cells before the atomics is worth.  And `score_windows` at K = 75 windows of W = 2,000 rows.

    python tools/score_time.py            # JSON on stdout, one record per line on stderr as it goes
"""
import contextlib, io, json, os, platform, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS, WARM = 12, 1
SIZES = (2000, 10000, 150000)
VARIABLES = (0, 0.95, "binary", False, 10, 50, 2000)


def labels(kind, n, rng):
    """(true, pred): pred is true with 20 % of the rows redrawn."""
    if kind == "binary_noise95":
        true, values = (rng.random(n) < 0.05).astype(np.int64), 2
    elif kind == "binary_uniform":
        true, values = rng.integers(0, 2, n), 2
    else:
        values = int(kind.split("_")[1])
        true = rng.integers(0, values, n)
    pred = true.copy()
    hit = rng.random(n) < 0.2
    pred[hit] = rng.integers(0, values, int(hit.sum()))
    return true, pred


def leg(me, mode, true, pred):
    if mode == "host":
        os.environ["MUSED_SCORE"] = "host"
    ms, res = [], None
    try:
        for i in range(WARM + CALLS):
            res, _ = me.get_initial_results()
            with contextlib.redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                me.compute_all_metrics(res, *VARIABLES, pred, true, 2, 1)
                dt = time.perf_counter() - t0
            if i >= WARM:
                ms.append(1e3 * dt)
    finally:
        os.environ.pop("MUSED_SCORE", None)
    return float(np.median(ms)), res


def kernel_us(me, torch, true, pred, cells_cap):
    """Median device time of the launch alone, labels resident as int32."""
    import ctypes as C

    from mused_amd import _lib
    from mused_amd import engine as eng

    t, p = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in (true, pred))
    n_seg, seg_len = (1, t.shape[0]) if t.dim() == 1 else tuple(t.shape)
    ws = torch.empty(int(_lib.lib().mused_score_ws_bytes(n_seg, cells_cap)), dtype=torch.uint8, device=t.device)
    out = torch.empty((n_seg, 8), dtype=torch.float64, device=t.device)
    info = torch.empty((n_seg, 8), dtype=torch.int32, device=t.device)
    st = torch.cuda.current_stream()
    us = []
    for i in range(WARM + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call("mused_score_labels", eng.ptr(t), eng.ptr(p), n_seg, seg_len, cells_cap, eng.ptr(out), eng.ptr(info), eng.ptr(ws),
                  ws.numel(), C.c_void_p(st.cuda_stream))
        b.record()
        b.synchronize()
        if i >= WARM:
            us.append(1e3 * a.elapsed_time(b))
    assert not info[:, 5].any().item()
    return float(np.median(us))


def measure():
    import sklearn
    import torch

    from mused_amd import metrics_evaluation as me
    from mused_amd import scores

    rng = np.random.default_rng(0)
    out = {"calls": CALLS, "machine": platform.node(), "cpu": platform.processor() or platform.machine(),
           "gpu": torch.cuda.get_device_name(0), "scikit_learn": sklearn.__version__, "runs": []}
    sets = [(kind, n) for n in SIZES for kind in ("binary_noise95", "classes_4", "classes_150")] + [("binary_uniform", 150000)]
    for kind, n in sets:
        true, pred = labels(kind, n, rng)
        before = me.score_fallbacks
        dev_ms, dev = leg(me, "device", true, pred)
        fallbacks = me.score_fallbacks - before
        host_ms, host = leg(me, "host", true, pred)
        diff = max(abs(dev[k][0] - host[k][0]) for k in scores.KEYS)
        rec = dict(labels=kind, n=n, device_ms_median=dev_ms, host_ms_median=host_ms, kernel_us_median=kernel_us(me, torch, true, pred, me.RUN_CELLS_CAP),
                   fallbacks=fallbacks, max_abs_diff=diff)
        out["runs"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    K, W = 75, 2000
    true, pred = labels("classes_4", K * W, rng)
    true, pred = true.reshape(K, W), pred.reshape(K, W)
    legs = {}
    for mode in ("device", "host"):
        if mode == "host":
            os.environ["MUSED_SCORE"] = "host"
        ms = []
        for i in range(WARM + (CALLS if mode == "device" else 3)):
            t0 = time.perf_counter()
            legs[mode] = me.score_windows(true, pred)
            if i >= WARM:
                ms.append(1e3 * (time.perf_counter() - t0))
        os.environ.pop("MUSED_SCORE", None)
        legs[mode + "_ms"] = float(np.median(ms))
    rec = dict(labels="score_windows classes_4", K=K, W=W, device_ms_median=legs["device_ms"], host_ms_median=legs["host_ms"],
               kernel_us_median=kernel_us(me, torch, true, pred, me.WINDOW_CELLS_CAP),
               max_abs_diff=float(np.abs(legs["device"] - legs["host"]).max()))
    out["runs"].append(rec)
    print(json.dumps(rec), file=sys.stderr, flush=True)
    return out


if __name__ == "__main__":
    print(json.dumps(measure(), indent=1))
