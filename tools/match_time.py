"""Per-window cost of the "sSVDMC_pot" label matching: `match_clusters_on_device` / `match_chain_on_device` (csrc/match.hip)
against the host specification `match_clusters(..., "pot")` (mused_amd/sinkhorn.py, the stand-in for the reference's POT
call) on label pairs (W, kp, kn, noise) and on a 20-window chain at W = 10000, k = 8.  Wall time of a call from NumPy labels
to NumPy labels for both (the median of 12 calls), plus the kernel's time between events around the C call; labels compared.
JSON on stdout."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mused_amd import matrix_operations as mo

CALLS, WARM = 12, 2
# the last pair is the largest size class of the kernel (part of K in the workspace)
PAIRS = ((10000, 150, 150, .5), (2000, 50, 50, .1), (2000, 8, 8, .02), (2000, 2, 2, .2), (20000, 256, 256, .5))


def case(seed, W, kp, kn, noise):
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, kp, W)
    perm = rng.permutation(max(kp, kn))
    new = perm[prev] % kn
    return prev, np.where(rng.random(W) < noise, rng.integers(0, kn, W), new)


def chain(K=20, W=10000, k=8, noise=.02, seed=0):
    rng = np.random.default_rng(seed)
    cur, out = rng.integers(0, k, W), []
    for _ in range(K):
        out.append(cur)
        cur = np.where(rng.random(W) < noise, rng.integers(0, k, W), rng.permutation(k)[cur])
    return np.array(out)


def median_ms(fn):
    ms, res = [], None
    for i in range(WARM + CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        if i >= WARM:
            ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), res


def launch_ms(raw, prev):
    """The kernel alone: events around the C call, every buffer allocated before, info read after the second event."""
    import ctypes as C
    from mused_amd import _lib, engine as eng
    rd = torch.from_numpy(raw.astype(np.int32)).cuda()
    pd = None if prev is None else torch.from_numpy(prev.astype(np.int32)).cuda()
    K, W = rd.shape
    matched = torch.empty((K, W), dtype=torch.int32, device="cuda")
    info = torch.empty((K, 8), dtype=torch.int32, device="cuda")
    ws = torch.empty(int(_lib.lib().mused_match_pot_ws_bytes()), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    ms = []
    for i in range(WARM + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call("mused_match_pot_chain", eng.ptr(rd), K, W, eng.ptr(pd) if pd is not None else None, 3, eng.ptr(matched),
                  eng.ptr(info), None, eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
        e1.record()
        e1.synchronize()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), info.cpu().numpy()


def host_chain(raw):
    prev, out = None, []
    for r in raw:
        prev = mo.match_clusters(prev, r, "pot", 3)
        out.extend(prev)
    return np.array(out)


out = {"calls_timed": CALLS, "pairs": [], "chain": None}
for W, kp, kn, noise in PAIRS:
    prev, new = case(0, W, kp, kn, noise)
    before = mo.match_fallbacks
    dev_ms, lab_dev = median_ms(lambda: mo.match_clusters_on_device(prev, new, 3))
    fb = mo.match_fallbacks - before
    host_ms, lab_host = median_ms(lambda: mo.match_clusters(prev, new, "pot", 3))
    ev_ms, info = launch_ms(new.reshape(1, -1), prev)
    out["pairs"].append(dict(W=W, kp=kp, kn=kn, noise=noise, P=int(info[0, 0]), N=int(info[0, 1]), iterations=int(info[0, 2]),
                             device_wall_ms_median=dev_ms, kernel_ms_median=ev_ms, host_wall_ms_median=host_ms,
                             fallbacks=fb, same_labels=bool(np.array_equal(lab_dev, lab_host))))
raw = chain()
before = mo.match_fallbacks
dev_ms, lab_dev = median_ms(lambda: mo.match_chain_on_device(raw))
fb = mo.match_fallbacks - before
host_ms, lab_host = median_ms(lambda: host_chain(raw))
ev_ms, info = launch_ms(raw, None)
out["chain"] = dict(windows=len(raw), W=raw.shape[1], k=8, iterations=[int(x) for x in info[:, 2]],
                    device_wall_ms_median=dev_ms, kernel_ms_median=ev_ms, host_wall_ms_median=host_ms, fallbacks=fb,
                    same_labels=bool(np.array_equal(lab_dev, lab_host)))
print(json.dumps(out, indent=1))
