"""Per-window cost of the label matching on the device, `match_clusters_on_device` / `match_chain_on_device`, against the
host `match_clusters`: --method pot (csrc/match.hip against mused_amd/sinkhorn.py, the stand-in for the reference's POT
call) on label pairs (W, kp, kn, noise), --method hungarian (csrc/match_hung.hip against SciPy) on the same shapes and
(2000, 4, 4) with labels that drift between groups of 8, so that the solver walks augmenting paths; both on a 20-window
chain at W = 10000, k = 8.  Wall time of a call from NumPy labels to NumPy labels for both (the median of 12 calls), plus
the kernel's time between events around the C call (for hungarian also with a min_overlap no count reaches: everything
but the solver); labels compared.  --wide: the wide Hungarian chain (csrc/match_wide.hip, any int32 label, up to 4,096 labels
a side) on the generator shapes of tests/test_match_wide_host.py, a DBSCAN-like infeasible pair and one narrow shape through
both entries; device wall (median of 12 calls after one warm-up), kernels alone (events), and the host `match_clusters`,
the route such windows took before (timed once where one call takes longer than half a second).  JSON on stdout."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mused_amd import matrix_operations as mo

ap = argparse.ArgumentParser()
ap.add_argument("--method", choices=("pot", "hungarian"), default="pot")
ap.add_argument("--wide", action="store_true")
ARGS = ap.parse_args()
METHOD, WIDE = ("hungarian" if ARGS.wide else ARGS.method), ARGS.wide
HUNG = METHOD == "hungarian"
CALLS, WARM = 12, 2
# the last pair is the largest size class of the kernel (part of K in the workspace)
PAIRS = ((10000, 150, 150, .5), (2000, 50, 50, .1), (2000, 8, 8, .02), (2000, 2, 2, .2), (20000, 256, 256, .5))


def drift_case(seed, W, kp, kn):
    """tests/test_match_hung_host.py's generator: a new label stays in its previous label's group of 8 or moves to the next
    group for 15 % of the rows.  As there, groups of 4 at 4 x 4 (with groups of 8 on 4 labels nothing would drift)."""
    g = 4 if (kp, kn) == (4, 4) else 8
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, kp, W)
    base = (prev // g) * g + np.where(rng.random(W) < 0.15, g, 0)
    return prev, (base + rng.integers(0, g, W)) % kn


def case(seed, W, kp, kn, noise):
    if HUNG:
        return drift_case(seed, W, kp, kn)
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


def launch_ms(raw, prev, min_overlap=3):
    """The kernel alone: events around the C call, every buffer allocated before, info read after the second event."""
    import ctypes as C
    from mused_amd import _lib, engine as eng
    rd = torch.from_numpy(raw.astype(np.int32)).cuda()
    pd = None if prev is None else torch.from_numpy(prev.astype(np.int32)).cuda()
    K, W = rd.shape
    matched = torch.empty((K, W), dtype=torch.int32, device="cuda")
    info = torch.empty((K, 8), dtype=torch.int32, device="cuda")
    entry, ws_entry = mo._MATCH_ENTRIES[METHOD][:2]
    ws = torch.empty(int(getattr(_lib.lib(), ws_entry)()), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    ms = []
    for i in range(WARM + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call(entry, eng.ptr(rd), K, W, eng.ptr(pd) if pd is not None else None, min_overlap, eng.ptr(matched),
                  eng.ptr(info), None, eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
        e1.record()
        e1.synchronize()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), info.cpu().numpy()


def host_chain(raw):
    prev, out = None, []
    for r in raw:
        prev = mo.match_clusters(prev, r, METHOD, 3)
        out.extend(prev)
    return np.array(out)


def wide_pair(seed, k, per, g, noise):
    """tests/test_match_wide_host.py's generator."""
    rng = np.random.default_rng(seed)
    W = k * per
    cur = rng.integers(0, k, W)
    base = (cur // g) * g + np.where(rng.random(W) < 0.15, g, 0)
    new = (base + rng.integers(0, g, W)) % k
    if noise > 0:
        cur = np.where(rng.random(W) < noise, -1, cur)
        new = np.where(rng.random(W) < noise, -1, new)
    return cur, new


def dbscan_like(seed=0, W=2000, clusters=400, noise=0.30):
    """400 labels a side in clusters of a few rows and 30 % noise, no positional relation between the sides: infeasible."""
    rng = np.random.default_rng(seed)
    def side():
        lab = rng.integers(0, clusters, W)
        lab[:clusters] = np.arange(clusters)
        return np.where(rng.random(W) < noise, -1, lab)[rng.permutation(W)]
    return side(), side()


def wide_launch_ms(new, prev):
    """The seven kernels of a window alone: events around the C call, every buffer allocated before."""
    import ctypes as C
    from mused_amd import _lib, engine as eng
    rd = torch.from_numpy(new.astype(np.int32)).cuda().reshape(1, -1)
    pd = torch.from_numpy(prev.astype(np.int32)).cuda()
    K, W = rd.shape
    matched = torch.empty((K, W), dtype=torch.int32, device="cuda")
    info = torch.empty((K, 8), dtype=torch.int32, device="cuda")
    ws = torch.empty(int(_lib.lib().mused_match_hung_wide_ws_bytes(W)), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    ms = []
    for i in range(WARM + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.call("mused_match_hung_wide_chain", eng.ptr(rd), K, W, eng.ptr(pd), 3, 0, eng.ptr(matched), eng.ptr(info), None,
                  eng.ptr(ws), ws.numel(), C.c_void_p(st.cuda_stream))
        e1.record()
        e1.synchronize()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), info.cpu().numpy()


def wide_table():
    from mused_amd import hungarian as hg
    global WARM
    WARM = 1
    shapes = [("generator", (264, 40, 8)), ("generator", (304, 24, 4)), ("generator", (1040, 24, 4)), ("generator", (1040, 40, 8)),
              ("dbscan-like", None), ("narrow", (6000, 150, 150))]
    rows = []
    for kind, sh in shapes:
        prev, new = (wide_pair(0, *sh, 0.0) if kind == "generator" else dbscan_like() if kind == "dbscan-like"
                     else drift_case(0, *sh))
        before = mo.match_fallbacks
        dev_ms, lab_dev = median_ms(lambda: mo.match_clusters_on_device(prev, new, 3, method="hungarian", wide="only"))
        fb = mo.match_fallbacks - before
        ev_ms, info = wide_launch_ms(new, prev)
        t0 = time.perf_counter()
        lab_host = mo.match_clusters(prev, new, "hungarian", 3)
        first = 1e3 * (time.perf_counter() - t0)
        host_ms, host_calls = (first, 1) if first > 500 else (median_ms(lambda: mo.match_clusters(prev, new, "hungarian", 3))[0], CALLS)
        row = dict(kind=kind, shape=sh, W=len(new), P=int(info[0, 0]), N=int(info[0, 1]), steps=int(info[0, 2]),
                   feasible=int(info[0, 3]), flags=int(info[0, 4]), device_wall_ms_median=dev_ms, kernel_ms_median=ev_ms,
                   host_wall_ms=host_ms, host_calls_timed=host_calls, fallbacks=fb,
                   same_labels=bool(np.array_equal(np.asarray(lab_dev), np.asarray(lab_host))),
                   same_as_specification=bool(np.array_equal(np.asarray(lab_dev), np.asarray(hg.match_labels(prev, new, 3)[0]))))
        if kind == "narrow":   # the narrow chain stays the first choice here: the two entries are only compared
            row["narrow_device_wall_ms_median"] = median_ms(lambda: mo.match_clusters_on_device(prev, new, 3, method="hungarian"))[0]
            row["narrow_kernel_ms_median"] = launch_ms(new.reshape(1, -1), prev)[0]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


if WIDE:
    print(json.dumps({"method": "hungarian-wide", "calls_timed": CALLS, "warm_up": 1, "pairs": wide_table()}, indent=1))
    sys.exit(0)

out = {"method": METHOD, "calls_timed": CALLS, "pairs": [], "chain": None}
for W, kp, kn, noise in PAIRS + (((2000, 4, 4, 0),) if HUNG else ()):
    prev, new = case(0, W, kp, kn, noise)
    before = mo.match_fallbacks
    dev_ms, lab_dev = median_ms(lambda: mo.match_clusters_on_device(prev, new, 3, method=METHOD))
    fb = mo.match_fallbacks - before
    host_ms, lab_host = median_ms(lambda: mo.match_clusters(prev, new, METHOD, 3))
    ev_ms, info = launch_ms(new.reshape(1, -1), prev)
    row = dict(W=W, kp=kp, kn=kn, noise=noise, P=int(info[0, 0]), N=int(info[0, 1]), iterations=int(info[0, 2]),
               feasible=int(info[0, 3]), device_wall_ms_median=dev_ms, kernel_ms_median=ev_ms, host_wall_ms_median=host_ms,
               fallbacks=fb, same_labels=bool(np.array_equal(lab_dev, lab_host)))
    if HUNG:   # `iterations` are the solver's Dijkstra steps; their cost from the same launch without a solve
        row["kernel_ms_without_solve"] = launch_ms(new.reshape(1, -1), prev, min_overlap=W + 1)[0]
        row["us_per_step"] = 1e3 * (ev_ms - row["kernel_ms_without_solve"]) / max(row["iterations"], 1)
    out["pairs"].append(row)
raw = chain()
before = mo.match_fallbacks
dev_ms, lab_dev = median_ms(lambda: mo.match_chain_on_device(raw, method=METHOD))
fb = mo.match_fallbacks - before
host_ms, lab_host = median_ms(lambda: host_chain(raw))
ev_ms, info = launch_ms(raw, None)
out["chain"] = dict(windows=len(raw), W=raw.shape[1], k=8, iterations=[int(x) for x in info[:, 2]],
                    device_wall_ms_median=dev_ms, kernel_ms_median=ev_ms, host_wall_ms_median=host_ms, fallbacks=fb,
                    same_labels=bool(np.array_equal(lab_dev, lab_host)))
print(json.dumps(out, indent=1))
