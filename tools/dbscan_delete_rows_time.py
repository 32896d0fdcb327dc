"""Cost of deleting ANY rows from a DBSCAN_incr state (mused_dbscan_incr_delete_rows, csrc/dbscan_incr.hip) and of looking rows up
by value (mused_rows_find, csrc/rows_find.hip), on the stream of tools/dbscan_window_time.py (permuted order): 20,000 rows
held, d = 50, eps = 4.0.

Three deletes of 2,000 rows each, every one from the same state of 20,000 rows (the state arrays are copied back before each
call; HIP events around the call, the median of `--repeats` calls behind one warm-up call):
    random     a random subset: every cluster loses rows (the worst case, as a slide of the permuted stream)
    cluster    the rows of the largest cluster, filled up to 2,000 with rows of the next largest
    prefix     rows 0 .. 1,999 through the new entry, and beside it mused_dbscan_incr_delete(2,000)
Against each: ONE `mused_dbscan` refit of the 18,000 survivors, the only way to those labels without the delete (the median of
`--repeats` calls behind a warm one), and whether the labels agree.

mused_rows_find at (n, q) = (20,000, 2,000) and (150,000, 2,000), a quarter of the queries not held, against the NumPy rule
(mused_amd/rows_find.py) on a host copy (wall clock, rows already on the host).

    python tools/dbscan_delete_rows_time.py [--min-samples 5]        # JSON on stdout
"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dbscan_window_time import D, EPS, W, rows  # noqa: E402

HELD, M = 20000, 2000


def timed(fn, repeats):
    """-> (median ms of `repeats` calls behind one warm-up call, the last result)."""
    import torch

    ts, out = [], None
    for i in range(1 + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if i:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [float(t) for t in ts], out


def deletes(ms, repeats):
    import torch
    from mused_amd import _lib
    from mused_amd import matrix_operations as mo
    from mused_amd.engine import ptr
    from mused_amd.incdbscan import IncrementalDBSCAN

    X = rows(HELD, "permuted")
    Xd = torch.from_numpy(X).cuda()
    c = IncrementalDBSCAN(EPS, ms)
    for lo in range(0, HELD, W):
        c.insert(Xd[lo:lo + W])
    assert not c._host_mode and c.n == HELD
    labels = c.labels()
    sizes = np.bincount(labels[labels >= 0])
    by_size = np.argsort(-sizes, kind="stable")
    cluster = np.concatenate([np.flatnonzero(labels == k) for k in by_size])[:M]
    sets = dict(random=np.sort(np.random.default_rng(2).choice(HELD, M, replace=False)), cluster=np.sort(cluster), prefix=np.arange(M))
    master = [t[:HELD].clone() for t in (c._nrm, c._count, c._parent, c._best)]
    work = [t.clone() for t in master]
    held, out_rows = c._rows(), torch.empty((HELD, D), dtype=torch.float64, device="cuda")
    lab = torch.empty(HELD, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    ws = torch.empty(int(L.mused_dbscan_incr_delete_rows_ws_bytes(HELD, D, c.chunk)), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    info = (C.c_int * 6)()

    def restore():
        for w, m in zip(work, master):
            w.copy_(m)

    res = dict(min_samples=ms, held=HELD, deleted=M, d=D, eps=EPS, clusters=int(len(sizes)), largest_cluster=int(sizes.max()), cases={})
    for name, idx in sets.items():
        dele = torch.from_numpy(idx.astype(np.int32)).cuda()

        def general():
            restore()   # (four copies of 20,000 entries inside the timed span: microseconds)
            _lib.call("mused_dbscan_incr_delete_rows", ptr(held), held.stride(0), D, ptr(out_rows), D, *(ptr(t) for t in work), HELD,
                      ptr(dele), M, EPS, ms, c.chunk, ptr(lab), info, ptr(ws), ws.numel(), st)
            return list(info)

        t_ms, calls, inf = timed(general, repeats)
        got = lab[:HELD - M].cpu().numpy()
        keep = np.ones(HELD, dtype=bool)
        keep[idx] = False
        surv = Xd[torch.from_numpy(keep).cuda()].contiguous()
        r_ms, r_calls, (rl, rinfo) = timed(lambda: mo.dbscan_launch(surv, EPS, ms), repeats)
        rec = dict(delete_rows_ms=t_ms, delete_rows_ms_calls=calls, lost_core=inf[3], R=inf[4], B=inf[5], core=inf[2], clusters=inf[1],
                   refit_ms=r_ms, refit_ms_calls=r_calls, refit_flags=int(rinfo[0]),
                   same_labels_as_refit=bool(np.array_equal(rl.cpu().numpy(), got)),
                   rows_packed=bool(torch.equal(out_rows[:HELD - M].view(torch.int64), surv.view(torch.int64))))
        if name == "prefix":
            def oldest():
                restore()
                _lib.call("mused_dbscan_incr_delete", ptr(held), held.stride(0), D, *(ptr(t) for t in work), HELD, M, EPS, ms, c.chunk,
                          ptr(lab), info, ptr(ws), ws.numel(), st)
                return list(info)

            rec["delete_oldest_ms"], rec["delete_oldest_ms_calls"], inf2 = timed(oldest, repeats)
            rec["same_info_as_delete_oldest"] = inf2 == inf
            rec["same_labels_as_delete_oldest"] = bool(np.array_equal(lab[:HELD - M].cpu().numpy(), got))
        res["cases"][name] = rec
        print(f"  ms={ms} {name}: {t_ms:.2f} ms, refit {r_ms:.2f} ms", file=sys.stderr, flush=True)
    return res


def lookups(repeats):
    import torch
    from mused_amd import _lib
    from mused_amd.engine import ptr
    from mused_amd.rows_find import rows_find

    out = []
    for n in (20000, 150000):
        X = rows(n, "permuted")
        rng = np.random.default_rng(3)
        Q = X[rng.integers(0, n, M)].copy()
        miss = rng.random(M) < 0.25
        Q[miss] += 1.0
        Xd, Qd = torch.from_numpy(X).cuda(), torch.from_numpy(Q).cuda()
        ws = torch.empty(int(_lib.lib().mused_rows_find_ws_bytes(n, M, D)), dtype=torch.uint8, device="cuda")
        idx = torch.empty(M, dtype=torch.int32, device="cuda")
        info = torch.empty(4, dtype=torch.int32, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        t_ms, calls, _ = timed(lambda: _lib.call("mused_rows_find", ptr(Xd), D, n, ptr(Qd), D, M, D, ptr(idx), ptr(info), ptr(ws),
                                                 ws.numel(), st), repeats)
        host = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            want = rows_find(X, Q)
            host.append(1e3 * (time.perf_counter() - t0))
        out.append(dict(n=n, q=M, d=D, rows_find_ms=t_ms, rows_find_ms_calls=calls, numpy_rule_ms=float(np.median(host)),
                        found=int(info[0]), not_found=int(info[1]), same_as_rule=bool(np.array_equal(idx.cpu().numpy(), want))))
        print(f"  rows_find n={n}: {t_ms:.3f} ms, NumPy rule {out[-1]['numpy_rule_ms']:.1f} ms", file=sys.stderr, flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-samples", type=int, nargs="+", default=[2, 5])
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(dict(deletes=[deletes(ms, a.repeats) for ms in a.min_samples], lookups=lookups(a.repeats)), indent=1))
