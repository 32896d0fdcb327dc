"""Per-window cost of the "sSVDMC_mini" clusterer (main.py:82-86: partial_fit(X).predict(X) on one MiniBatchKMeans):
the device class (mused_amd.cluster) against scikit-learn at (W, d, k) = (10000, 128, 150) and (2000, 50, 150).  Wall time
per window for both, plus the device time between events on the class's stream (enqueue of the step .. end of predict).
JSON on stdout."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sklearn.cluster import MiniBatchKMeans as SkMiniBatch
from mused_amd.cluster import MiniBatchKMeans

steps, warm = 12, 3
out = {"steps_timed": steps, "shapes": []}
for W, d, k in ((10000, 128, 150), (2000, 50, 150)):
    rng = np.random.default_rng(0)
    mu = rng.normal(scale=3.0, size=(8, d))
    batches = [mu[rng.integers(0, 8, W)] + rng.normal(size=(W, d)) for _ in range(warm + steps)]
    dev = [torch.from_numpy(X).cuda() for X in batches]
    st = torch.cuda.Stream()
    ours = MiniBatchKMeans(n_clusters=k, random_state=0, batch_size=W, stream=st)
    ref = SkMiniBatch(n_clusters=k, random_state=0, batch_size=W)
    torch.cuda.synchronize()
    wall_dev, wall_ref, ev_ms, same = [], [], [], True
    for t in range(warm + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        lab = ours.partial_fit(dev[t]).predict(dev[t])
        t1 = time.perf_counter()
        e1.record(st)
        lab_ref = ref.partial_fit(batches[t]).predict(batches[t])
        t2 = time.perf_counter()
        e1.synchronize()
        same = same and np.array_equal(lab, lab_ref) and np.array_equal(ours.cluster_centers_, ref.cluster_centers_)
        if t >= warm:
            wall_dev.append(1e3 * (t1 - t0))
            wall_ref.append(1e3 * (t2 - t1))
            ev_ms.append(e0.elapsed_time(e1))
    out["shapes"].append(dict(W=W, d=d, k=k, device_wall_ms_median=float(np.median(wall_dev)),
                              device_stream_ms_median=float(np.median(ev_ms)),
                              sklearn_wall_ms_median=float(np.median(wall_ref)),
                              bitwise_equal_to_sklearn=bool(same)))
print(json.dumps(out, indent=1))
