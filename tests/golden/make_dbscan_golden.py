#!/usr/bin/env python3
"""Golden event labels of the reference's batch approach "DBSCAN_batch" (main.py:132-167: kNN adjacency of the whole subset
per modality, fuse_matrices, perform_svd_reduction, then DBSCAN(eps, min_samples) on the embedding), through the
reference's OWN process_batch_data.

Same inputs and the same way of capturing the labels as make_batch_golden.py; only eps and min_samples are new.  Also stores
what decides whether the labels are reproducible beyond rounding: the smallest |d2 - eps^2| over the pairs of the
reference's embedding and the margin tau there (mused_amd/dbscan.py).  Stores only data.

    python tests/golden/make_dbscan_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_batch_golden as mb  # noqa: E402  (loads the reference modules through make_golden)
from mused_amd import dbscan as spec  # noqa: E402
from mused_amd import synth  # noqa: E402

mg = mb.mg

# tag -> (case of make_batch_golden.CASES whose inputs are used, eps, min_samples)
CASES = {
    "batch_dbscan_blob_s0_e150_m2": ("batch_blob_s0", 1.5, 2),
    "batch_dbscan_blob_s0_e050_m5": ("batch_blob_s0", 0.5, 5),
    "batch_dbscan_sed4_s7_e150_m2": ("batch_sed4_s7", 1.5, 2),
}


def case_dbscan(tag, base, eps, min_samples):
    kind, n, d, ell, k, seed, n_clusters = mb.CASES[base]
    mods, types_, labels = mb.batch_inputs(kind, n, d, seed)
    captured = {}

    def fake_metrics(results, subset_size, noise_rate, label_mode, sorting, reduced_dim, k_basis,
                     window_size, clusters, true_labels, t1, t0):
        captured["clusters"] = np.asarray(clusters).copy()
        return results

    orig_metrics, orig_dbscan = mg.ref_me.compute_all_metrics, mg.ref_main.perform_dbscan_clustering

    def spy_dbscan(data, **kw):
        captured["embedding"] = np.asarray(data, dtype=np.float64).copy()
        return orig_dbscan(data, **kw)

    mg.ref_me.compute_all_metrics = fake_metrics
    mg.ref_main.perform_dbscan_clustering = spy_dbscan
    try:
        mg.quiet(mg.ref_main.process_batch_data, {}, mods, types_, ell, k, n_clusters, seed, "DBSCAN_batch", labels, 0.0,
                 "all", False, eps, min_samples, 3, 2000)
    finally:
        mg.ref_me.compute_all_metrics = orig_metrics
        mg.ref_main.perform_dbscan_clustering = orig_dbscan
    allc = captured["clusters"].astype(np.int64)
    E = captured["embedding"]
    margin, tau = spec.margins(E, eps)
    assert np.array_equal(spec.dbscan_labels(E, eps, min_samples), allc), "the closed-form rule differs from scikit-learn"
    mg.save(
        tag,
        meta=np.array([n, d, ell, k, seed, n_clusters, min_samples]),
        eps=np.array(eps),
        base=np.array(base),
        kind=np.array(kind),
        types=np.array(types_),
        input_digest=np.array([synth.array_digest(m) if m.dtype.kind == "f" else "" for m in mods]),
        all_clusters=allc,
        labels_sha=np.array(hashlib.sha256(allc.tobytes()).hexdigest()),
        summary=np.array([len(set(allc[allc >= 0])), int((allc < 0).sum())]),
        margin=np.array([margin, tau]),
    )
    print(tag, "clusters", len(set(allc[allc >= 0])), "noise", int((allc < 0).sum()), "margin", margin, "tau", tau)


def main():
    only = set(filter(None, (sys.argv[1] if len(sys.argv) > 1 else "").split(",")))
    for tag, args in CASES.items():
        if not only or tag in only:
            case_dbscan(tag, *args)


if __name__ == "__main__":
    main()
