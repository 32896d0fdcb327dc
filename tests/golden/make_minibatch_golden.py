#!/usr/bin/env python3
"""Golden event labels of the reference's "sSVDMC_mini" approach (main.py:82-86: one MiniBatchKMeans(n_clusters_total,
random_state=seed, batch_size=W) for the stream, partial_fit(reduced).predict(reduced) per window, then the Hungarian
chain), through the reference's OWN window loop.

Reuses make_golden.py's loading of the reference modules (stubs for the absent third-party imports) and its way of
capturing the labels (metrics_evaluation.compute_all_metrics replaced for the run).  Stores only data.

    python tests/golden/make_minibatch_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (loads the reference modules)
from mused_amd import synth  # noqa: E402

# tag -> (n, d, W, ell, k, seed, n_clusters_total)
CASES = {
    "c1_stream_mini_blob_s0": (5000, 64, 500, 16, 50, 0, 4),
    "c1_stream_mini150_blob_s0": (5000, 64, 500, 16, 50, 0, 150),
    "refdef_stream_mini_blob_s0": (20000, 256, 2000, 50, 50, 0, 150),
}


def case_stream_mini(tag, n, d, W, ell, k, seed, n_clusters_total):
    X, labels = synth.blob_stream(n, d, seed, n_centres=4 if d < 256 else 8, sep=2.0)
    captured = {}

    def fake_metrics(results, subset_size, noise_rate, label_mode, sorting, reduced_dim, k_basis,
                     window_size, clusters, true_labels, t1, t0):
        captured["clusters"] = np.asarray(clusters).copy()
        return results

    orig = mg.ref_me.compute_all_metrics
    mg.ref_me.compute_all_metrics = fake_metrics
    try:
        mg.quiet(mg.ref_main.process_streaming_data, {}, [X.astype(np.float64)], [""], W, ell, k, n_clusters_total, seed,
                 "sSVDMC_mini", labels, 1, 0.0, "all", False, 1.5, 2)
    finally:
        mg.ref_me.compute_all_metrics = orig
    allc = captured["clusters"].astype(np.int64)
    mg.save(
        tag,
        meta=np.array([n, d, W, ell, k, seed]),
        kind=np.array("blob"),
        input_digest=np.array([synth.array_digest(X)]),
        all_clusters=allc,
        labels_sha=np.array(hashlib.sha256(allc.tobytes()).hexdigest()),
        n_clusters_total=np.array(n_clusters_total),
    )


def main():
    only = set(filter(None, (sys.argv[1] if len(sys.argv) > 1 else "").split(",")))
    for tag, args in CASES.items():
        if not only or tag in only:
            case_stream_mini(tag, *args)


if __name__ == "__main__":
    main()
