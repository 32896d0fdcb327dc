#!/usr/bin/env python3
"""Golden values of the reference's OWN `metrics_evaluation.compute_all_metrics` on the label pairs of
tests/metrics_cases.py.

Run only where the reference is present (/root/reference, read-only).  Imports its `metrics_evaluation` at run time, calls
`get_initial_results()` and `compute_all_metrics(...)` per case and stores ONLY data in tests/golden/metrics_cases.npz:
per case a digest of the two label arrays, the seven appended values, the label entropies scikit-learn computes (the
generator condition of tests/metrics_cases.py is asserted here) and, once, the keys of get_initial_results() in order.

    python tests/golden/make_metrics_golden.py
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

import metrics_evaluation as ref_me  # noqa: E402  (the reference module)
from sklearn.metrics.cluster import entropy  # noqa: E402

import metrics_cases as mc  # noqa: E402

assert os.path.dirname(os.path.abspath(ref_me.__file__)) == "/root/reference"
MIN_MEAN_ENTROPY = 0.05
VARIABLES = (1234, 0.95, "binary", False, 10, 50, 2000)   # the independent variables handed to every call


def main():
    arrs = {}
    keys0, variables = ref_me.get_initial_results()
    arrs["result_keys"] = np.array(list(keys0))
    arrs["independent_variables"] = np.array(list(variables))
    arrs["names"] = np.array(mc.CASE_NAMES)
    for name in mc.CASE_NAMES:
        true, pred = mc.case(name)
        results, _ = ref_me.get_initial_results()
        with contextlib.redirect_stdout(io.StringIO()) as log:
            ref_me.compute_all_metrics(results, *VARIABLES, pred, true, 3_500_000_000, 1_000_000_000)
        values = np.array([float(results[k][0]) for k in mc.KEYS])
        h = np.array([entropy(true), entropy(pred)])
        single = len(np.unique(true)) == 1 and len(np.unique(pred)) == 1   # NMI is the exact 1.0 there
        assert single or h.mean() >= MIN_MEAN_ENTROPY, (name, h)
        arrs[f"{name}__digest"] = np.array(mc.digest(true, pred))
        arrs[f"{name}__values"] = values
        arrs[f"{name}__entropy"] = h
        arrs[f"{name}__processing_time"] = np.array(results["processing_time"][0])
        arrs[f"{name}__log"] = np.array(log.getvalue())
        print(name, len(true), values, "H", h)
    path = os.path.join(HERE, "metrics_cases.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
