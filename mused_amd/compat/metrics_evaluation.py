"""Drop-in module: put this directory on sys.path and mused's `main.py:6` import line (`import metrics_evaluation`)
resolves to the MI355X path: the seven metrics of a run from one launch of csrc/score.hip, and the three truth-free indices
(silhouette, Davies-Bouldin, Calinski-Harabasz) of csrc/silhouette.hip, and the nine numbering-free partition scores (ARI, AMI,
V-measure, ..., matched accuracy) of csrc/score_partitions.hip."""
from mused_amd.metrics_evaluation import (  # noqa: F401
    compute_all_metrics,
    compute_internal_metrics,
    compute_partition_metrics,
    get_initial_results,
    partition_windows,
    score_windows,
    silhouette_samples_on_device,
)
