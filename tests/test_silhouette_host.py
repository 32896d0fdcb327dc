"""mused_amd/silhouette.py (the NumPy rules csrc/silhouette.hip implements) against scikit-learn, within the bound of
tests/silhouette_cases.py; the separations that bound needs; scikit-learn's error texts; and the selector's rule (the highest
silhouette wins, ties to the smaller k) with scikit-learn's KMeans and silhouette as a stand-in for the device."""
import numpy as np
import pytest

import silhouette_cases as sc
from mused_amd import silhouette as sil


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_numpy_rules_match_sklearn(case):
    ref_s, ref_db, ref_ch = sc.reference(case.name)
    sb, score_b, db_b, ch_b = sc.bounds(case.name)
    s = sil.silhouette_samples_numpy(case.X, case.labels)
    db = sil.davies_bouldin_numpy(case.X, case.labels)
    ch = sil.calinski_harabasz_numpy(case.X, case.labels)
    err = np.abs(s - ref_s)
    print(f"{case.name}: samples max err {err.max():.3e} (bound at it {sb[err.argmax()]:.3e}, largest bound {sb.max():.3e}), "
          f"score err {abs(s.mean() - ref_s.mean()):.3e} / {score_b:.3e}, DB err {abs(db - ref_db):.3e} / {db_b:.3e}, "
          f"CH rel err {abs(ch - ref_ch) / abs(ref_ch):.3e} / {ch_b:.3e}")
    assert (err <= sb).all()
    assert abs(s.mean() - ref_s.mean()) <= score_b
    assert abs(db - ref_db) <= db_b
    assert abs(ch - ref_ch) <= ch_b * abs(ref_ch)


@pytest.mark.parametrize("case", [c for c in sc.CASES if not c.dup], ids=[c.name for c in sc.CASES if not c.dup])
def test_cases_are_separated_enough(case):
    """Without duplicated rows the smallest pair distance keeps every bound below 1e-8: a case that fails is a badly chosen
    input.  (Davies-Bouldin: a row alone in its cluster IS its centroid, a duplicated pair by construction -- scikit-learn's
    expansion leaves sqrt(rounding) there, the sqrt(2 E) branch; its bound is asserted for the cases without such a row.)"""
    sb, score_b, db_b, ch_b = sc.bounds(case.name)
    print(f"{case.name}: min pair distance {sc.min_pair_distance(case.X):.3e}, bounds {sb.max():.3e} {db_b:.3e} {ch_b:.3e}")
    assert sc.min_pair_distance(case.X) > 0.0
    assert sb.max() < 1e-8 and score_b < 1e-8 and ch_b < 1e-8
    if np.bincount(np.unique(case.labels, return_inverse=True)[1]).min() > 1:
        assert db_b < 1e-8


def test_conventions():
    by = {c.name: c for c in sc.CASES}
    c = by["singletons"]
    s = sil.silhouette_samples_numpy(c.X, c.labels)
    alone = np.isin(c.labels, [0, 1, 3])
    assert alone.sum() == 3 and (s[alone] == 0.0).all() and (s[~alone] != 0.0).all()
    c = by["all_identical_integers"]
    assert sil.calinski_harabasz_numpy(c.X, c.labels) == 1.0 == sc.reference(c.name)[2]
    assert sil.davies_bouldin_numpy(c.X, c.labels) == 0.0 == sc.reference(c.name)[1]
    assert (sil.silhouette_samples_numpy(c.X, c.labels) == 1.0).all()
    c = by["any_int32_labels"]
    assert set(np.unique(c.labels)) == {-1, 0, 5, sc.I32_MAX, sc.I32_MIN}


@pytest.mark.parametrize("name,X,labels,text", sc.error_cases(), ids=[e[0] for e in sc.error_cases()])
def test_error_texts(name, X, labels, text):
    from sklearn import metrics as skm

    for ours, theirs in ((sil.silhouette_samples_numpy, skm.silhouette_samples),
                         (sil.davies_bouldin_numpy, skm.davies_bouldin_score),
                         (sil.calinski_harabasz_numpy, skm.calinski_harabasz_score)):
        with pytest.raises(ValueError) as theirs_err:
            theirs(X, labels)
        with pytest.raises(ValueError) as ours_err:
            ours(X, labels)
        assert str(ours_err.value) == str(theirs_err.value) == text


def test_selector_rule_on_four_blobs():
    """What select_n_clusters_on_device must reproduce: on 4 well-separated blobs the silhouette picks k = 4, and the gap to
    the runner-up is orders above the tolerance -- which is what makes the GPU test of the selector meaningful."""
    from sklearn import metrics as skm
    from sklearn.cluster import KMeans

    X, _ = sc.four_blobs()
    scores = {}
    for k in range(2, 8):
        lab = KMeans(n_clusters=k, random_state=0).fit_predict(X)
        scores[k] = float(skm.silhouette_score(X, lab))
        assert abs(float(sil.silhouette_samples_numpy(X, lab).mean()) - scores[k]) <= sc.score_bound(X, lab)
    best = min(k for k in scores if scores[k] == max(scores.values()))   # ties to the smaller k
    ranked = sorted(scores.values(), reverse=True)
    print(scores)
    assert best == 4
    assert ranked[0] - ranked[1] >= 1e-3
