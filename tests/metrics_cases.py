"""Label pairs shared by tests/test_scores_host.py and tests/test_gpu_score.py: (name, true, pred) as read-only int64
arrays, seeded.  The reference's seven values per case are recorded in tests/golden/metrics_cases.npz
(tests/golden/make_metrics_golden.py), keyed by name, with a digest of the two arrays.

Generator condition (checked where the fixture is made, on the reference side): in every case whose NMI is compared
within a tolerance the mean of the two label entropies is >= 0.05 -- the NMI tolerance divides by it.

Table sizes cover every path of csrc/score.hip: tables in LDS (up to 24,576 cells: `lds_edge` is exactly that), tables
in the workspace (`lds_over` is one column more; `wide`), 0, 1 and 2 non-event true values (-1 and 0), tails of the
four-row loads (n = 1, 5, 1025, 4097) and both ends of the label range."""
import functools
import hashlib

import numpy as np

KEYS = ("f1_score", "nmi_score", "nmi_e_score", "precision", "recall", "accuracy", "mae")


def _present(rng, n, values):
    """n draws from `values`, every value at least once, shuffled."""
    values = np.asarray(values, dtype=np.int64)
    assert n >= len(values)
    out = np.concatenate([values, values[rng.integers(0, len(values), n - len(values))]])
    return out[rng.permutation(n)]


def _noisy(rng, true, values, rate):
    """`true` with a share `rate` of the rows redrawn from `values`."""
    values = np.asarray(values, dtype=np.int64)
    pred = true.copy()
    hit = rng.random(len(true)) < rate
    pred[hit] = values[rng.integers(0, len(values), int(hit.sum()))]
    return pred


def _build():
    cases = {}

    def add(name, true, pred):
        true, pred = np.asarray(true, dtype=np.int64), np.asarray(pred, dtype=np.int64)
        assert true.shape == pred.shape and true.ndim == 1
        true.setflags(write=False)
        pred.setflags(write=False)
        cases[name] = (true, pred)

    rng = np.random.default_rng(20240)
    t = (rng.random(4000) < 0.05).astype(np.int64)                 # binary labels, noise rate 0.95
    add("binary_noise95", t, _noisy(rng, t, [0, 1], 0.1))
    t = _present(rng, 4000, range(4))
    add("types_4x4", t, _noisy(rng, (t + 1) % 4, range(4), 0.2))
    t = _present(rng, 6000, range(150))
    p = _noisy(rng, t, range(150), 0.3)
    p[:150] = rng.permutation(150)
    add("all_150x150", t, p)
    t = _present(rng, 5000, range(4))
    p = t * 175 + rng.integers(0, 175, 5000) - 1                    # about 700 clusters, -1 among them
    p[:700] = np.arange(-1, 699)
    add("dbscan_like", t, p)
    t = _present(rng, 20000, range(151))
    p = (t * 4 + rng.integers(0, 100, 20000)) % 700
    p[:700] = rng.permutation(700)
    add("wide_151x700", t, p)
    add("independent_4x5", _present(rng, 3000, range(4)), _present(rng, 3000, range(5)))
    add("one_pred_cluster", _present(rng, 2000, range(4)), np.full(2000, 7))
    t = _present(rng, 2000, [0, 3])
    add("no_second_event_class", t, _noisy(rng, t, [0, 1, 3], 0.3))
    add("both_single_class", np.full(100, 2), np.full(100, 5))
    t = _present(rng, 2000, range(5))
    add("identical", t, t.copy())
    add("all_events", _present(rng, 1500, [1, 2, 3]), _present(rng, 1500, [1, 2, 3, 4]))
    add("n5", [0, 1, 1, 2, 0], [0, 1, 2, 2, 1])
    add("n1", [3], [4])
    for n in (1025, 4097):
        t = _present(rng, n, range(3))
        add(f"tail_n{n}", t, _noisy(rng, t, range(4), 0.25))
    t = _present(rng, 3000, [-1, 0, 7, 65534])
    add("range_ends", t, _noisy(rng, t, [-1, 1, 300, 65534], 0.3))
    t = _present(rng, 8000, range(96))
    p = (t * 3 + rng.integers(0, 40, 8000)) % 256
    p[:256] = rng.permutation(256)
    add("lds_edge_96x256", t, p)
    p = (t * 3 + rng.integers(0, 40, 8000)) % 257
    p[:257] = rng.permutation(257)
    add("lds_over_96x257", t, p)
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    return _build()


CASE_NAMES = ["binary_noise95", "types_4x4", "all_150x150", "dbscan_like", "wide_151x700", "independent_4x5", "one_pred_cluster",
              "no_second_event_class", "both_single_class", "identical", "all_events", "n5", "n1", "tail_n1025", "tail_n4097",
              "range_ends", "lds_edge_96x256", "lds_over_96x257"]


def case(name):
    return all_cases()[name]


def digest(true, pred):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(true, dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(pred, dtype=np.int64).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def windows(width=500):
    """Seven windows of `width` rows with a different class set each: (true (7, width), pred (7, width)), int64.  Window 2
    has a single true class, window 4 no event rows (true <= 0 only)."""
    rng = np.random.default_rng(77)
    sets = [([0, 1, 2], [0, 1, 2]), ([0, 5, 9, 11], [1, 5, 9]), ([4], [0, 4, 6]), ([-1, 0, 2, 3], [-1, 2, 3, 8]),
            ([-1, 0], [0, 1, 2]), (list(range(40)), list(range(10, 60))), ([0, 1], [0, 1])]
    true, pred = [], []
    for tv, pv in sets:
        t = _present(rng, width, tv)
        true.append(t)
        pred.append(_noisy(rng, np.where(np.isin(t, pv), t, pv[0]), pv, 0.3))
    true, pred = np.stack(true), np.stack(pred)
    true.setflags(write=False)
    pred.setflags(write=False)
    return true, pred
