"""The wide Hungarian label chain on the device (csrc/match_wide.hip: any int32 label value, up to 4,096 distinct labels a
side) against the narrow chain where both apply, against the host specification `hungarian.match_labels` and SciPy's
assignment beyond the narrow limits, its flags (8, 16, 32) and the host routes behind them, edge shapes, chains in one call,
the unchanged defaults of the public functions, and DBSCAN_incr through the pipeline."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from test_match_hung_host import TIE_WIDE_SHAPES, TUPLES, host_tie, pair, tie_pair
from test_match_pot_host import drift_chain
from test_match_wide_host import I32_MAX, I32_MIN, MIN_OVERLAP, dbscan_like, spec_chain, spec_pair, wide_chain, wide_pair

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mused_amd import hungarian as hg  # noqa: E402
from mused_amd import matrix_operations as mo  # noqa: E402

MAXC = 4096


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.int32))).cuda()


def wide(raw, prev, min_overlap=MIN_OVERLAP, max_steps=0):
    """One mused_match_hung_wide_chain call from NumPy labels -> (matched NumPy, info, assign NumPy)."""
    matched, info, assign = mo.match_wide_launch(_dev(np.atleast_2d(raw)), _dev(prev), min_overlap, want_assign=True,
                                                 max_steps=max_steps)
    return matched.cpu().numpy(), info, assign.cpu().numpy()


def narrow(raw, prev, min_overlap=MIN_OVERLAP):
    matched, info, assign = mo.match_chain_launch(_dev(np.atleast_2d(raw)), _dev(prev), min_overlap, want_plan=True,
                                                  method="hungarian")
    return matched.cpu().numpy(), info, assign.cpu().numpy()


def fast_overlap_costs(prev_clusters, new_clusters, min_overlap):
    """What mo._overlap_costs returns, from one contingency pass: the host route's own P x N loop takes seconds to minutes
    at the sizes whose flags are tested here.  The assignment behind it is still match_clusters' SciPy call."""
    up, un, _, cnt = hg.overlap_counts(prev_clusters, new_clusters)
    return up, un, hg.costs_of(cnt, min_overlap)


def expect_assign(cost):
    rows, cols = linear_sum_assignment(cost)
    e = np.full(MAXC, -1)
    e[rows] = cols
    return e


def check_against_specification(prev, new):
    labels, P, N, steps, feasible = hg.match_labels(prev, new, MIN_OVERLAP)
    matched, info, assign = wide(new, prev)
    print(f"P {P} N {N} steps {steps}: device info {info[0].tolist()}")
    assert info[0].tolist() == [P, N, steps, int(feasible), 0, 0, 1, 0]
    assert np.array_equal(matched[0], labels)
    if feasible:
        up, un, _, cnt = hg.overlap_counts(prev, new)
        assert np.array_equal(assign[0], expect_assign(hg.costs_of(cnt, MIN_OVERLAP)))
    else:
        assert (assign == -1).all() and np.array_equal(matched[0], new)
    before = mo.match_fallbacks
    out = mo.match_clusters_on_device(prev, new, MIN_OVERLAP, method="hungarian", wide=True)
    assert mo.match_fallbacks == before and (out is new) == (labels is new) and np.array_equal(np.asarray(out), labels)


# ---- wide equals narrow where both apply -------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", TUPLES + [("tie", 65, 64), ("tie", 256, 256)], ids=lambda t: "-".join(str(x) for x in t))
def test_equals_the_narrow_chain_on_its_table(t):
    prev, new = tie_pair(0, *t[1:]) if t[0] == "tie" else pair(1, *t)
    m_n, i_n, a_n = narrow(new, prev)
    m_w, i_w, a_w = wide(new, prev)
    assert int(i_n[0, 6]) == 1 and np.array_equal(i_w[:, [0, 1, 2, 3, 4, 6]], i_n[:, [0, 1, 2, 3, 4, 6]])
    assert np.array_equal(m_w, m_n) and np.array_equal(a_w[:, :256], a_n) and (a_w[:, 256:] == -1).all()


def test_equals_the_narrow_chain_on_a_drifting_chain():
    raw = drift_chain()
    m_n, i_n, a_n = narrow(raw, None)
    m_w, i_w, a_w = wide(raw, None)
    assert i_n[:, 6].tolist() == [1] * len(raw) and i_n[:, 3].tolist() == [0, 1, 1, 0, 0, 1]
    assert np.array_equal(i_w[:, [0, 1, 2, 3, 4, 6]], i_n[:, [0, 1, 2, 3, 4, 6]])
    assert np.array_equal(m_w, m_n) and np.array_equal(a_w[:, :256], a_n) and (a_w[:, 256:] == -1).all()


# ---- beyond the narrow limits, against match_labels ------------------------------------------------------------------------------

def tie_spec(P, N):
    """spec_pair's keys for the two-valued cost table of seed 0."""
    h = host_tie(0, P, N)
    return dict(h, steps=h["spec"][2], rows=h["scipy"][0], cols=h["scipy"][1])


@pytest.mark.parametrize("c", [(0, 264, 40, 8), (1, 264, 40, 8), (0, 1040, 40, 8)] + [("tie",) + s for s in TIE_WIDE_SHAPES],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_generator_pair_against_the_specification(c):
    h = tie_spec(*c[1:]) if c[0] == "tie" else spec_pair(*c)
    matched, info, assign = wide(h["new"], h["prev"])
    print(f"case {c}: device info {info[0].tolist()}, specification steps {h['steps']}")
    assert info[0].tolist() == [h["P"], h["N"], h["steps"], 1, 0, 0, 1, 0]
    assert np.array_equal(matched[0], h["labels"])
    e = np.full(MAXC, -1)
    e[h["rows"]] = h["cols"]
    assert np.array_equal(assign[0], e)
    before = mo.match_fallbacks
    out = mo.match_clusters_on_device(h["prev"], h["new"], MIN_OVERLAP, method="hungarian",
                                      wide="only" if c[0] == "tie" else True)
    assert mo.match_fallbacks == before and np.array_equal(np.asarray(out), h["labels"])


def test_scattered_int32_values():
    """(304, 24, 4) seed 1 (with -1 rows) through an injective map onto scattered int32 values, negative ones and both
    extremes included: the sort order of the labels changes, so the expectation is recomputed from the mapped labels."""
    h = spec_pair(1, 304, 24, 4)
    rng = np.random.default_rng(11)
    pool = np.setdiff1d(np.concatenate([rng.integers(I32_MIN, I32_MAX, 400), [-1, 0, -7, 5000]]), [I32_MIN, I32_MAX])
    # labels -1 and 0 of the pair take the two extremes, the others 303 scattered values
    vals = np.concatenate([[I32_MIN, I32_MAX], pool[rng.permutation(len(pool))][:303]])
    assert len(np.unique(vals)) == 305 and (vals < 0).sum() > 50
    prev, new = vals[h["prev"] + 1], vals[h["new"] + 1]
    assert I32_MIN in prev and I32_MAX in new
    check_against_specification(prev, new)


def test_both_orientations_of_a_rectangular_pair():
    prev, new = wide_pair(0, 264, 40, 8, 0.0)
    fewer = np.where(new < 8, new + 8, new)   # one block of labels dropped from `new`
    for a, b, shape in ((prev, fewer, (264, 256)), (fewer, prev, (256, 264))):   # P > N: the transposed branch; P < N
        up, un, _, _ = hg.overlap_counts(a, b)
        assert (len(up), len(un)) == shape
        check_against_specification(a, b)


# ---- flags ------------------------------------------------------------------------------------------------------------------------

def test_flag_16_where_scipy_raises(monkeypatch):
    h = spec_pair(3, 1040, 24, 4)
    assert h["raises"] and h["feasible"]
    raw = np.array([h["prev"], h["new"]])
    matched, info, assign = wide(raw, None)
    assert info[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 0] and np.array_equal(matched[0], h["prev"])
    assert info[1, :2].tolist() == [h["P"], h["N"]] and int(info[1, 3]) == 1
    assert int(info[1, 4]) == mo.MATCH_FLAG_ASSIGN == 16 and int(info[1, 6]) == 0 and (assign == -1).all()
    monkeypatch.setattr(mo, "_overlap_costs", fast_overlap_costs)
    before = mo.match_fallbacks
    with pytest.raises(ValueError):
        mo.match_clusters_on_device(h["prev"], h["new"], MIN_OVERLAP, method="hungarian", wide=True)
    assert mo.match_fallbacks == before + 1


def test_flag_8_beyond_4096_labels(monkeypatch):
    lab = np.repeat(np.arange(MAXC + 1), 3)   # 4,097 distinct labels, W = 4,097 * 3, prev = new
    matched, info, _ = wide(lab, lab)
    assert info[0].tolist() == [MAXC + 1, MAXC + 1, 0, 0, 8, 0, 0, 0]
    _, info, _ = wide(lab, np.zeros_like(lab))   # one side alone
    assert info[0].tolist() == [1, MAXC + 1, 0, 0, 8, 0, 0, 0]
    monkeypatch.setattr(mo, "_overlap_costs", fast_overlap_costs)
    before = mo.match_fallbacks
    out = mo.match_clusters_on_device(lab, lab, MIN_OVERLAP, method="hungarian", wide=True)
    assert mo.match_fallbacks == before + 1 and np.array_equal(np.asarray(out), lab)
    # the largest window, every row a label of its own: the hash sets stop filling, the probing stays bounded
    big = np.arange(1 << 20)
    _, info, _ = wide(big, big[::-1].copy())
    assert info[0].tolist() == [MAXC + 1, MAXC + 1, 0, 0, 8, 0, 0, 0]
    check_against_specification(big % 3 - 1, (big // 5) % 4)   # and the same W with 3 x 4 labels: counts near 2^20 / 12
    # 4,096 a side is inside: the identity, every row its own column
    lab = np.repeat(np.arange(MAXC), 3)[::-1].copy()
    matched, info, assign = wide(lab, lab)
    assert info[0].tolist() == [MAXC, MAXC, MAXC, 1, 0, 0, 1, 0]
    assert np.array_equal(matched[0], lab) and np.array_equal(assign[0], np.arange(MAXC))


def test_flag_32_when_the_step_budget_is_spent():
    prev, new = pair(0, 300, 8, 8)
    labels, P, N, steps, feasible = hg.match_labels(prev, new, MIN_OVERLAP)
    assert feasible and steps > 1
    matched, info, _ = wide(new, prev, max_steps=1)
    assert info[0].tolist() == [P, N, 1, 1, 32, 0, 0, 0]
    _, info, _ = wide(new, prev, max_steps=steps)   # exactly enough
    assert info[0].tolist() == [P, N, steps, 1, 0, 0, 1, 0]
    before = mo.match_fallbacks
    out = mo.match_clusters_on_device(prev, new, MIN_OVERLAP, method="hungarian", wide="only", max_steps=1)
    assert mo.match_fallbacks == before + 1 and np.array_equal(np.asarray(out), labels)
    out = mo.match_chain_on_device(np.array([prev, new]), method="hungarian", wide="only", max_steps=1)
    assert mo.match_fallbacks == before + 2 and np.array_equal(out, np.concatenate([prev, labels]))


def test_a_label_beyond_int32_takes_the_host_route():
    prev, new = pair(0, 300, 8, 8)
    new = np.where(new == 2, 1 << 40, new.astype(np.int64))
    ref = mo.match_clusters(prev, new, "hungarian", MIN_OVERLAP)
    before = mo.match_fallbacks
    out = mo.match_clusters_on_device(prev, new, MIN_OVERLAP, method="hungarian", wide=True)
    assert mo.match_fallbacks == before + 1 and np.array_equal(np.asarray(out), np.asarray(ref))
    raw = np.array([prev, new, prev])
    out = mo.match_chain_on_device(raw, method="hungarian", wide=True)
    assert np.array_equal(out, spec_chain(raw)[0])
    assert mo.match_fallbacks == before + 2 + int((1 << 40) in out[300:600])   # window 2 too if the label survived the matching


# ---- edges ------------------------------------------------------------------------------------------------------------------------

def test_edge_shapes():
    check_against_specification(np.array([4]), np.array([-1]))                  # W = 1: infeasible, passes through
    matched, info, _ = wide(np.array([-1]), np.array([-1]), min_overlap=1)      # W = 1, matched
    assert info[0].tolist() == [1, 1, 1, 1, 0, 0, 1, 0] and matched[0].tolist() == [-1]
    noise = np.full(1025, -1)
    check_against_specification(noise, noise)                                   # W = 1,025, every row noise: 1 x 1
    check_against_specification(np.arange(1025) % 3, noise)
    prev, new = dbscan_like()                                                   # infeasible, 401 x 401
    assert len(new) % 64 != 0
    check_against_specification(prev, new)
    matched, info, _ = wide(new, prev)
    assert info[0, 2:4].tolist() == [0, 0] and np.array_equal(matched[0], new)
    assert mo.match_clusters_on_device(prev, new, MIN_OVERLAP, method="hungarian", wide="only") is new
    prev, new = wide_pair(2, 264, 40, 8, 0.05)                                  # W = 10,523: no multiple of 64 or of 256
    check_against_specification(prev[:-37], new[:-37])
    with pytest.raises(ValueError, match="outside"):
        mo.match_wide_launch(torch.zeros((1, (1 << 20) + 1), dtype=torch.int32, device="cuda"), None, 3)


# ---- chains -----------------------------------------------------------------------------------------------------------------------

def test_chain_in_one_call_and_split():
    raw = wide_chain()
    W = raw.shape[1]
    ref, ref_info = spec_chain(raw)
    matched, info, _ = wide(raw, None)
    assert info[:, 6].tolist() == [1] * 6 and np.array_equal(matched.ravel(), ref)
    assert [tuple(int(x) for x in r[:4]) for r in info] == [(P, N, s, int(f)) for P, N, s, f in ref_info]
    assert min(s for _, _, s, _ in ref_info[1:]) > 264   # augmenting paths inside the chain
    head, _, _ = wide(raw[:2], None)
    tail, tail_info, _ = wide(raw[2:], head[1])
    assert np.array_equal(np.concatenate([head.ravel(), tail.ravel()]), ref) and np.array_equal(tail_info, info[2:])
    before = mo.match_fallbacks
    assert np.array_equal(mo.match_chain_on_device(raw, method="hungarian", wide=True), ref)
    first = mo.match_chain_on_device(raw[:2], method="hungarian", wide="only")
    rest = mo.match_chain_on_device(torch.from_numpy(raw[2:]).cuda(), prev0=first[W:], method="hungarian", wide=True)
    assert np.array_equal(np.concatenate([first, rest]), ref) and mo.match_fallbacks == before


def test_chain_continues_behind_a_flag_8_window(monkeypatch):
    """Window 1 has 4,097 labels (flag 8: the host's); its matched labels have 4,096 (SciPy gives label 0 the previous 7, which
    is a label of its own), so windows 2 and 3 are back on the device with P = 4,096 and the transposed solver."""
    W = (MAXC + 1) * 3
    raw = np.array([np.full(W, 7), np.repeat(np.arange(MAXC + 1), 3), (np.arange(W) // 3) % 5, (np.arange(W) // 3) % 4])
    ref, ref_info = spec_chain(raw)
    assert [i[:2] for i in ref_info] == [(0, 0), (1, MAXC + 1), (MAXC, 5), (5, 4)]
    _, info, _ = wide(raw, None)
    assert info[:, 6].tolist() == [1, 0, 0, 0] and info[1].tolist() == [1, MAXC + 1, 0, 0, 8, 0, 0, 0] and not info[2:].any()
    monkeypatch.setattr(mo, "_overlap_costs", fast_overlap_costs)
    before = mo.match_fallbacks
    assert np.array_equal(mo.match_chain_on_device(raw, method="hungarian", wide=True), ref)
    assert mo.match_fallbacks == before + 1


# ---- the defaults of the public functions ---------------------------------------------------------------------------------------

def test_defaults_unchanged_and_wide_counts_no_fallback():
    raw = drift_chain(seed=1).astype(np.int64)
    big = raw.copy()
    big[2] = np.where(big[2] == 1, 5000, big[2])   # tests/test_gpu_match_hung.py: a label beyond 1023 in window 2
    rng = np.random.default_rng(3)
    many = np.stack([rng.integers(0, 8, 3000), rng.permutation(3000) % 300, rng.integers(0, 8, 3000)])   # N = 300 > 256
    for chain, fallbacks in ((big, 1), (many, 2)):
        before = mo.match_fallbacks
        default = mo.match_chain_on_device(chain, method="hungarian")
        assert mo.match_fallbacks - before == fallbacks
        before = mo.match_fallbacks
        assert np.array_equal(mo.match_chain_on_device(chain, method="hungarian", wide=True), default)
        assert np.array_equal(default, spec_chain(chain)[0]) and mo.match_fallbacks == before
        before = mo.match_fallbacks
        one = mo.match_clusters_on_device(chain[1], chain[2], 3, method="hungarian")
        assert mo.match_fallbacks == before + 1
        assert np.array_equal(np.asarray(mo.match_clusters_on_device(chain[1], chain[2], 3, method="hungarian", wide=True)),
                              np.asarray(one))
        assert mo.match_fallbacks == before + 1


def test_match_wide_host_restores_the_host_route(monkeypatch):
    raw = drift_chain(seed=1).astype(np.int64)
    raw[2] = np.where(raw[2] == 1, 5000, raw[2])
    monkeypatch.setenv("MUSED_MATCH_WIDE", "host")
    before = mo.match_fallbacks
    out = mo.match_chain_on_device(raw, method="hungarian", wide=True)
    assert mo.match_fallbacks == before + 1 and np.array_equal(out, spec_chain(raw)[0])


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------

def test_dbscan_incr_stream_matches_on_the_device(monkeypatch):
    """tests/test_gpu_dbscan_incr_stream.py's stream at eps = 0.15, min_samples = 3 (about 20 clusters a window, border and
    noise rows): every window holds -1.  The host match_clusters is never reached; under MUSED_MATCH_WIDE=host it is."""
    from sklearn.cluster import DBSCAN

    from mused_amd import incdbscan, synth
    from mused_amd.pipeline import process_streaming_data

    W, ELL, K, eps, ms = 256, 8, 5, 0.15, 3
    X, labels = synth.blob_stream(4 * W, 16, 0, n_centres=4)
    embeddings = []
    real = incdbscan.IncrementalDBSCAN.insert

    def recording(self, rows):
        embeddings.append(rows.cpu().numpy().copy() if isinstance(rows, torch.Tensor) else np.array(rows))
        return real(self, rows)

    monkeypatch.setattr(incdbscan.IncrementalDBSCAN, "insert", recording)
    host = mo.match_clusters
    reached = []

    def refusing(*a, **kw):
        reached.append(1)
        raise AssertionError("the host match_clusters was reached")

    def run():
        embeddings.clear()
        res = process_streaming_data({}, [X.astype(np.float64)], [""], W, ELL, K, 4, 0, "DBSCAN_incr", labels, 1, 0.0, "types",
                                     False, eps, ms)
        return np.asarray(res["all_clusters"])

    monkeypatch.delenv("MUSED_MATCH", raising=False)
    monkeypatch.delenv("MUSED_MATCH_WIDE", raising=False)
    monkeypatch.setattr(mo, "match_clusters", refusing)
    before = mo.match_fallbacks
    got = run()
    assert not reached and mo.match_fallbacks == before
    raws = [DBSCAN(eps=eps, min_samples=ms).fit_predict(np.concatenate(embeddings[:t + 1]))[-W:] for t in range(4)]
    assert all(-1 in r for r in raws)
    assert got.shape == (4 * W,) and np.array_equal(got, spec_chain(raws)[0])

    def counting(*a, **kw):
        reached.append(1)
        return host(*a, **kw)

    monkeypatch.setattr(mo, "match_clusters", counting)
    monkeypatch.setenv("MUSED_MATCH_WIDE", "host")
    assert np.array_equal(run(), got) and len(reached) >= 3 and mo.match_fallbacks >= before + 3
