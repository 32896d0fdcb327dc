"""Hungarian label matching on the device (csrc/match_hung.hip) against the host `match_clusters(..., "hungarian")`, SciPy's
assignment and the host specification (mused_amd/hungarian.py): labels, P, N, feasibility, Dijkstra step counts and the
assignment on the table of label pairs, the reference's own outputs, the case where SciPy raises, the host routes, chains
in one launch, and the Hungarian approaches through the pipeline."""
import numpy as np
import pytest

from conftest import load_golden, regen_inputs
from test_match_hung_host import MIN_OVERLAP, SEEDS, TIE_SEEDS, TIE_SHAPES, TUPLES, host_pair, host_tie
from test_match_pot_host import drift_chain

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mused_amd import distributed as mdist  # noqa: E402
from mused_amd import matrix_operations as mo  # noqa: E402

# (seed, W, kp, kn) of the drifting pairs, then ("tie", seed, P, N) of the two-valued cost tables
CASES = [(s,) + t for t in TUPLES for s in SEEDS] + [("tie", s) + t for t in TIE_SHAPES for s in TIE_SEEDS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def launch(raw, prev, min_overlap=MIN_OVERLAP):
    """One mused_match_hung_chain launch from NumPy labels -> (matched NumPy, info, assign NumPy)."""
    raw_dev = torch.from_numpy(np.atleast_2d(raw).astype(np.int32)).cuda()
    prev_dev = None if prev is None else torch.from_numpy(np.asarray(prev).astype(np.int32)).cuda()
    matched, info, assign = mo.match_chain_launch(raw_dev, prev_dev, min_overlap, want_plan=True, method="hungarian")
    return matched.cpu().numpy(), info, assign.cpu().numpy()


def host_chain(raw, prev=None):
    out = []
    for r in raw:
        prev = mo.match_clusters(prev, r, "hungarian", MIN_OVERLAP)
        out.extend(prev)
    return np.array(out)


def table_chain(seed=1, W=6000, k=150, windows=6):
    """The table's generator applied to its own output: every window drifts from the one before.  Seed 1 is the first one
    whose six windows SciPy solves: with seeds 0, 2 and 3 the host loop itself ends in SciPy's ValueError at window 5, 4 and
    4 (the case test_scipy_raises_case_sets_the_assign_flag covers)."""
    rng = np.random.default_rng(seed)
    cur, out = rng.integers(0, k, W), []
    for _ in range(windows):
        out.append(cur)
        base = (cur // 8) * 8 + np.where(rng.random(W) < 0.15, 8, 0)
        cur = (base + rng.integers(0, 8, W)) % k
    return np.array(out)


@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_pair_against_scipy_and_the_specification(c):
    h = host_tie(*c[1:]) if c[0] == "tie" else host_pair(*c)
    matched, info, assign = launch(h["new"], h["prev"])
    P, N, steps, feasible, flags, _, done, _ = (int(x) for x in info[0])
    print(f"case {c}: P {P} N {N} steps {steps} (specification {h['spec'][2]}) feasible {feasible} flags {flags}")
    before = mo.match_fallbacks
    labels = np.asarray(mo.match_clusters_on_device(h["prev"], h["new"], MIN_OVERLAP, method="hungarian"))
    assert mo.match_fallbacks == before
    assert flags == 0 and done == 1
    assert (P, N) == (h["P"], h["N"]) and bool(feasible) == h["feasible"]
    assert np.array_equal(labels, h["labels"]) and np.array_equal(matched[0], h["labels"])
    expect = np.full(256, -1)
    if h["feasible"]:
        assert steps == h["spec"][2]
        rows, cols = h["scipy"]
        expect[rows] = cols
    else:   # match_clusters returns before the assignment: the window passes through
        assert steps == 0 and np.array_equal(matched[0], h["new"])
    assert np.array_equal(assign[0], expect)


def test_reference_outputs():
    g = load_golden("edges")
    out = mo.match_clusters_on_device(g["match_prev"], g["match_new"], 3, method="hungarian")
    assert np.array_equal(np.asarray(out), g["match_out"])
    out = mo.match_clusters_on_device(g["match_prev"], g["match_new_inf"], 3, method="hungarian")
    assert np.array_equal(np.asarray(out), g["match_out_inf"])


def test_no_previous_window_and_infeasible_costs():
    new = np.array([3] * 20 + [4] * 20 + [8] * 20)
    assert mo.match_clusters_on_device(None, new, 3, method="hungarian") is new
    assert mo.match_clusters_on_device([], new, 3, method="hungarian") is new
    prev = np.array([0, 0, 0, 1, 1, 1])
    inf_new = np.array([0, 1, 2, 0, 1, 2])   # no overlap reaches 3
    assert mo.match_clusters(prev, inf_new, "hungarian", 3) is inf_new
    assert mo.match_clusters_on_device(prev, inf_new, 3, method="hungarian") is inf_new
    matched, info, assign = launch(inf_new, prev)
    assert info[0].tolist() == [2, 3, 0, 0, 0, 0, 1, 0] and np.array_equal(matched[0], inf_new) and (assign == -1).all()
    with pytest.raises(ValueError, match="Invalid method"):
        mo.match_clusters_on_device(prev, inf_new, 3, method="nope")
    with pytest.raises(ValueError, match="Invalid method"):
        mo.match_chain_on_device(inf_new.reshape(1, -1), method="nope")


def test_scipy_raises_case_sets_the_assign_flag():
    """Every row and column has a finite entry, but rows 1 and 2 share their only column: no complete assignment."""
    prev = np.array([0] * 9 + [1] * 3 + [2] * 3)
    new = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2] + [0] * 3 + [0] * 3)
    with pytest.raises(ValueError):
        mo.match_clusters(prev, new, "hungarian", 3)
    _, info, _ = launch(new, prev)
    assert info[0, :2].tolist() == [3, 3] and int(info[0, 3]) == 1
    assert int(info[0, 4]) == mo.MATCH_FLAG_ASSIGN == 16 and int(info[0, 6]) == 0
    with pytest.raises(ValueError):
        mo.match_clusters_on_device(prev, new, 3, method="hungarian")
    # as window 2 of a chain: windows 0 and 1 are written, the chain ends there
    raw = np.array([prev, prev, new])
    matched, info, _ = launch(raw, None)
    assert info[:, 6].tolist() == [1, 1, 0] and info[:, 4].tolist() == [0, 0, 16]
    assert np.array_equal(matched[:2], raw[:2])
    with pytest.raises(ValueError):
        mo.match_chain_on_device(raw, method="hungarian")


def test_labels_and_sizes_beyond_the_kernel_take_the_host_route():
    raw = drift_chain(seed=1).astype(np.int64)
    big = raw.copy()
    big[2] = np.where(big[2] == 1, 5000, big[2])            # a label beyond 1023 in window 2
    _, info, _ = launch(np.minimum(big, 1024), None)
    assert info[:, 6].tolist() == [1, 1, 0, 0, 0, 0] and int(info[2, 4]) == mo.MATCH_FLAG_RANGE
    before = mo.match_fallbacks
    ref = host_chain(big)
    assert 5000 not in ref   # the assignment gives that cluster a previous label: window 3 is back on the device
    assert np.array_equal(mo.match_chain_on_device(big, method="hungarian"), ref)
    assert mo.match_fallbacks - before == 1
    one_before = mo.match_fallbacks
    one = mo.match_clusters_on_device(big[1], big[2], 3, method="hungarian")
    assert np.array_equal(np.asarray(one), np.asarray(mo.match_clusters(big[1], big[2], "hungarian", 3)))
    assert mo.match_fallbacks == one_before + 1
    rng = np.random.default_rng(3)
    wide = np.stack([rng.integers(0, 8, 3000), rng.permutation(3000) % 300, rng.integers(0, 8, 3000)])   # N = 300 > 256
    _, info, _ = launch(wide, None)
    assert info[:, 6].tolist() == [1, 0, 0] and int(info[1, 4]) == mo.MATCH_FLAG_SIZE and int(info[1, 1]) == 300
    before = mo.match_fallbacks
    assert np.array_equal(mo.match_chain_on_device(wide, method="hungarian"), host_chain(wide))
    assert mo.match_fallbacks - before == 2   # window 1 (N = 300) and window 2 (P = 300)
    one_before = mo.match_fallbacks
    one = mo.match_clusters_on_device(wide[0], wide[1], 3, method="hungarian")
    assert np.array_equal(np.asarray(one), np.asarray(mo.match_clusters(wide[0], wide[1], "hungarian", 3)))
    assert mo.match_fallbacks == one_before + 1


@pytest.mark.parametrize("name", ["drift", "table"])
def test_chain_in_one_launch_and_split(name):
    raw = drift_chain() if name == "drift" else table_chain()
    ref = host_chain(raw)
    assert np.array_equal(ref, mdist.replay_label_chain(raw, mo.match_clusters))
    before = mo.match_fallbacks
    assert np.array_equal(mo.match_chain_on_device(raw, method="hungarian"), ref)
    W = raw.shape[1]
    head = mo.match_chain_on_device(raw[:2], method="hungarian")
    tail = mo.match_chain_on_device(torch.from_numpy(raw[2:]).cuda(), prev0=head[W:], method="hungarian")
    assert np.array_equal(np.concatenate([head, tail]), ref)
    assert mo.match_fallbacks == before
    matched, info, _ = launch(raw, None)
    assert info[:, 6].tolist() == [1] * len(raw) and np.array_equal(matched.ravel(), ref)
    chain = ref.reshape(raw.shape)
    feas = [int(mo._feasible(mo._overlap_costs(a, b, MIN_OVERLAP)[2])) for a, b in zip(chain[:-1], raw[1:])]
    assert info[:, 3].tolist() == [0] + feas
    if name == "drift":
        assert feas == [1, 1, 0, 0, 1]
    else:
        assert feas == [1] * 5 and int(info[1:, 2].min()) > 150   # augmenting paths inside the chain


def test_inputs_and_edge_shapes():
    h = host_pair(1, 300, 9, 7)   # P > N
    dev = torch.device("cuda")
    for dt in (torch.int32, torch.int64):
        out = mo.match_clusters_on_device(torch.from_numpy(h["prev"]).to(dev, dt), torch.from_numpy(h["new"]).to(dev, dt), 3,
                                          method="hungarian")
        assert np.array_equal(np.asarray(out), h["labels"])
    new_t = torch.from_numpy(h["new"]).to(dev)
    assert mo.match_clusters_on_device(None, new_t, 3, method="hungarian") is new_t
    new = np.array([3] * 20 + [4] * 20 + [8] * 20)
    six, two = np.full(60, 6), np.full(60, 2)
    shapes = [(six, new), (new, two), (six, two),                                    # P = 1, N = 1, both
              (np.arange(60) % 5, np.arange(60) // 20), (np.arange(60) // 20, np.arange(60) % 5),   # P > N, P < N
              (np.repeat(np.arange(6), 10), np.repeat(np.arange(4), 15)), (np.repeat(np.arange(4), 15), np.repeat(np.arange(6), 10))]
    for prev, nw in shapes:
        ref = mo.match_clusters(prev, nw, "hungarian", 3)
        out = mo.match_clusters_on_device(prev, nw, 3, method="hungarian")
        assert (out is nw) == (ref is nw)
        assert np.array_equal(np.asarray(out), np.asarray(ref))
        _, info, assign = launch(nw, prev)
        up, un, cost = mo._overlap_costs(prev, nw, 3)
        assert info[0, :2].tolist() == [len(up), len(un)] and int(info[0, 3]) == int(mo._feasible(cost))
        if mo._feasible(cost):
            from scipy.optimize import linear_sum_assignment

            expect = np.full(256, -1)
            rows, cols = linear_sum_assignment(cost)
            expect[rows] = cols
            assert np.array_equal(assign[0], expect)


def _count_launches(monkeypatch):
    calls = []
    real = mo.match_chain_launch

    def wrapped(*a, **kw):
        calls.append((kw.get("method", "pot"), int(a[0].shape[0])))
        return real(*a, **kw)

    monkeypatch.setattr(mo, "match_chain_launch", wrapped)
    return calls


def test_pipeline_approach_ssvdmc_takes_the_device_route(monkeypatch):
    from mused_amd.pipeline import process_streaming_data

    g = load_golden("c1_stream_blob_s0")
    mods, labels, (n, d, W, ell, k, seed) = regen_inputs(g)
    args = ({}, mods, [""] * len(mods), W, ell, k, len(np.unique(labels)), seed, "sSVDMC", labels, 1, 0.0, "types", False,
            1.5, 2)
    calls = _count_launches(monkeypatch)
    monkeypatch.delenv("MUSED_MATCH", raising=False)
    dev_out = np.asarray(process_streaming_data(*args)["all_clusters"])
    n_dev = len(calls)
    assert n_dev >= 1 and {m for m, _ in calls} == {"hungarian"}
    monkeypatch.setenv("MUSED_MATCH", "host")
    host_out = np.asarray(process_streaming_data(*args)["all_clusters"])
    assert len(calls) == n_dev
    assert np.array_equal(dev_out, host_out)


def test_lane_pipeline_replays_the_chain_on_the_device(monkeypatch):
    """The three windows of the SWFDMC fixture on two lanes (the stream test_gpu_headline_shapes.py pins to the sequential
    specification, so SciPy is known to solve every window of it)."""
    from mused_amd import synth
    from mused_amd.pipeline import SwfdmcLanes

    g = load_golden("swfdmc_w10k_m1_3win")
    W, ell, k, seed, n_windows = (int(x) for x in g["meta"][:5])
    d = int(g["meta"][5])
    wins = [synth.stream_window("blob", t, W, d, seed) for t in range(n_windows)]
    labels = [w[1] for w in wins]
    calls = _count_launches(monkeypatch)
    outs = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("MUSED_MATCH", mode)
        windows = [[torch.from_numpy(w[0].astype(np.float64)).cuda()] for w in wins]
        R = SwfdmcLanes.r_of_first_window(windows[0], W, k)
        before = len(calls)
        with SwfdmcLanes(W, ell, k, seed, 2, R, modality_types=[""]) as lanes:
            outs[mode] = np.asarray(lanes.run(windows, labels), dtype=np.int64)
        # the lanes' own pipeline matches window by window as well: the final replay is the launch over all windows at once
        assert (("hungarian", n_windows) in calls[before:]) == (mode == "device")
        assert (len(calls) > before) == (mode == "device")
    assert np.array_equal(outs["device"], outs["host"])
    assert np.array_equal(outs["device"], g["all_clusters"].astype(np.int64))
