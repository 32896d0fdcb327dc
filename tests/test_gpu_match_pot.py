"""Sinkhorn label matching on the device (csrc/match.hip) against the host specification (mused_amd/sinkhorn.py): labels,
P, N, feasibility, iteration counts and the plan on the table of label pairs, the flag budget, chains in one launch, the
host fallbacks, and approach "sSVDMC_pot" through the pipeline."""
import numpy as np
import pytest

from conftest import load_golden, regen_inputs
from test_match_pot_host import PLAN_FACTOR, SEEDS, TUPLES, drift_chain, host_case, host_chain, plan_spread

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mused_amd import matrix_operations as mo  # noqa: E402

CASES = [(s,) + t for t in TUPLES for s in SEEDS]
MAX_FLAGGED = 2   # of the 39 pairs


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_DEVICE = {}


def device_case(c):
    """One launch per case, shared by the tests: dict(info, plan, labels (through the public entry), fallbacks)."""
    if c not in _DEVICE:
        h = host_case(*c)
        dev = torch.device("cuda")
        raw = torch.from_numpy(h["new"].astype(np.int32)).to(dev).reshape(1, -1)
        prev = torch.from_numpy(h["prev"].astype(np.int32)).to(dev)
        matched, info, plans = mo.match_chain_launch(raw, prev, 3, want_plan=True)
        P, N = int(info[0, 0]), int(info[0, 1])
        before = mo.match_fallbacks
        labels = np.asarray(mo.match_clusters_on_device(h["prev"], h["new"], 3))
        _DEVICE[c] = dict(info=info[0].copy(), raw_labels=matched[0].cpu().numpy(),
                          plan=plans[0, :P * N].cpu().numpy().reshape(P, N) if P * N <= 65536 else None,
                          labels=labels, fallbacks=mo.match_fallbacks - before)
    return _DEVICE[c]


@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_pair_against_host_specification(c):
    h, d = host_case(*c), device_case(c)
    P, N, iters, feasible, flags, margin_bits, done = (int(x) for x in d["info"][:7])
    margin = float(np.array([margin_bits], dtype=np.int32).view(np.float32)[0])
    print(f"case {c}: P {P} N {N} iters {iters} (host {h.get('iters')}) feasible {feasible} flags {flags} "
          f"margin {margin:.3e} (host {h.get('margin')})")
    assert np.array_equal(d["labels"], h["labels"])            # flagged or not: a flagged pair comes back through the host
    assert (P, N) == (h["P"], h["N"])
    assert done == (flags == 0) and d["fallbacks"] == (flags != 0)
    if flags & ~(mo.MATCH_FLAG_SELECT | mo.MATCH_FLAG_STOP):
        pytest.fail(f"range / size flag {flags} on a pair within the kernel's limits")
    assert bool(feasible) == h["feasible"]
    if flags & mo.MATCH_FLAG_STOP:
        return   # the chain ended inside the iteration: feasibility was established, nothing else was written
    if not h["feasible"]:
        assert np.array_equal(d["raw_labels"], h["new"])
        return
    if flags == 0:
        assert iters == h["iters"]
        assert np.array_equal(d["raw_labels"], h["labels"])
        rel = float(np.max(np.abs(d["plan"] - h["plan"]) / h["plan"]))
        print(f"  plan: largest relative difference {rel:.3e}, bound {PLAN_FACTOR * plan_spread():.3e}")
        assert rel <= PLAN_FACTOR * plan_spread()
        assert margin == pytest.approx(h["margin"], rel=1e-5, abs=1e-30)


def test_flag_budget():
    flagged = [c for c in CASES if int(device_case(c)["info"][4]) != 0]
    print("flagged:", [(c, int(device_case(c)["info"][4])) for c in flagged])
    assert len(flagged) <= MAX_FLAGGED


def test_tensor_and_int64_inputs():
    h = host_case(1, 2000, 8, 6, .3)
    dev = torch.device("cuda")
    for dt in (torch.int32, torch.int64):
        out = mo.match_clusters_on_device(torch.from_numpy(h["prev"]).to(dev, dt), torch.from_numpy(h["new"]).to(dev, dt), 3)
        assert np.array_equal(np.asarray(out), h["labels"])
    new = torch.from_numpy(h["new"]).to(dev)
    assert mo.match_clusters_on_device(None, new, 3) is new
    inf = host_case(1, 64, 3, 5, .5)
    assert not inf["feasible"] and mo.match_clusters_on_device(inf["prev"], inf["new"], 3) is inf["new"]


def test_chain_in_one_launch_and_split():
    raw = drift_chain()
    ref = host_chain(raw)
    before = mo.match_fallbacks
    out = mo.match_chain_on_device(raw)
    assert np.array_equal(out, ref)
    W = raw.shape[1]
    head = mo.match_chain_on_device(raw[:2])
    tail = mo.match_chain_on_device(torch.from_numpy(raw[2:]).cuda(), prev0=head[W:])
    assert np.array_equal(np.concatenate([head, tail]), ref)
    assert mo.match_fallbacks == before   # none of these windows is near a decision
    # the launch itself: six windows done, windows 3 and 4 infeasible and passed through
    m, info, _ = mo.match_chain_launch(torch.from_numpy(raw.astype(np.int32)).cuda(), None, 3)
    assert info[:, 6].tolist() == [1] * 6 and info[:, 3].tolist() == [0, 1, 1, 0, 0, 1]
    assert np.array_equal(m.cpu().numpy().ravel(), ref)


def test_chain_falls_back_on_labels_and_sizes_beyond_the_kernel():
    raw = drift_chain(seed=1).astype(np.int64)
    big = raw.copy()
    big[2] = np.where(big[2] == 1, 5000, big[2])            # a label beyond 1023 in window 2
    before = mo.match_fallbacks
    assert np.array_equal(mo.match_chain_on_device(big), host_chain(big))
    # window 2 on the host, and window 3, whose previous labels hold the 5000 if it survives the matching
    assert 1 <= mo.match_fallbacks - before <= 2
    rng = np.random.default_rng(3)
    wide = np.stack([rng.integers(0, 8, 3000), rng.permutation(3000) % 300, rng.integers(0, 8, 3000)])   # N = 300 > 256
    before = mo.match_fallbacks
    assert np.array_equal(mo.match_chain_on_device(wide), host_chain(wide))
    assert mo.match_fallbacks - before >= 1
    m, info, _ = mo.match_chain_launch(torch.from_numpy(wide.astype(np.int32)).cuda(), None, 3)
    assert info[:, 6].tolist() == [1, 0, 0] and int(info[1, 4]) == mo.MATCH_FLAG_SIZE and int(info[1, 1]) == 300


@pytest.mark.parametrize("as_tensor", [False, True])
def test_out_of_range_label_in_a_window_without_previous(as_tensor):
    """Window 0 passes through when there is no previous window; the device copy holds 1024 for every label outside
    [0, 1024), so the kernel must flag that window too and the true values come from the host."""
    raw = drift_chain(seed=2).astype(np.int64)
    raw[0] = np.where(raw[0] == 0, 5000, np.where(raw[0] == 1, 70000, raw[0]))   # two distinct values beyond the range
    ref = host_chain(raw)
    assert set(ref[:raw.shape[1]]) >= {5000, 70000}
    before = mo.match_fallbacks
    out = mo.match_chain_on_device(torch.from_numpy(raw).cuda() if as_tensor else raw)
    assert np.array_equal(out, ref)
    assert mo.match_fallbacks - before >= 2   # window 0, and window 1 against its labels
    m, info, _ = mo.match_chain_launch(torch.from_numpy(np.minimum(raw, 1024).astype(np.int32)).cuda(), None, 3)
    assert info[:, 6].tolist() == [0] * 6 and int(info[0, 4]) == mo.MATCH_FLAG_RANGE
    one = mo.match_clusters_on_device(raw[0], raw[1], 3)          # out-of-range previous labels: the host's answer
    assert np.array_equal(np.asarray(one), np.asarray(mo.match_clusters(raw[0], raw[1], "pot", 3)))


def test_pipeline_approach_pot(monkeypatch):
    from mused_amd.pipeline import StreamPipeline, process_streaming_data

    g = load_golden("c1_stream_blob_s0")
    mods, labels, (n, d, W, ell, k, seed) = regen_inputs(g)
    raws = {}
    for approach in ("sSVDMC", "sSVDMC_pot"):
        with StreamPipeline(W, ell, k, seed, approach) as pipe:
            pipe.run(mods, labels)
            raws[approach] = np.array([t["raw"] for t in pipe.trace])
    assert np.array_equal(raws["sSVDMC"], raws["sSVDMC_pot"])
    ref = host_chain(raws["sSVDMC"])
    args = ({}, mods, [""] * len(mods), W, ell, k, len(np.unique(labels)), seed, "sSVDMC_pot", labels, 1, 0.0, "types", False,
            1.5, 2)
    dev_out = process_streaming_data(*args)["all_clusters"]
    assert np.array_equal(np.asarray(dev_out), ref)
    monkeypatch.setenv("MUSED_MATCH", "host")
    host_out = process_streaming_data(*args)["all_clusters"]
    assert np.array_equal(np.asarray(host_out), ref)
