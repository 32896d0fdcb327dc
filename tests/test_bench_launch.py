"""`python bench.py --gpus N` starts its N ranks itself (a child `python -m torch.distributed.run`, one rank per GPU): the
launch path on the CPU (gloo, no GPU touched) and, on a GPU box, a whole two-rank run of the small workload with both ranks
on the one device (gloo collectives) -- the path the driver's N > 1 runs take, minus RCCL."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, lines


def test_bench_starts_its_own_ranks():
    p, lines = _run(["--gpus", "2", "--launch-check"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["ranks_counted"] == 2


def test_bench_rejects_a_world_size_that_contradicts_gpus():
    p, lines = _run(["--gpus", "2", "--launch-check"], {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and not lines


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_without_an_external_launcher():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p, lines = _run(["--gpus", "2", "--workload", "c1", "--steps", "4", "--warmup", "2", "--no-cpu-baseline", "--no-single-lane"],
                    {"MUSED_DIST_BACKEND": "gloo", "MUSED_FORCE_DEVICE": "0"}, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["rccl_ranks"] == 2 and res["config"]["collective_backend"] == "gloo"
    assert res["value"] > 0


def test_bench_output_dump_keeps_a_fixed_sample_within_its_budget(tmp_path):
    """--dump-outputs: float64 files, at most DUMP_BYTES in all, the same sample of an oversized array on every call."""
    code = ("import sys, numpy as np, bench; bench.DUMP_BYTES = 1 << 20; "
            "r = np.random.default_rng(1); "
            "bench.dump_outputs(sys.argv[1], {'big': r.standard_normal((4, 64, 2048)), 'small': np.arange(10, dtype=np.int64)})")
    for sub in ("a", "b"):
        p = subprocess.run([sys.executable, "-c", code, str(tmp_path / sub)], cwd=ROOT, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
    import numpy as np

    files = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert files == ["big.npy", "big_index.npy", "small.npy"]
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= (1 << 20) + 3 * 256
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b)
    big, idx = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big_index.npy").astype(np.int64)
    full = np.random.default_rng(1).standard_normal((4, 64, 2048))
    assert big.shape[:2] == (4, 64) and 0 < big.shape[2] < 2048 and np.array_equal(big, full[..., idx])
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), np.arange(10))


@pytest.mark.gpu
def test_bench_dumps_the_last_step_and_keeps_the_extras_behind_full(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import numpy as np

    runs = {}
    for tag, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        p, lines = _run(["--workload", "c1", "--steps", "6", "--warmup", "2", "--dump-outputs", str(tmp_path / tag)] + extra,
                        timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        assert len(lines) == 1
        runs[tag] = json.loads(lines[0])
    for res in runs.values():
        assert res["steps"] == 6 and res["ms_per_step"] > 0 and res["value"] > 0
        assert res["unit"] == "rows/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert runs["plain"]["roofline"] is None and runs["plain"]["single_lane"] is None
    assert runs["full"]["roofline"] is not None and runs["full"]["single_lane"] is not None
    assert runs["full"]["stages_ms"]["rsvd_ms"] > 0
    assert runs["plain"]["config"]["labels_sha16"] == runs["full"]["config"]["labels_sha16"]
    W = runs["plain"]["config"]["W"]
    for name in ("labels", "labels_last_step", "eigenstep_sigma_last_step", "sketch", "sketch_sigma", "sketch_level_delta"):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.dtype == np.float64 and np.isfinite(a).all()
        assert np.array_equal(a, b), name                     # the same inputs and the same path: the same outputs
    assert np.load(tmp_path / "plain" / "labels.npy").shape == (6 * W,)
    assert np.load(tmp_path / "plain" / "sketch.npy").shape[1:] == (16, 64)
