"""On the GPU: the Lloyd kernels (csrc/kmeans.hip) through mused_kmeans_lloyd itself against the high-precision reference
of tests/lloyd_cases.py -- labels, the report {iterations, stop code, empty flag}, the centres, every E/M-step kernel the
library can pick (64 / 32 / 16 rows per sub-tile and the row-per-thread kernel, the latter also forced on the tiled cases in
a child process and compared bit for bit), the max_iter and tolerance exits, the empty-cluster flag with the wrapper's
fallback, and the argument checks."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lloyd_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MUSED_ERR_ARG = -1
LAB_SENT = -7
CEN_SENT = -12345.678
GUARD = 64
INFO_SENT = -9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def P(t):
    return C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # a copy: the cases' arrays are read-only


class Buffers:
    """The device arguments of one call: rows in a pitched buffer whose padding is NaN, a workspace of 0xFF bytes, labels
    and centres with a band of sentinels behind them."""

    def __init__(self, X, mean, C0, ld=0):
        from mused_amd import _lib

        self.n, self.d = X.shape
        self.k = len(C0)
        self.ld = ld or self.d
        buf = np.full((self.n, self.ld), np.nan)
        buf[:, : self.d] = X
        self.X = dev(buf)
        self.mean = dev(mean)
        self.cen = torch.full((self.k * self.d + GUARD,), CEN_SENT, dtype=torch.float64, device="cuda")
        self.cen[: self.k * self.d] = dev(C0).reshape(-1)
        self.lab = torch.full((self.n + GUARD,), LAB_SENT, dtype=torch.int32, device="cuda")
        self.ws_bytes = int(_lib.lib().mused_kmeans_ws_bytes(self.n, self.d, self.k))
        self.ws = torch.full((self.ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda")
        self.info = (C.c_int * 4)(*[INFO_SENT] * 4)

    def args(self, tol, max_iter, **over):
        a = dict(X=P(self.X), ld=self.ld, n=self.n, d=self.d, k=self.k, mean=P(self.mean), cen=P(self.cen), tol=tol,
                 max_iter=max_iter, lab=P(self.lab), info=self.info, ws=P(self.ws), ws_bytes=self.ws_bytes, st=S())
        a.update(over)
        return tuple(a.values())

    def read(self):
        torch.cuda.synchronize()
        lab, cen = self.lab.cpu().numpy(), self.cen.cpu().numpy()
        assert (lab[self.n:] == LAB_SENT).all(), "labels written past n"
        assert (cen[self.k * self.d:] == CEN_SENT).all(), "centres written past k * d"
        return lab[: self.n].copy(), cen[: self.k * self.d].reshape(self.k, self.d).copy(), list(self.info)


def run_case(c):
    """mused_kmeans_lloyd on a case -> (labels, centres, info), the guard bands checked."""
    from mused_amd import _lib

    X, mean, C0, tol = lc.inputs(c)
    b = Buffers(X, mean, C0, c.ld)
    _lib.call("mused_kmeans_lloyd", *b.args(tol, c.max_iter))
    return b.read()


_RUNS = {}


def first_run(c):
    """The case's first run in this process, kept for the tests that compare with it."""
    if c not in _RUNS:
        _RUNS[c] = run_case(c)
    return _RUNS[c]


def centre_bound(c):
    """Per element: a sequential fp64 sum of at most n terms times a reciprocal, plus the centring, against the same in
    extended precision -- (n + 8) 2^-53 max |X - mean|."""
    X, mean, _, _ = lc.inputs(c)
    return (c.n + 8) * 2.0 ** -53 * float(np.abs(X - mean).max())


def assert_matches_reference(c, got):
    lab, cen, info = got
    r = lc.reference(c)
    print(f"{c.name}: info {info} reference {[r.iters, r.code, r.empty, 0]} labels differing "
          f"{np.count_nonzero(lab != r.labels)} centres off by {float(np.abs(cen - r.centers).max()):.3g} "
          f"(bound {centre_bound(c):.3g})")
    assert info == [r.iters, r.code, r.empty, 0]
    assert np.array_equal(lab, r.labels), f"{np.count_nonzero(lab != r.labels)} labels differ from the reference"
    assert float(np.abs(cen - r.centers).max()) <= centre_bound(c)


# ---- the table ----------------------------------------------------------------------------------------------------
def test_every_kernel_occurs_in_the_table():
    from mused_amd import _lib

    got = {_lib.lib().mused_kmeans_assign_rows(c.d, c.k) for c in lc.TABLE}
    assert got == {64, 32, 16, 0}


@pytest.mark.parametrize("c", lc.TABLE, ids=[c.name for c in lc.TABLE])
def test_table_case_is_the_references(c):
    from mused_amd import _lib

    assert _lib.lib().mused_kmeans_assign_rows(c.d, c.k) == c.rows
    got = first_run(c)
    assert_matches_reference(c, got)
    again = run_case(c)
    assert np.array_equal(again[0], got[0]) and again[2] == got[2]
    assert np.array_equal(bits(again[1]), bits(got[1])), "a second call gave other bits"


# ---- the derived cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", lc.MAX_ITER, ids=[c.name for c in lc.MAX_ITER])
def test_max_iter_exit(c):
    r = lc.reference(c)
    got = first_run(c)
    assert got[2][:2] == ([c.max_iter, 0] if c.max_iter < 8 else [8, 1])
    assert_matches_reference(c, got)
    assert r.iters == got[2][0]


def test_forced_tolerance_exit():
    got = first_run(lc.FORCED_TOL)
    assert got[2][:2] == [lc.FORCED_TOL_ITER, 2]
    assert_matches_reference(lc.FORCED_TOL, got)


@pytest.mark.parametrize("c", lc.EMPTY, ids=[c.name for c in lc.EMPTY])
def test_empty_cluster_raises_the_flag(c):
    assert lc.reference(c).empty == 1
    _, _, info = run_case(c)
    assert info[2] == 1


# ---- plain against tiled ------------------------------------------------------------------------------------------
def _child(out):
    """In a child process started with MUSED_KMEANS_ASSIGN=p: the tiled cases on the row-per-thread kernel -> out (.npz)."""
    from mused_amd import _lib

    res = {}
    for c in lc.TILED:
        lab, cen, info = run_case(c)
        res[c.name + "_rows"] = np.array(_lib.lib().mused_kmeans_assign_rows(c.d, c.k))
        res[c.name + "_labels"], res[c.name + "_centers"], res[c.name + "_info"] = lab, cen, np.array(info)
    np.savez(out, **res)


def test_plain_kernel_gives_the_tiled_kernels_bits(tmp_path):
    """csrc/kmeans.hip promises that the staged kernels are bit-identical to the row-per-thread one (same sums in the same
    order).  The switch is read once per process, so the plain runs happen in a fresh child."""
    out = str(tmp_path / "plain.npz")
    env = dict(os.environ, MUSED_KMEANS_ASSIGN="p")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    z = np.load(out)
    for c in lc.TILED:
        lab, cen, info = first_run(c)
        assert int(z[c.name + "_rows"]) == 0, "the child did not run the row-per-thread kernel"
        assert list(z[c.name + "_info"]) == info, c.name
        assert np.array_equal(z[c.name + "_labels"], lab), c.name
        assert np.array_equal(bits(z[c.name + "_centers"]), bits(cen)), f"{c.name}: the centres differ in their bits"


# ---- the wrapper --------------------------------------------------------------------------------------------------
# what the seed kernel says about the 3-distinct-points input: once three distinct centres are chosen every potential is
# zero and every further candidate ties, so the kernel flags the window and the host-seeded path runs
SEED_KERNEL_FLAGS_THREE_POINTS = True


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_wrapper_leaves_the_device_path_on_an_empty_cluster(seed, monkeypatch):
    from sklearn.cluster import KMeans

    from mused_amd import _lib
    from mused_amd import matrix_operations as mo

    X = lc.three_points(seed)
    infos, host_seeded, sk_calls = [], [], []
    real_call, real_seeded, real_sk = _lib.call, mo._km_host_seeded, mo.perform_clustering

    def call(name, *args):
        real_call(name, *args)
        if name == "mused_kmeans_lloyd":
            infos.append(list(args[10]))

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(mo, "_km_host_seeded", lambda *a: host_seeded.append(1) or real_seeded(*a))
    monkeypatch.setattr(mo, "perform_clustering", lambda *a: sk_calls.append(1) or real_sk(*a))
    monkeypatch.delenv("MUSED_KMEANS_SEED", raising=False)
    before = mo.km_fallbacks
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # scikit-learn: fewer distinct points than clusters
        got = mo.perform_clustering_on_device(torch.from_numpy(X).cuda(), 5, seed)
        want = KMeans(5, random_state=seed).fit_predict(X)
    print(f"seed {seed}: lloyd info {infos} host-seeded {host_seeded} scikit-learn calls {sk_calls}")
    assert len(infos) == 1 and infos[0][2] == 1, "mused_kmeans_lloyd ran once and reported an empty cluster"
    assert sk_calls == [1], "the labels came from perform_clustering"
    assert np.array_equal(got, want)
    # one fallback either way: the empty cluster on the device-seeded path, or the seed kernel's flag before it (the empty
    # cluster met on the host-seeded path after that is not counted again)
    assert mo.km_fallbacks == before + 1
    assert host_seeded == ([1] if SEED_KERNEL_FLAGS_THREE_POINTS else [])


# ---- rejected arguments -------------------------------------------------------------------------------------------
def test_bad_arguments_rejected_without_launch():
    """k d = 8193, k > n, ld < d and a workspace one byte short: MUSED_ERR_ARG, and labels, centres and info untouched."""
    from mused_amd import _lib

    lib = _lib.lib()
    rng = np.random.default_rng(0)
    for n, d, k, over, msg in [(4, 8193, 1, {}, b"k * d must be <= 8192"), (3, 4, 4, {}, b"bad arguments"),
                               (20, 6, 3, {"ld": 5}, b"bad arguments"), (300, 6, 3, {"ws_bytes": -1}, b"workspace too small")]:
        X, C0 = rng.standard_normal((n, d)), rng.standard_normal((k, d))
        b = Buffers(X, X.mean(axis=0), C0)
        if "ws_bytes" in over:
            over = {"ws_bytes": b.ws_bytes - 1}
        assert lib.mused_kmeans_lloyd(*b.args(1e-4, 300, **over)) == MUSED_ERR_ARG
        assert msg in lib.mused_last_error()
        lab, cen, info = b.read()
        assert (lab == LAB_SENT).all() and info == [INFO_SENT] * 4
        assert np.array_equal(bits(cen), bits(C0))


if __name__ == "__main__":
    _child(sys.argv[1])
