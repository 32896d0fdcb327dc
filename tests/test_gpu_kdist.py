"""mused_kth_distance and mused_eps_knee (csrc/kdist.hip) through the C ABI: the k-th squared distances against the NumPy
rule (mused_amd/kdist.py) and against scikit-learn's NearestNeighbors, both within kdist.kd2_bound; the knee entry against
kdist.knee / eps_from_curve applied to THE DEVICE'S OWN kd2, bit for bit; the flags, reproducibility, a permutation of the
rows, the workspace, a stream of the caller's.  The cases and why they are the ones: tests/kdist_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import kdist_cases as kc
from mused_amd import kdist

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 64
FLAG_NONFINITE, FLAG_FLAT = 2, 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _pitched(X, pitch):
    """X on the device with rows `pitch` doubles apart; the padding holds NaN, which nothing may read."""
    buf = torch.full((len(X), pitch), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, : X.shape[1]] = torch.tensor(X, device="cuda")
    return buf


def run_knee(kd2_dev, n, sp):
    """mused_eps_knee on a device array: ((i*, nxt, v[i*], v[nxt], eps, flags), the sorted curve as NumPy); a canary behind
    the workspace, the output prefilled."""
    from mused_amd import _lib
    from mused_amd.engine import ptr

    nb = int(_lib.lib().mused_eps_knee_ws_bytes(n))
    assert nb == kc.ws_knee(n)                                                     # the query is exact
    ws = torch.full((nb + CANARY,), 0xa5, dtype=torch.uint8, device="cuda")
    out = torch.full((48,), 0x77, dtype=torch.uint8, device="cuda")
    _lib.call("mused_eps_knee", ptr(kd2_dev), n, ptr(out), ptr(ws), nb, sp)
    torch.cuda.synchronize()
    assert (ws[nb:] == 0xa5).all()
    h = out.cpu().numpy()
    i, f = h.view(np.int64), h.view(np.float64)
    return (int(i[0]), int(i[1]), float(f[2]), float(f[3]), float(f[4]), int(i[5])), ws[: 8 * n].view(torch.float64).cpu().numpy()


def run(X, k, ld=None, stream=None):
    """Both entries once: (kd2, info, knee tuple, sorted curve) as NumPy, outputs prefilled with -7 and a canary behind each
    workspace."""
    from mused_amd import _lib
    from mused_amd.engine import ptr

    n, d = X.shape
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        Xd = _pitched(X, ld or d)
        nb = int(_lib.lib().mused_kth_distance_ws_bytes(n, k))
        assert nb == kc.ws_kth(n, k)                                               # the query is exact
        ws = torch.full((nb + CANARY,), 0xa5, dtype=torch.uint8, device="cuda")   # the workspace carries nothing
        kd2 = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        sp = C.c_void_p(st.cuda_stream)
        _lib.call("mused_kth_distance", ptr(Xd), n, d, Xd.stride(0), k, ptr(kd2), ptr(info), ptr(ws), nb, sp)
        st.synchronize()
        assert (ws[nb:] == 0xa5).all()                                             # nothing written behind ws_bytes
        info_h = info.cpu().numpy()
        if info_h[0]:
            return kd2.cpu().numpy(), info_h, None, None
        knee, curve = run_knee(kd2, n, sp)
        return kd2.cpu().numpy(), info_h, knee, curve


@functools.lru_cache(maxsize=None)
def device_result(name):
    c = kc.case(name)
    return run(c.X, c.k, c.ld)


def check_knee(kd2, knee, curve):
    """The knee entry against the NumPy rule on the same kd2: the curve, the indices and eps, bit for bit."""
    v = np.sort(np.sqrt(kd2))
    assert curve.tobytes() == v.tobytes()
    if v[-1] == v[0]:
        assert knee[5] == FLAG_FLAT and knee[:2] == (-1, -1) and all(x != x for x in knee[2:5])
        with pytest.raises(ValueError, match="flat"):
            kdist.knee(v)
        return
    i, nxt = kdist.knee(v)
    assert knee[5] == 0 and knee[:2] == (i, nxt)
    assert np.array(knee[2:5]).tobytes() == np.array([v[i], v[nxt], kdist.eps_from_curve(v)]).tobytes()


@pytest.mark.parametrize("case", kc.CASES, ids=kc.CASE_IDS)
def test_every_case(case):
    n = case.X.shape[0]
    kd2, info, knee, curve = device_result(case.name)
    assert tuple(info) == (0, kc.slices(n), 8 if case.k <= 8 else 64, 0)
    bound = case.bound
    err_sk = np.abs(kd2 - case.sklearn)
    rows = np.arange(n) if case.rows is None else case.rows
    err_rule = np.abs(kd2[rows] - case.rule)
    print(f"{case.name}: largest |device - rule| / bound {(err_rule / bound[rows]).max():.4f}, |device - sklearn| / bound "
          f"{(err_sk / bound).max():.4f}, knee {knee}")
    assert (kd2 >= 0).all()
    assert (err_rule <= bound[rows]).all()
    assert (err_sk <= bound).all()
    check_knee(kd2, knee, curve)


def test_exact_inputs_give_exact_values():
    """Integer ramp and eighths: every product and sum is exact, so the device equals the rule bit for bit -- in particular
    the last row tile of the ramp, which sees every distance descend (all entries pass the filter), loses none."""
    for name in ("ramp_n1000_k64", "ramp_n1000_k8", "two_point_blobs_k2"):
        c = kc.case(name)
        assert device_result(name)[0].tobytes() == c.rule.tobytes()
    i = np.arange(1000)
    for k, name in ((64, "ramp_n1000_k64"), (8, "ramp_n1000_k8")):
        lo = np.minimum(i, 999 - i)               # rows nearer on the short side
        want = np.where(lo >= k // 2, k // 2, k - 1 - lo).astype(np.float64) ** 2
        assert (device_result(name)[0] == want).all()
    kd2 = device_result("two_point_blobs_k2")[0]
    assert (kd2 == 0.0).sum() == 150 and (kd2 == 0.015625).sum() == 150


def test_k_one_is_all_zeros_and_flat():
    for name in ("n1_d3_k1", "n128_d3_k1"):
        kd2, info, knee, _ = device_result(name)
        assert (kd2 == 0.0).all() and info[0] == 0 and knee[5] == FLAG_FLAT


@pytest.mark.parametrize("value", [float("nan"), float("inf"), 1e200], ids=["nan", "inf", "overflowing_norm"])
@pytest.mark.parametrize("k", [3, 20])
def test_a_non_finite_row_sets_the_flag_and_writes_nothing(value, k):
    X = kc.gaussian(300, 4, 40).copy()
    X[171, 2] = value
    kd2, info, _, _ = run(X, k)
    assert info[0] == FLAG_NONFINITE and (kd2 == -7.0).all()


@pytest.mark.parametrize("name", ["n257_d3_k2_pitch5", "n2000_d51_k64", "n5000_d50_k9", "ramp_n1000_k64"])
def test_two_calls_give_the_same_bytes(name):
    c = kc.case(name)
    first, again = device_result(name), run(c.X, c.k, c.ld)
    assert first[0].tobytes() == again[0].tobytes() and first[2] == again[2] and first[3].tobytes() == again[3].tobytes()


@pytest.mark.parametrize("name", ["n257_d3_k2_pitch5", "n2000_d51_k64", "two_point_blobs_k2"])
def test_permuted_rows_give_permuted_values(name):
    c = kc.case(name)
    p = np.random.default_rng(5).permutation(c.X.shape[0])
    kd2, info, knee, curve = run(c.X[p], c.k, c.ld)
    base = device_result(name)[0]
    assert info[0] == 0 and (np.abs(kd2 - base[p]) <= c.bound[p]).all()
    check_knee(kd2, knee, curve)               # the rule on THIS run's values
    # the sorted curves agree within the bound of the rows they come from: rank by rank, the largest bound covers it
    assert (np.abs(np.sort(kd2) - np.sort(base)) <= c.bound.max()).all()


def test_on_a_stream_of_the_callers():
    c = kc.case("n2000_d50_k2_blobs")
    got = run(c.X, c.k, c.ld, stream=torch.cuda.Stream())
    base = device_result(c.name)
    assert got[0].tobytes() == base[0].tobytes() and got[2] == base[2]


def test_workspace_queries_and_refusals():
    from mused_amd import _lib
    from mused_amd._lib import MusedError
    from mused_amd.engine import ptr

    L = _lib.lib()
    q, qk = L.mused_kth_distance_ws_bytes, L.mused_eps_knee_ws_bytes
    assert q(0, 1) == -1 and q((1 << 19) + 1, 2) == -1 and q(10, 0) == -1 and q(10, 11) == -1 and q(100, 65) == -1
    assert q(1 << 19, 64) == kc.ws_kth(1 << 19, 64) and q(64, 64) == kc.ws_kth(64, 64)
    assert all(q(n, k) == kc.ws_kth(n, k) for n in range(1, 40000, 1237) for k in (1, 8, 9, 64) if k <= n)
    assert qk(0) == -1 and qk((1 << 19) + 1) == -1 and qk(1 << 19) == kc.ws_knee(1 << 19)
    n, d, k = 200, 6, 4
    Xd = torch.tensor(kc.gaussian(n, d, 41), device="cuda")
    kd2 = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    need = kc.ws_kth(n, 64)
    ws = torch.full((max(need, kc.ws_knee(n)),), 0xa5, dtype=torch.uint8, device="cuda")
    out = torch.full((48,), 0x77, dtype=torch.uint8, device="cuda")
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # ws_bytes - 1, a pitch below d, n, d and k outside the domain: refused with an error code, nothing launched
    for n_, d_, ld_, k_, nb in ((n, d, d, k, kc.ws_kth(n, k) - 1), (n, d, d - 1, k, need), (0, d, d, k, need), (n, 0, d, k, need),
                                (n, d, d, 0, need), (n, d, d, 65, need), (50, d, d, 51, need)):
        with pytest.raises(MusedError):
            _lib.call("mused_kth_distance", ptr(Xd), n_, d_, ld_, k_, ptr(kd2), ptr(info), ptr(ws), nb, sp)
    for n_, nb in ((n, kc.ws_knee(n) - 1), (0, kc.ws_knee(n))):
        with pytest.raises(MusedError):
            _lib.call("mused_eps_knee", ptr(kd2), n_, ptr(out), ptr(ws), nb, sp)
    torch.cuda.synchronize()
    assert (kd2 == -7.0).all() and (info == -7).all() and (ws == 0xa5).all() and (out == 0x77).all()


# ---- the knee entry on curves of its own ------------------------------------------------------------------------------------
def _knee_of(kd2):
    d = torch.tensor(np.asarray(kd2, dtype=np.float64), device="cuda")
    return run_knee(d, len(kd2), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_knee_sorts_full_bit_patterns():
    """Values over 200 binades with equal high words and equal low words among them, zeros and repeats: both radix rounds
    matter, and 5,000 values take several sort tiles."""
    rng = np.random.default_rng(9)
    a = rng.random(5000) ** 8 * 1e12
    a[::7] = a[3]
    a[1::11] = 0.0
    a[2::13] = np.ldexp(1.0, rng.integers(-300, 300, size=len(a[2::13])))     # low word 0
    a[5::17] = np.ldexp(1.0 + 2.0 ** -52 * rng.integers(1, 1 << 20, size=len(a[5::17])), 40)   # one high word, low words differ
    knee, curve = _knee_of(a)
    check_knee(a, knee, curve)


def test_knee_first_maximum_on_a_plateau():
    knee, curve = _knee_of(np.array([0.0, 0.0, 1.0, 2.0, 4.0]) ** 2)
    assert knee == (1, 2, 0.0, 1.0, 0.5, 0) and list(curve) == [0.0, 0.0, 1.0, 2.0, 4.0]
    # 3,000 equal maxima spread over every thread of the reduction: g = 0 at both ends and on the diagonal in between
    n = 3001
    knee, _ = _knee_of((np.arange(n) / 8.0) ** 2)
    assert knee[:2] == (0, 1) and knee[5] == 0
    knee, _ = _knee_of(np.array([9.0, 4.0]))
    assert knee == (0, 1, 2.0, 3.0, 2.5, 0)


def test_knee_flags():
    for bad in (-1.0, float("nan"), float("inf")):
        a = np.arange(300, dtype=np.float64)
        a[123] = bad
        assert _knee_of(a)[0][5] & FLAG_NONFINITE
    assert _knee_of(np.full(300, 2.5))[0][5] == FLAG_FLAT
    assert _knee_of(np.array([0.0, -0.0, 0.0]))[0][5] == FLAG_FLAT
