"""On the GPU: SeqBasedSWFD at l = 128 with rotations whose buffers are partly empty -- d = 40 (at most 40 kept rows: every
Gram matrix of order 256 is solved at an order of at most 168, csrc/trd.hip `offs`) and d = 300 (kept rows up to 127: orders
from 128 to 255 share a launch; a rotation never fills all 256 rows, the shrink always drops direction l - 1) -- with an epoch end that is no multiple of l (N = 600: 88 pending rows).  Two epochs of a seeded
Gaussian stream with a few heavy directions, one lane and three lock-step lanes, against oracle/swfd_oracle.py at the
tolerances of the l = 128 comparisons of tests/test_gpu_path.py (1e-8 sigma_1 / 1e-8 sigma_1^2)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, ELL, LANES = 600, 128, 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def streams(d):
    """LANES streams of 2 N rows: unit Gaussian noise plus five heavy directions of decaying weight."""
    rng = np.random.default_rng(100 + d)
    out = []
    for _ in range(LANES):
        dirs = np.linalg.qr(rng.standard_normal((d, 5)))[0].T
        coef = rng.standard_normal((2 * N, 5)) * np.array([12.0, 8.0, 5.0, 3.0, 2.0])
        out.append(rng.standard_normal((2 * N, d)) + coef @ dirs)
    X = np.stack(out)
    return X, float((X ** 2).sum(2).max())


@pytest.mark.parametrize("d", [40, 300])
def test_partly_empty_rotations_match_the_oracle_and_lanes_equal_singles(d):
    from mused_amd.swfd import SeqBasedSWFD as Dev
    from oracle.swfd_oracle import SeqBasedSWFD as Ora

    X, R = streams(d)
    lanes = Dev(N=N, R=R, d=d, sketch_dim=ELL, lanes=LANES)
    singles = [Dev(N=N, R=R, d=d, sketch_dim=ELL) for _ in range(LANES)]
    oracle = Ora(N=N, R=R, d=d, sketch_dim=ELL)     # (of lane 0: the other lanes are held to their singles, bit for bit)
    Xd = torch.from_numpy(X).cuda()
    t = 0
    for step in [250, 350, 600]:   # ragged blocks; get() at both epoch ends
        lanes.fit_lanes(Xd[:, t:t + step])
        for b in range(LANES):
            singles[b].fit(Xd[b, t:t + step])
        oracle.fit(X[0, t:t + step])
        t += step
        if t % N:
            continue
        Bl, sl, ll, dl = lanes.get()            # (get() raises on a non-zero status word)
        for b in range(LANES):
            Bs, ss, ls, ds = singles[b].get()
            assert int(ll[b]) == ls and np.array_equal(Bl[b], Bs) and np.array_equal(sl[b], ss) and dl[b] == ds, (t, b)
            if b == 0:
                Bo, so, lo, do = oracle.get()
                assert ls == lo, (t, ls, lo)
                np.testing.assert_allclose(ss, so, rtol=0, atol=1e-8 * so[0], err_msg=f"t={t}")
                np.testing.assert_allclose(Bs.T @ Bs, Bo.T @ Bo, rtol=0, atol=1e-8 * so[0] ** 2, err_msg=f"t={t}")
                assert abs(ds - do) <= 1e-8 * so[0] ** 2
    import ctypes as C

    from mused_amd import _lib

    st = (C.c_longlong * 18)()     # {rotations, solves, solves by order: bucket b = (16 b, 16 b + 16]}
    fn = _lib.lib().mused_swfd_debug_orders
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p]
    assert fn(singles[0]._h, st) == 1
    assert st[0] == 10 and st[1] > 0 and sum(st[2:18]) == st[1]         # 5 rotations per epoch
    if d == 40:
        assert sum(st[2 + 11:18]) == 0                                  # none above order 40 + 128 <= 176
    else:                                                               # the mixture is there: orders above 240 and below
        assert st[2 + 15] > 0 and sum(st[2:2 + 14]) > 0
    lanes.close()
    for sk in singles:
        sk.close()
