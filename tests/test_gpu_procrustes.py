"""csrc/procrustes.hip against scipy.linalg.orthogonal_procrustes.

One tolerance, per input: max |R_device - R_scipy| <= 4 u(A, B), u = 2^-52 (r + sqrt(m)) | |A|^T |B| |_F / sigma_r(A^T B)
(mused_amd.procrustes.unit).  Orthogonality max |R^T R - I| <= 8 r 2^-52, scale within r 2^-50 relative, two runs the same
bits.  r: 1 (trivial), 2, 3, 7 (odd round-robin, a bye), 63 / 64 / 65 (around a wave), 127 / 128 (the LDS ceiling);
m: r, r + 1, 257 (one row past a split-K chunk), 1,000.  Every input has sigma_r / sigma_1 = 1 / 16 or more: far from the flag."""
import functools

import numpy as np
import pytest
from scipy.linalg import orthogonal_procrustes

import procrustes_cases as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RS = [1, 2, 3, 7, 63, 64, 65, 127, 128]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ms(r):
    return sorted({m for m in (r, r + 1, 257, 1000) if m >= r})


@functools.lru_cache(maxsize=None)
def _case(m, r):
    """(A, B, SciPy's R, SciPy's scale, 4 u), computed once and left unchanged."""
    A, B, _ = pc.pair(m, r, 1000 * r + m, cond=16.0, det=-1 if r % 2 else None)
    R, scale = orthogonal_procrustes(A, B)
    from mused_amd import procrustes as pr

    R.setflags(write=False)
    return A, B, R, scale, 4.0 * pr.unit(A, B)


def _assert_matches(R, scale, ref, r):
    _, _, R_ref, scale_ref, tol = ref
    share = np.abs(R - R_ref).max() / tol
    print(f"r={r} m={ref[0].shape[0]} share of 4u = {share:.4f}")
    assert share <= 1.0
    assert np.abs(R.T @ R - np.eye(r)).max() <= 8 * r * 2.0 ** -52
    assert abs(scale - scale_ref) <= r * 2.0 ** -50 * scale_ref


@pytest.mark.parametrize("r", RS)
def test_kernel_matches_scipy(r):
    from mused_amd import matrix_operations as mo

    before = mo.procrustes_fallbacks
    for m in _ms(r):
        ref = _case(m, r)
        Ad, Bd = torch.from_numpy(ref[0]).cuda(), torch.from_numpy(ref[1]).cuda()
        R, scale = mo.orthogonal_procrustes_on_device(Ad, Bd)
        assert R.is_cuda and scale.is_cuda and R.shape == (r, r) and scale.dim() == 0
        R2, scale2 = mo.orthogonal_procrustes_on_device(Ad, Bd)
        assert torch.equal(R, R2) and torch.equal(scale, scale2)          # two runs: the same bits
        _assert_matches(R.cpu().numpy(), float(scale), ref, r)
    assert mo.procrustes_fallbacks == before


@pytest.mark.parametrize("r", [3, 64, 127])
def test_pitched_and_offset_views(r):
    from mused_amd import matrix_operations as mo

    m = 257
    ref = _case(m, r)
    rng = np.random.default_rng(1)
    bigA = torch.from_numpy(rng.standard_normal((m + 5, r + 3))).cuda()
    bigB = torch.from_numpy(rng.standard_normal((m + 9, r + 8))).cuda()
    bigA[3:3 + m, :r] = torch.from_numpy(ref[0]).cuda()
    bigB[9:, 2:2 + r] = torch.from_numpy(ref[1]).cuda()
    Av, Bv = bigA[3:3 + m, :r], bigB[9:, 2:2 + r]                         # lda = r + 3, ldb = r + 8, row and column offsets
    assert Av.stride(0) == r + 3 and Bv.stride(0) == r + 8
    before = mo.procrustes_fallbacks
    R, scale = mo.orthogonal_procrustes_on_device(Av, Bv)
    assert mo.procrustes_fallbacks == before
    _assert_matches(R.cpu().numpy(), float(scale), ref, r)
    Rc, _ = mo.orthogonal_procrustes_on_device(torch.from_numpy(ref[0]).cuda(), torch.from_numpy(ref[1]).cuda())
    assert torch.equal(R, Rc)                                             # the pitch does not reach the bits


def test_numpy_inputs_are_uploaded():
    from mused_amd import matrix_operations as mo

    ref = _case(257, 7)
    R, scale = mo.orthogonal_procrustes_on_device(ref[0], ref[1])
    _assert_matches(R.cpu().numpy(), float(scale), ref, 7)


def test_r_129_goes_to_the_host():
    from mused_amd import matrix_operations as mo

    A, B, _ = pc.pair(300, 129, 5, cond=16.0)
    before = mo.procrustes_fallbacks
    R, scale = mo.orthogonal_procrustes_on_device(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
    assert mo.procrustes_fallbacks == before + 1
    R_ref, scale_ref = orthogonal_procrustes(A, B)
    assert np.array_equal(R.cpu().numpy(), R_ref) and float(scale) == scale_ref


def test_entry_rejects_r_129_before_any_launch():
    import ctypes as C

    from mused_amd import _lib

    L = _lib.lib()
    assert L.mused_procrustes_ws_bytes(300, 129) == -1 and L.mused_procrustes_ws_bytes(0, 4) == -1
    x = torch.zeros(8, dtype=torch.float64, device="cuda")
    p = C.c_void_p(x.data_ptr())
    assert L.mused_procrustes(p, 129, p, 129, 300, 129, p, p, p, p, 64, None) == -4          # MUSED_ERR_UNSUPPORTED
    assert L.mused_svd_jacobi_small(p, 129, 129, p, p, p, None) == -4
    assert L.mused_procrustes_apply(p, 129, 4, 129, p, p, 129, None, 0, 0, None, p, None) == -4
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0                                                           # nothing ran


@pytest.mark.parametrize("name", ["m_below_r", "zero_column"])
def test_flagged_inputs_reach_scipy_and_are_counted(name):
    from mused_amd import matrix_operations as mo
    from mused_amd import procrustes as pr

    A, B = pc.degenerate()[name]
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    _, _, info, _ = mo.procrustes_launch(Ad, Bd, torch.cuda.current_stream())
    assert int(info.cpu()[0]) & pr.FLAG_ILLCOND
    before = mo.procrustes_fallbacks
    R, scale = mo.orthogonal_procrustes_on_device(Ad, Bd)
    assert mo.procrustes_fallbacks == before + 1
    R_ref, scale_ref = orthogonal_procrustes(A, B)
    assert np.array_equal(R.cpu().numpy(), R_ref) and float(scale) == scale_ref


def test_r_1_zero_product_is_flagged():
    from mused_amd import matrix_operations as mo
    from mused_amd import procrustes as pr

    Ad = torch.zeros((4, 1), dtype=torch.float64, device="cuda")
    _, _, info, _ = mo.procrustes_launch(Ad, Ad + 1.0, torch.cuda.current_stream())
    assert int(info.cpu()[0]) & pr.FLAG_ILLCOND
    R, _ = mo.orthogonal_procrustes_on_device(Ad - 2.0, Ad + 1.0)        # M = -8: R = sign(M)
    assert R.cpu().numpy().tolist() == [[-1.0]]


@pytest.mark.parametrize("name", ["nan_in_A", "inf_in_B"])
def test_nonfinite_input_raises(name):
    from mused_amd import matrix_operations as mo

    A, B = pc.nonfinite()[name]
    before = mo.procrustes_fallbacks
    with pytest.raises(ValueError, match="infs or NaNs"):
        mo.orthogonal_procrustes_on_device(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
    E = np.vstack([A, A])
    with pytest.raises(ValueError, match="infs or NaNs"):
        mo.align_embedding_on_device(torch.from_numpy(E).cuda(), torch.from_numpy(np.vstack([B, B])).cuda(), A.shape[0])
    assert mo.procrustes_fallbacks == before


# ---- the SVD kernel alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RS)
def test_svd_jacobi_small(r):
    from mused_amd import matrix_operations as mo

    rng = np.random.default_rng(r)
    M = pc.conditioned(r, r, rng, 100.0)
    big = torch.zeros((r, r + 5), dtype=torch.float64, device="cuda")
    big[:, :r] = torch.from_numpy(M).cuda()
    W, sigma, info = mo.svd_jacobi_small_launch(big[:, :r])               # ldm = r + 5
    W2, sigma2, info2 = mo.svd_jacobi_small_launch(torch.from_numpy(M).cuda())
    assert torch.equal(W, W2) and torch.equal(sigma, sigma2) and torch.equal(info, info2)
    W, sigma, info = W.cpu().numpy(), sigma.cpu().numpy(), info.cpu().numpy()
    assert info[0] == 0 and 1 <= info[1] < 30 and info[2] == 0 and info[3] == 0
    print(f"r={r} sweeps={info[1]}")
    # W^T W is diagonal to the rotation threshold: the kernel left every pair with |w_p.w_q| <= 2^-50 |w_p| |w_q| by its own
    # dot products; NumPy's differ from those by at most r 2^-52 |w_p| |w_q| (an r-term sum, either order)
    G = W.T @ W
    nrm = np.sqrt(np.diag(G))
    off = np.abs(G - np.diag(np.diag(G))) / np.outer(nrm, nrm)
    assert off.max() <= 2.0 ** -50 + r * 2.0 ** -52
    assert np.abs(sigma - nrm).max() <= r * 2.0 ** -52 * nrm.max()      # two evaluations of a sum of r squares, rooted
    s_ref = np.linalg.svd(M, compute_uv=False)
    assert np.abs(np.sort(sigma)[::-1] - s_ref).max() <= r * 2.0 ** -50 * s_ref[0]
    # W = M V with V orthogonal: the rows of W keep the lengths of the rows of M
    assert np.abs(np.linalg.norm(W, axis=1) - np.linalg.norm(M, axis=1)).max() <= r * 2.0 ** -50 * s_ref[0]


@pytest.mark.parametrize("r", [1, 6, 65, 128])
def test_orthogonal_columns_return_after_one_sweep(r):
    from mused_amd import matrix_operations as mo

    rng = np.random.default_rng(r)
    M = np.zeros((r, r))
    M[rng.permutation(r), np.arange(r)] = rng.uniform(0.5, 2.0, r) * rng.choice([-1.0, 1.0], r)   # exactly orthogonal columns
    W, sigma, info = mo.svd_jacobi_small_launch(torch.from_numpy(M).cuda())
    assert info.cpu().numpy().tolist() == [0, 1, 0, 0]
    assert np.array_equal(W.cpu().numpy(), M) and np.array_equal(sigma.cpu().numpy(), np.abs(M).sum(0))


# ---- the product and its sums -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W_, r, shift", [(64, 5, 32), (250, 65, 125), (1000, 128, 250), (33, 1, 1), (16400, 3, 8200)])
def test_align_embedding(W_, r, shift):
    from mused_amd import matrix_operations as mo
    from mused_amd import procrustes as pr

    rng = np.random.default_rng(W_ + r)
    E_ref = pc.conditioned(W_, r, rng, 9.0)
    E_new = np.vstack([E_ref[shift:] @ pc.orthogonal(r, rng), pc.conditioned(shift, r, rng, 9.0) if shift >= r
                       else rng.standard_normal((shift, r))])
    E_new += 1e-3 * rng.standard_normal(E_new.shape) / np.sqrt(W_)
    En, Er = torch.from_numpy(E_new).cuda(), torch.from_numpy(E_ref).cuda()
    keep = En.clone()
    before = mo.procrustes_fallbacks
    out, R, res, un = mo.align_embedding_on_device(En, Er, shift)
    out2, R2, res2, un2 = mo.align_embedding_on_device(En, Er, shift)
    assert mo.procrustes_fallbacks == before
    assert torch.equal(En, keep) and out.data_ptr() != En.data_ptr()
    assert torch.equal(out, out2) and torch.equal(R, R2) and (res, un) == (res2, un2)
    A, B = E_new[:W_ - shift], E_ref[shift:]
    R_ref = orthogonal_procrustes(A, B)[0]
    Rh = R.cpu().numpy()
    assert np.abs(Rh - R_ref).max() <= 4 * pr.unit(A, B)
    # out = E R: two evaluations of an r-term sum, each within (r + 2) 2^-53 |E_i| |R_j| of the exact one, |R_j| = 1
    rows = np.linalg.norm(E_new, axis=1)[:, None]
    assert (np.abs(out.cpu().numpy() - E_new @ Rh) <= (r + 2) * 2.0 ** -52 * rows).all()
    nb = np.linalg.norm(B)
    # the sums: squares of m r differences, each known to the product's error above
    assert abs(res - np.linalg.norm(A @ Rh - B) / nb) <= 1e-12 * max(un, 1.0)
    assert abs(un - np.linalg.norm(A - B) / nb) <= 1e-12 * max(un, 1.0)
    assert res <= un


def test_apply_refuses_aliased_output():
    import ctypes as C

    from mused_amd import _lib

    E = torch.zeros((8, 4), dtype=torch.float64, device="cuda")
    R = torch.eye(4, dtype=torch.float64, device="cuda")
    ws = torch.zeros(24576, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    rc = _lib.lib().mused_procrustes_apply(p(E), 4, 8, 4, p(R), p(E[2:]), 4, None, 0, 0, None, p(ws), None)
    assert rc == -1                                                                                # MUSED_ERR_ARG


def test_host_mode_is_scipy(monkeypatch):
    from mused_amd import matrix_operations as mo

    ref = _case(257, 7)
    monkeypatch.setenv("MUSED_ALIGN", "host")
    before = mo.procrustes_fallbacks
    R, scale = mo.orthogonal_procrustes_on_device(torch.from_numpy(ref[0]).cuda(), torch.from_numpy(ref[1]).cuda())
    assert mo.procrustes_fallbacks == before
    assert np.array_equal(R.cpu().numpy(), ref[2]) and float(scale) == ref[3]
