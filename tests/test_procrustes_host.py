"""The NumPy rule of mused_amd/procrustes.py against scipy.linalg.orthogonal_procrustes (no GPU).

One tolerance, per input: max |R_rule - R_scipy| <= 4 u(A, B), u = 2^-52 (r + sqrt(m)) | |A|^T |B| |_F / sigma_r(A^T B)
(procrustes.unit).  Orthogonality max |R^T R - I| <= 8 r 2^-52 (the Newton-Schulz step), scale within r 2^-50 relative."""
import numpy as np
import pytest
from scipy.linalg import orthogonal_procrustes

import procrustes_cases as pc
from mused_amd import procrustes as pr


def _check(A, B, R, scale):
    r = A.shape[1]
    R_ref, scale_ref = orthogonal_procrustes(A, B)
    u = pr.unit(A, B)
    share = np.abs(R - R_ref).max() / (4.0 * u)
    print(f"m={A.shape[0]} r={r} share of 4u = {share:.4f}")
    assert share <= 1.0
    assert np.abs(R.T @ R - np.eye(r)).max() <= 8 * r * 2.0 ** -52
    assert abs(scale - scale_ref) <= r * 2.0 ** -50 * scale_ref
    return share


@pytest.mark.parametrize("case", pc.HOST_CASES, ids=lambda c: f"m{c[0]}-r{c[1]}")
def test_rule_matches_scipy(case):
    m, r, cond, noise, det, mean = case
    A, B, _ = pc.pair(m, r, 100 + m + r, cond, noise, det, mean)
    R, scale, flags, sweeps = pr.orthogonal_procrustes_rule(A, B)
    assert flags == 0 and 1 <= sweeps < pr.MAX_SWEEPS
    _check(A, B, R, scale)


@pytest.mark.parametrize("name", ["m_below_r", "zero_column"])
def test_degenerate_inputs_are_flagged(name):
    A, B = pc.degenerate()[name]
    flags = pr.orthogonal_procrustes_rule(A, B)[2]
    assert flags & pr.FLAG_ILLCOND and not flags & pr.FLAG_NONFINITE


def test_zero_matrix_is_flagged():
    A = np.zeros((6, 3))
    assert pr.orthogonal_procrustes_rule(A, A)[2] & pr.FLAG_ILLCOND
    assert pr.orthogonal_procrustes_rule(np.zeros((4, 1)), np.ones((4, 1)))[2] & pr.FLAG_ILLCOND   # r = 1, M = 0


@pytest.mark.parametrize("name", ["nan_in_A", "inf_in_B"])
def test_nonfinite_is_flagged_and_raises_in_align(name):
    A, B = pc.nonfinite()[name]
    R, scale, flags, sweeps = pr.orthogonal_procrustes_rule(A, B)
    assert flags == pr.FLAG_NONFINITE and sweeps == 0 and np.isnan(R).all()
    with pytest.raises(ValueError, match="infs or NaNs"):
        pr.align_rule(np.vstack([A, A]), np.vstack([B, B]), A.shape[0])
    with pytest.raises(ValueError):   # SciPy's own answer to the same input
        orthogonal_procrustes(A, B)


def test_equal_inputs_give_the_identity():
    A = pc.pair(120, 12, 3, cond=25.0)[0]
    R, scale, flags, _ = pr.orthogonal_procrustes_rule(A, A)
    assert flags == 0
    assert np.abs(R - np.eye(12)).max() <= 4 * pr.unit(A, A)
    assert abs(scale - (A * A).sum()) <= 12 * 2.0 ** -50 * scale   # trace(A^T A)


@pytest.mark.parametrize("det", [1, -1])
def test_exact_rotation_is_recovered(det):
    A, _, Q = pc.pair(90, 9, 4, cond=16.0, det=det)
    B = A @ Q
    R, _, flags, _ = pr.orthogonal_procrustes_rule(A, B)
    assert flags == 0
    # B itself is A Q rounded: the rounding of an r-term product moves the polar factor like a perturbation of M does
    assert np.abs(R - Q).max() <= 4 * pr.unit(A, B)
    assert np.sign(np.linalg.det(R)) == det


def test_all_singular_values_equal():
    rng = np.random.default_rng(5)
    A = np.linalg.qr(rng.standard_normal((80, 10)))[0]    # orthonormal columns: A^T A = I
    Q = pc.orthogonal(10, rng)
    B = A @ Q
    R, scale, flags, sweeps = pr.orthogonal_procrustes_rule(A, B)
    assert flags == 0
    _check(A, B, R, scale)
    assert abs(scale - 10.0) <= 10 * 2.0 ** -50 * 10.0


def test_schedule_covers_every_pair_once():
    for r in (1, 2, 3, 7, 8, 65, 128):
        seen = set()
        for P, Q in pr.schedule(r):
            assert (P < Q).all() and len(set(P) | set(Q)) == 2 * len(P)   # disjoint pairs inside a step
            seen |= set(zip(P.tolist(), Q.tolist()))
        assert seen == {(p, q) for p in range(r) for q in range(p + 1, r)}


@pytest.mark.parametrize("seed", range(6))
def test_alignment_never_increases_the_distance(seed):
    rng = np.random.default_rng(seed)
    W, r, shift = 64, 5, 32
    E_ref = pc.conditioned(W, r, rng, 9.0)
    E_new = np.vstack([E_ref[shift:] @ pc.orthogonal(r, rng), pc.conditioned(shift, r, rng, 9.0)])
    E_new += 1e-2 * rng.standard_normal(E_new.shape) * (seed % 3)   # seeds 0, 3: exact, the others noisy
    out, R, res, un = pr.align_rule(E_new, E_ref, shift)
    assert res <= un
    assert np.array_equal(out, E_new @ R)
    assert np.abs(R.T @ R - np.eye(r)).max() <= 8 * r * 2.0 ** -52
    if seed % 3 == 0:
        assert res <= 1e-13 < un
