"""tests/jacobi_cases.py without a device: every table row gets the kernel family and padded order it was written for from
eig_choose() (mused_debug_eig_choice touches no device), the table reaches every (family, padded order) instance, the
checker accepts LAPACK's eigh on every builder and rejects five named defects under both tolerance rows."""
import ctypes

import numpy as np
import pytest

import jacobi_cases as jc
from test_eig_choice import SWITCHES, _lib


def choice(monkeypatch, n, batch, sweeps, flags, need):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    fn = _lib().mused_debug_eig_choice
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 8)()
    assert fn(n, batch, sweeps, flags, need, out) == 0
    return tuple(out)


@pytest.mark.parametrize("c", jc.CASES + jc.FIXED_CASES + (jc.MIXED_CASE,), ids=jc.case_id)
def test_every_row_gets_the_family_it_was_written_for(monkeypatch, c):
    got = choice(monkeypatch, c.n, c.batch, c.sweeps, c.flags, c.need)
    assert got[:3] == (c.direct, c.jacobi, c.ldn)
    assert got[6:] == (0 if c.flags & jc.NO_SORT else 1, 0 if c.flags & jc.FIXED_SWEEPS else 1)
    if c in jc.CASES and c.n in jc.DEGENERATE_ORDERS:  # the batch of the degenerate matrices stays in the family
        assert choice(monkeypatch, c.n, max(c.batch, 4), c.sweeps, 0, 0)[:3] == (0, c.jacobi, c.ldn)


def test_the_table_reaches_every_instance():
    assert {(c.jacobi, c.ldn) for c in jc.CASES} == jc.INSTANCES
    assert all(c.flags == 0 and c.sweeps == jc.SWEEP_CAP for c in jc.CASES)
    # padding inside a class: zero columns next to live ones, in every family
    assert {c.n for c in jc.CASES} >= {2, 62, 130, 258, 514, 900}
    # one order per family carries the degenerate matrices
    fam = {(c.jacobi, c.ldn <= 256) for c in jc.CASES if c.n in jc.DEGENERATE_ORDERS}
    assert fam == {(jc.QUEUE, True), (jc.WAVE, True), (jc.WAVE, False), (jc.ROW, False)}


def test_the_queue_rows_sit_on_the_bound(monkeypatch):
    """The WaveGraph rows of orders <= 256 are the first batch past the queue's 224 units per round."""
    for c in jc.CASES:
        if c.jacobi == jc.WAVE and c.ldn <= 256:
            assert choice(monkeypatch, c.n, c.batch - 1, c.sweeps, 0, 0)[1] == jc.QUEUE, c


ALL = [(name, n) for name in jc.BUILDERS for n in (2, 62, 64, 130)] + [("scaled+100", 64), ("scaled-100", 64), ("heavy", 320)]


def build(name, n):
    if name.startswith("scaled"):
        return jc.scaled(n, int(name[6:]))
    if name == "heavy":
        return jc.heavy(n)
    return jc.BUILDERS[name](n)


def lapack(m):
    w, V = np.linalg.eigh(m.G)
    return np.maximum(w, 0.0), V


@pytest.mark.parametrize("name,n", ALL)
def test_the_checker_accepts_lapack(name, n):
    m = build(name, n)
    assert np.array_equal(m.G, m.G.T)
    w, V = lapack(m)
    got = jc.check_solution(m.G, w, V, m.tol, m.ref, name)
    # ... in any column order, and with the null space returned as zero vectors
    perm = np.random.default_rng(0).permutation(n)
    jc.check_solution(m.G, w[perm], V[:, perm], m.tol, m.ref, name)
    dead = w <= jc.LIVE * max(np.abs(m.G).max(), 1e-300)
    V0 = V.copy()
    V0[:, dead] = 0.0
    jc.check_solution(m.G, w, V0, m.tol, m.ref, name)
    assert all(np.isfinite(x) for x in got)


def test_the_gram_reference_is_relatively_accurate():
    m = jc.gram(64)
    assert not m.ref[:16].any() and (m.ref[16:] > 0).all()   # n / 4 exact zeros


def defects(m):
    """name -> (evals, V) of LAPACK's solution with one defect; i / j = the largest / smallest live eigenvalue."""
    w, V = lapack(m)
    scale = np.abs(m.G).max()
    live = np.flatnonzero(w > jc.LIVE * scale)
    i, j = live[np.argmax(w[live])], live[np.argmin(w[live])]
    out = {}
    e = w.copy()
    e[i] += 1e-9 * scale
    out["eigenvalue moved by 1e-9 scale"] = (e, V)
    R = V.copy()
    t = 1e-6
    R[:, i], R[:, j] = np.cos(t) * V[:, i] + np.sin(t) * V[:, j], np.cos(t) * V[:, j] - np.sin(t) * V[:, i]
    out["two columns rotated by 1e-6"] = (w, R)
    Z = V.copy()
    Z[:, i] = 0.0
    out["live column zeroed"] = (w, Z)
    e = w.copy()
    e[i], e[j] = w[j], w[i]
    out["eigenvalues swapped without their vectors"] = (e, V)
    Sc = V.copy()
    Sc[:, i] *= 1.0 + 1e-6
    out["column scaled by 1 + 1e-6"] = (w, Sc)
    return out


@pytest.mark.parametrize("tol", sorted(jc.TOLERANCES))
@pytest.mark.parametrize("name", ["separated", "gram", "clustered", "diagonal"])
def test_the_checker_rejects_each_defect(name, tol):
    m = jc.BUILDERS[name](64)
    w, V = lapack(m)
    jc.check_solution(m.G, w, V, jc.TOLERANCES[tol], m.ref, name)   # the clean solution passes this row
    for what, (e, W) in defects(m).items():
        with pytest.raises(AssertionError):
            jc.check_solution(m.G, e, W, jc.TOLERANCES[tol], m.ref, f"{name}, {what}")


def test_the_checker_rejects_a_live_eigenvalue_on_a_dead_column_and_nan():
    m = jc.gram(64)
    w, V = lapack(m)
    e = w.copy()
    e[0] = -1e-6 * np.abs(m.G).max()
    with pytest.raises(AssertionError):
        jc.check_solution(m.G, e, V, jc.TOL_CLUSTERED, m.ref)
    V = V.copy()
    V[3, 5] = np.nan
    with pytest.raises(AssertionError):
        jc.check_solution(m.G, w, V, jc.TOL_CLUSTERED, m.ref)
