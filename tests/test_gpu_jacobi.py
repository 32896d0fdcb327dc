"""The one-sided block Jacobi (csrc/eig.hip) family by family on the device: every kernel instance of tests/jacobi_cases.py
against the fp64 reference, and the plan states a second solve inherits (mused_debug_eig_plan_*: a plan that outlives one
solve).  Families are reached through the plan's shape only; no case touches the queue's timeout.

Tolerances are those of jacobi_cases.py (the project's own, from test_gpu_primitives.py) for every family; the measured
quantities are printed per row before they are asserted (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest

import jacobi_cases as jc
from test_eig_choice import SWITCHES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    lib = _lib.lib()
    vp, i = C.c_void_p, C.c_int
    lib.mused_debug_eig_choice.restype = i
    lib.mused_debug_eig_choice.argtypes = [i] * 5 + [C.POINTER(i)]
    lib.mused_debug_eig_plan_create.restype = i
    lib.mused_debug_eig_plan_create.argtypes = [i, i, i, i, i, vp, i, C.POINTER(vp)]
    lib.mused_debug_eig_plan_run.restype = i
    lib.mused_debug_eig_plan_run.argtypes = [vp, vp, vp, vp, vp, i, vp]
    lib.mused_debug_eig_plan_destroy.restype = i
    lib.mused_debug_eig_plan_destroy.argtypes = [vp]
    return _lib


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def choice(L, n, batch, sweeps, flags=0, need=0):
    out = (C.c_int * 8)()
    L.check(L.lib().mused_debug_eig_choice(n, batch, sweeps, flags, need, out))
    return tuple(out)[:3]


def syevj(L, G, sweeps=jc.SWEEP_CAP):
    batch, n = G.shape[:2]
    dG = dev(G)
    ev = torch.empty((batch, n), dtype=torch.float64, device="cuda")
    V = torch.empty((batch, n, n), dtype=torch.float64, device="cuda")
    L.call("mused_syevj_batched", P(dG), n, batch, sweeps, P(ev), P(V), S())
    torch.cuda.synchronize()
    return ev.cpu().numpy(), V.cpu().numpy()


class Plan:
    """mused_debug_eig_plan_*: run() returns (evals, V, working copy as batch x ldn (columns) x ldn (rows))."""

    def __init__(self, L, n, batch, sweeps=jc.SWEEP_CAP, flags=0, need=0, rep=None, own_graph=1):
        self.L, self.n, self.batch = L, n, batch
        self.ldn = choice(L, n, batch, sweeps, flags, need)[2]
        self.rep = None if rep is None else torch.tensor(rep, dtype=torch.int32, device="cuda")
        self.h = C.c_void_p()
        L.check(L.lib().mused_debug_eig_plan_create(n, batch, sweeps, flags, need, P(self.rep), own_graph, C.byref(self.h)))

    def run(self, G, allow_graph=1, vectors=True):
        assert G.shape == (self.batch, self.n, self.n)
        dG = dev(G)
        ev = torch.full((self.batch, self.n), np.nan, dtype=torch.float64, device="cuda") if vectors else None
        V = torch.full((self.batch, self.n, self.n), np.nan, dtype=torch.float64, device="cuda") if vectors else None
        Gc = torch.full((self.batch, self.ldn, self.ldn), np.nan, dtype=torch.float64, device="cuda")
        self.L.check(self.L.lib().mused_debug_eig_plan_run(self.h, P(dG), P(ev), P(V), P(Gc), allow_graph, S()))
        torch.cuda.synchronize()
        return (ev.cpu().numpy() if vectors else None, V.cpu().numpy() if vectors else None, Gc.cpu().numpy())

    def close(self):
        if self.h:
            self.L.lib().mused_debug_eig_plan_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def check_batch(mats, ev, V, what):
    """Each distinct matrix against the reference once, its copies for bit equality with it."""
    for b in range(len(ev)):
        k = b % len(mats)
        if b < len(mats):
            m = mats[k]
            got, dead = jc.measure(m.G, ev[b], V[b], m.ref)
            print(f"{what} {m.name:10s} eig_top {got.eig_top:.2e} eig_all {got.eig_all:.2e} resid {got.resid:.2e} orth {got.orth:.2e}")
            jc.check_solution(m.G, ev[b], V[b], m.tol, m.ref, f"{what} {m.name}")
        else:
            assert np.array_equal(ev[b], ev[k]) and np.array_equal(V[b], V[k]), f"{what}: copy {b} of matrix {k} differs"


# ------------------------------------------------ (a) every instance against the reference ----------------------------------
@pytest.mark.parametrize("c", jc.CASES, ids=jc.case_id)
def test_every_instance_meets_the_reference(L, c):
    """Separated and Gram (and clustered where the batch holds three) through mused_syevj_batched at every table row; at the
    orders of jc.DEGENERATE_ORDERS the zero matrix, a diagonal one, a rank-one one and a clustered one as a second batch of
    the same family."""
    assert choice(L, c.n, c.batch, c.sweeps) == (c.direct, c.jacobi, c.ldn)
    mats = jc.batch_matrices(c)
    ev, V = syevj(L, jc.fill(mats, c.batch), c.sweeps)
    check_batch(mats, ev, V, jc.case_id(c))
    if c.n in jc.DEGENERATE_ORDERS:
        batch = max(c.batch, 4)
        assert choice(L, c.n, batch, c.sweeps) == (c.direct, c.jacobi, c.ldn)
        mats = jc.extra_matrices(c.n)
        ev, V = syevj(L, jc.fill(mats, batch), c.sweeps)
        check_batch(mats, ev, V, jc.case_id(c))


# ------------------------------------------------ (b) a matrix does not depend on its batch ---------------------------------
@pytest.mark.parametrize("n,batch,alone", [(128, 5, 1), (256, 57, 57), (320, 5, 1), (640, 5, 1)])
def test_a_matrix_does_not_depend_on_its_batch(L, n, batch, alone):
    """The same matrix at positions 0, middle and last of a batch, between other matrices, and in a batch of the same family
    without them (alone where the family allows a batch of one; the sweep graph of order 256 starts at 57 matrices: there the
    other batch holds it at another position between other neighbours).  The sweep graphs run one workgroup per block pair
    and launch.  The queue hands the same units (one block-pair round of one matrix) to whichever workgroup is free, but a
    round of a matrix is only queued when the last unit of its previous round has been counted in, and its units touch
    disjoint columns: the order in which units are taken changes no operand (osjq_kernel).  Bits must be equal in all
    families."""
    fam = choice(L, n, batch, jc.SWEEP_CAP)
    assert choice(L, n, alone, jc.SWEEP_CAP) == fam
    t = jc.clustered(n, seed=1)
    others = [jc.separated(n, seed=2), jc.gram(n, seed=3), jc.diagonal(n)]
    G = np.stack([others[b % 3].G for b in range(batch)])
    pos = (0, batch // 2, batch - 1)
    for b in pos:
        G[b] = t.G
    ev, V = syevj(L, G)
    jc.check_solution(t.G, ev[0], V[0], t.tol, t.ref, f"n={n}")
    for b in pos[1:]:
        assert np.array_equal(ev[b], ev[0]) and np.array_equal(V[b], V[0]), b
    G2 = np.stack([others[(b + 1) % 3].G for b in range(alone)])
    G2[alone // 3] = t.G
    ev2, V2 = syevj(L, G2)
    assert np.array_equal(ev2[alone // 3], ev[0]) and np.array_equal(V2[alone // 3], V[0])


# ------------------------------------------------ (c) queue and sweep graph agree -------------------------------------------
def test_queue_and_sweep_graph_agree_at_order_256(L):
    """57 matrices of order 256 are the sweep graph's, the first 56 of them the queue's.  Both meet the reference, and -- the
    unit of work, its arithmetic and the rolling stop being the same code (osjw_unit) -- both return the same bits."""
    n = 256
    assert choice(L, n, 57, jc.SWEEP_CAP)[1] == jc.WAVE and choice(L, n, 56, jc.SWEEP_CAP)[1] == jc.QUEUE
    mats = [jc.separated(n, seed=4), jc.gram(n, seed=5), jc.clustered(n, seed=6)]
    G = jc.fill(mats, 57)
    evw, Vw = syevj(L, G)
    evq, Vq = syevj(L, G[:56])
    check_batch(mats, evw, Vw, "wave256")
    check_batch(mats, evq, Vq, "queue256")
    print("queue vs sweep graph: max |d evals| %.3e, max |d V| %.3e" % (np.abs(evw[:56] - evq).max(), np.abs(Vw[:56] - Vq).max()))
    assert np.array_equal(evw[:56], evq) and np.array_equal(Vw[:56], Vq)


# ------------------------------------------------ (d) plan reuse ------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(128, 3), (256, 57), (320, 3), (640, 3)])
def test_a_plan_solves_the_same_after_other_work(L, n, batch):
    """A (clustered matrices: many rounds), then B (diagonal and zero matrices, which need none, and one separated matrix),
    then A again on ONE plan: convergence flags, the queue's counters and its unit ring are inherited from the solve before.
    Every result equals the same batch on a fresh plan bit for bit.  Flags are only ever raised, so what a stale one can do
    is prolong a solve -- which shows where the matrix before it needed MORE rounds and the matrix itself keeps cosines a
    further round would still rotate (a multiple eigenvalue): hence the rank-deficient Gram batch D and A with its matrices
    moved on by one place behind it."""
    A = np.stack([jc.clustered(n, seed=10 + (b % 3)).G for b in range(batch)])
    Bm = [jc.diagonal(n), jc.zero(n), jc.separated(n, seed=11)]
    B = jc.fill(Bm, batch)
    D = np.stack([jc.gram(n, seed=12 + (b % 3)).G for b in range(batch)])
    batches = {"A": A, "B": B, "D": D, "A moved": np.roll(A, 1, axis=0)}
    fresh = {}
    for name, G in batches.items():
        with Plan(L, n, batch) as p:
            fresh[name] = p.run(G)
    with Plan(L, n, batch) as p:
        for step, name in enumerate(("A", "B", "A", "D", "A moved", "B", "A")):
            got = p.run(batches[name])
            assert same_bits(got, fresh[name]), f"solve {step} ({name}) differs from a fresh plan's"
    check_batch(Bm, fresh["B"][0], fresh["B"][1], f"reuse n={n}")


# ------------------------------------------------ (e) graph replay == plain launches ----------------------------------------
@pytest.mark.parametrize("n,batch", [(256, 2), (320, 2), (640, 2)])
def test_graph_replay_equals_plain_launches(L, n, batch):
    """own_graph = 1 / allow_graph = 1 (the plan replays its private hipGraph) against own_graph = 0 (plain launches on the
    caller's stream: what rsvd.hip's plan does inside the eigenstep's own capture) and against a plan that has a graph but
    is told not to use it."""
    mats = [jc.gram(n, seed=20), jc.clustered(n, seed=21)]
    G = jc.fill(mats, batch)
    with Plan(L, n, batch, own_graph=1) as p:
        g = p.run(G, allow_graph=1)
        g0 = p.run(G, allow_graph=0)
    with Plan(L, n, batch, own_graph=0) as p:
        plain = p.run(G, allow_graph=1)
    assert same_bits(g, plain) and same_bits(g0, plain)
    check_batch(mats, g[0], g[1], f"graph n={n}")


# ------------------------------------------------ (f) rep -------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 320])
def test_duplicates_are_skipped_and_representatives_unchanged(L, n):
    """rep = [0, 0, 2, 2, 2, 5]: matrices 1, 3 and 4 are not solved.  The representatives come out bit for bit as without
    rep.  A skipped matrix is never queued (osjq_init_kernel) / its workgroups return at once (osjw_kernel,
    osj_round_kernel): its working copy is still the packed input, and osj_norms_kernel / osj_extract_kernel, which run over
    the whole batch, return the norms of the input's columns as its `evals` and the normalised columns as its `V`."""
    rep = [0, 0, 2, 2, 2, 5]
    mats = [jc.separated(n, seed=30), jc.gram(n, seed=31), jc.clustered(n, seed=32)]
    G = np.stack([mats[r % 3].G for r in range(6)])   # six different positions, three different matrices
    with Plan(L, n, 6) as p:
        ev0, V0, Gc0 = p.run(G)
    with Plan(L, n, 6, rep=rep) as p:
        ev, V, Gc = p.run(G)
    ldn = Gc.shape[1]
    for b in range(6):
        if rep[b] == b:
            assert np.array_equal(ev[b], ev0[b]) and np.array_equal(V[b], V0[b]) and np.array_equal(Gc[b], Gc0[b]), b
            m = mats[b % 3]
            jc.check_solution(m.G, ev[b], V[b], m.tol, m.ref, f"rep n={n} matrix {b}")
        else:
            packed = np.zeros((ldn, ldn))
            packed[:n, :n] = G[b].T
            assert np.array_equal(Gc[b], packed), b
            nrm = np.linalg.norm(G[b], axis=0)
            np.testing.assert_allclose(ev[b], nrm, rtol=n * jc.EPS, atol=0)
            np.testing.assert_allclose(V[b] * ev[b][None, :], G[b], rtol=4 * jc.EPS, atol=0)


# ------------------------------------------------ (g) fixed sweeps, no sort -------------------------------------------------
@pytest.mark.parametrize("c", jc.FIXED_CASES, ids=jc.case_id)
def test_fixed_sweeps_without_sort_rotate_the_columns_orthogonally(L, c):
    """The pre-rotation plan: 5 sweeps whatever they meet, columns stay in place.  The working copy is G J with J orthogonal:
    Gc Gc^T = G^2 to n * sweeps * eps * |G|_2^2 (one rounding per rotation and column, growing linearly; products in
    np.longdouble), the off-diagonal mass of Gc^T Gc is below the input's, pad rows and columns are exactly zero."""
    assert choice(L, c.n, c.batch, c.sweeps, c.flags) == (c.direct, c.jacobi, c.ldn)
    mats = [jc.separated(c.n, seed=40), jc.gram(c.n, seed=41), jc.clustered(c.n, seed=42)]
    G = jc.fill(mats, c.batch)
    with Plan(L, c.n, c.batch, sweeps=c.sweeps, flags=c.flags) as p:
        _, _, Gc = p.run(G, vectors=False)
    LD = np.longdouble
    for b in range(c.batch):
        if b >= 3:
            assert np.array_equal(Gc[b], Gc[b % 3]), b
            continue
        A = Gc[b].T                                   # rows x columns
        assert not A[c.n:].any() and not A[:, c.n:].any()
        A = A[: c.n, : c.n].astype(LD)
        Gl = G[b].astype(LD)
        norm2 = float(mats[b].ref.max())
        err = float(np.abs(A @ A.T - Gl @ Gl).max())
        bound = c.n * c.sweeps * jc.EPS * norm2 ** 2
        off = lambda M: float(np.sqrt(((M - np.diag(np.diag(M))) ** 2).sum()))
        after, before = off(A.T @ A), off(Gl.T @ Gl)
        print(f"{jc.case_id(c)} {mats[b].name:10s} |Gc Gc^T - G^2| {err:.3e} (bound {bound:.3e}), off-diagonal {before:.3e} -> {after:.3e}")
        assert err <= bound
        assert after < before


# ------------------------------------------------ (h) mixed batch behind trdx ----------------------------------------------
def test_mixed_batch_behind_the_blocked_direct_solver(L):
    """Order 320, TOP_HALF, batch 4: two separated matrices, which the blocked direct solver (trdx.hip) certifies, and two with
    a 100-fold eigenvalue above the cut, which it rejects (trd_common.h: no 6 significant eigenvalues within 1e-7 lam_0) and the
    sweep graph solves through jrep; osj_norms_kernel must skip exactly the accepted ones.  The leading 160 pairs of all four
    meet the reference at the clustered row -- the level of the direct solver's certificate (cosines <= TRD_COS_MAX = 1e-8);
    what this test is about is the routing --, and a second solve on the same plan (jrep / nrej reset) returns the same bits."""
    c = jc.MIXED_CASE
    n, need = c.n, c.n // 2
    assert choice(L, c.n, c.batch, c.sweeps, c.flags) == (2, 1, 320)
    mats = [jc.separated(n, seed=50), jc.heavy(n, seed=51), jc.heavy(n, seed=52), jc.separated(n, seed=53)]
    G = jc.fill(mats, 4)
    with Plan(L, n, 4, flags=c.flags) as p:
        r1 = p.run(G)
        r2 = p.run(G)
    assert same_bits(r1, r2)
    ev, V, Gc = r1
    tol = jc.TOL_CLUSTERED
    for b, m in enumerate(mats):
        scale = np.abs(m.G).max()
        # who solved it: the direct solver leaves columns 0 .. need - 1 (need = 160 is a multiple of 32) in descending order
        # and zeros elsewhere (trdx_solve); the Jacobi leaves all 320 columns of these full-rank matrices
        if m.name == "separated":
            assert not Gc[b][need:].any() and not ev[b][need:].any() and (np.diff(ev[b][:need]) <= 0).all(), b
        else:
            assert (ev[b] >= 0.5 * m.ref.min()).all(), b   # (smallest eigenvalue 0.25)
        top = np.argsort(-ev[b])[:need]
        e, W = ev[b][top], V[b][:, top]
        ref = m.ref[::-1][:need]
        d_eig = np.abs(e - ref).max() / scale
        resid = np.abs(m.G @ W - W * e[None, :]).max() / scale
        orth = np.abs(W.T @ W - np.eye(need)).max()
        print(f"mixed320 {m.name:10s} eig {d_eig:.2e} resid {resid:.2e} orth {orth:.2e}")
        assert d_eig <= tol.eig_all and resid <= tol.resid and orth <= tol.orth, (b, m.name)


# ------------------------------------------------ (i) scale -----------------------------------------------------------------
@pytest.mark.parametrize("n", [128, 320, 640])
def test_scaling_by_a_power_of_two(L, n):
    """The separated matrix times 2^100 and 2^-100: the tolerances of (a) relative to the scaled scale, eigenvectors within
    1e-11 of the unscaled run's, up to sign."""
    mats = [jc.separated(n), jc.scaled(n, 100), jc.scaled(n, -100)]
    ev, V = syevj(L, jc.fill(mats, 3))
    check_batch(mats, ev, V, f"scale n={n}")
    for b in (1, 2):
        sgn = np.sign((V[b] * V[0]).sum(0))
        sgn[sgn == 0] = 1.0
        d = np.abs(V[b] * sgn[None, :] - V[0]).max()
        print(f"scale n={n} {mats[b].name}: max |dV| {d:.3e}")
        assert d <= 1e-11
