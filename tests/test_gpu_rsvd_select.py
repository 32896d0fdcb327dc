"""The eigenstep's selection tail (csrc/rsvd.hip: rsvd_decide_kernel, the Bt Cm product, col_sign_kernel, col_scale_kernel)
through mused_rsvd_select on eigenpairs the test supplies, against a np.longdouble reference:

  order   eigenvalues descending, equal ones by ascending index (over all en entries, the zero padding included)
  sigma   sqrt(max(lam, 0)); within eps sigma of the longdouble root (a correctly rounded root is within eps / 2)
  Cm      U[:rc, order[i]] / sigma_i, or 0 where sigma_i <= 1e-12 sigma_0 (no case has a sigma within a factor 2 of that line)
  V       Bt Cm within (rc + 2) eps |Bt| |Cm|: rc products and rc - 1 additions in any order, and the two roundings of Cm
          (root and quotient); eps = 2^-52
  sign    of the FIRST entry of largest magnitude of each column, + for a non-negative one.  On rounded columns the two
          largest magnitudes of the reference differ by more than twice the bound (asserted without a GPU), so the device
          decides by the same entry; on the exact cases (U a permutation, eigenvalues powers of 4, Bt small integers, columns
          holding +x and -x) nothing rounds, and order, signs and V are compared for equality."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

torch = pytest.importorskip("torch")

LD = np.longdouble
EPS = 2.0 ** -52
DROP_REL = 1e-12
N_MAX = 1000
GUARD = 64
SENT = -12345.678


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    r_max: int      # of the handle: en = (r_max + 1) & ~1
    rc: int
    n: int
    n_comp: int
    kind: str       # distinct | ties2 | ties5 | negative | tiny | zeros | exact

    @property
    def en(self):
        return (self.r_max + 1) & ~1


def _c(kind, r_max, rc, n, n_comp):
    return Case(f"{kind}_en{(r_max + 1) & ~1}_rc{rc}_n{n}_k{n_comp}", r_max, rc, n, n_comp, kind)


CASES = [
    _c("distinct", 3, 3, 1, 1), _c("distinct", 3, 3, 63, 3), _c("distinct", 138, 138, 257, 128),
    _c("distinct", 138, 60, 63, 2), _c("distinct", 266, 266, 1000, 266), _c("distinct", 266, 266, 63, 1),
    _c("ties2", 3, 3, 63, 2), _c("ties2", 138, 138, 257, 128), _c("ties2", 266, 266, 257, 2),
    _c("ties5", 138, 138, 63, 128), _c("ties5", 266, 266, 257, 128), _c("ties5", 138, 60, 257, 2),
    _c("negative", 3, 3, 63, 3), _c("negative", 138, 138, 257, 138), _c("negative", 266, 200, 63, 200),
    _c("tiny", 3, 3, 63, 3), _c("tiny", 138, 138, 1000, 128), _c("tiny", 266, 266, 257, 266),
    _c("zeros", 3, 3, 1, 1), _c("zeros", 138, 138, 257, 128),
    _c("exact", 3, 3, 63, 3), _c("exact", 3, 2, 1, 2), _c("exact", 138, 138, 1000, 128), _c("exact", 138, 138, 257, 138),
    _c("exact", 266, 266, 1000, 266), _c("exact", 266, 140, 257, 128),
]
IDS = [c.name for c in CASES]


def _orthogonal(rng, m):
    return np.linalg.qr(rng.standard_normal((m, m)))[0]


@functools.lru_cache(maxsize=None)
def inputs(c):
    """(evals en, U en x en, Bt n x rc), read-only.  Rows and columns rc .. en - 1 are the Gram's zero padding: eigenvalue 0,
    eigenvector e_j."""
    rng = np.random.default_rng([c.r_max, c.rc, c.n, c.n_comp, sum(map(ord, c.kind))])
    en, rc, n, k = c.en, c.rc, c.n, c.n_comp
    U = np.eye(en)
    evals = np.zeros(en)
    if c.kind == "exact":
        perm = rng.permutation(rc)
        U[:rc, :rc] = np.eye(rc)[:, perm]
        # powers of 4 with repeats (equal eigenvalues go by index): sigma over 2^-9 .. 2^9, far above the 1e-12 line
        evals[:rc] = 4.0 ** rng.integers(-9, 10, rc)
        Bt = rng.integers(-7, 8, (n, rc)).astype(np.float64)
        pairs = [(0, n - 1), (63, 64), (255, 256), (5, 261), (64, 128), (300, 44), (n - 1, n - 2), (256, 0)]
        for j in range(rc):      # column j holds +-9 at two rows, above every other magnitude: the first of them decides
            p, q = pairs[j % len(pairs)]
            p, q = p % n, q % n
            s = 1.0 if (j // len(pairs)) % 2 == 0 else -1.0
            Bt[p, j] = 9.0 * s
            if q != p:
                Bt[q, j] = -9.0 * s
    else:
        U[:rc, :rc] = _orthogonal(rng, rc)
        lam = np.sort(rng.uniform(0.5, 100.0, rc))[::-1].copy()
        cut = min(k, rc - 1)                      # sorted positions cut - 1 and cut straddle the n_comp cut
        if c.kind == "ties2":
            lam[cut] = lam[cut - 1]                   # across the cut
            if cut >= 4:
                lam[1] = lam[0]                       # inside
        elif c.kind == "ties5":
            lo = max(cut - 2, 0)
            lam[lo:lo + 5] = lam[lo]                  # five equal ones across the cut
            if lo >= 8:
                lam[2:7] = lam[2]                     # and five inside
        elif c.kind == "negative":
            lam[rc // 2:] = -lam[rc // 2:] * np.where(np.arange(rc - rc // 2) % 2, 1e-15, 1.0)   # rounding-sized and large ones
        elif c.kind == "tiny":
            lam[rc // 3:] = lam[0] * 1e-26 * np.linspace(1.0, 0.5, rc - rc // 3)
        elif c.kind == "zeros":
            lam[:] = 0.0
        evals[:rc] = lam[rng.permutation(rc)]     # the solver hands them over unsorted
        Bt = rng.standard_normal((n, rc))
    Bt = np.ascontiguousarray(Bt)
    for a in (evals, U, Bt):
        a.setflags(write=False)
    return evals, U, Bt


@dataclasses.dataclass(frozen=True)
class Ref:
    order: np.ndarray
    sigma: np.ndarray     # n_comp, longdouble
    V: np.ndarray         # n x n_comp longdouble, signs applied
    bound: np.ndarray     # n x n_comp
    dropped: np.ndarray   # n_comp bool: the column is exactly zero
    sign_margin: float    # min over the kept columns of (largest - second largest magnitude) / (their two bounds); inf if exact
    drop_margin: float    # min | log2(sigma_i / (1e-12 sigma_0)) | over the positive sigmas


@functools.lru_cache(maxsize=None)
def reference(c):
    evals, U, Bt = inputs(c)
    rc, k = c.rc, c.n_comp
    order = np.argsort(-evals, kind="stable")
    sig_all = np.sqrt(np.maximum(evals.astype(LD), 0))
    sigma = sig_all[order[:k]]
    s0 = sig_all[order[0]]
    keep = (sigma > LD(DROP_REL) * s0) & (sigma > 0)
    Cm = np.zeros((rc, k), dtype=LD)
    Cm[:, keep] = U[:rc, order[:k][keep]].astype(LD) / sigma[keep]
    Bl = Bt.astype(LD)
    V = Bl @ Cm
    bound = (rc + 2) * EPS * (np.abs(Bl) @ np.abs(Cm))
    mag = np.abs(V)
    first = mag.argmax(axis=0)                        # first index of the largest magnitude
    sign = np.where(V[first, np.arange(k)] < 0, -1.0, 1.0)
    margin = np.inf
    if c.kind != "exact" and c.n > 1:
        for i in np.flatnonzero(keep):
            two = np.argsort(-mag[:, i], kind="stable")[:2]
            margin = min(margin, float((mag[two[0], i] - mag[two[1], i]) / (bound[two[0], i] + bound[two[1], i])))
    pos = sig_all[sig_all > 0]
    drop_margin = float(np.min(np.abs(np.log2((pos / (LD(DROP_REL) * s0)).astype(np.float64))))) if len(pos) else np.inf
    return Ref(order, sigma, V * sign, bound, ~keep, margin, drop_margin)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_no_case_is_decided_by_rounding(c):
    ref = reference(c)
    print(f"{c.name}: sign margin {ref.sign_margin:.3g} bounds, drop margin 2^{ref.drop_margin:.3g}")
    assert ref.sign_margin > 2.0
    assert ref.drop_margin > 1.0


def test_cases_reach_what_they_promise():
    assert {c.en for c in CASES} == {4, 138, 266} and any(c.en > c.rc for c in CASES)
    assert {c.n for c in CASES} == {1, 63, 257, 1000}
    assert {1, 2, 128} <= {c.n_comp for c in CASES} and any(c.n_comp == c.rc for c in CASES)
    for c in CASES:
        evals, _, _ = inputs(c)
        ref = reference(c)
        srt = evals[ref.order]
        k = c.n_comp
        if c.kind in ("ties2", "ties5"):
            run = 2 if c.kind == "ties2" else 5
            assert k < c.en and srt[k - 1] == srt[k] and srt[k - 1] > 0, "equal eigenvalues across the cut"
            same = np.flatnonzero(srt == srt[k - 1])
            assert len(same) >= run and np.all(np.diff(ref.order[same]) > 0), "and they are taken by ascending index"
            assert c.rc < 8 or np.any(np.diff(ref.order[:c.rc]) < 0), "which is not the order of the others"
        if c.kind == "negative":
            assert (srt[:k] < 0).any() and ref.dropped.any()
        if c.kind == "tiny":
            assert ref.dropped.any() and (ref.sigma[ref.dropped] > 0).all()
        if c.kind == "zeros":
            assert ref.dropped.all()
        if c.kind == "exact":
            assert len(np.unique(evals[:c.rc])) < c.rc or c.rc < 4, "repeated powers of 4"
            assert not ref.dropped.any() and np.all(ref.bound >= 0)
            assert np.array_equal(ref.V, np.round(ref.V * 2.0 ** 30) / 2.0 ** 30), "nothing to round"
    assert any(c.kind == "ties5" and c.n_comp > 8 for c in CASES), "five equal eigenvalues inside the cut too"


# ---- on the device ---------------------------------------------------------------------------------------------------
def P(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def handles():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    made = {}
    for r_max in sorted({c.r_max for c in CASES}):
        h = C.c_void_p()
        _lib.call("mused_rsvd_create", N_MAX, r_max, 1, 0, C.byref(h))
        made[r_max] = h
    yield made
    for h in made.values():
        _lib.call("mused_rsvd_destroy", h)


def select(h, c):
    from mused_amd import _lib

    evals, U, Bt = inputs(c)
    dev = [torch.from_numpy(np.array(a, order="C")).cuda() for a in (evals, U, Bt)]
    nv = c.n * c.n_comp
    dV = torch.full((nv + GUARD,), SENT, dtype=torch.float64, device="cuda")
    dS = torch.full((c.n_comp + GUARD,), SENT, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.call("mused_rsvd_select", h, P(dev[0]), P(dev[1]), P(dev[2]), c.n, c.rc, c.n_comp, P(dV), P(dS), st)
    torch.cuda.synchronize()
    V, sig = dV.cpu().numpy(), dS.cpu().numpy()
    assert np.all(V[nv:] == SENT) and np.all(sig[c.n_comp:] == SENT), "written behind an output"
    return V[:nv].reshape(c.n, c.n_comp), sig[:c.n_comp]


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_selection_tail(handles, c):
    ref = reference(c)
    V, sig = select(handles[c.r_max], c)
    assert np.isfinite(V).all() and np.isfinite(sig).all()
    # sigma
    assert np.all(np.diff(sig) <= 0) and np.all(sig >= 0)
    assert np.all(np.abs(sig.astype(LD) - ref.sigma) <= EPS * ref.sigma)
    # dropped columns are exactly zero
    assert np.all(V[:, ref.dropped] == 0.0)
    # every column in svd_flip's normal form: its first entry of largest magnitude is not negative
    first = np.abs(V).argmax(axis=0)
    assert np.all(V[first, np.arange(c.n_comp)] >= 0.0)
    if c.kind == "exact":
        assert np.array_equal(sig, ref.sigma.astype(np.float64))
        assert np.array_equal(V, ref.V.astype(np.float64)), "order, signs and values, nothing rounds"
    else:
        err = np.abs(V.astype(LD) - ref.V)
        worst = float(np.max(np.where(ref.bound > 0, err / np.where(ref.bound > 0, ref.bound, 1), np.where(err > 0, np.inf, 0))))
        print(f"{c.name}: max |V - ref| / bound = {worst:.3g}")
        assert worst <= 1.0


@pytest.mark.gpu
def test_argument_checks(handles):
    from mused_amd import _lib

    Lib = _lib.lib()
    h = handles[3]
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n, r, k in [(0, 3, 1), (N_MAX + 1, 3, 1), (10, 4, 1), (10, 0, 1), (10, 3, 4), (10, 3, 0)]:
        assert Lib.mused_rsvd_select(h, P(buf), P(buf), P(buf), n, r, k, P(buf), P(buf), st) != 0
        assert b"mused_rsvd_select" in Lib.mused_last_error()
    assert Lib.mused_rsvd_select(h, None, P(buf), P(buf), 10, 3, 1, P(buf), P(buf), st) != 0
    torch.cuda.synchronize()
