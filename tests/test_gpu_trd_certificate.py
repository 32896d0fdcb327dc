"""The neighbour-cosine rule of the direct eigensolver's certificate (csrc/trd.hip, kernel D) on its own: a double or triple
eigenvalue is too small a cluster for the cluster rule (6 eigenvalues), so only the cosines between the vectors of neighbours
in the spectrum can send such a matrix to the Jacobi solver.  Kernel D forms them from its register tiles -- columns c + 1 ..
c + 4 by lane shuffles inside a wave's 16 columns, through LDS across a wave boundary -- and the groups below sit inside a
wave, across several wave boundaries, and in the last wave."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_trd import run_trd  # noqa: E402

GROUPS = {                         # first and last index of the eigenvalues that are made equal
    "pair_5_6": (5, 6),            # inside wave 0
    "pair_15_16": (15, 16),        # across waves 0 | 1: the only pair is a crossing one
    "triple_15_17": (15, 17),      # across, distances 1 and 2
    "five_12_16": (12, 16),        # across, up to distance 4
    "pair_31_32": (31, 32),        # across waves 1 | 2
    "pair_63_64": (63, 64),        # across waves 3 | 4
    "pair_111_112": (111, 112),    # across waves 6 | 7
    "pair_120_121": (120, 121),    # inside the last wave
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_multiple_eigenvalues_below_the_cluster_size_are_rejected_by_the_cosines():
    rng = np.random.default_rng(5)
    Q = np.linalg.qr(rng.standard_normal((256, 256)))[0]
    Gs = []
    for grp in list(GROUPS.values()) + [()]:
        w = np.linspace(9.0, 1.0, 256)
        if grp:
            w[grp[0]:grp[-1] + 1] = w[grp[0]]     # indices grp[0] .. grp[-1]: one eigenvalue, at most 5-fold
        G = (Q * w) @ Q.T
        Gs.append(0.5 * (G + G.T))
    out, d, e, lam, res, done = run_trd(Gs)
    for b, name in enumerate(GROUPS):
        assert done[b] == 0, name                       # vectors of one eigenspace: not orthogonal to 1e-8
        assert np.array_equal(out[b], Gs[b]), name      # ... and the input is left for the Jacobi solver
    assert done[-1] == 1                                # the same spectrum without a multiple eigenvalue is certified
    V = out[-1][:128].T / np.linalg.norm(out[-1][:128].T, axis=0)
    assert np.abs(V.T @ V - np.eye(128)).max() < 1e-9
