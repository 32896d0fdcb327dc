"""The direct eigensolver (csrc/trd.hip) bit for bit against a recording: tests/golden/trd_bits.npz holds d, e of the
tridiagonal matrix, the eigenvalues, the certificate's verdict and a SHA-256 of the returned matrix, as the solver produced
them before kernel D was shortened (certificate from the register tiles, double-buffered staging, coalesced stores).
Changes inside kernels A and D must leave every one of these bits alone.

The cases (tests/golden/make_trd_bits.py builds them: exact integer Gram matrices, the same on every host) reach every path
of a Householder step: all 254 steps with the register-block boundaries (full256), a run of identity reflectors in the
middle (blockdiag) and at every step (diagonal), a deflating tail (rank40), embedded orders whose first step falls inside a
block (n200), on the last column of a block (n129), near the end (n33, n2), and three different matrices in one launch."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_trd_bits", os.path.join(GOLDEN, "make_trd_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = ["full256", "blockdiag", "diagonal", "rank40", "n200", "n129", "n33", "n2", "batch3"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def recorded():
    return np.load(gen.FIXTURE, allow_pickle=False)


@pytest.fixture(scope="module")
def inputs():
    c = gen.cases()
    assert list(c) == CASES
    return c


@pytest.mark.parametrize("name", CASES)
def test_direct_solver_bits_match_the_recording(name, recorded, inputs):
    Gs, n, need = inputs[name]
    got, out = gen.record(name, Gs, n, need)
    done = got[f"{name}/done"]
    assert np.array_equal(done, recorded[f"{name}/done"]), (name, done)
    for key in ("d", "e", "lam"):
        a, b = got[f"{name}/{key}"], recorded[f"{name}/{key}"]
        assert a.dtype == np.int64 and a.shape == b.shape
        bad = np.argwhere(a != b)
        assert bad.size == 0, (name, key, len(bad), bad[:4].tolist())
    assert got[f"{name}/sha"].tolist() == recorded[f"{name}/sha"].tolist(), name
    for b, G in enumerate(Gs):
        if done[b] == 0:  # rejected: the recorded hash is that of the untouched input
            assert hashlib.sha256(np.ascontiguousarray(G).tobytes()).hexdigest() == str(recorded[f"{name}/sha"][b])
