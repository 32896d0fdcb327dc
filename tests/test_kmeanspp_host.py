"""Host half of the device k-means++ seeding (no GPU): `kmeanspp_draws` takes from RandomState(seed) exactly what
`sklearn.cluster.kmeans_plusplus` takes, in the same order, and a replay of `_kmeans_plusplus` fed those draws instead of
a generator picks scikit-learn's rows."""
import numpy as np
import pytest
from sklearn.cluster import kmeans_plusplus
from sklearn.datasets import make_blobs

from mused_amd import matrix_operations as mo

CASES = [(500, 2), (2000, 8), (300, 150), (1024, 1024)]


def replay_kmeanspp(X, k, first, U):
    """sklearn 1.7 `_kmeans_plusplus` (unit weights) with the draws handed in: row indices of the k centres."""
    n = X.shape[0]
    xsq = np.einsum("ij,ij->i", X, X)

    def dist(rows):
        D = -2.0 * (X[rows] @ X.T)
        D += xsq[rows][:, None]
        D += xsq[None, :]
        return np.maximum(D, 0.0)

    indices = np.full(k, -1, dtype=int)
    indices[0] = first
    closest = dist(np.array([first]))[0]
    pot = closest.sum()
    for c in range(1, k):
        cand = np.searchsorted(np.cumsum(closest, dtype=np.float64), U[c - 1] * pot)
        np.clip(cand, None, n - 1, out=cand)
        D = np.minimum(closest, dist(cand))
        pots = D.sum(axis=1)
        best = int(np.argmin(pots))
        pot, closest, indices[c] = pots[best], D[best], cand[best]
    return indices


@pytest.mark.parametrize("n,k", CASES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_draws_leave_the_generator_where_sklearn_leaves_it(n, k, seed):
    X = np.random.RandomState(100 + seed).standard_normal((n, 4))
    rs = np.random.RandomState(seed)
    _, idx = kmeans_plusplus(X, k, random_state=rs)
    first, U = mo.kmeanspp_draws(n, k, seed)
    assert U.shape == (k - 1, 2 + int(np.log(k))) and U.dtype == np.float64
    assert first == idx[0]
    mine = np.random.RandomState(seed)   # handed in as the generator: advanced by the same draws
    f2, U2 = mo.kmeanspp_draws(n, k, mine)
    assert f2 == first and np.array_equal(U2, U)
    a, b = rs.get_state(), mine.get_state()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("n,k", [c for c in CASES if c[0] >= 10 * c[1]])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_replay_with_the_draws_picks_sklearns_rows(n, k, seed):
    X, _ = make_blobs(n, 16, centers=max(k, 3), random_state=seed)
    X = X - X.mean(axis=0)
    _, idx = kmeans_plusplus(X, k, random_state=np.random.RandomState(seed))
    first, U = mo.kmeanspp_draws(n, k, seed)
    assert np.array_equal(replay_kmeanspp(X, k, first, U), idx)
