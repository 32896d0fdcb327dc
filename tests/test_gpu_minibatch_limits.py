"""On the GPU: the MiniBatchKMeans kernels (csrc/minibatch.hip) through their C entries at the declared limits
(k <= 1024, d <= 512): the E step against an argmin with a rounding bound and on exact ties, the ordered centre update
bitwise against a NumPy replica of scikit-learn's update_center_dense, the reassignment, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = np.finfo(np.float64).eps
MUSED_ERR_ARG = -1
LAB_SENT = -7


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows_dev(X, ld):
    """X (n x d) in a device buffer of pitch ld >= d (padding NaN: a read outside the rows poisons the result)."""
    n, d = X.shape
    buf = np.full((n, ld), np.nan)
    buf[:, :d] = X
    return dev(buf)


def ws_for(L, n, d, k):
    return torch.empty(int(L.lib().mused_mbkm_ws_bytes(n, d, k)), dtype=torch.uint8, device="cuda")


def assign(L, Xd, ld, n, d, k, Cd):
    lab = torch.full((n + 5,), LAB_SENT, dtype=torch.int32, device="cuda")
    ws = ws_for(L, n, d, k)
    L.call("mused_kmeans_assign", P(Xd), ld, n, d, k, P(Cd), P(lab), P(ws), ws.numel(), S())
    out = host(lab)
    assert (out[n:] == LAB_SENT).all(), "labels written past n"
    return out[:n]


def assign_tiles(d, k):
    """Python copy of km_stream_tiles (csrc/kmeans_common.h) with the budget of csrc/minibatch.hip: (TR rows,
    PT = 256 / TR lanes per row, KT centres per tile)."""
    cap = 17920 // (d + 1)
    for tr in (32, 16):
        pt = 256 // tr
        kt = cap - tr
        kt = k if kt >= k else (kt // pt) * pt
        if kt >= 1 and (kt >= pt or kt == k):
            return tr, pt, kt
    raise AssertionError("no tile")


# ------------------------------------------------------------------ E step ----------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 15, 16, 17, 1023, 1024])
@pytest.mark.parametrize("d", [1, 255, 256, 257, 447, 448, 511, 512])
def test_assign_against_argmin(L, d, k):
    """Labels of mused_kmeans_assign against argmin_j |c_j|^2 - 2 x.c_j in NumPy: where the two best reference values are
    further apart than the rounding of both computations the label is the argmin; elsewhere the chosen centre is within
    the rounding of the minimum.  Half the centres are perturbed rows, so that many rows have close candidates."""
    n = 97
    rng = np.random.default_rng(d * 4096 + k)
    X = rng.standard_normal((n, d))
    Cc = rng.standard_normal((k, d))
    near = rng.choice(n, size=k // 2, replace=False) if k // 2 <= n else rng.integers(0, n, k // 2)
    Cc[: k // 2] = X[near] + 0.3 * rng.standard_normal((k // 2, d))
    ld = d + 3 if (d + k) % 2 else d
    lab = assign(L, rows_dev(X, ld), ld, n, d, k, dev(Cc))
    assert ((lab >= 0) & (lab < k)).all()
    csq = (Cc * Cc).sum(1)
    D = csq[None, :] - 2.0 * (X @ Cc.T)
    tol = 2 * (d + 2) * EPS * (csq[None, :] + 2.0 * (np.abs(X) @ np.abs(Cc).T))
    best = D.argmin(1)
    r = np.arange(n)
    lower = D - tol
    lower[r, best] = np.inf
    clear = lower.min(1) > D[r, best] + tol[r, best]
    assert np.array_equal(lab[clear], best[clear]), f"{np.count_nonzero(lab[clear] != best[clear])} clear rows mislabelled"
    assert (D[r, lab] - tol[r, lab] <= (D + tol).min(1)).all(), "a label is not within the rounding of the minimum"


def _tie_pairs(k, pt, kt):
    """Disjoint (a, b) pairs, b - a = off, a in lane `lane` of its row group: the same lane's pair (PT apart) and the same
    lane two pairs on (2 PT); other lanes of the row group (1, PT - 1, PT + 1 apart; mostly with the lower index in the
    highest lane, where a reduction that prefers the higher lane would show); other centre tiles (KT, KT + 1, 2 KT + 3)."""
    offs = [(pt, pt - 1), (2 * pt, pt - 1), (1, pt - 1), (1, 0), (pt - 1, pt - 1), (pt + 1, pt - 1), (kt, pt - 1),
            (kt + 1, 0), (2 * kt + 3, pt - 1)]
    used, pairs = set(), []
    for off, lane in offs:
        for q in range(k // pt + 1):
            a = q * pt + lane
            if off > 0 and a + off < k and a not in used and a + off not in used:
                pairs.append((a, a + off))
                used.update((a, a + off))
                break
    return pairs


@pytest.mark.parametrize("d,k", [(64, 1024), (447, 1024), (448, 1024), (512, 1024), (512, 300)])
def test_assign_exact_ties_lowest_index(L, d, k):
    """Bit-identical copies of a centre compute identical distances wherever they sit (same lane, other lane of the row
    group, other centre tile): the lowest index wins, as in scikit-learn."""
    tr, pt, kt = assign_tiles(d, k)
    pairs = _tie_pairs(k, pt, kt)
    assert len(pairs) >= 7 and any(b - a >= kt for a, b in pairs) and any(0 < b - a < pt for a, b in pairs)
    rng = np.random.default_rng(d + k)
    Cc = 3.0 * rng.standard_normal((k, d))
    for a, b in pairs:
        Cc[b] = Cc[a]
    reps = 5  # rows per pair: they fall in different rows of a row tile, so in different lane groups
    owner = np.repeat([a for a, _ in pairs], reps)
    X = Cc[owner] + 0.01 * rng.standard_normal((len(owner), d))
    n = len(owner)
    lab = assign(L, rows_dev(X, d + 1), d + 1, n, d, k, dev(Cc))
    assert np.array_equal(lab, owner), f"tr={tr} pt={pt} kt={kt}: rows {np.flatnonzero(lab != owner)} took {lab[lab != owner]}"


# ------------------------------------------------------------------ update ----------------------------------------------------
def replica_update(X, lab, C0, cnt0):
    """update_center_dense (scikit-learn _k_means_minibatch.pyx) in NumPy, one IEEE operation per step: per cluster with rows
    c * count, + x for its rows in sample order, count += rows, c * (1 / count); clusters without rows unchanged."""
    k = len(C0)
    m = np.bincount(lab, minlength=k)
    order = np.argsort(lab, kind="stable")
    start = np.concatenate([[0], np.cumsum(m)[:-1]])
    acc = C0 * cnt0[:, None]
    for s in range(int(m.max())):
        js = np.flatnonzero(m > s)
        acc[js] = acc[js] + X[order[start[js] + s]]
    C, cnt = C0.copy(), cnt0.copy()
    hit = m > 0
    cnt[hit] = cnt0[hit] + m[hit]
    C[hit] = acc[hit] * (1.0 / cnt[hit])[:, None]
    return C, cnt


@pytest.mark.parametrize("n,d,k,ld", [(2500, 255, 6, 258), (3000, 256, 5, 256), (2100, 257, 7, 261), (2600, 512, 6, 515),
                                      (1500, 512, 1, 512), (1100, 130, 1, 131), (1800, 300, 40, 300)])
def test_step_update_bitwise_replica(L, n, d, k, ld):
    """mused_mbkm_step: the labels are the E step's (mused_kmeans_assign on the same centres), and the centres and counts
    equal the NumPy replica fed the device's labels bit for bit.  n > 1024 (several list passes per cluster), clusters of
    more rows than one LDS slab (7168 / d), two far centres that get no rows, large non-integer counts."""
    rng = np.random.default_rng(n + d + k)
    mu = 4.0 * rng.standard_normal((k, d))
    X = mu[rng.integers(0, k, n)] + rng.standard_normal((n, d))
    C0 = np.concatenate([mu + 0.5 * rng.standard_normal((k, d)), 1e3 + rng.standard_normal((2, d))])
    kk = k + 2
    cnt0 = np.array([1e6 + 0.5, 123456.75, 3.0, 0.0, 7e9 + 0.25, 1.0, 2.5e5 + 0.125][: kk] + [99.5] * max(0, kk - 7))[:kk]
    cnt0 = rng.permutation(cnt0)
    Xd, Cd, cd = rows_dev(X, ld), dev(C0), dev(cnt0)
    lab_assign = assign(L, Xd, ld, n, d, kk, Cd)
    lab = torch.full((n + 5,), LAB_SENT, dtype=torch.int32, device="cuda")
    ws = ws_for(L, n, d, kk)
    L.call("mused_mbkm_step", P(Xd), ld, n, d, kk, P(Cd), P(cd), P(lab), P(ws), ws.numel(), S())
    lab = host(lab)
    assert (lab[n:] == LAB_SENT).all()
    lab = lab[:n]
    assert np.array_equal(lab, lab_assign)
    m = np.bincount(lab, minlength=kk)
    big = int(m.argmax())
    assert (m[k:] == 0).all() and m[big] > 7168 // d and len(np.unique(np.flatnonzero(lab == big) // 1024)) >= 2
    C_ref, cnt_ref = replica_update(X, lab, C0, cnt0)
    Cm, cm = host(Cd), host(cd)
    assert (bits(Cm[m == 0]) == bits(C0[m == 0])).all(), "a centre without rows changed"
    assert (bits(cm) == bits(cnt_ref)).all(), "counts differ from the replica"
    bad = (bits(Cm) != bits(C_ref)).any(1)
    assert not bad.any(), f"centres {np.flatnonzero(bad)} differ from the replica"


# ------------------------------------------------------------------ reassign --------------------------------------------------
def test_reassign_pairs_and_counts(L):
    """mused_mbkm_reassign: m = 0 writes the counts only; m = k copies the valid (src, dst) pairs, skips pairs with src
    outside [0, n) or dst outside [0, k), and writes the counts exactly."""
    n, d, k, ld = 300, 257, 40, 262
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, d))
    C0 = rng.standard_normal((k, d))
    cnt0 = rng.random(k) * 1e6
    Xd, Cd, cd = rows_dev(X, ld), dev(C0), dev(cnt0)
    # (every device buffer is held by a name until the kernel has run: a temporary freed at once can be handed to the
    # next allocation before the kernel reads it)
    new1 = rng.random(k) * 1e3
    new1_d = dev(new1)
    L.call("mused_mbkm_reassign", P(Xd), ld, n, d, k, None, None, 0, P(new1_d), P(Cd), P(cd), S())
    assert (bits(host(Cd)) == bits(C0)).all() and (bits(host(cd)) == bits(new1)).all()

    dst = rng.permutation(k).astype(np.int32)
    src = rng.integers(0, n, k).astype(np.int32)
    src[[0, 5, 9]] = [-1, n, n + 1000]
    dst[[2, 7, 11]] = [-1, k, -100000]
    new2 = rng.random(k) * 1e3
    src_d, dst_d, new2_d = dev(src), dev(dst), dev(new2)
    L.call("mused_mbkm_reassign", P(Xd), ld, n, d, k, P(src_d), P(dst_d), k, P(new2_d), P(Cd), P(cd), S())
    want = C0.copy()
    for s, g in zip(src, dst):
        if 0 <= s < n and 0 <= g < k:
            want[g] = X[s]
    assert (bits(host(Cd)) == bits(want)).all()
    assert (bits(host(cd)) == bits(new2)).all()


def test_limits_rejected_without_launch(L):
    """k = 1025 or d = 513: MUSED_ERR_ARG from the E step and the step, labels, centres and counts untouched."""
    lib = L.lib()
    for n, d, k in [(50, 4, 1025), (50, 513, 4)]:
        rng = np.random.default_rng(d + k)
        X, C0, cnt0 = rng.standard_normal((n, d)), rng.standard_normal((k, d)), rng.random(k)
        Xd, Cd, cd = dev(X), dev(C0), dev(cnt0)
        lab = torch.full((n,), LAB_SENT, dtype=torch.int32, device="cuda")
        ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
        assert lib.mused_kmeans_assign(P(Xd), d, n, d, k, P(Cd), P(lab), P(ws), ws.numel(), S()) == MUSED_ERR_ARG
        assert b"k <= 1024 and d <= 512" in lib.mused_last_error()
        assert lib.mused_mbkm_step(P(Xd), d, n, d, k, P(Cd), P(cd), P(lab), P(ws), ws.numel(), S()) == MUSED_ERR_ARG
        assert b"k <= 1024 and d <= 512" in lib.mused_last_error()
        assert (host(lab) == LAB_SENT).all()
        assert (bits(host(Cd)) == bits(C0)).all() and (bits(host(cd)) == bits(cnt0)).all()
