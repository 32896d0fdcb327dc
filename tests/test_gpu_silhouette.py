"""mused_silhouette and mused_cluster_indices (csrc/silhouette.hip) through the C ABI against scikit-learn's
silhouette_samples, davies_bouldin_score and calinski_harabasz_score, within the bound of tests/silhouette_cases.py: every
case, the flags, bitwise reproducibility, a permutation of the rows, the workspace, a stream of the caller's."""
import ctypes as C
import functools

import numpy as np
import pytest

import silhouette_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def A(b):
    return (b + 255) & ~255


def slices(n):
    """Column slices of mused_silhouette: about 512 workgroups below 256 row tiles, at most 16, one from 256 tiles on."""
    tiles = (n + 127) // 128
    return 1 if tiles >= 256 else min(tiles, 512 // tiles, 16)


def _ws_common(n, d):
    return (4 * A(4 * n) + A(4 * 256 * ((n + 1023) // 1024)) + A(4 * n) + A(4 * (n + 1)) + A(16) + A(8 * n)
            + A(8 * n * ((d + 1) // 2 * 2)))


def ws_silhouette(n, d):
    """The workspace of mused_silhouette, array by array (each on a multiple of 256 bytes)."""
    return _ws_common(n, d) + (A(8 * 4 * slices(n) * n) if slices(n) > 1 else 0)


def ws_indices(n, d):
    return _ws_common(n, d) + A(8 * n * d) + A(8 * d) + 5 * A(8 * n)


def _pitched(X, pitch):
    """X on the device with rows `pitch` doubles apart; the padding holds NaN, which nothing may read."""
    buf = torch.full((len(X), pitch), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, : X.shape[1]] = torch.tensor(X, device="cuda")
    return buf


def run(X, labels, ld=None, stream=None):
    """Both entries once: (samples, silhouette info bytes, out, indices info) as NumPy, outputs pre-filled with -7 and a canary
    behind each workspace."""
    from mused_amd import _lib
    from mused_amd.engine import ptr

    n, d = X.shape
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        Xd = _pitched(X, ld or d)
        lab = torch.tensor(np.asarray(labels, dtype=np.int32), device="cuda")
        nb_s, nb_i = int(_lib.lib().mused_silhouette_ws_bytes(n, d)), int(_lib.lib().mused_cluster_indices_ws_bytes(n, d))
        assert nb_s == ws_silhouette(n, d) and nb_i == ws_indices(n, d)          # the query is exact
        ws_s = torch.full((nb_s + CANARY,), 0xa5, dtype=torch.uint8, device="cuda")   # the workspace carries nothing
        ws_i = torch.full((nb_i + CANARY,), 0xa5, dtype=torch.uint8, device="cuda")
        samples = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
        info_s = torch.full((16,), 0x77, dtype=torch.uint8, device="cuda")
        out = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
        info_i = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        sp = C.c_void_p(st.cuda_stream)
        _lib.call("mused_silhouette", ptr(Xd), n, d, Xd.stride(0), ptr(lab), ptr(samples), ptr(info_s), ptr(ws_s), nb_s, sp)
        _lib.call("mused_cluster_indices", ptr(Xd), n, d, Xd.stride(0), ptr(lab), ptr(out), ptr(info_i), ptr(ws_i), nb_i, sp)
        st.synchronize()
        assert (ws_s[nb_s:] == 0xa5).all() and (ws_i[nb_i:] == 0xa5).all()       # nothing written behind ws_bytes
        return samples.cpu().numpy(), info_s.cpu().numpy(), out.cpu().numpy(), info_i.cpu().numpy()


def head(info_s):
    """(flags, clusters, sum) of mused_silhouette's info_out."""
    return int(info_s[:4].view(np.int32)[0]), int(info_s[4:8].view(np.int32)[0]), float(info_s[8:].view(np.float64)[0])


@functools.lru_cache(maxsize=None)
def device_result(name):
    c = next(c for c in sc.CASES if c.name == name)
    return run(c.X, c.labels, c.ld)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.CASE_IDS)
def test_every_case_matches_sklearn(case):
    ref_s, ref_db, ref_ch = sc.reference(case.name)
    sb, score_b, db_b, ch_b = sc.bounds(case.name)
    samples, info_s, out, info_i = device_result(case.name)
    flags, clusters, total = head(info_s)
    err = np.abs(samples - ref_s)
    print(f"{case.name}: samples max err {err.max():.3e} (bound at it {sb[err.argmax()]:.3e}), score err "
          f"{abs(total / case.n - ref_s.mean()):.3e} / {score_b:.3e}, DB err {abs(out[0] - ref_db):.3e} / {db_b:.3e}, CH rel err "
          f"{abs(out[1] - ref_ch) / abs(ref_ch):.3e} / {ch_b:.3e}")
    assert flags == 0 and clusters == len(np.unique(case.labels))
    assert tuple(info_i) == (0, clusters, 0, 0)
    assert (err <= sb).all()
    assert abs(total / case.n - ref_s.mean()) <= score_b
    assert abs(out[0] - ref_db) <= db_b
    assert abs(out[1] - ref_ch) <= ch_b * abs(ref_ch)


MULTI_TILE = ["n257_d17_straddle", "n384_d50_aligned", "n1000_d129", "n130_129_labels", "singletons"]


@pytest.mark.parametrize("name", MULTI_TILE)
def test_without_column_slices(name, monkeypatch):
    """The path of n > 32,640 (one slice: the tile kernel settles every cluster itself), taken here by MUSED_SIL_SLICES=1 at
    sizes scikit-learn scores in no time; by default these cases run 2, 3 and 8 slices."""
    from mused_amd import _lib

    c = next(c for c in sc.CASES if c.name == name)
    assert _lib.lib().mused_silhouette_slices(c.n) == slices(c.n) > 1
    monkeypatch.setenv("MUSED_SIL_SLICES", "1")
    samples, info_s, _, _ = run(c.X, c.labels, c.ld)
    ref_s = sc.reference(name)[0]
    sb, score_b, _, _ = sc.bounds(name)
    assert head(info_s)[0] == 0
    assert (np.abs(samples - ref_s) <= sb).all() and abs(head(info_s)[2] / c.n - ref_s.mean()) <= score_b
    assert (np.abs(samples - device_result(name)[0]) <= sb).all()


def test_slice_counts():
    from mused_amd import _lib

    q = _lib.lib().mused_silhouette_slices
    assert [q(n) for n in (1, 128, 129, 257, 1000, 2048, 4096, 10000, 20000, 32640, 32641, 150000, 1 << 19)] \
        == [1, 1, 2, 3, 8, 16, 16, 6, 3, 2, 1, 1, 1]
    assert q(0) == -1 and q((1 << 19) + 1) == -1
    assert all(q(n) == slices(n) for n in range(1, 40000, 127))


def test_conventions_on_the_device():
    by = {c.name: c for c in sc.CASES}
    c = by["singletons"]
    s = device_result(c.name)[0]
    alone = np.isin(c.labels, [0, 1, 3])
    assert (s[alone] == 0.0).all() and (s[~alone] != 0.0).all()
    s, _, out, _ = device_result("all_identical_integers")
    assert (s == 1.0).all() and out[0] == 0.0 and out[1] == 1.0


@pytest.mark.parametrize("name,X,labels,text", sc.error_cases(), ids=[e[0] for e in sc.error_cases()])
def test_flags_and_untouched_outputs(name, X, labels, text):
    samples, info_s, out, info_i = run(X, labels)
    flags, clusters, total = head(info_s)
    want = 2 if "contains" in text else 4
    assert flags & want and info_i[0] & want
    if want == 4:
        assert flags == 4 and clusters == len(np.unique(labels)) == info_i[1]
    assert (samples == -7.0).all() and (out == -7.0).all() and total != total


@pytest.mark.parametrize("name", ["n257_d17_straddle", "n130_129_labels", "n1000_d129"])
def test_two_calls_give_the_same_bytes(name):
    c = next(c for c in sc.CASES if c.name == name)
    first, again = device_result(name), run(c.X, c.labels, c.ld)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["n257_d17_straddle", "singletons", "duplicates_across_and_within"])
def test_permuted_rows_give_permuted_samples(name):
    c = next(c for c in sc.CASES if c.name == name)
    p = np.random.default_rng(5).permutation(c.n)
    samples, info_s, out, _ = run(c.X[p], c.labels[p], c.ld)
    base, _, base_out, _ = device_result(name)
    sb, score_b, db_b, ch_b = sc.bounds(name)
    assert (np.abs(samples - base[p]) <= sb[p]).all()
    assert abs(head(info_s)[2] - head(device_result(name)[1])[2]) / c.n <= score_b
    assert abs(out[0] - base_out[0]) <= db_b and abs(out[1] - base_out[1]) <= ch_b * abs(base_out[1])


def test_workspace_queries_and_refusals():
    from mused_amd import _lib
    from mused_amd._lib import MusedError

    L = _lib.lib()
    for q in (L.mused_silhouette_ws_bytes, L.mused_cluster_indices_ws_bytes):
        assert q(0, 4) == -1 and q((1 << 19) + 1, 4) == -1 and q(10, 0) == -1 and q(10, 1 << 20) == -1
        assert q(1 << 19, 50) > 0
    from mused_amd.engine import ptr

    c = next(c for c in sc.CASES if c.name == "n128_d15")
    n, d = c.X.shape
    Xd, lab = torch.tensor(c.X, device="cuda"), torch.tensor(c.labels, device="cuda")
    out = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    ws = torch.full((ws_indices(n, d),), 0xa5, dtype=torch.uint8, device="cuda")
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # ws_bytes - 1, a pitch below d, n and d outside the domain: refused with an error code, nothing launched
    for entry, need in (("mused_silhouette", ws_silhouette(n, d)), ("mused_cluster_indices", ws_indices(n, d))):
        for n_, d_, ld_, nb in ((n, d, d, need - 1), (n, d, d - 1, need), (0, d, d, need), (n, 0, d, need)):
            with pytest.raises(MusedError):
                _lib.call(entry, ptr(Xd), n_, d_, ld_, ptr(lab), ptr(out), ptr(info), ptr(ws), nb, sp)
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (info == -7).all() and (ws == 0xa5).all()


def test_on_a_stream_of_the_callers():
    c = next(c for c in sc.CASES if c.name == "n1000_d129")
    st = torch.cuda.Stream()
    got = run(c.X, c.labels, c.ld, stream=st)
    for a, b in zip(device_result(c.name), got):
        assert a.tobytes() == b.tobytes()
