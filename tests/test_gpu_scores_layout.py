"""mused_row_sq_norms, mused_pairwise_scores, mused_knn_topk and mused_knn_fused on the cases of tests/scores_cases.py:
the same values under four layouts (pitch d, pitch d + 3, no row on a 16-byte line, every row on one; NaN wherever no value
lies) must give the same bits, duplicate rows the same norms and scores, everything within the rounding band of the
longdouble reference, and neighbour lists that are valid for that band and break the planted ties by column.

Measured on the MI355X, largest |device - reference| over its band across the twelve cases and four layouts: norms 0.068,
squared L2 0.231, cosine 0.184 (of 1).  When row_sqnorm_kernel still summed rows on a 16-byte line in another order than the
rest, test_layout_independence_and_accuracy failed for float32 at d = 9, 33, 50, 130 and for float64 at d = 3, 9, 33, 50, 130
(norms, and with them both scores, of the layouts whose rows do not all start on a line; planted pairs with two norms at
pitch d or d + 3 wherever that pitch is no multiple of a line), and test_selection_under_every_layout for all of those but
float32 d = 9 and float64 d = 33.  d = 1 (both types) and float32 d = 3 passed: a lane holds one term in either order."""
import ctypes as C

import numpy as np
import pytest

import scores_cases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd import _lib

    return _lib


def P(t):
    return C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def place(dtype, d, name):
    """The rows of a case in layout `name` on the device: (tensor that owns the memory, pointer to row 0, pitch)."""
    buf, off, ld = sc.layout(sc.rows(dtype, d), name)
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    ptr = t.data_ptr() + off * buf.dtype.itemsize
    assert np.array_equal((ptr + np.arange(sc.N) * ld * buf.dtype.itemsize) % 16, sc.line_offsets(dtype, d, name))
    return t, C.c_void_p(ptr), ld


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def worst(err, band):
    err, band = np.abs(np.asarray(err, dtype=sc.LD)), np.asarray(band, dtype=sc.LD) * np.ones_like(err)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(band > 0, err / np.where(band > 0, band, 1), np.where(err > 0, np.inf, 0.0))
    return float(np.max(q))


@pytest.mark.parametrize("dtype,d", sc.CASES, ids=sc.IDS)
def test_layout_independence_and_accuracy(L, dtype, d):
    dt = L.F32 if dtype == np.float32 else L.F64
    n = sc.N
    out = {}
    for name in sc.LAYOUTS:
        keep, ptr, ld = place(dtype, d, name)
        nrm = torch.full((n + 1,), np.nan, dtype=torch.float64, device="cuda")
        ws = torch.full((n + 1,), np.nan, dtype=torch.float64, device="cuda")
        l2 = torch.full((n * n + 1,), np.nan, dtype=torch.float64, device="cuda")
        cos = torch.full((n * n + 1,), np.nan, dtype=torch.float64, device="cuda")
        L.call("mused_row_sq_norms", ptr, dt, n, d, ld, P(nrm), S())
        L.call("mused_pairwise_scores", ptr, dt, n, d, ld, L.METRIC_L2, P(ws), P(l2), S())
        L.call("mused_pairwise_scores", ptr, dt, n, d, ld, L.METRIC_COSINE, P(ws), P(cos), S())
        torch.cuda.synchronize()
        nrm, l2, cos = nrm.cpu().numpy(), l2.cpu().numpy(), cos.cpu().numpy()
        assert np.isnan(nrm[n]) and np.isnan(l2[n * n]) and np.isnan(cos[n * n]), "written past the outputs"
        out[name] = (nrm[:n], l2[:n * n].reshape(n, n), cos[:n * n].reshape(n, n))
        del keep
    rn, rl, rc = sc.reference(dtype, d)
    bn, bl, bc = sc.bands(dtype, d)
    report, nan_free = [], True
    for name in sc.LAYOUTS:
        nrm, l2, cos = out[name]
        nan_free = nan_free and not (np.isnan(nrm).any() or np.isnan(l2).any() or np.isnan(cos).any())
        report.append((name, worst(nrm - rn, bn), worst(l2 - rl, bl), worst(cos - rc, bc)))
        print(f"{sc.IDS[sc.CASES.index((dtype, d))]} {name}: |dev - ref| / band  norms {report[-1][1]:.3f}  l2 {report[-1][2]:.3f}  "
              f"cosine {report[-1][3]:.3f}")
    diff = {what: [name for name in sc.LAYOUTS if not np.array_equal(bits(out[name][i]), bits(out["aligned"][i]))]
            for i, what in enumerate(("norms", "l2", "cosine"))}
    pairs = {name: [(a, b) for a, b in sc.PAIRS if bits(out[name][0])[a] != bits(out[name][0])[b]] for name in sc.LAYOUTS}
    print("layouts that differ from 'aligned':", diff, " pairs with two norms:", pairs)

    assert nan_free, "NaN from the padding reached an output"
    # layout independence, exact
    assert diff == {"norms": [], "l2": [], "cosine": []}
    for name in sc.LAYOUTS:
        nrm, l2, cos = out[name]
        assert pairs[name] == [], name
        for a, b in sc.PAIRS:
            for M in (l2, cos):
                assert np.array_equal(bits(M[:, a]), bits(M[:, b])), (name, a, b, "columns")
                assert np.array_equal(bits(M[a, :]), bits(M[b, :])), (name, a, b, "rows")
    # accuracy against the longdouble reference
    for name, qn, ql, qc in report:
        assert qn <= 1 and ql <= 1 and qc <= 1, (name, qn, ql, qc)


def _topk(L, ptr, dt, d, ld, k, metric):
    n = sc.N
    w = (n + 63) // 64 + 2
    ws = torch.empty(n * n, dtype=torch.float64, device="cuda")
    nr = torch.empty(n, dtype=torch.float64, device="cuda")
    idx = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
    mask = torch.full((n, w), -1, dtype=torch.int64, device="cuda")
    L.call("mused_knn_topk", ptr, dt, n, d, ld, k, metric, P(ws), P(nr), P(idx), P(mask), w, S())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), mask.cpu().numpy().view(np.uint64)


def _fused(L, ptr, dt, d, ld, k, metric):
    n, cap = sc.N, 1024
    nb = L.lib().mused_knn_fused_ws_bytes(n, cap)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    w = (n + 63) // 64 + 2
    idx = torch.full((n, k), -1, dtype=torch.int32, device="cuda")
    mask = torch.full((n, w), -1, dtype=torch.int64, device="cuda")
    ovf = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    L.call("mused_knn_fused", ptr, dt, n, d, ld, k, metric, P(ws), nb, cap, P(idx), P(mask), w, P(ovf), S())
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    return idx.cpu().numpy(), mask.cpu().numpy().view(np.uint64)


def _mask_of(idx, words):
    import adjacency_cases as ac

    sel = np.zeros((sc.N, sc.N), dtype=bool)
    np.put_along_axis(sel, idx.astype(np.int64), True, axis=1)
    np.fill_diagonal(sel, False)
    return ac.pack(sel, words)


@pytest.mark.parametrize("dtype,d", sc.CASES, ids=sc.IDS)
def test_selection_under_every_layout(L, dtype, d):
    dt = L.F32 if dtype == np.float32 else L.F64
    placed = {name: place(dtype, d, name) for name in sc.LAYOUTS}
    for metric in sc.METRICS:
        for k in sc.KS:
            for entry in (_topk, _fused):
                got = {name: entry(L, placed[name][1], dt, d, placed[name][2], k, metric) for name in sc.LAYOUTS}
                idx0, mask0 = got["aligned"]
                for name in sc.LAYOUTS:
                    assert np.array_equal(got[name][0], idx0), (entry.__name__, metric, k, name, "lists differ between layouts")
                    assert np.array_equal(got[name][1], mask0), (entry.__name__, metric, k, name, "masks differ between layouts")
                sc.check_topk(dtype, d, metric, k, idx0)
                assert np.array_equal(mask0, _mask_of(idx0, mask0.shape[1])), (entry.__name__, metric, k)
