"""mused_dbscan_incr_delete_rows (csrc/dbscan_incr.hip) against its specification (IncrementalSpec.delete_rows) and scikit-learn:
through the C ABI and through mused_amd.incdbscan.IncrementalDBSCAN (delete_rows, find, labels_of, by_value).  After EVERY
operation the labels of the rows held must EQUAL DBSCAN(eps, min_samples).fit_predict on those rows, count[] and the border
minima must equal the spec's, a delete's info word must equal the spec's and the rows packed into X_out must be the survivors,
bit for bit -- on streams that are checked on the CPU to hold no pair within the rounding margin of eps.  Shapes are chosen
against the kernel's 128-row tile and a staging panel of 128 rows."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import dbscan_incr_cases as ic
import dbscan_incr_delete_cases as dc
import dbscan_incr_delete_rows_cases as rc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DIMS = [1, 3, 50]
FLAG_LIST = 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


class CabiState:
    """The caller's side of mused_dbscan_incr_insert / _delete / _delete_rows: two row buffers with a row pitch (the padding
    holds NaN, which nothing may read), the rows held behind an offset of the current one; state arrays that start as garbage."""

    def __init__(self, d, ld, capacity, chunk):
        from mused_amd import _lib

        self.d, self.chunk, self.n, self.off, self.cur, self.capacity = d, chunk, 0, 0, 0, capacity
        self.bufs = [torch.full((capacity, ld or d), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
        self.nrm = torch.full((capacity,), float("nan"), dtype=torch.float64, device="cuda")
        self.count, self.parent, self.best, self.labels = (torch.full((capacity,), -7, dtype=torch.int32, device="cuda")
                                                           for _ in range(4))
        L = _lib.lib()
        self.rows_bytes = int(L.mused_dbscan_incr_delete_rows_ws_bytes(capacity, d, chunk))
        # O(n) beside the staging panel
        assert 0 < self.rows_bytes <= 56 * capacity + 4 * ((capacity + 127) // 128) + 4 * ((capacity + 1023) // 1024) \
            + 8 * chunk * (d + 1) + 17 * 256
        assert self.rows_bytes >= int(L.mused_dbscan_incr_delete_ws_bytes(capacity, d, chunk))
        self.nbytes = max(self.rows_bytes, int(L.mused_dbscan_incr_ws_bytes(capacity, d, chunk)))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def arrays(self):
        return (*self.bufs, self.nrm, self.count, self.parent, self.best, self.labels)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _call(self, name, a, b, eps, ms):
        from mused_amd import _lib
        from mused_amd.engine import ptr

        held = self.bufs[self.cur][self.off:]
        info = (C.c_int * 6)(*([-7] * 6))
        _lib.call(name, ptr(held), held.stride(0), self.d, ptr(self.nrm), ptr(self.count), ptr(self.parent), ptr(self.best), a, b,
                  float(eps), int(ms), self.chunk, ptr(self.labels), info, ptr(self.ws), self.nbytes, self._stream())
        return np.array(info[:])

    def insert(self, batch, eps, ms):
        n0, w = self.n, len(batch)
        self.bufs[self.cur][self.off + n0:self.off + n0 + w, :self.d] = torch.tensor(batch, device="cuda")
        info = self._call("mused_dbscan_incr_insert", n0, w, eps, ms)
        self.n = n0 + w
        return info

    def delete(self, m, eps, ms):
        info = self._call("mused_dbscan_incr_delete", self.n, m, eps, ms)
        self.n -= m
        self.off = self.off + m if self.n else 0
        return info

    def delete_rows(self, idx, eps, ms, m=None, ws_bytes=None, chunk=None, d=None, ld_out=None, out=None):
        """idx: the list as it is handed over (the caller sorts); m: the length given (default: len(idx))."""
        from mused_amd import _lib
        from mused_amd.engine import ptr

        dele = torch.tensor(np.asarray(idx, dtype=np.int32), device="cuda")
        m = len(dele) if m is None else m
        held = self.bufs[self.cur][self.off:]
        out = self.bufs[self.cur ^ 1] if out is None else out
        info = (C.c_int * 6)(*([-7] * 6))
        _lib.call("mused_dbscan_incr_delete_rows", ptr(held), held.stride(0), self.d if d is None else d, ptr(out),
                  out.stride(0) if ld_out is None else ld_out, ptr(self.nrm), ptr(self.count), ptr(self.parent), ptr(self.best),
                  self.n, ptr(dele), m, float(eps), int(ms), self.chunk if chunk is None else chunk, ptr(self.labels), info,
                  ptr(self.ws), self.nbytes if ws_bytes is None else ws_bytes, self._stream())
        info = np.array(info[:])
        if info[0] == 0:
            self.n -= m
            self.cur, self.off = self.cur ^ 1, 0
        return info

    def host(self):
        n = self.n
        return tuple(t[:n].cpu().numpy().astype(np.int64) for t in (self.labels, self.count, self.best))

    def rows(self):
        return self.bufs[self.cur][self.off:self.off + self.n, :self.d].cpu().numpy()

    def roots(self):
        """find(i) for every row held, on the host (parent[] itself depends on the order in which the unions happened)."""
        p = self.parent[:self.n].cpu().numpy().astype(np.int64)
        while True:
            pp = p[p]
            if np.array_equal(pp, p):
                return p
            p = pp


_STREAMS = {}


def _stream(key, ops, eps, ms):
    _STREAMS.setdefault(key, (ops, eps, ms))
    return key


@functools.lru_cache(maxsize=None)
def _expected(key):
    """The spec's replay of a stream, checked against scikit-learn's refit and the direct counts: per operation (labels, count,
    non-core mask, best, last_delete or None, rows held).  Computed once per stream."""
    from mused_amd import dbscan as spec
    from mused_amd.dbscan_incr import IncrementalSpec

    ops, eps, ms = _STREAMS[key]
    s = IncrementalSpec(eps, ms)
    out = []
    for (kind, arg), held in zip(ops, rc.replay(ops)):
        labels = rc.apply(s, kind, arg)
        assert s.flags == 0, "the spec itself went to the host: the case is decided by the fallback"
        if len(held):
            assert not spec.ambiguous(held, eps)
            want, n_core = ic.refit(held, eps, ms)
            assert np.array_equal(labels, want) and np.array_equal(s.count, dc.counts(held, eps))
        out.append((labels, s.count.copy(), s.count < ms, s.best.copy(), None if kind == "ins" else s.last_delete, held))
    return out


def _run_cabi(key, ld=0, chunk=128):
    """Replays a stream through the C ABI and compares with the spec after every operation; -> the infos of the deletes."""
    ops, eps, ms = _STREAMS[key]
    d = ops[0][1].shape[1]
    st = CabiState(d, ld, sum(len(a) for k, a in ops if k == "ins"), chunk)
    infos = []
    for (kind, arg), (labels, count, noncore, best, last, held) in zip(ops, _expected(key)):
        if kind == "ins":
            assert st.insert(arg, eps, ms)[0] == 0
        else:
            info = st.delete(arg, eps, ms) if kind == "del" else st.delete_rows(np.sort(arg), eps, ms)
            assert tuple(info) == last, (tuple(info), last)
            infos.append(info)
        got_labels, got_count, got_best = st.host()
        assert np.array_equal(got_labels, labels)
        assert np.array_equal(got_count, count)
        assert np.array_equal(got_best[noncore], best[noncore])
        assert st.n == len(held) and np.array_equal(st.rows().view(np.int64), held.view(np.int64))   # the packed rows, bit for bit
        if len(held):
            roots, core = st.roots(), ~noncore
            assert (roots <= np.arange(st.n)).all() and (roots[noncore] == np.flatnonzero(noncore)).all()
            assert np.array_equal(np.unique(roots[core], return_inverse=True)[1], labels[core])
    return infos


# ---- the hand-built cases, spread over several row tiles, the deleted rows taken from the middle ----------------------------
def _hand_keys(d):
    return [f"{name}_d{d}" for name, _, _, _ in dc.hand_cases(d)]


@pytest.mark.parametrize("key", [k for d in DIMS for k in _hand_keys(d)])
def test_hand_built_streams_from_the_middle(key):
    """dc.hand_cases with far noise rows behind every row and behind 130 far rows that stay: the rows a delete takes start in
    the second tile, and the info words are those of the deletes of the oldest rows."""
    name, d = key.rsplit("_d", 1)
    ops, eps, ms = next((o, e, m) for n, o, e, m in dc.hand_cases(int(d)) if n == name)
    rows = sum(len(a) for k, a in ops if k == "ins")
    ops = rc.from_the_middle(dc.spread_ops(ops, max(1, 520 // rows - 1)), 130)
    assert 300 <= max(len(h) for h in rc.replay(ops)) <= 700
    _run_cabi(_stream(key, ops, eps, ms))


# ---- shapes and delete sets -------------------------------------------------------------------------------------------------
def _set_ops(d, ms):
    """529 rows in five tiles; then one row, exactly rows 128 .. 255 (a whole tile), 171 more rows, every other row, 300 rows seen
    before, 129 scattered rows, all core rows of what is then cluster 0, everything, and an insert into the empty state."""
    X = dc.blobs(700, d, 60 + d)
    rng = np.random.default_rng(d)
    ops = [("ins", X[:300]), ("ins", X[300:529]), ("rows", np.array([200])), ("rows", np.arange(128, 256)), ("ins", X[529:]),
           ("rows", np.arange(0, 571, 2)), ("ins", X[:300])]
    held = rc.replay(ops)[-1]
    assert len(held) == 585
    ops.append(("rows", rng.choice(585, 129, replace=False)))
    held = rc.replay(ops)[-1]
    labels = ic.refit(held, 0.8, ms)[0]
    ops.append(("rows", np.flatnonzero((labels == 0) & (dc.counts(held, 0.8) >= ms))))
    ops += [("rows", np.arange(len(rc.replay(ops)[-1]))), ("ins", X[100:420])]
    return ops


@pytest.mark.parametrize("ms", [2, 5])
@pytest.mark.parametrize("pitch", [0, 11])
@pytest.mark.parametrize("d", DIMS)
def test_delete_sets_on_blobs(d, pitch, ms):
    """Three blobs and noise in random order.  pitch 11: rows 11 doubles apart, or d + 11 where d is larger (odd pitches take
    the scalar load path), in both row buffers."""
    key = f"sets_d{d}_ms{ms}"
    if key not in _STREAMS:
        _stream(key, _set_ops(d, ms), 0.8, ms)
    infos = _run_cabi(key, ld=0 if not pitch else (11 if d <= 11 else d + 11))
    assert tuple(infos[-1]) == (0,) * 6                    # everything
    assert infos[2][4] > 128                               # every other row: R spans several staging panels


def _hub_ops(d):
    """300 rows at 0, 290 at 0.9 and 290 at -0.9 of a line, in random order, min_samples = 600: the rows at 0 see all 880 and are
    the core rows, the 580 others see 590 and are border rows.  5 core rows and 265 border rows go: the rows at 0 still see 610,
    R = the 295 core rows left, B = the 315 border rows left."""
    rng = np.random.default_rng(90 + d)
    xs = np.repeat([0.0, 0.9, -0.9], [300, 290, 290])
    perm = rng.permutation(880)
    X = dc.line(xs, d, rng)[perm]
    centre = np.flatnonzero(xs[perm] == 0.0)
    side = np.flatnonzero(xs[perm] != 0.0)
    dele = np.concatenate([rng.choice(centre, 5, replace=False), rng.choice(side, 265, replace=False)])
    return [("ins", X[:500]), ("ins", X[500:]), ("rows", dele)]


@pytest.mark.parametrize("d", DIMS)
def test_all_three_lists_span_several_panels(d):
    infos = _run_cabi(_stream(f"hub_d{d}", _hub_ops(d), dc.EPS, 600), chunk=128)
    assert tuple(infos[0]) == (0, 1, 295, 0, 295, 315)      # |D| = 270, |R| = 295, |B| = 315: each above 256


# ---- the prefix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", [2, 5])
@pytest.mark.parametrize("d", DIMS)
def test_prefix_equals_the_delete_of_the_oldest_rows(d, ms):
    """dele = 0 .. m - 1 against mused_dbscan_incr_delete(m): nrm, count, best of the non-core rows, labels and info bit for bit,
    the roots of parent[] (its trees depend on the order of the unions, in either entry), and the rows."""
    eps = 0.8
    X = dc.blobs(600, d, 60 + d)
    ld = 0 if ms == 2 else 13 + d                         # (the same pitch on both sides: the norms' summation order hangs on it)
    a, b = CabiState(d, ld, 600, 128), CabiState(d, ld, 600, 128)
    for st in (a, b):
        st.insert(X[:350], eps, ms)
        st.insert(X[350:], eps, ms)
    for m in (1, 128, 77, 300):
        ia, ib = a.delete(m, eps, ms), b.delete_rows(np.arange(m), eps, ms)
        assert np.array_equal(ia, ib) and a.n == b.n
        n = a.n
        for ta, tb in ((a.nrm, b.nrm), (a.count, b.count), (a.labels, b.labels)):
            assert torch.equal(_bits(ta[:n]), _bits(tb[:n]))
        noncore = (a.count[:n] < ms).cpu().numpy()
        assert np.array_equal(a.host()[2][noncore], b.host()[2][noncore])
        assert (b.best[:n][~torch.from_numpy(noncore).cuda()] == 0x7fffffff).all()
        assert np.array_equal(a.roots(), b.roots())
        assert np.array_equal(a.rows().view(np.int64), b.rows().view(np.int64))
    ia, ib = a.delete(a.n, eps, ms), b.delete_rows(np.arange(b.n), eps, ms)
    assert tuple(ia) == tuple(ib) == (0,) * 6


# ---- a bad list, the C entry's refusals ------------------------------------------------------------------------------------------
def _untouched(state, st):
    torch.cuda.synchronize()
    for was, now in zip(state, st.arrays()):
        assert torch.equal(_bits(was), _bits(now))


def test_a_bad_list_and_argument_errors_leave_everything_untouched():
    from mused_amd import _lib
    from mused_amd._lib import MusedError

    ws_bytes = _lib.lib().mused_dbscan_incr_delete_rows_ws_bytes
    assert ws_bytes(0, 8, 128) == -1 and ws_bytes((1 << 19) + 1, 8, 128) == -1 and ws_bytes(1 << 19, 8, 128) > 0
    assert ws_bytes(100, 0, 128) == -1 and ws_bytes(100, 8, 0) == -1 and ws_bytes(100, 8, 130) == -1
    eps, ms = 0.8, 3
    X = dc.blobs(300, 8, 79)
    st = CabiState(8, 0, 320, 128)
    st.insert(X, eps, ms)
    state = [t.clone() for t in st.arrays()]
    # descending, repeated, out of range at either end, in the 1st, 2nd and 3rd block of 256 entries of the check
    for bad in ([5, 4], [7, 7], [0, 300], [-1, 3], [299, 300], list(range(280)) + [278], list(range(1, 258)) + [256],
                list(range(20, 300))[::-1]):
        info = st.delete_rows(bad, eps, ms)
        assert tuple(info) == (FLAG_LIST, 0, 0, 0, 0, 0) and st.n == 300
    _untouched(state, st)
    need = ws_bytes(300, 8, 128)
    own = st.bufs[st.cur]
    for kw in (dict(m=0), dict(m=301), dict(m=-3), dict(ws_bytes=need - 1), dict(chunk=130), dict(chunk=0), dict(d=0), dict(ld_out=7),
               dict(out=own), dict(out=own[150:]), dict(out=own[299:])):          # X_out overlaps the rows held
        with pytest.raises(MusedError):
            st.delete_rows(np.arange(50), eps, ms, **kw)
        assert st.n == 300
    with pytest.raises(MusedError):
        st.delete_rows(np.arange(50), -1.0, ms)
    _untouched(state, st)
    # and the state still works
    info = st.delete_rows(np.arange(0, 300, 3), eps, ms)
    keep = np.arange(300) % 3 != 0
    want, n_core = ic.refit(X[keep], eps, ms)
    assert np.array_equal(st.host()[0], want) and info[0] == 0 and info[1] == want.max() + 1 and info[2] == n_core
    assert np.array_equal(st.rows().view(np.int64), X[keep].view(np.int64))


# ---- the class ------------------------------------------------------------------------------------------------------------------
def test_class_delete_rows_on_arrays_masks_and_tensors():
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    eps, ms = 0.8, 3
    X = dc.blobs(500, 3, 78)
    before = mo.dbscan_incr_fallbacks
    c = IncrementalDBSCAN(eps, ms, chunk=128)
    c.insert(X[:300]).insert(torch.from_numpy(X[300:]).cuda())
    keep = np.ones(500, dtype=bool)

    def gone(idx):
        pos = np.flatnonzero(keep)
        keep[pos[idx]] = False

    assert c.delete_rows([7, 3, 499 - 60]) is c            # any order; a row of the last batch: get_cluster_labels is spent
    gone([7, 3, 439])
    assert c.n == 497 and np.array_equal(c.labels(), ic.refit(X[keep], eps, ms)[0]) and c._last is None
    c.insert(X[:40])
    keep = np.concatenate([keep, np.ones(40, dtype=bool)])
    X = np.concatenate([X, X[:40]])
    c.delete_rows(torch.arange(100, 300, 2, device="cuda", dtype=torch.int32))
    gone(np.arange(100, 300, 2))
    assert np.array_equal(c.get_cluster_labels(c._last), ic.refit(X[keep], eps, ms)[0][-40:]) and c._last_lo == c.n - 40
    mask = np.zeros(c.n, dtype=bool)
    mask[[0, 5, 200]] = True
    c.delete_rows(mask)
    gone([0, 5, 200])
    tmask = torch.zeros(c.n, dtype=torch.bool, device="cuda")
    tmask[10:140] = True
    c.delete_rows(tmask).delete_oldest(3)
    gone(np.arange(10, 140))
    gone([0, 1, 2])
    assert c.n == keep.sum() and np.array_equal(c.labels(), ic.refit(X[keep], eps, ms)[0])
    assert np.array_equal(c._rows().cpu().numpy().view(np.int64), X[keep].view(np.int64))
    state = c.labels()
    for bad in ([], [c.n], [-1], [4, 4], np.zeros(c.n + 1, dtype=bool), [0.5], torch.tensor([3, 3], device="cuda"),
                torch.tensor([c.n], device="cuda"), torch.zeros(c.n - 1, dtype=torch.bool, device="cuda")):
        with pytest.raises(ValueError):
            c.delete_rows(bad)
    assert c.n == keep.sum() and np.array_equal(c.labels(), state)
    # find and labels_of: rows held, a row that is not, a row held twice
    from mused_amd.rows_find import rows_find

    ask = np.concatenate([X[keep][[5, 2]], [[9.0, 9.0, 9.0]], X[keep][[5, 5]]])   # (row 5 is held twice: X[:40] came again)
    pos = rows_find(X[keep], ask)
    assert pos[0] == 5 and pos[1] == 2 and pos[2] == -1 and pos[3] > 5 and pos[4] == -1
    assert np.array_equal(c.find(ask), pos) and np.array_equal(c.find(torch.from_numpy(ask).cuda()), pos)
    assert np.array_equal(c.labels_of(ask[:2]), state[[5, 2]])
    with pytest.raises(ValueError, match="not held"):
        c.labels_of(ask)
    with pytest.raises(ValueError, match="oldest rows"):   # by_value is off: the present errors stay
        c.delete(ask[:1])
    c.delete_rows(np.arange(c.n))                          # everything
    assert c.n == 0 and len(c.labels()) == 0 and np.array_equal(c.find(ask), [-1] * 5)
    assert np.array_equal(c.insert(X[:100]).labels(), ic.refit(X[:100], eps, ms)[0])
    assert mo.dbscan_incr_fallbacks == before and not c._host_mode


def test_class_max_rows_with_deletes_of_any_rows():
    """Windows of 64 rows under max_rows = 300, and after every third insert 50 random rows go: labels against the refit of the
    rows held; both row buffers together stay within 2 (max_rows + largest window) rows."""
    from mused_amd import dbscan as spec
    from mused_amd.incdbscan import IncrementalDBSCAN

    W, M, eps, ms = 64, 300, 0.8, 5
    X = dc.blobs(24 * W, 3, 77)
    assert not spec.ambiguous(X, eps)
    rng = np.random.default_rng(0)
    c = IncrementalDBSCAN(eps, ms, chunk=128, max_rows=M)
    held = np.empty((0, 3))
    for t in range(24):
        b = X[t * W:(t + 1) * W]
        held = np.concatenate([held, b])[-M:]
        got = c.insert(b).get_cluster_labels(b)
        want = ic.refit(held, eps, ms)[0]
        assert c.n == len(held) and np.array_equal(c.labels(), want) and np.array_equal(got, want[-W:])
        if t % 3 == 2:
            idx = rng.choice(len(held), 50, replace=False)
            c.delete_rows(idx if t % 2 else torch.from_numpy(idx).cuda())
            held = np.delete(held, idx, axis=0)
            assert np.array_equal(c.labels(), ic.refit(held, eps, ms)[0])
        stored = c._X.shape[0] + (0 if c._X2 is None else c._X2.shape[0])
        assert stored <= 2 * (M + W) and c._off + c.n <= c._X.shape[0] and c._nrm.shape[0] <= 2 * (M + W)
        if c._two:
            assert stored <= 2 * M
    assert not c._host_mode


def test_class_host_mode_after_a_flagged_insert():
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    eps, ms = 0.75, 2
    first = np.array([[0.0, 0.0], [eps, 0.0], [5.0, 5.0], [5.2, 5.0], [0.3, 0.0], [5.0, 5.0]])
    before = mo.dbscan_incr_fallbacks
    c = IncrementalDBSCAN(eps, ms, by_value=True)
    c.insert(first)
    assert c._host_mode and mo.dbscan_incr_fallbacks == before + 1
    assert np.array_equal(c.find(first[[5, 2, 2]]), [2, 5, -1])
    c.delete_rows([1, 3])
    held = first[[0, 2, 4, 5]]
    assert np.array_equal(c.labels(), ic.refit(held, eps, ms)[0]) and mo.dbscan_incr_fallbacks == before + 2
    with pytest.warns(UserWarning, match="1 of 2 rows"):
        c.delete(np.array([[5.0, 5.0], [7.0, 7.0]]))
    held = held[[0, 2, 3]]
    assert np.array_equal(c.labels(), ic.refit(held, eps, ms)[0]) and mo.dbscan_incr_fallbacks == before + 3
    got = c.get_cluster_labels(np.array([[0.3, 0.0], [1.0, 1.0]]))
    assert got.dtype == np.float64 and got[0] == 0.0 and np.isnan(got[1])
    with pytest.raises(ValueError):
        c.delete_rows([3])


def test_class_by_value():
    from mused_amd.incdbscan import IncrementalDBSCAN

    eps, ms = 0.8, 3
    X = dc.blobs(400, 3, 81)
    c = IncrementalDBSCAN(eps, ms, chunk=128, by_value=True)
    c.insert(X[:250]).insert(X[250:])
    want = ic.refit(X, eps, ms)[0]
    got = c.get_cluster_labels(X[250:])                     # the reference's call
    assert got.dtype == np.float64 and np.array_equal(got, want[250:])
    ask = np.concatenate([X[[300, 17]], [[50.0, 50.0, 50.0]], X[[17]]])
    got = c.get_cluster_labels(torch.from_numpy(ask).cuda())
    assert np.array_equal(got[:2], want[[300, 17]]) and np.isnan(got[2:]).all()
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="IncrementalDBSCAN.delete")    # every row is held: no warning
        assert c.delete(X[100:220]) is c
    keep = np.ones(400, dtype=bool)
    keep[100:220] = False
    assert np.array_equal(c.labels(), ic.refit(X[keep], eps, ms)[0])
    with pytest.warns(UserWarning, match="2 of 4 rows"):
        c.delete(ask)                                       # row 17 is held once: its second occurrence is skipped too
    keep[[300, 17]] = False
    assert c.n == keep.sum() and np.array_equal(c.labels(), ic.refit(X[keep], eps, ms)[0])
    with pytest.warns(UserWarning, match="1 of 1 rows"):
        c.delete(ask[2:3])                                  # nothing is held: nothing happens
    assert c.n == keep.sum()
