"""mused_dbscan_incr_delete (csrc/dbscan_incr.hip) against its specification and scikit-learn: through the C ABI and through
mused_amd.incdbscan.IncrementalDBSCAN (delete_oldest, delete, max_rows) and the pipeline.  After EVERY operation the labels of
the rows held must EQUAL DBSCAN(eps, min_samples).fit_predict on those rows, count[] and the border minima must equal the
spec's, and a delete's info word must equal the spec's -- on streams that are checked on the CPU to hold no pair within the
rounding margin of eps, on which the spec never raises its flag and no operation may go to the host.  Shapes are chosen against
the kernel's 128-row tile and a staging panel of 128 rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import dbscan_incr_cases as ic
import dbscan_incr_delete_cases as dc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DIMS = [1, 3, 50]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class CabiState:
    """The caller's side of mused_dbscan_incr_insert / _delete: rows with a row pitch (the padding holds NaN, which nothing may
    read) behind an offset that a delete advances, state arrays that start as garbage."""

    def __init__(self, d, ld, capacity, chunk):
        from mused_amd import _lib

        self.d, self.chunk, self.n, self.off, self.capacity = d, chunk, 0, 0, capacity
        self.buf = torch.full((capacity, ld or d), float("nan"), dtype=torch.float64, device="cuda")
        self.nrm = torch.full((capacity,), float("nan"), dtype=torch.float64, device="cuda")
        self.count, self.parent, self.best, self.labels = (torch.full((capacity,), -7, dtype=torch.int32, device="cuda")
                                                           for _ in range(4))
        L = _lib.lib()
        self.del_bytes = int(L.mused_dbscan_incr_delete_ws_bytes(capacity, d, chunk))
        # O(n) beside the staging panel
        assert 0 < self.del_bytes <= 44 * capacity + 4 * ((capacity + 127) // 128) + 8 * chunk * (d + 1) + 13 * 256
        self.nbytes = max(self.del_bytes, int(L.mused_dbscan_incr_ws_bytes(capacity, d, chunk)))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def _call(self, name, a, b, eps, ms, ws_bytes=None, chunk=None, d=None):
        from mused_amd import _lib
        from mused_amd.engine import ptr

        held = self.buf[self.off:]
        info = (C.c_int * 6)(*([-7] * 6))
        _lib.call(name, ptr(held), held.stride(0), self.d if d is None else d, ptr(self.nrm), ptr(self.count), ptr(self.parent),
                  ptr(self.best), a, b, float(eps), int(ms), self.chunk if chunk is None else chunk, ptr(self.labels), info,
                  ptr(self.ws), self.nbytes if ws_bytes is None else ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return np.array(info[:])

    def insert(self, batch, eps, ms):
        n0, w = self.n, len(batch)
        self.buf[self.off + n0:self.off + n0 + w, :self.d] = torch.tensor(batch, device="cuda")
        info = self._call("mused_dbscan_incr_insert", n0, w, eps, ms)
        self.n = n0 + w
        return info

    def delete(self, m, eps, ms, **kw):
        info = self._call("mused_dbscan_incr_delete", self.n, m, eps, ms, **kw)
        self.n -= m
        self.off = self.off + m if self.n else 0
        return info

    def host(self):
        n = self.n
        return tuple(t[:n].cpu().numpy().astype(np.int64) for t in (self.labels, self.count, self.best))


@functools.lru_cache(maxsize=None)
def _expected(ops_key):
    """The spec's replay of a stream, checked against scikit-learn's refit and the direct counts: per operation (labels, count,
    non-core mask, best, last_delete or None).  Computed once per stream."""
    from mused_amd import dbscan as spec
    from mused_amd.dbscan_incr import IncrementalSpec

    ops, eps, ms = _STREAMS[ops_key]
    s = IncrementalSpec(eps, ms)
    out = []
    for (kind, arg), held in zip(ops, dc.replay(ops)):
        labels = s.insert(arg) if kind == "ins" else s.delete_oldest(arg)
        assert s.flags == 0, "the spec itself went to the host: the case is decided by the fallback"
        if len(held):
            assert not spec.ambiguous(held, eps)
            want, n_core = ic.refit(held, eps, ms)
            assert np.array_equal(labels, want) and np.array_equal(s.count, dc.counts(held, eps))
        out.append((labels, s.count.copy(), s.count < ms, s.best.copy(), s.last_delete if kind == "del" else None))
    return out


_STREAMS = {}


def _stream(key, ops, eps, ms):
    _STREAMS[key] = (ops, eps, ms)
    return key


def _run_cabi(key, ld=0, chunk=128):
    """Replays a stream through the C ABI and compares with the spec after every operation; -> the infos of the deletes."""
    ops, eps, ms = _STREAMS[key]
    d = ops[0][1].shape[1]
    peak = max(len(h) for h in dc.replay(ops))
    total = sum(len(a) for k, a in ops if k == "ins")
    st = CabiState(d, ld, total, chunk)
    infos = []
    for (kind, arg), (labels, count, noncore, best, last) in zip(ops, _expected(key)):
        if kind == "ins":
            info = st.insert(arg, eps, ms)
            assert info[0] == 0
        else:
            info = st.delete(arg, eps, ms)
            assert tuple(info) == last, (tuple(info), last)
            infos.append(info)
        got_labels, got_count, got_best = st.host()
        assert np.array_equal(got_labels, labels)
        assert np.array_equal(got_count, count)
        assert np.array_equal(got_best[noncore], best[noncore])
    assert peak <= total
    return infos


# ---- the hand-built cases of the host test, spread over several row tiles ---------------------------------------------------
def _hand(d):
    out = []
    for name, ops, eps, ms in dc.hand_cases(d):
        rows = sum(len(a) for k, a in ops if k == "ins")
        out.append(_stream(f"{name}_d{d}", dc.spread_ops(ops, max(1, 640 // rows - 1)), eps, ms))
    return out


@pytest.mark.parametrize("key", [k for d in DIMS for k in _hand(d)])
def test_hand_built_streams_across_tiles(key):
    """Chain, bridge, border row between two clusters (the smaller-numbered one deleted / only affected), untouched far cluster,
    lost core status, m == n followed by an insert: with far noise rows behind every row, so that 300 to 700 rows are held and
    the rows that interact lie in different tiles."""
    ops = _STREAMS[key][0]
    assert 300 <= max(len(h) for h in dc.replay(ops)) <= 700
    _run_cabi(key)


# ---- shapes --------------------------------------------------------------------------------------------------------------
def _blob_ops(d, seed):
    X = dc.blobs(700, d, seed)
    # 529 rows in five tiles; a delete that ends on a tile boundary, a single row, 77 rows; 171 more rows; 201 rows; 59 rows seen before; all but one row
    return [("ins", X[:300]), ("ins", X[300:529]), ("del", 128), ("del", 1), ("del", 77), ("ins", X[529:700]), ("del", 201),
            ("ins", X[:59]), ("del", 351)]


@pytest.mark.parametrize("ms", [1, 2, 5])
@pytest.mark.parametrize("pitch", [0, 11])
@pytest.mark.parametrize("d", DIMS)
def test_delete_sizes_on_blobs(d, pitch, ms):
    """Three blobs and noise in random order: every delete touches every cluster.  pitch 11: rows 11 doubles apart, or d + 11
    where d is larger (odd pitches take the scalar load path, and the rows held start at an odd offset of the buffer)."""
    key = _stream(f"blobs_d{d}_ms{ms}", _blob_ops(d, 60 + d), 0.8, ms)
    infos = _run_cabi(key, ld=0 if not pitch else (11 if d <= 11 else d + 11))
    assert infos[0][4] > 128                               # R spans several staging panels


def _hub_ops(d):
    """150 rows at 0, 150 at 0.9 and 150 at -0.9 of a line, in random order, min_samples = 400: the rows at 0 see all 450 and
    are the core rows, the 300 others see 300 and are border rows.  10 rows go: R = the core rows left, B = every border row.
    60 more go: the core rows see fewer than 400 and all lose core status (R empty, B = every row held)."""
    rng = np.random.default_rng(90 + d)
    X = dc.line(np.repeat([0.0, 0.9, -0.9], 150), d, rng)[rng.permutation(450)]
    return [("ins", X[:200]), ("ins", X[200:]), ("del", 10), ("del", 60), ("del", 129)]


@pytest.mark.parametrize("d", DIMS)
def test_both_staging_lists_span_several_panels(d):
    key = _stream(f"hub_d{d}", _hub_ops(d), dc.EPS, 400)
    infos = _run_cabi(key, chunk=128)
    assert infos[0][4] > 128 and infos[0][5] > 256          # |R|, |B|
    assert infos[1][2] == 0 and infos[1][3] > 100 and infos[1][4] == 0 and infos[1][5] == 380   # no core row is left: all in B


# ---- the class --------------------------------------------------------------------------------------------------------------
def test_bounded_stream_of_any_length():
    """40 windows of 64 rows under max_rows = 300: labels after every insert against the refit of the rows held, the buffers
    within 2 (max_rows + largest window), the rows copied to the front when the tail runs out."""
    from mused_amd import dbscan as spec
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    W, M, eps, ms = 64, 300, 0.8, 5
    X = dc.blobs(40 * W, 3, 77)
    assert not spec.ambiguous(X, eps)
    before = mo.dbscan_incr_fallbacks
    c = IncrementalDBSCAN(eps, ms, chunk=128, max_rows=M)
    offs = []
    for t in range(40):
        lo, hi = t * W, (t + 1) * W
        b = X[lo:hi] if t % 2 else torch.from_numpy(X[lo:hi]).cuda()
        got = c.insert(b).get_cluster_labels(b)
        held = X[max(0, hi - M):hi]                     # (the first delete drops 20 rows, every later one 64)
        want = ic.refit(held, eps, ms)[0]
        assert c.n == len(held) and np.array_equal(c.labels(), want) and np.array_equal(got, want[-W:])
        assert c._X.shape[0] <= 2 * (M + W) and c._nrm.shape[0] <= 2 * (M + W) and c._off + c.n <= c._X.shape[0]
        offs.append(c._off)
    assert any(b < a for a, b in zip(offs, offs[1:]))      # the survivors moved to the front at least once
    assert mo.dbscan_incr_fallbacks == before and not c._host_mode
    with pytest.raises(ValueError):                        # a window larger than max_rows
        c.insert(X[:M + 1])


def test_delete_oldest_and_delete_by_rows():
    from mused_amd.incdbscan import IncrementalDBSCAN

    eps, ms = 0.8, 3
    X = dc.blobs(500, 3, 78)
    c = IncrementalDBSCAN(eps, ms, chunk=128)
    c.insert(X[:300]).insert(torch.from_numpy(X[300:500]).cuda())
    assert c.delete_oldest(130) is c
    assert np.array_equal(c.labels(), ic.refit(X[130:500], eps, ms)[0])
    assert np.array_equal(c.get_cluster_labels(c._last), ic.refit(X[130:500], eps, ms)[0][-200:])
    state = c.labels()
    for bad in (X[131:140], X[130:140][::-1], X[130:140] * (1.0 + 2.0 ** -52), X[130:140, :2], np.nextafter(X[130:131], 9.0)):
        with pytest.raises(ValueError, match="oldest rows"):
            c.delete(bad)
    with pytest.raises(ValueError):
        c.delete_oldest(0)
    with pytest.raises(ValueError):
        c.delete_oldest(371)
    assert c.n == 370 and np.array_equal(c.labels(), state)
    assert c.delete(X[130:140]) is c and c.delete(torch.from_numpy(X[140:141]).cuda()) is c
    assert np.array_equal(c.labels(), ic.refit(X[141:500], eps, ms)[0])
    c.delete_oldest(359)                                   # m == n
    assert c.n == 0 and len(c.labels()) == 0
    assert np.array_equal(c.insert(X[:100]).labels(), ic.refit(X[:100], eps, ms)[0])


def test_a_flagged_insert_then_deletes_on_the_host():
    """A pair at exactly eps sends the object to the host for good; deletes there drop the rows from the host copy and refit."""
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    eps, ms = 0.75, 2
    first = np.array([[0.0, 0.0], [eps, 0.0], [5.0, 5.0], [5.2, 5.0], [0.3, 0.0]])
    later = np.array([[9.0, 9.0], [9.1, 9.0], [0.1, 0.0]])
    before = mo.dbscan_incr_fallbacks
    c = IncrementalDBSCAN(eps, ms, max_rows=7)
    c.insert(first)
    assert c._host_mode and mo.dbscan_incr_fallbacks == before + 1
    c.delete_oldest(1)
    assert np.array_equal(c.labels(), ic.refit(first[1:], eps, ms)[0]) and mo.dbscan_incr_fallbacks == before + 2
    c.insert(later)                                        # 4 + 3 rows: nothing to delete
    assert np.array_equal(c.labels(), ic.refit(np.concatenate([first[1:], later]), eps, ms)[0])
    c.insert(first[2:4])                                   # 9 rows: the two oldest go first
    held = np.concatenate([first[3:], later, first[2:4]])
    assert c.n == 7 and np.array_equal(c.labels(), ic.refit(held, eps, ms)[0])
    with pytest.raises(ValueError, match="oldest rows"):
        c.delete(held[1:2])
    c.delete(held[:2])
    assert np.array_equal(c.labels(), ic.refit(held[2:], eps, ms)[0])


# ---- the C entry's refusals ---------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_state_untouched():
    from mused_amd import _lib
    from mused_amd._lib import MusedError

    ws_bytes = _lib.lib().mused_dbscan_incr_delete_ws_bytes
    assert ws_bytes(0, 8, 128) == -1 and ws_bytes((1 << 19) + 1, 8, 128) == -1 and ws_bytes(1 << 19, 8, 128) > 0
    assert ws_bytes(100, 0, 128) == -1 and ws_bytes(100, 8, 0) == -1 and ws_bytes(100, 8, 130) == -1
    eps, ms = 0.8, 3
    X = dc.blobs(200, 8, 79)
    st = CabiState(8, 0, 256, 128)
    st.insert(X, eps, ms)
    arrays = (st.nrm, st.count, st.parent, st.best, st.labels)
    state = [t.clone() for t in arrays]
    need = ws_bytes(200, 8, 128)
    for kw, m in ((dict(), 0), (dict(), 201), (dict(), -3), (dict(ws_bytes=need - 1), 50), (dict(chunk=130), 50), (dict(chunk=0), 50),
                  (dict(d=0), 50)):
        with pytest.raises(MusedError):
            st.delete(m, eps, ms, **kw)
        st.n, st.off = 200, 0
    with pytest.raises(MusedError):
        st.delete(50, -1.0, ms)
    st.n, st.off = 200, 0
    torch.cuda.synchronize()
    for was, now in zip(state, arrays):
        bits = torch.int64 if was.dtype == torch.float64 else torch.int32   # (the unwritten norms are NaN)
        assert torch.equal(was.view(bits), now.view(bits))
    # and the state still works
    info = st.delete(50, eps, ms)
    want, n_core = ic.refit(X[50:], eps, ms)
    assert np.array_equal(st.host()[0], want) and info[0] == 0 and info[1] == want.max() + 1 and info[2] == n_core


# ---- through the pipeline -------------------------------------------------------------------------------------------------
W, ELL, K = 256, 8, 5
EPS_P, MS_P = 0.15, 3      # an eps of the embeddings' own scale (tests/test_gpu_dbscan_incr_stream.py)


def _pipeline_run(monkeypatch, max_rows, env=None):
    from mused_amd import incdbscan, synth
    from mused_amd import matrix_operations as mo
    from mused_amd.pipeline import StreamPipeline, process_streaming_data

    X, labels = synth.blob_stream(6 * W, 16, 0, n_centres=4)
    embeddings = []
    real = incdbscan.IncrementalDBSCAN.insert

    def recording(self, rows):
        embeddings.append(rows.cpu().numpy().copy() if isinstance(rows, torch.Tensor) else np.array(rows))
        return real(self, rows)

    monkeypatch.setattr(incdbscan.IncrementalDBSCAN, "insert", recording)
    before = mo.dbscan_incr_fallbacks
    if env is not None or max_rows is None:
        if env is not None:
            monkeypatch.setenv("MUSED_DBSCAN_INCR_ROWS", env)
        else:
            monkeypatch.delenv("MUSED_DBSCAN_INCR_ROWS", raising=False)
        got = process_streaming_data({}, [X.astype(np.float64)], [""], W, ELL, K, 4, 0, "DBSCAN_incr", labels, 1, 0.0, "types",
                                     False, EPS_P, MS_P)["all_clusters"]
    else:
        with StreamPipeline(W, ELL, K, 0, "DBSCAN_incr", [""], 1, eps=EPS_P, min_samples=MS_P, dbscan_max_rows=max_rows) as pipe:
            got = pipe.run([X.astype(np.float64)], np.asarray(labels))
    assert mo.dbscan_incr_fallbacks == before and len(embeddings) == 6
    return np.asarray(got), embeddings


def _replay_on_spec(embeddings, max_rows):
    from mused_amd import matrix_operations as mo
    from mused_amd.dbscan_incr import IncrementalSpec

    s = IncrementalSpec(EPS_P, MS_P, max_rows=max_rows)
    out, prev = [], None
    for e in embeddings:
        labels = s.insert(e)[-W:]
        assert s.flags == 0
        matched = mo.match_clusters(prev, labels, method="hungarian", min_overlap=3)
        if matched is None or len(matched) == 0:   # main.py:114-116
            matched = np.full(W, 0)
        prev = matched
        out.extend(matched)
    return np.array(out), s


@pytest.mark.parametrize("how", ["argument", "environment"])
def test_pipeline_over_a_sliding_window(how, monkeypatch):
    """6 windows of 256 rows with at most 600 rows held: from the third window on 168 rows go before each insert."""
    got, embeddings = _pipeline_run(monkeypatch, 600, env="600" if how == "environment" else None)
    want, s = _replay_on_spec(embeddings, 600)
    assert s.n == 600 and s.last_delete is not None
    assert got.shape == (6 * W,) and np.array_equal(got, want)


def test_pipeline_unset_holds_every_row(monkeypatch):
    got, embeddings = _pipeline_run(monkeypatch, None)
    want, s = _replay_on_spec(embeddings, None)
    assert s.n == 6 * W and s.last_delete is None and np.array_equal(got, want)
    from mused_amd.pipeline import StreamPipeline

    with pytest.raises(ValueError):
        StreamPipeline(W, ELL, K, 0, "DBSCAN_incr", dbscan_max_rows=W - 1)
