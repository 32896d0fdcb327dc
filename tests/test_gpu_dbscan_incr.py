"""csrc/dbscan_incr.hip against scikit-learn's refit: through the C ABI (mused_dbscan_incr_insert) and through
mused_amd.incdbscan.IncrementalDBSCAN.  After EVERY insert the labels of all rows so far must EQUAL
DBSCAN(eps, min_samples).fit_predict(prefix), info's cluster and core counts must equal scikit-learn's, the flag word must be
clear and no insert may have gone to the host -- on inputs that are checked on the CPU to hold no pair within the rounding
margin of eps (mused_amd.dbscan.ambiguous).  Shapes are chosen against the kernel's 128-row tile."""
import ctypes as C
import functools

import numpy as np
import pytest

import dbscan_incr_cases as ic

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = 0.8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class CabiState:
    """The caller's side of mused_dbscan_incr_insert: rows with a row pitch (the padding holds NaN, which nothing may read),
    state arrays that start as garbage (nothing of them may be read before it is written)."""

    def __init__(self, d, ld, capacity, chunk):
        from mused_amd import _lib

        self.d, self.chunk, self.n = d, chunk, 0
        self.buf = torch.full((capacity, ld or d), float("nan"), dtype=torch.float64, device="cuda")
        self.X = self.buf[:, :d]
        self.nrm = torch.full((capacity,), float("nan"), dtype=torch.float64, device="cuda")
        self.count, self.parent, self.best, self.labels = (torch.full((capacity,), -7, dtype=torch.int32, device="cuda")
                                                           for _ in range(4))
        self.nbytes = int(_lib.lib().mused_dbscan_incr_ws_bytes(capacity, d, chunk))
        # O(n) beside the staging panel: no n x n array, list or bitmask
        assert 0 < self.nbytes <= 16 * capacity + 8 * ((capacity + 127) // 128) + 8 * chunk * (d + 1) + 8 * 256
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")

    def insert(self, batch, eps, ms, ws_bytes=None):
        from mused_amd import _lib
        from mused_amd.engine import ptr

        n0, w = self.n, len(batch)
        self.X[n0:n0 + w] = torch.tensor(batch, device="cuda")
        info = (C.c_int * 6)(*([-7] * 6))
        _lib.call("mused_dbscan_incr_insert", ptr(self.buf), self.buf.stride(0), self.d, ptr(self.nrm), ptr(self.count),
                  ptr(self.parent), ptr(self.best), n0, w, float(eps), int(ms), self.chunk, ptr(self.labels), info,
                  ptr(self.ws), self.nbytes if ws_bytes is None else ws_bytes,
                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        self.n = n0 + w
        return self.labels[:self.n].cpu().numpy(), np.array(info[:])


@functools.lru_cache(maxsize=None)
def _pool(d):
    """429 rows (the largest prefix plus the largest insert): three blobs and 20 % noise, in random order; no pair within
    the rounding margin of EPS (and then none of any prefix either)."""
    from mused_amd import dbscan as spec

    rng = np.random.default_rng(40 + d)
    n = 429
    cen = 3.0 * rng.standard_normal((3, d)) / np.sqrt(d)
    X = cen[rng.integers(0, 3, n)] + (0.55 / np.sqrt(d)) * rng.standard_normal((n, d))
    noise = rng.random(n) < 0.2
    X[noise] = 3.0 * rng.standard_normal((int(noise.sum()), d)) / np.sqrt(d)
    assert not spec.ambiguous(X, EPS)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _want(d, ms, n):
    lab, n_core = ic.refit(_pool(d)[:n], EPS, ms)
    lab.setflags(write=False)
    return lab, n_core


def _check(labels, info, want, n_core):
    assert info[0] == 0, "a flag on an input that is decided far beyond rounding"
    assert np.array_equal(labels, want)
    assert info[1] == want.max() + 1 and info[2] == n_core   # clusters, core rows
    assert info[3] == info[4] + info[5]


@pytest.mark.parametrize("ms", [1, 2, 3, 5])
@pytest.mark.parametrize("pitch", [0, 11])
@pytest.mark.parametrize("d", [1, 8, 15, 16, 50])
def test_insert_sizes_on_prefixes(d, pitch, ms):
    """Inserts of 1, 127, 128, 129 rows on top of 0, 1, 127, 128, 300 rows.  pitch 11: rows 11 doubles apart, or d + 11 where
    d is larger (odd pitches take the scalar load path; 15 columns at pitch 26 the vector path with a partial last group)."""
    ld = 0 if not pitch else (11 if d <= 11 else d + 11)
    X = _pool(d)
    for p in (0, 1, 127, 128, 300):
        for w in (1, 127, 128, 129):
            st = CabiState(d, ld, 512, 128)
            if p:
                _check(*st.insert(X[:p], EPS, ms), *_want(d, ms, p))
            labels, info = st.insert(X[p:p + w], EPS, ms)
            _check(labels, info, *_want(d, ms, p + w))


def test_dirty_rows_exceed_the_staging_chunk():
    """300 rows that all turn core in one insert (min_samples = 1) go through a 128-row staging panel in three pieces; so do
    the core rows whose root moved when the border passes run (min_samples = 3)."""
    X = _pool(8)
    for ms in (1, 3):
        st = CabiState(8, 0, 512, 128)
        labels, info = st.insert(X[:300], EPS, ms)
        _check(labels, info, *_want(8, ms, 300))
        assert info[4] > 128 and info[4] == _want(8, ms, 300)[1]
        labels, info = st.insert(X[300:429], EPS, ms)
        _check(labels, info, *_want(8, ms, 429))


@pytest.mark.parametrize("case", ic.hand_cases(), ids=lambda c: c[0])
def test_hand_built_streams_across_tiles(case):
    """The hand-built streams of the host test with 70 far noise rows behind every row: a centre, its satellites, a link and
    its activator lie in different 128-row tiles.  Through the C ABI and through the class (device tensors and ndarrays)."""
    from mused_amd import dbscan as spec
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    _, batches, eps, ms = case
    batches = ic.spread(batches, 70)
    total = sum(len(b) for b in batches)
    d = batches[0].shape[1]
    st = CabiState(d, 0, total, 128)
    before = mo.dbscan_incr_fallbacks
    by_tensor, by_array = IncrementalDBSCAN(eps, ms, chunk=128), IncrementalDBSCAN(eps, ms)
    seen = None
    for b in batches:
        seen = b if seen is None else np.concatenate([seen, b])
        assert not spec.ambiguous(seen, eps)
        want, n_core = ic.refit(seen, eps, ms)
        _check(*st.insert(b, eps, ms), want, n_core)
        bd = torch.from_numpy(b).cuda()
        got = by_tensor.insert(bd).get_cluster_labels(bd)
        assert got.dtype == np.int64 and np.array_equal(got, want[-len(b):])
        assert np.array_equal(by_tensor.labels(), want)
        assert by_tensor.last_info[1] == want.max() + 1 and by_tensor.last_info[2] == n_core
        assert np.array_equal(by_array.insert(b).get_cluster_labels(b), want[-len(b):])
        assert np.array_equal(by_array.labels(), want)
    assert mo.dbscan_incr_fallbacks == before


def test_state_tensors_double(monkeypatch):
    """100 + 100 + 100 rows from a first capacity of 128: the state moves to 256 and to 512 rows between inserts."""
    from mused_amd import incdbscan
    from mused_amd import matrix_operations as mo

    monkeypatch.setattr(incdbscan, "_FIRST_CAPACITY", 128)
    X = _pool(8)
    before = mo.dbscan_incr_fallbacks
    c = incdbscan.IncrementalDBSCAN(EPS, 3, chunk=128)
    caps = []
    for lo in (0, 100, 200):
        b = X[lo:lo + 100]
        got = c.insert(b).get_cluster_labels(b)
        want = _want(8, 3, lo + 100)[0]
        assert np.array_equal(c.labels(), want) and np.array_equal(got, want[lo:])
        caps.append(c._X.shape[0])
    assert caps == [128, 256, 512]
    assert mo.dbscan_incr_fallbacks == before
    with pytest.raises(ValueError):                        # not the last batch
        c.get_cluster_labels(X[:100])
    with pytest.raises(ValueError):                        # another number of columns
        c.insert(np.zeros((3, 5)))


def test_pair_at_exactly_eps_raises_the_flag_and_the_host_answers():
    from mused_amd import dbscan as spec
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    eps, ms = 0.75, 2
    first = np.array([[0.0, 0.0], [eps, 0.0], [5.0, 5.0], [5.2, 5.0]])
    later = [np.array([[9.0, 9.0], [9.1, 9.0]]), np.array([[0.1, 0.0]])]
    st = CabiState(2, 0, 128, 128)
    _, info = st.insert(first, eps, ms)
    assert info[0] & spec.FLAG_AMBIGUOUS and not info[0] & spec.FLAG_NONFINITE
    # the pair may also arrive in two inserts
    st = CabiState(2, 0, 128, 128)
    _, info = st.insert(first[:1], eps, ms)
    assert info[0] == 0
    _, info = st.insert(first[1:], eps, ms)
    assert info[0] & spec.FLAG_AMBIGUOUS
    before = mo.dbscan_incr_fallbacks
    c = IncrementalDBSCAN(eps, ms)
    seen = first
    assert np.array_equal(c.insert(first).get_cluster_labels(first), ic.refit(seen, eps, ms)[0])
    assert mo.dbscan_incr_fallbacks == before + 1
    for k, b in enumerate(later):
        seen = np.concatenate([seen, b])
        want = ic.refit(seen, eps, ms)[0]
        assert np.array_equal(c.insert(torch.from_numpy(b).cuda()).labels(), want)
        assert mo.dbscan_incr_fallbacks == before + 2 + k
    # a hair away from it the device answers itself
    c = IncrementalDBSCAN(0.7501, ms)
    assert np.array_equal(c.insert(first).labels(), ic.refit(first, 0.7501, ms)[0])
    assert mo.dbscan_incr_fallbacks == before + 3


def test_nan_row_raises_as_scikit_learn_and_ends_the_object():
    from mused_amd import dbscan as spec
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    X = np.array(_pool(8)[:150])
    bad = X[100:150].copy()
    bad[27, 3] = np.nan
    st = CabiState(8, 0, 256, 128)
    st.insert(X[:100], EPS, 3)
    _, info = st.insert(bad, EPS, 3)
    assert info[0] & spec.FLAG_NONFINITE
    with pytest.raises(ValueError):                        # (scikit-learn raises too; its wording varies with its version)
        mo.perform_dbscan_clustering(np.concatenate([X[:100], bad]), EPS, 3)
    before = mo.dbscan_incr_fallbacks
    c = IncrementalDBSCAN(EPS, 3)
    c.insert(X[:100])
    with pytest.raises(ValueError) as dev:
        c.insert(bad)
    assert str(dev.value) == "Input contains NaN or infinity."
    with pytest.raises(ValueError):
        c.insert(X[100:150])
    assert mo.dbscan_incr_fallbacks == before


def test_host_switch(monkeypatch):
    from mused_amd import matrix_operations as mo
    from mused_amd.incdbscan import IncrementalDBSCAN

    X = _pool(8)
    monkeypatch.setenv("MUSED_DBSCAN", "host")
    before = mo.dbscan_incr_fallbacks
    c = IncrementalDBSCAN(EPS, 3)
    for lo in (0, 100):
        b = X[lo:lo + 100]
        assert np.array_equal(c.insert(b).get_cluster_labels(b), _want(8, 3, lo + 100)[0][lo:])
    assert c._X is None and mo.dbscan_incr_fallbacks == before   # the host as a whole, uncounted


def test_limits_and_a_short_workspace():
    from mused_amd import _lib
    from mused_amd._lib import MusedError

    ws_bytes = _lib.lib().mused_dbscan_incr_ws_bytes
    assert ws_bytes(0, 8, 128) == -1 and ws_bytes((1 << 19) + 1, 8, 128) == -1
    assert ws_bytes(1, 8, 128) > 0 and ws_bytes(1 << 19, 8, 128) > 0
    assert ws_bytes(100, 0, 128) == -1 and ws_bytes(100, 8, 0) == -1 and ws_bytes(100, 8, 130) == -1
    assert ws_bytes(100, 8, 1 << 17) == -1
    X = _pool(8)
    st = CabiState(8, 0, 256, 128)
    st.insert(X[:100], EPS, 3)
    state = [t.clone() for t in (st.nrm, st.count, st.parent, st.best, st.labels)]
    need = ws_bytes(200, 8, 128)
    with pytest.raises(MusedError):                        # one byte short for 200 rows: refused, nothing written
        st.insert(X[100:200], EPS, 3, ws_bytes=need - 1)
    st.n = 100
    with pytest.raises(MusedError):                        # past 2^19 rows in all
        from mused_amd.engine import ptr

        info = (C.c_int * 6)()
        _lib.call("mused_dbscan_incr_insert", ptr(st.buf), st.buf.stride(0), 8, ptr(st.nrm), ptr(st.count), ptr(st.parent),
                  ptr(st.best), 1 << 19, 1, EPS, 3, 128, ptr(st.labels), info, ptr(st.ws), st.nbytes, None)
    with pytest.raises(MusedError):
        st.insert(X[100:200], -1.0, 3)
    st.n = 100
    torch.cuda.synchronize()
    for was, now in zip(state, (st.nrm, st.count, st.parent, st.best, st.labels)):
        bits = torch.int64 if was.dtype == torch.float64 else torch.int32   # (the unwritten norms are NaN)
        assert torch.equal(was.view(bits), now.view(bits))
    # and the state still works
    labels, info = st.insert(X[100:200], EPS, 3)
    _check(labels, info, *_want(8, 3, 200))
