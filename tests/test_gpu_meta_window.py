"""Windows of a metadata stream that was encoded once (mused_amd/meta.py, csrc/meta_window.hip) against the present
path: `adjacency_on_device` on the raw slice of the window, bit for bit on `Adjacency.to_numpy()`."""
import ctypes as C
import functools

import numpy as np
import pytest

import meta_cases as mc
from conftest import assert_valid_topk

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd.engine import WindowEngine

    e = WindowEngine(512)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _corpus(name, t):
    from mused_amd import meta

    return meta.encode(getattr(mc, name)()[t], t)


_REF = {}


def _present(eng, name, t, s, e, k):
    """The yardstick, computed once per case and left unchanged: the parent's path on the raw slice."""
    from mused_amd import matrix_operations as mo

    key = (name, t, s, e, k)
    if key not in _REF:
        _REF[key] = mo.adjacency_on_device(getattr(mc, name)()[t][s:e], t, k, engine=eng).to_numpy()
        _REF[key].setflags(write=False)
    return _REF[key]


def _device(eng, name, t, s, e, k):
    from mused_amd import matrix_operations as mo

    return mo.adjacency_on_device(_corpus(name, t).window(s, e), t, k, engine=eng).to_numpy()


@pytest.mark.parametrize("t", mc.TYPES)
@pytest.mark.parametrize("s,e", mc.WINDOWS)
def test_window_equals_the_present_path(eng, monkeypatch, t, s, e):
    monkeypatch.delenv("MUSED_META", raising=False)
    calls = []
    real = type(eng).meta_window_adjacency
    monkeypatch.setattr(type(eng), "meta_window_adjacency", lambda self, w, kk: calls.append(kk) or real(self, w, kk))
    A, ref = _device(eng, "stream", t, s, e, mc.K), _present(eng, "stream", t, s, e, mc.K)
    assert A.dtype == ref.dtype and A.shape == (e - s, e - s)
    assert np.array_equal(A, ref)
    valid = mc.host_valid(mc.stream()[t][s:e], t)
    assert len(calls) == (1 if valid.any() else 0)   # the device path was taken (an empty window returns before it)
    assert not A[~valid].any() and not A[:, ~valid].any()
    if (s, e) == (200, 210):
        assert not A.any()
    if (s, e) == (200, 214) and t != "username":   # four valid rows, fewer than k: every valid row selects all the others
        want = np.zeros((14, 14))
        want[10:, 10:] = 1.0 - np.eye(4)
        assert np.array_equal(A, want)


@pytest.mark.parametrize("t", mc.TYPES)
@pytest.mark.parametrize("k", [0, 1, 130, 500])
def test_values_of_k(eng, monkeypatch, t, k):
    monkeypatch.delenv("MUSED_META", raising=False)
    s, e = mc.ORACLE_WINDOW
    A = _device(eng, "stream", t, s, e, k)
    assert np.array_equal(A, _present(eng, "stream", t, s, e, k))
    if k == 0 and t != "username":   # "tags": nothing is selected; "location" / "time": a row selects only itself
        dup = np.arange(164, 167) - s if t == "location" else np.arange(0)
        assert not np.delete(A, dup, axis=0).any()
        if len(dup):   # the rows that share a location tie at distance 0: each selects the first of them, not itself
            assert A[dup].sum(1).tolist() == [0, 1, 1] and A[dup[1:], dup[0]].all()


@pytest.mark.parametrize("s,e", [(0, 70), (37, 167), (0, 400)])
def test_ties_go_to_the_smaller_row(eng, monkeypatch, s, e):
    """Whole-hour time stamps (equal differences), six rows at one location across the end of (37, 167), identical tag
    sets / empty sets / a repeated tag: invalid rows keep their place, so the tie order is that of the gathered rows."""
    monkeypatch.delenv("MUSED_META", raising=False)
    for k in (3, mc.K):
        assert np.array_equal(_device(eng, "ties", "time", s, e, k), _present(eng, "ties", "time", s, e, k))
        for t in ("location", "tags"):
            assert np.array_equal(_device(eng, "stream", t, s, e, k), _present(eng, "stream", t, s, e, k)), (t, k)
    if (s, e) == (37, 167):
        A = _device(eng, "stream", "location", s, e, 2)   # k + 1 = 3 of the rows 164, 165, 166 that share a location
        r = np.arange(164, 167) - s
        assert np.array_equal(A[np.ix_(r, r)], 1.0 - np.eye(3)) and A[r].sum() == 6


def test_window_longer_than_a_workgroup(monkeypatch):
    """2,300 rows: every loop of the 1,024-thread selection kernel runs more than once, and a mask row has 36 words."""
    from mused_amd import matrix_operations as mo
    from mused_amd import meta, synth
    from mused_amd.engine import WindowEngine

    monkeypatch.delenv("MUSED_META", raising=False)
    cols, _ = synth.metadata_stream(2600, 5, missing=0.3, integer_time=True)
    cols["tags"][np.random.default_rng(5).random(2600) < 0.3, 0] = ""
    big = WindowEngine(2300)
    try:
        for t in mc.TYPES:
            A = mo.adjacency_on_device(meta.encode(cols[t], t).window(150, 2450), t, 40, engine=big)
            assert torch.equal(A.mask, mo.adjacency_on_device(cols[t][150:2450], t, 40, engine=big).mask), t
    finally:
        big.close()


def test_users_straddling_the_window(eng, monkeypatch):
    monkeypatch.delenv("MUSED_META", raising=False)
    s, e = mc.ORACLE_WINDOW
    A = _device(eng, "stream", "username", s, e, mc.K)
    assert np.array_equal(A, _present(eng, "stream", "username", s, e, mc.K))
    assert np.flatnonzero(A[0]).tolist() == [1] and np.flatnonzero(A[1]).tolist() == [0]          # rows 37, 38 of 35..38
    assert np.flatnonzero(A[165 - s]).tolist() == [166 - s] and np.flatnonzero(A[166 - s]).tolist() == [165 - s]


@pytest.mark.parametrize("t", mc.TYPES)
def test_window_against_the_oracle(eng, monkeypatch, t):
    """One window with s > 0 per type, held to the oracle like test_metadata_branches_match_reference_and_oracle."""
    from oracle import mo_oracle as omo

    monkeypatch.delenv("MUSED_META", raising=False)
    s, e = mc.ORACLE_WINDOW
    rows = mc.stream()[t][s:e]
    A = _device(eng, "stream", t, s, e, mc.K)
    assert np.array_equal(A, omo.create_adjacency_matrix(rows, t, mc.K))
    if t in ("tags", "time"):
        valid, S, kk = omo.metadata_scores(rows, t, mc.K)
        assert_valid_topk(A, valid, S, kk)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _unpack(mask, n):
    bits = np.unpackbits(mask.cpu().numpy().view(np.uint8), axis=1, bitorder="little")
    return bits[:, :n].astype(np.float64), bits[:, n:]


@pytest.mark.parametrize("t", ["location", "time", "tags"])
def test_entries_through_the_c_abi(eng, t):
    """mused_meta_window_records / mused_meta_window_tags called directly: the masks of the tests above, a buffer filled
    with ones comes back with every invalid row, every bit and every word past the last column zero, and every invalid
    argument is an error."""
    from mused_amd import _lib
    from mused_amd.engine import stream_ptr, words_for

    c = _corpus("stream", t)
    d = c.device_arrays("cuda")
    kk = {"location": mc.K + 1, "time": 3 * mc.K + 1, "tags": mc.K}[t]

    def run(s, e, k=kk, words=None, n_rows=c.N, kind=None, mask=None):
        n = e - s
        words = words_for(n) + 2 if words is None else words
        if mask is None:
            mask = torch.full((max(n, 1), max(words, 1)), -1, dtype=torch.int64, device="cuda")
        if t == "tags":
            _lib.call("mused_meta_window_tags", _ptr(d["rowptr"]), _ptr(d["tag"]), _ptr(d["gpostptr"]), _ptr(d["gpostrow"]),
                      _ptr(d["vrank"]), n_rows, c.V, s, e, k, _ptr(mask), words, stream_ptr())
        else:
            _lib.call("mused_meta_window_records", _ptr(d["rec"]), _ptr(d["vrank"]), n_rows,
                      {"location": 0, "time": 1}[t] if kind is None else kind, s, e, k, _ptr(mask), words, stream_ptr())
        return mask

    for s, e in [(37, 167), (120, 160), (200, 214), (0, 400)]:
        A, past = _unpack(run(s, e), e - s)
        assert np.array_equal(A, _present(eng, "stream", t, s, e, mc.K)), (s, e)
        assert not past.any()
        valid = mc.host_valid(mc.stream()[t][s:e], t)
        assert not A[~valid].any() and not A[:, ~valid].any()
    ones = torch.full((4, 3), -1, dtype=torch.int64, device="cuda")
    assert run(50, 50, mask=ones) is ones and bool((ones == -1).all())   # e == s: a successful no-op
    bad = [dict(s=-1, e=10), dict(s=20, e=10), dict(s=390, e=401), dict(s=0, e=64, k=0), dict(s=0, e=130, words=2),
           dict(s=0, e=10, n_rows=5)]
    if t != "tags":
        bad += [dict(s=0, e=10, kind=2), dict(s=0, e=10, kind=-1)]
    for kw in bad:
        with pytest.raises(_lib.MusedError):
            run(**kw)
    # a window above the cap: the range check passes (n_rows is only compared), nothing is launched
    cap = 15000 if t == "tags" else 16384
    with pytest.raises(_lib.MusedError):
        run(0, cap + 1, n_rows=cap + 1, words=words_for(cap + 1), mask=ones)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["env", "host_only", "classic"])
def test_fallbacks_take_the_host_records_path(eng, monkeypatch, mode):
    from mused_amd import matrix_operations as mo
    from mused_amd import meta
    from mused_amd.engine import WindowEngine

    monkeypatch.delenv("MUSED_META", raising=False)
    windows = [(37, 167), (120, 160), (200, 214)]
    want = {(t, w): _device(eng, "stream", t, *w, mc.K) for t in mc.TYPES for w in windows}

    def boom(self, window, kk):
        raise AssertionError("the device path was taken")

    monkeypatch.setattr(WindowEngine, "meta_window_adjacency", boom)
    with pytest.raises(AssertionError):
        _device(eng, "stream", "time", 37, 167, mc.K)
    use = eng
    if mode == "env":
        monkeypatch.setenv("MUSED_META", "host")
    if mode == "classic":
        use = WindowEngine(512)
        use.knn_mode = "classic"
    try:
        for t in mc.TYPES:
            c = meta.encode(mc.stream()[t], t, max_entries=100) if mode == "host_only" else _corpus("stream", t)
            assert c.host_only == (mode == "host_only")
            for w in windows:
                A = mo.adjacency_on_device(c.window(*w), t, mc.K, engine=use).to_numpy()
                assert np.array_equal(A, want[(t, w)]), (t, w)
    finally:
        if use is not eng:
            use.close()


@pytest.mark.parametrize("ratio", [1, 2])
def test_stream_labels_do_not_depend_on_the_mode(monkeypatch, ratio):
    """Five modalities through process_streaming_data: MUSED_META=device and =host give the same event labels."""
    from mused_amd import synth
    from mused_amd.pipeline import process_streaming_data

    cols, labels = synth.metadata_stream(900, 3, missing=0.25)
    text, _ = synth.text_stream(900, 3)
    mods = [cols["location"], cols["time"], cols["username"], cols["tags"], text]
    types_ = ["location", "time", "username", "tags", "text"]
    out = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("MUSED_META", mode)
        res = process_streaming_data({}, mods, types_, 300, 6, 10, len(np.unique(labels)), 0, "sSVDMC", labels, ratio, 0.0,
                                     "types", False, 1.5, 2)
        out[mode] = np.asarray(res["all_clusters"])
    assert len(out["device"]) == (900 if ratio == 1 else 1500)
    assert np.array_equal(out["device"], out["host"])
