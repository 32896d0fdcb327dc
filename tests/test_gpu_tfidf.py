"""csrc/tfidf.hip on the device against the specification (mused_amd/tfidf.py, itself pinned to scikit-learn by
tests/test_tfidf_host.py) bit for bit, and the "text" modality's device path against MUSED_TEXT=host (the per-window
TfidfVectorizer call) through the public interface: adjacency masks, a stream, a batch."""
import numpy as np
import pytest
import torch

import tfidf_cases as tc

pytestmark = pytest.mark.gpu
K = 15


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mused_amd.engine import WindowEngine

    e = WindowEngine(1500)
    yield e
    e.close()


def host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name,which,s,e", tc.WINDOWS, ids=tc.WINDOW_IDS)
def test_device_window_equals_the_specification(eng, name, which, s, e):
    """mused_tfidf_window / mused_tfidf_dense: window CSR (column ids, global ids, once- and twice-normalised values),
    posting lists and V_w equal the specification's; the scattered matrix equals T.todense()."""
    c, want = tc.corpus(which), tc.spec(which, s, e)
    w = eng.tfidf_window(c, s, e)
    info = host(w.info)
    assert (w.n, w.nnz, w.n_terms) == (want.n, len(want.term), c.V)
    assert list(info) == [want.n_cols, 0, len(want.term), 0]
    assert w.read_info() == want.n_cols
    assert np.array_equal(host(w.rowptr), want.indptr)
    assert np.array_equal(host(w.term), want.term) and np.array_equal(host(w.col), want.indices)
    assert np.array_equal(bits(host(w.val)), bits(want.data))
    assert np.array_equal(bits(host(w.val2)), bits(want.data2))
    assert np.array_equal(host(w.postptr), want.postptr) and np.array_equal(host(w.postrow), want.postrow)
    assert np.array_equal(bits(host(w.postval)), bits(want.postval))
    T, _ = tc.sklearn_tfidf(which, s, e)
    dense = host(eng.tfidf_dense(w, want.n_cols))
    assert dense.shape == T.shape and np.array_equal(bits(dense), bits(np.asarray(T.todense())))


def test_a_window_the_host_did_not_size_for_raises_the_flag(eng):
    """The kernels recount the window's documents from the device arrays: when the host sized the idf table and the
    outputs for another count, every workgroup leaves before it reads or writes a row and the flag word says so."""
    import copy

    from mused_amd._lib import MusedError

    c = copy.copy(tc.corpus("mixed"))
    c._dev = {}
    c.device_arrays(eng.device)          # the true arrays are on the device ...
    c.vrank = c.vrank.copy()
    c.vrank[300] += 1                    # ... and the host believes in one document more (row 121 is invalid: room for it)
    w = eng.tfidf_window(c, 100, 300)
    assert host(w.info)[1] == 1
    with pytest.raises(MusedError, match="not the one the host sized for"):
        w.read_info()


def _mask(x, sparse, engine):
    from mused_amd import matrix_operations as mo

    return host(mo.adjacency_on_device(x, "text", K, engine=engine, text_sparse=sparse).mask)


@pytest.mark.parametrize("sparse", [True, False], ids=["sparse", "dense"])
@pytest.mark.parametrize("name,which,s,e", tc.WINDOWS, ids=tc.WINDOW_IDS)
def test_adjacency_masks_equal_the_host_path(eng, monkeypatch, name, which, s, e, sparse):
    monkeypatch.setenv("MUSED_TEXT", "host")
    want = _mask(tc.records(which)[s:e], sparse, eng)
    monkeypatch.setenv("MUSED_TEXT", "device")
    got = _mask(tc.corpus(which).window(s, e), sparse, eng)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert want.any()


def test_raw_strings_take_the_device_path(eng, monkeypatch):
    """Strings are tokenised as a corpus of their own: no TfidfVectorizer.fit_transform on the device path."""
    from sklearn.feature_extraction.text import TfidfVectorizer

    from mused_amd import matrix_operations as mo

    rec = tc.records("mixed")[100:300]
    monkeypatch.setenv("MUSED_TEXT", "host")
    want = _mask(rec, None, eng)
    monkeypatch.setenv("MUSED_TEXT", "device")

    def no_host(*a, **k):
        raise AssertionError("the device path called TfidfVectorizer.fit_transform")

    monkeypatch.setattr(TfidfVectorizer, "fit_transform", no_host)
    assert np.array_equal(_mask(rec, None, eng), want)
    assert np.array_equal(_mask(tc.corpus("mixed")[100:300], None, eng), want)
    A = mo.create_adjacency_matrix(rec, "text", K)
    assert A.shape == (200, 200) and A.dtype == np.float64


def test_host_only_corpus_takes_the_host_path(eng, monkeypatch):
    from mused_amd import text

    monkeypatch.delenv("MUSED_TEXT", raising=False)
    c = text.tokenise(tc.records("mixed"), max_row_terms=299)
    assert c.host_only
    got = _mask(c.window(200, 400), True, eng)
    assert np.array_equal(got, _mask(tc.corpus("mixed").window(200, 400), True, eng))


def test_blank_and_tokenless_windows(eng, monkeypatch):
    from mused_amd import tfidf

    monkeypatch.setenv("MUSED_TEXT", "device")
    c = tc.corpus("mixed")
    assert not _mask(np.array([["", ""]] * 4), None, eng).any()
    assert not _mask(c.window(tc.HALF_BLANK_ROW + 1, tc.HALF_BLANK_ROW + 2), None, eng).any()
    for x in (c.window(tc.HALF_BLANK_ROW, tc.HALF_BLANK_ROW + 2), np.array([["a", ""], ["", "b c"], ["", ""]])):
        with pytest.raises(ValueError) as err:
            _mask(x, None, eng)
        assert str(err.value) == tfidf.EMPTY_VOCABULARY


@pytest.mark.parametrize("ratio", [1, 2])
def test_stream_labels_equal_the_host_path(monkeypatch, ratio):
    from mused_amd import synth
    from mused_amd.pipeline import process_streaming_data

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rec = tc.records("mixed")
    X, labels = synth.blob_stream(600, 12, 1, n_centres=4)
    out = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("MUSED_TEXT", mode)
        res = process_streaming_data({}, [X.astype(np.float64), rec], ["", "text"], 300, 6, K, 4, 0, "sSVDMC", labels, ratio,
                                     0.0, "types", False, 1.5, 2)
        out[mode] = np.asarray(res["all_clusters"])
    assert len(out["host"]) == 300 * (2 if ratio == 1 else 3)
    assert np.array_equal(out["device"], out["host"])


def test_batch_labels_equal_the_host_path(monkeypatch):
    from mused_amd import synth
    from mused_amd.pipeline import process_batch_data

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 1200
    types_ = ["location", "time", "username", "text"]
    cols, labels = synth.metadata_stream(n, 3)
    cols["text"], _ = synth.text_stream(n, 3)
    mods = [cols[t] for t in types_]
    out, timings = {}, {}
    for mode in ("host", "device"):
        monkeypatch.setenv("MUSED_TEXT", mode)
        timings[mode] = {}
        res = process_batch_data({}, mods, types_, 8, 10, 5, 0, "SVDMC_batch", labels, 0.0, "all", False, 0.5, 5, 3, 2000,
                                 timings=timings[mode])
        out[mode] = np.asarray(res["all_clusters"])
    assert "tokenise[3]" in timings["device"] and "tokenise[3]" not in timings["host"]
    assert len(out["host"]) == n and np.array_equal(out["device"], out["host"])
