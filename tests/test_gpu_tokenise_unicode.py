"""The code-point kernels of csrc/tokenise.hip (mused_tokenise_cp_*) on the device against the host tokeniser
(mused_amd.text.tokenise, scikit-learn's analyser) field for field on text that is not ASCII, their limits and argument
checks, and the routing of such text through the public interface."""
import ctypes as C

import numpy as np
import pytest
import torch

import token_cases as tk
import unicode_token_cases as uc

pytestmark = pytest.mark.gpu
K = 15
LARGE = ("term", "cnt", "pos", "gpostptr", "gpostrow", "gpostent")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("name", uc.CASES)
def test_device_corpus_equals_the_host_tokenisers(name):
    from mused_amd import text

    before = text.tokenise_fallbacks
    got = text.tokenise_codepoints_on_device(uc.records(name))
    assert text.tokenise_fallbacks == before
    tk.assert_equal_corpora(got, uc.host_corpus(name))
    assert got.V == 0 or "_lazy" in vars(got)


def test_a_full_table_with_long_probe_chains_gives_the_same_arrays():
    """20,000 tokens, all distinct, in a table of exactly 20,000 slots: the smallest that holds them (one slot less
    raises the flag instead of probing for ever)."""
    from mused_amd import text

    want = uc.host_corpus("distinct")
    T = int(want.cnt.sum())
    assert T == want.V == 20000 and not any(t.isascii() for t in want.vocabulary)
    tk.assert_equal_corpora(text.tokenise_codepoints_on_device(uc.records("distinct"), table_slots=T), want)
    with pytest.raises(ValueError, match="do not fit a table"):
        text.tokenise_codepoints_on_device(uc.records("distinct"), table_slots=T - 1)


@pytest.mark.parametrize("name", ["hand", "sparse", "residues"])
def test_an_ascii_corpus_gives_the_byte_paths_corpus(name):
    from mused_amd import text

    before = text.tokenise_fallbacks
    got, want = text.tokenise_codepoints_on_device(tk.records(name)), text.tokenise_on_device(tk.records(name))
    assert text.tokenise_fallbacks == before and "_lazy" in vars(got) and "_lazy" in vars(want)
    tk.assert_equal_corpora(got, want)


def test_two_calls_give_identical_bytes():
    from mused_amd import text

    for name in ("sparse_swapped", "hand"):
        a, b = (text.tokenise_codepoints_on_device(uc.records(name)) for _ in range(2))
        dev = [c.device_arrays("cuda") for c in (a, b)]
        for f in text._DEVICE_FIELDS:
            assert torch.equal(dev[0][f], dev[1][f]), f
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
        assert a.vocabulary == b.vocabulary


def test_max_doc_tokens_at_a_documents_count_and_one_below():
    from mused_amd import text

    rec, want = uc.records("hand"), uc.host_corpus("hand")
    longest = int(np.max(np.add.reduceat(want.cnt, want.rowptr[:-1][np.diff(want.rowptr) > 0])))
    assert longest == uc.REPEATS + 1
    before = text.tokenise_fallbacks
    at = text.tokenise_codepoints_on_device(rec, max_doc_tokens=longest)
    assert text.tokenise_fallbacks == before and "_lazy" in vars(at)
    tk.assert_equal_corpora(at, want)
    below = text.tokenise_codepoints_on_device(rec, max_doc_tokens=longest - 1)
    assert text.tokenise_fallbacks == before + 1 and "_lazy" not in vars(below)
    tk.assert_equal_corpora(below, want)


def test_no_host_tokenising_and_no_upload_of_the_large_arrays(monkeypatch):
    from sklearn.feature_extraction.text import TfidfVectorizer

    from mused_amd import text

    def no_host(*a, **k):
        raise AssertionError("the device tokeniser built scikit-learn's analyser")

    monkeypatch.setattr(TfidfVectorizer, "build_analyzer", no_host)
    c = text.tokenise_codepoints_on_device(uc.records("sparse_swapped"))
    built = {f: c._lazy[f].data_ptr() for f in LARGE}
    uploads = []
    real = torch.from_numpy
    monkeypatch.setattr(torch, "from_numpy", lambda a: uploads.append(a) or real(a))
    dev = c.device_arrays("cuda")
    assert not uploads and dev is c.device_arrays(torch.device("cuda", torch.cuda.current_device()))
    assert {f: dev[f].data_ptr() for f in LARGE} == built
    assert not any(f in vars(c) for f in LARGE)        # the host copies are fetched on first access only
    for f in ("rowptr", "vrank", "vrow"):
        assert isinstance(vars(c)[f], np.ndarray) and np.array_equal(dev[f].cpu().numpy(), getattr(c, f))
    monkeypatch.undo()
    assert np.array_equal(c.term, uc.host_corpus("sparse_swapped").term) and "term" in vars(c)


def test_rejected_arguments_leave_the_outputs_untouched():
    from mused_amd import _lib, text, tokens

    L = _lib.lib()
    rec, valid = text._valid_rows(uc.records("hand"))
    buf, docptr = text.corpus_codepoints(rec, valid)
    B, D = len(buf), len(docptr) - 1
    cap = B // 2 + 1
    ws_bytes = int(L.mused_tokenise_cp_ws_bytes(B, D, 0))
    assert ws_bytes > 0
    assert [int(L.mused_tokenise_cp_ws_bytes(*a)) for a in ((0, D, 0), (-1, D, 0), (B, 0, 0), (B, -3, 0), (B, D, -1), (2 ** 30, D, 0),
                                                            (B, B + 1, 0))] == [-1] * 7
    i32 = lambda m: torch.full((m,), -7, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    buf_d = torch.from_numpy(buf.view(np.int32)).cuda()
    table = tokens.class_table()
    table_d = torch.from_numpy(table.view(np.int32)).cuda()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    outs = {f: i32(cap) for f in ("voc_start", "voc_len", "term", "cnt", "pos", "gpostrow", "gpostent")}
    outs.update(info=i32(4), doc_rowptr=i32(D + 1), gpostptr=i32(cap + 1))
    rank, vrow = torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.zeros(D, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def scan(n_cp=B, cls=ptr(table_d), n_cls=len(table), dp=docptr, n_docs=D, slots=0, max_doc=8192, voc_cap=cap, ws_b=ws_bytes,
             off=0):
        dp = np.ascontiguousarray(dp, dtype=np.int32)
        return L.mused_tokenise_cp_scan(C.c_void_p(buf_d.data_ptr() + off), n_cp, cls, n_cls, dp.ctypes.data_as(C.c_void_p), n_docs,
                                        slots, max_doc, ptr(outs["voc_start"]), ptr(outs["voc_len"]), voc_cap, ptr(outs["info"]),
                                        ptr(ws), ws_b, stream)

    def build(n_cp=B, n_docs=D, slots=0, T=10, V=5, doc_tokens=4, ws_b=ws_bytes):
        return L.mused_tokenise_cp_build(n_cp, n_docs, slots, T, V, doc_tokens, ptr(rank), ptr(vrow), ptr(outs["doc_rowptr"]),
                                         ptr(outs["term"]), ptr(outs["cnt"]), ptr(outs["pos"]), ptr(outs["gpostptr"]),
                                         ptr(outs["gpostrow"]), ptr(outs["gpostent"]), ptr(outs["info"]), ptr(ws), ws_b, stream)

    first_not_zero, last_short, descending = docptr.copy(), docptr.copy(), docptr.copy()
    first_not_zero[0] = 1
    last_short[-1] -= 1
    descending[3] = descending[2]
    bad = [scan(n_cp=-B), scan(n_cp=2 ** 30), scan(n_docs=-1), scan(n_docs=0), scan(slots=-2), scan(cls=None), scan(n_cls=127),
           scan(n_cls=0x110001), scan(n_cls=-1), scan(off=4), scan(dp=first_not_zero), scan(dp=last_short), scan(dp=descending),
           scan(max_doc=0), scan(max_doc=8193), scan(voc_cap=0), scan(ws_b=ws_bytes - 1),
           build(n_cp=-1), build(n_docs=-D), build(T=0), build(T=-4), build(T=cap + 1, V=5), build(V=0), build(V=11),
           build(V=2 ** 24, T=2 ** 25), build(doc_tokens=0), build(doc_tokens=8193), build(slots=5), build(ws_b=ws_bytes - 1)]
    assert bad == [-1] * len(bad)   # MUSED_ERR_ARG
    assert b"workspace" in L.mused_last_error()
    torch.cuda.synchronize()
    for f, t in outs.items():
        assert bool((t == -7).all()), f
    assert scan() == 0              # and the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    assert outs["info"].cpu().numpy()[0] == int(uc.host_corpus("hand").cnt.sum())


def _count_calls(monkeypatch):
    from mused_amd import text

    calls = {"codepoints": 0, "bytes": 0, "host": 0}
    real = {"codepoints": text.tokenise_codepoints_on_device, "bytes": text.tokenise_on_device, "host": text.tokenise}

    def counted(which):
        def run(*a, **k):
            calls[which] += 1
            return real[which](*a, **k)
        return run

    monkeypatch.setattr(text, "tokenise_codepoints_on_device", counted("codepoints"))
    monkeypatch.setattr(text, "tokenise_on_device", counted("bytes"))
    monkeypatch.setattr(text, "tokenise", counted("host"))
    return calls


def test_stream_labels_are_equal_under_both_settings(monkeypatch):
    from mused_amd import synth
    from mused_amd.pipeline import process_streaming_data

    calls = _count_calls(monkeypatch)
    rec = uc.records("mixed_swapped")
    X, labels = synth.blob_stream(600, 12, 1, n_centres=4)
    out = {}
    monkeypatch.setenv("MUSED_TEXT", "device")
    for mode in ("host", "device"):
        monkeypatch.setenv("MUSED_TOKENISE", mode)
        res = process_streaming_data({}, [X.astype(np.float64), rec], ["", "text"], 300, 6, K, 4, 0, "sSVDMC", labels, 1, 0.0,
                                     "types", False, 1.5, 2)
        out[mode] = np.asarray(res["all_clusters"])
    assert calls == {"codepoints": 1, "bytes": 0, "host": 1}     # and the new function never called the host's
    assert len(out["host"]) == 600 and np.array_equal(out["device"], out["host"])


def test_batch_labels_are_equal_under_both_settings(monkeypatch):
    from mused_amd import synth
    from mused_amd.pipeline import process_batch_data

    calls = _count_calls(monkeypatch)
    n = 1200
    types_ = ["location", "time", "username", "text"]
    cols, labels = synth.metadata_stream(n, 3)
    cols["text"] = synth.swap_letters(synth.text_stream(n, 3)[0], uc.SWAP_SHARE, 5)
    mods = [cols[t] for t in types_]
    out = {}
    monkeypatch.setenv("MUSED_TEXT", "device")
    for mode in ("host", "device"):
        monkeypatch.setenv("MUSED_TOKENISE", mode)
        res = process_batch_data({}, mods, types_, 8, 10, 5, 0, "SVDMC_batch", labels, 0.0, "all", False, 0.5, 5, 3, 2000)
        out[mode] = np.asarray(res["all_clusters"])
    assert calls == {"codepoints": 1, "bytes": 0, "host": 1}
    assert len(out["host"]) == n and np.array_equal(out["device"], out["host"])
