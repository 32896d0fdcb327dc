"""mused_amd/tokens.py, the byte rule the device tokeniser follows, against scikit-learn's analyser and the host tokeniser
(mused_amd.text.tokenise); the host preparation of `tokenise_on_device` and its routing of text that is not ASCII."""
import numpy as np
import pytest

import token_cases as tk


def test_the_byte_rule_gives_scikit_learns_tokens_on_random_ascii():
    from sklearn.feature_extraction.text import TfidfVectorizer

    from mused_amd import tokens

    analyse = TfidfVectorizer().build_analyzer()
    rng = np.random.default_rng(5)
    # all 128 byte values, with word bytes, blanks and case pairs drawn more often so that runs of every length appear
    pool = np.concatenate([np.arange(128), np.frombuffer(b"abcxyzABCXYZ019__  \t\n", dtype=np.uint8)] * 1).astype(np.uint8)
    seen = np.zeros(128, dtype=bool)
    for _ in range(20000):
        raw = pool[rng.integers(0, len(pool), size=int(rng.integers(0, 40)))]
        seen[raw] = True
        doc = raw.tobytes().decode("ascii")
        assert tokens.analyse(doc) == analyse(doc), repr(doc)
    assert seen.all()


def _spec_corpus(name):
    """The arrays of the specification, spread over all rows and posted as TextCorpus does."""
    from mused_amd import text, tokens

    rec, valid = text._valid_rows(tk.records(name))
    if not valid.any():
        buf, docptr = np.zeros(0, np.uint8), np.zeros(1, np.int32)
    else:
        buf, docptr = text.corpus_buffer(rec, valid)
    voc, rowptr, term, cnt, pos = tokens.corpus_arrays(buf, docptr)
    return text.TextCorpus(rec, voc, rowptr[np.concatenate([[0], np.cumsum(valid)])], term, cnt, pos, valid), buf, docptr


@pytest.mark.parametrize("name", tk.CASES)
def test_the_rule_gives_the_host_tokenisers_corpus(name):
    got, _, _ = _spec_corpus(name)
    tk.assert_equal_corpora(got, tk.host_corpus(name))


@pytest.mark.parametrize("name", ["hand", "mixed", "residues"])
def test_the_buffer_is_the_references_strings_with_a_separator_each(name):
    from mused_amd import tokens

    _, buf, docptr = _spec_corpus(name)
    d = tk.records(name)
    vd = d[np.any(d != "", axis=1)]
    strings = (np.where(vd[:, 0] != "", vd[:, 0], " ") + " " + np.where(vd[:, 1] != "", vd[:, 1], " ")).tolist()
    assert buf.tobytes() == "".join(s + chr(tokens.SEPARATOR) for s in strings).encode("ascii")
    assert docptr.dtype == np.int32 and np.array_equal(np.diff(docptr), [len(s) + 1 for s in strings])
    assert not tokens.IS_WORD[tokens.SEPARATOR]


def test_the_residue_case_covers_every_residue_of_the_scan_block():
    from mused_amd import tokens

    _, buf, _ = _spec_corpus("residues")
    start, length = tokens.token_spans(buf)
    assert len(buf) == 3 * tk.SCAN_BLOCK
    assert len(np.unique(start % tk.SCAN_BLOCK)) == tk.SCAN_BLOCK
    assert len(np.unique((start + length) % tk.SCAN_BLOCK)) == tk.SCAN_BLOCK
    assert np.any((start < tk.SCAN_BLOCK) & (start + length > tk.SCAN_BLOCK))


def test_a_corpus_that_is_not_ascii_takes_the_host_path_and_is_counted(monkeypatch):
    from mused_amd import _lib, text

    def no_device(*a, **k):
        raise AssertionError("a corpus that is not ASCII reached the device library")

    monkeypatch.setattr(_lib, "lib", no_device)
    rec = np.array([["plain ascii", "text"], ["café MÜNCHEN", "İstanbul Σίσυφος"], ["", ""]])
    before = text.tokenise_fallbacks
    got = text.tokenise_on_device(rec)
    assert text.tokenise_fallbacks == before + 1
    tk.assert_equal_corpora(got, text.tokenise(rec))
    assert "café" in got.vocabulary
    assert text.corpus_buffer(*text._valid_rows(rec)) is None


def test_the_switch_is_read_at_every_call(monkeypatch):
    from mused_amd import text

    calls = []
    monkeypatch.setattr(text, "tokenise_on_device", lambda r, d=None: calls.append("device"))
    monkeypatch.setattr(text, "tokenise", lambda r: calls.append("host"))
    rec = tk.records("tokenless")
    for mode in ("device", "host", "device"):
        monkeypatch.setenv("MUSED_TOKENISE", mode)
        text.tokenise_for_device(rec)
    assert calls == ["device", "host", "device"]
    monkeypatch.setenv("MUSED_TOKENISE", "gpu")
    with pytest.raises(ValueError):
        text.tokenise_for_device(rec)
