"""The code-point rule of mused_amd/tokens.py -- the class table, U+0130, U+03A3 -- against `re`, scikit-learn's analyser
and the host tokeniser (mused_amd.text.tokenise); the host preparation of `tokenise_codepoints_on_device` and the routing
of `tokenise_for_device`."""
import re

import numpy as np
import pytest

import token_cases as tk
import unicode_token_cases as uc


def test_the_class_table_is_res_word_class_and_the_byte_rule_below_128():
    from mused_amd import tokens

    table = tokens.class_table()
    assert table.dtype == np.uint32 and table.shape == (tokens.N_CODEPOINTS,) == (0x110000,)
    word = re.compile(r"\w")
    want = np.fromiter((word.fullmatch(chr(cp)) is not None for cp in range(tokens.N_CODEPOINTS)), dtype=bool,
                       count=tokens.N_CODEPOINTS)
    assert np.array_equal((table & tokens.CP_WORD) != 0, want)
    assert int(want.sum()) > 100000 and want[0x4E2D] and want[0x10400] and not want[0x0307] and not want[0xD800]
    # below 128 the kernels take the ALU rule of the byte path
    assert np.array_equal((table[:128] & tokens.CP_WORD) != 0, tokens.IS_WORD[:128])
    assert np.array_equal(table[:128] & tokens.CP_MASK, tokens.LOWER[:128])
    assert not (table[:128] & tokens.CP_END).any()
    assert not table[tokens.SEPARATOR] & tokens.CP_WORD


def test_the_lowered_code_points_and_the_recorded_expanding_set():
    from mused_amd import tokens

    table = tokens.class_table()
    expanding = {cp: chr(cp).lower() for cp in range(tokens.N_CODEPOINTS) if len(chr(cp).lower()) != 1}
    assert tokens.expanding_codepoints() == expanding        # exactly the recorded set
    assert expanding == {0x130: "i\u0307"}                   # CPython: U+0130 alone
    assert len(tokens.unsupported_codepoints()) == 0
    low = np.fromiter((ord(chr(cp).lower()[0]) for cp in range(tokens.N_CODEPOINTS)), dtype=np.uint32, count=tokens.N_CODEPOINTS)
    assert np.array_equal(table & tokens.CP_MASK, low)
    ends = np.flatnonzero(table & tokens.CP_END)
    assert ends.tolist() == sorted(expanding)
    assert table[0x130] == ord("i") | tokens.CP_WORD | tokens.CP_END
    # lower-casing never changes the class, and is idempotent on what U+03A3 resolves to
    assert np.array_equal(table[low] & tokens.CP_WORD, table & tokens.CP_WORD)
    assert [int(table[ord(c)] & tokens.CP_MASK) for c in "σς"] == [ord("σ"), ord("ς")]


_POOLS = [
    "".join(chr(c) for c in range(0x20, 0x7F)),                                   # printable ASCII
    "".join(chr(c) for c in range(0xA1, 0x250)),                                  # Latin-1, Latin Extended-A and -B
    "".join(chr(c) for c in range(0x386, 0x3CF)) + "ΣσςΣσς",                      # Greek
    "".join(chr(c) for c in range(0x400, 0x460)),                                 # Cyrillic
    "İıIi" * 3,
    "\u0300\u0301\u0302\u0303\u0304\u0305\u0306\u0307\u0345\u02b0\u00b7\u00ad\u2019\u00a0\u200b",
    "".join(chr(c) for c in range(0x660, 0x66A)) + "文字化日本語中",                  # Arabic-Indic digits, CJK
    "".join(chr(c) for c in range(0x2C60, 0x2C80)) + "".join(chr(c) for c in range(0x2C00, 0x2C60)) + "ȺȾⱥⱦ",
    "".join(chr(c) for c in range(0x10400, 0x10450)),                             # Deseret, astral case pairs
    "\U0001f600\U0001f389\U0001f1e9\U0001f1ea\U0001f44d\U0001f3fd\u200d\u2764\ufe0f",                     # emoji
    "abcxyzABCXYZ019__  \t\n" + "ΑΣ ΣΑ αΣ Σα",
]


def test_the_code_point_rule_gives_scikit_learns_tokens_on_random_strings():
    from sklearn.feature_extraction.text import TfidfVectorizer

    from mused_amd import tokens

    analyse = TfidfVectorizer().build_analyzer()
    rng = np.random.default_rng(7)
    pools = [np.array([ord(c) for c in p], dtype=np.uint32) for p in _POOLS]
    with_sigma = with_dotted = tokens_seen = 0
    for _ in range(24000):
        # one to three pools a string, so that the scripts meet inside a run
        chosen = np.concatenate([pools[i] for i in rng.integers(0, len(pools), size=int(rng.integers(1, 4)))])
        doc = "".join(map(chr, chosen[rng.integers(0, len(chosen), size=int(rng.integers(0, 31)))]))
        want = analyse(doc)
        assert tokens.analyse_codepoints(doc) == want, repr(doc)
        with_sigma += "Σ" in doc
        with_dotted += "İ" in doc
        tokens_seen += len(want)
    assert with_sigma > 2000 and with_dotted > 500 and tokens_seen > 20000


def _spec_corpus(name):
    """The arrays of the specification, spread over all rows and posted as TextCorpus does."""
    from mused_amd import text, tokens

    rec, valid = text._valid_rows(uc.records(name))
    buf, docptr = text.corpus_codepoints(rec, valid)
    voc, rowptr, term, cnt, pos = tokens.codepoint_corpus_arrays(buf, docptr)
    return text.TextCorpus(rec, voc, rowptr[np.concatenate([[0], np.cumsum(valid)])], term, cnt, pos, valid), buf, docptr


@pytest.mark.parametrize("name", uc.CASES)
def test_the_rule_gives_the_host_tokenisers_corpus(name):
    got, _, _ = _spec_corpus(name)
    tk.assert_equal_corpora(got, uc.host_corpus(name))


def test_the_hand_made_case_holds_what_it_is_meant_to():
    voc = set(uc.host_corpus("hand").vocabulary)
    assert {"élan", "éé", "ai", "bi", "stanbul", "σοφος", "ος", "ж" * 300, "дом", "文字化けの文章", "mixedスクリプトtoken_ж9",
            uc.DESERET_SMALL, "中中", chr(0x24E2D) * 2, "٣٤٥", "345", "٣4", "_under_", "lastwörd", "fırstword"} <= voc
    assert not {"é", "i", "istanbul", "σοφοσ"} & voc
    assert uc.DESERET_CAPITALS not in voc
    want = uc.host_corpus("hand")
    row = uc.REPEATED_ROW
    assert int(want.cnt[want.rowptr[row]:want.rowptr[row + 1]].sum()) == uc.REPEATS + 1


@pytest.mark.parametrize("name", ["hand", "mixed_swapped", "residues"])
def test_the_buffer_is_the_references_strings_with_a_separator_each(name):
    from mused_amd import tokens

    _, buf, docptr = _spec_corpus(name)
    d = uc.records(name)
    vd = d[np.any(d != "", axis=1)]
    strings = (np.where(vd[:, 0] != "", vd[:, 0], " ") + " " + np.where(vd[:, 1] != "", vd[:, 1], " ")).tolist()
    assert buf.dtype == np.uint32
    decoded = buf.astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
    assert decoded.lower() == "".join((s + chr(tokens.SEPARATOR)).lower() for s in strings)
    # and but for U+03A3 the buffer is the strings themselves
    plain = "".join(s + chr(tokens.SEPARATOR) for s in strings)
    assert len(decoded) == len(plain) and all(a == b or b == "Σ" and a in "σς" for a, b in zip(decoded, plain))
    assert docptr.dtype == np.int32 and np.array_equal(np.diff(docptr), [len(s) + 1 for s in strings])


def test_an_ascii_corpus_gives_the_byte_buffer_widened():
    from mused_amd import text

    for name in ("hand", "mixed"):
        rec, valid = text._valid_rows(tk.records(name))
        buf8, docptr8 = text.corpus_buffer(rec, valid)
        buf32, docptr32 = text.corpus_codepoints(rec, valid)
        assert buf32.dtype == np.uint32 and np.array_equal(buf32, buf8.astype(np.uint32))
        assert docptr32.dtype == np.int32 and np.array_equal(docptr32, docptr8)


def test_what_is_no_code_point_or_too_long_is_the_hosts(monkeypatch):
    from mused_amd import text

    rec = np.array([["ab", "cd"], ["éf", ""]], dtype=str)
    assert text.corpus_codepoints(*text._valid_rows(rec)) is not None
    beyond = rec.copy()
    beyond.view(np.uint32)[0] = 0x110000        # cannot come from a str
    assert text.corpus_codepoints(*text._valid_rows(beyond)) is None
    monkeypatch.setattr(text, "_MAX_CODEPOINTS", 9)      # the two documents hold 6 + 5 elements
    assert text.corpus_codepoints(*text._valid_rows(rec)) is None


def test_the_residue_case_covers_every_residue_of_the_scan_block():
    from mused_amd import tokens

    _, buf, _ = _spec_corpus("residues")
    start, length = tokens.codepoint_token_spans(buf)
    assert len(buf) == 3 * uc.SCAN_BLOCK and int(buf.max()) > 127 and np.all(length == 2)
    assert len(np.unique(start % uc.SCAN_BLOCK)) == uc.SCAN_BLOCK
    assert len(np.unique((start + length) % uc.SCAN_BLOCK)) == uc.SCAN_BLOCK
    assert np.any(start // uc.SCAN_BLOCK != (start + length - 1) // uc.SCAN_BLOCK)


def test_routing_by_switch_row_count_and_script(monkeypatch):
    from mused_amd import text

    calls = []
    monkeypatch.setattr(text, "tokenise_on_device", lambda r, d=None: calls.append("bytes"))
    monkeypatch.setattr(text, "tokenise_codepoints_on_device", lambda r, d=None: calls.append("codepoints"))
    monkeypatch.setattr(text, "tokenise", lambda r: calls.append("host"))
    plain = np.array([["plain ascii", "text"]] * 4, dtype=str)
    one = plain.copy()
    one[2, 1] = "tèxt"                          # one character that is not ASCII
    monkeypatch.setenv("MUSED_TOKENISE", "device")
    text.tokenise_for_device(plain)
    text.tokenise_for_device(one)
    assert calls == ["bytes", "codepoints"]
    monkeypatch.setenv("MUSED_TOKENISE", "host")
    text.tokenise_for_device(plain)
    text.tokenise_for_device(one)
    assert calls == ["bytes", "codepoints", "host", "host"]
    # unset: each script has a threshold of its own, below which the host is chosen
    monkeypatch.delenv("MUSED_TOKENISE")
    monkeypatch.setattr(text, "TOKENISE_DEVICE_MIN_ROWS", 4)
    monkeypatch.setattr(text, "TOKENISE_CODEPOINTS_MIN_ROWS", 6)
    del calls[:]
    for rec in (plain, plain[:3], one, one[:3], np.concatenate([one, plain[:2]]), np.concatenate([plain, plain[:2]])):
        text.tokenise_for_device(rec)
    assert calls == ["bytes", "host", "host", "host", "codepoints", "bytes"]
    monkeypatch.setattr(text, "TOKENISE_DEVICE_MIN_ROWS", 6)
    monkeypatch.setattr(text, "TOKENISE_CODEPOINTS_MIN_ROWS", 4)
    del calls[:]
    for rec in (plain, one, one[:3]):
        text.tokenise_for_device(rec)
    assert calls == ["host", "codepoints", "host"]
