"""Inputs shared by tests/test_tokens_host.py and tests/test_gpu_tokenise.py: (title, description) records that exercise
the byte rule of mused_amd/tokens.py and the kernels of csrc/tokenise.hip.  Every corpus is built once, tokenised by the
host tokeniser once, and kept (and never modified)."""
import functools

import numpy as np

import tfidf_cases

SCAN_BLOCK = 4096   # bytes one workgroup of the token scan covers (csrc/tokenise.hip: TK_SCAN_TILE)
REPEATED_ROW = 9    # row of "hand" whose 500 tokens are one token
REPEATS = 500

CASES = ["mixed", "text_stream", "sparse", "hand", "distinct", "empty", "all_invalid", "tokenless", "residues", "crossing"]


def _hand():
    same8, same16 = "prefix08", "prefix0123456789"
    rows = [
        ["", ""],                                                  # invalid row at the start
        ["Token at byte zero", "MiXeD Case UPPER lower"],          # a token at byte 0 of the buffer
        ["under_score _lead trail_ a_b 9lives x86_64 007", "a b c d"],
        ["a", "b c"],                                              # valid, one-letter runs only: no token
        ["semi;colon,comma.dot!bang?what(paren)[brack]{brace}", "a-b--cd e'f \"gh\" i/j\\kl m+n=op <qr> #st @uv"],
        ["tab\tinside\tab", "new\nline\nand the\nseparator\n\nbyte ab\n"],
        ["", ""],                                                  # invalid row in the middle
        ["", "blank title"],
        ["blank description", ""],
        [" ".join(["again"] * REPEATS), "again"],                  # one token 500 times in a row (and once more)
        ["ab abc abcd", "abcd abc ab a"],
        [f"{same8}a {same8}b {same8}", f"{same16}x {same16}y {same16} {same16}x"],
        ["w" * 300, "w" * 299 + " " + "w" * 300],                  # a 300-byte token
        ["ends with token", "lastword"],                           # a document that ends in a token ...
        ["firstword starts the next", "\x00nul\x01ctl\x7fdel"],    # ... and the next one starts with one
        ["", ""],
        ["the last document ends at the last", "byte"],
        ["", ""],                                                  # invalid row at the end
    ]
    return np.array(rows, dtype=str)


def _distinct():
    """20,000 distinct tokens in 2,000 rows, ten a row, in no alphabetical order."""
    ids = np.random.default_rng(11).permutation(20000)
    words = np.array([f"t{i:05d}x{(i * 7919) % 20000:05d}" for i in ids]).reshape(2000, 10)
    return np.array([[" ".join(w[:4]), " ".join(w[4:])] for w in words], dtype=str)


def _residues():
    """Three scan blocks of bytes: every document is "pq rs" and its separator, six bytes, so token starts fall on 0, 3,
    6, ... and -- 3 and 4096 have no common factor -- on every residue of the block size, ends likewise; the token at
    byte 4095 lies across the first block boundary."""
    n = 3 * SCAN_BLOCK // 6
    two = lambda i: chr(97 + i % 26) + chr(97 + (i // 26) % 26)
    return np.array([[two(i), two(i * 5 + 3)] for i in range(n)], dtype=str)


def _crossing():
    """Runs of hundreds of bytes, so that most block boundaries of the scan fall inside a token."""
    return np.array([["r" * (500 + 37 * i), "s" * (1 + i % 3) + " tail"] for i in range(40)], dtype=str)


@functools.lru_cache(maxsize=None)
def records(name):
    from mused_amd import synth

    if name == "mixed":
        return tfidf_cases.records("mixed")
    if name == "text_stream":
        return synth.text_stream(500, 1)[0]
    if name == "sparse":
        return synth.sparse_text_stream(3000, 2)[0]
    if name == "empty":
        return np.zeros((0, 2), dtype=str)
    if name == "all_invalid":
        return np.array([["", ""]] * 5, dtype=str)
    if name == "tokenless":
        return np.array([["a", ""], ["", "b c"], ["", ""], ["x", "- ! ?"]], dtype=str)
    return {"hand": _hand, "distinct": _distinct, "residues": _residues, "crossing": _crossing}[name]()


@functools.lru_cache(maxsize=None)
def host_corpus(name):
    from mused_amd import text

    return text.tokenise(records(name))


def assert_equal_corpora(got, want):
    """Field for field: sizes, flags, vocabulary and the nine int32 arrays."""
    from mused_amd import text

    for f in ("N", "V", "nnz", "max_row_terms", "host_only"):
        assert getattr(got, f) == getattr(want, f), f
    assert got.vocabulary == want.vocabulary
    for f in text._DEVICE_FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == np.int32 and b.dtype == np.int32, f
        assert a.shape == b.shape and np.array_equal(a, b), f
