"""Inputs shared by tests/test_tokens_unicode_host.py and tests/test_gpu_tokenise_unicode.py: (title, description) records
that are not pure ASCII, for the code-point rule of mused_amd/tokens.py and the mused_tokenise_cp_* kernels of
csrc/tokenise.hip.  Every corpus is built once, tokenised by the host tokeniser once, and kept (and never modified)."""
import functools

import numpy as np

import tfidf_cases

SCAN_BLOCK = 2048   # code points one workgroup of the code-point scan covers (csrc/tokenise.hip: TK_CP_TILE)
REPEATED_ROW = 9    # row of "hand" whose 500 tokens are one token
REPEATS = 500
SWAP_SHARE = 0.3

CASES = ["hand", "residues", "crossing", "distinct", "mixed_swapped", "sparse_swapped", "tokenless", "mixed"]

DESERET_CAPITALS = "".join(chr(0x10400 + i) for i in range(6))
DESERET_SMALL = "".join(chr(0x10428 + i) for i in range(6))


def _hand():
    low16 = chr(0x4E2D)                       # U+4E2D and U+24E2D agree in their low 16 bits
    rows = [
        ["", ""],                                                         # invalid row at the start
        ["Élan at element zero", "MiXeD Ünïcödé ÇASE"],                   # a token at element 0 of the buffer
        ["é", "éé é éé"],                                                 # "é" alone is no token, "éé" is one
        ["aİb İİ İstanbul", "aİbİ xİ İx DİYARBAKIR ıI"],                  # U+0130 ends the run behind itself
        ["ΣΟΦΟΣ ΟΣ. Σ", "ὈΔΥΣΣΕΎΣ ΣΊΣΥΦΟΣ Σ' ΑΣ\u00ad ΑΣİ ΣΑΣ\u0301 Σ\u0345Α ΑΣ\u02b0"],   # every U+03A3 by the final-sigma rule
        ["e\u0301a cafe\u0301s", "non\u00a0breaking zero\u200bwidth mid\u00b7dot l\u2019apostrophe soft\u00adhyphen"],
        ["", ""],                                                         # invalid row in the middle
        ["", "blank title Straße"],
        ["blank description ĲSSEL", ""],
        [" ".join(["дом"] * REPEATS), "ДОМ"],                             # one token 500 times in a row (and once more)
        ["文字化けの文章", "日本語 한국어 mixedスクリプトtoken_ж9"],                    # an all-CJK run, a mixed-script token
        [DESERET_CAPITALS + " " + DESERET_SMALL, DESERET_CAPITALS[:3] + DESERET_SMALL[3:]],   # astral case pairs
        ["ж" * 300, "Ж" * 299 + " " + "ж" * 300],                        # a 300-code-point token
        [low16 + low16 + " " + chr(0x24E2D) + chr(0x24E2D), chr(0x24E2D) + low16 + " " + low16 + chr(0x24E2D)],
        ["_under_ §_x _é ٣٤٥ 345 ٣4 १२३", "x٣ 9é _٣_ ⅷ ²³ ǅ ǅa"],                  # '_' and the digits of two scripts (and more)
        ["ends with tokén", "lastwörd"],                                  # a document that ends in a token ...
        ["fırstword starts the next", "\x00nul\x01ctl\x7fdel \ud800lone\udfff 😀emoji😀"],   # ... and the next starts with one
        ["", ""],
        ["the last document ends at the last", "élément"],
        ["", ""],                                                         # invalid row at the end
    ]
    return np.array(rows, dtype=str)


def _distinct():
    """20,000 distinct tokens that are not ASCII in 2,000 rows, ten a row, in no alphabetical order."""
    ids = np.random.default_rng(11).permutation(20000)
    letters = "жéσ文" + chr(0x10428)
    words = np.array([f"{letters[i % 5]}{i:05d}ü{(i * 7919) % 20000:05d}" for i in ids]).reshape(2000, 10)
    return np.array([[" ".join(w[:4]), " ".join(w[4:])] for w in words], dtype=str)


def _residues():
    """Three scan blocks of code points: every document is "пр ст" and its separator, six elements, so token starts fall
    on 0, 3, 6, ... and -- 3 and the block size have no common factor -- on every residue of the block size, ends likewise;
    the token at element 2 * SCAN_BLOCK - 1 lies across the second block boundary."""
    n = 3 * SCAN_BLOCK // 6
    two = lambda i: chr(0x430 + i % 26) + chr(0x3B1 + (i // 26) % 17)
    return np.array([[two(i), two(i * 5 + 3)] for i in range(n)], dtype=str)


def _crossing():
    """Runs of hundreds of code points, so that most block boundaries of the scan fall inside a token."""
    return np.array([["ř" * (500 + 37 * i), "š" * (1 + i % 3) + " tail"] for i in range(40)], dtype=str)


@functools.lru_cache(maxsize=None)
def records(name):
    from mused_amd import synth

    if name == "mixed":
        return tfidf_cases.records("mixed")
    if name == "mixed_swapped":
        return synth.swap_letters(tfidf_cases.records("mixed"), SWAP_SHARE, 3)
    if name == "sparse_swapped":
        return synth.swap_letters(synth.sparse_text_stream(3000, 2)[0], SWAP_SHARE, 4)
    if name == "tokenless":
        return np.array([["é", ""], ["", "ж İ"], ["", ""], ["x", "- ! ? \u0301"]], dtype=str)
    return {"hand": _hand, "distinct": _distinct, "residues": _residues, "crossing": _crossing}[name]()


@functools.lru_cache(maxsize=None)
def host_corpus(name):
    from mused_amd import text

    return text.tokenise(records(name))
