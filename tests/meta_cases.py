"""Streams and windows shared by test_meta_host.py and test_gpu_meta_window.py (no test of its own).

`stream()` is synth.metadata_stream(400, 1, missing=0.3) with hand-made rows on top (every edit is listed below), `ties()` a
whole-hour time stream (equal time differences are common).  Rows 200..209 are invalid in EVERY column, rows 210..213
valid in every column, rows 120 and 159 invalid in every column."""
import functools

import numpy as np

TYPES = ("location", "time", "username", "tags")
N = 400
K = 15
# (37, 167): 130 rows, neither end a multiple of 64; (120, 160) begins and ends on an invalid row; (200, 210) holds no valid
# row; (200, 214) holds four valid rows, fewer than k
WINDOWS = [(0, 70), (37, 167), (100, 101), (0, 400), (330, 400), (120, 160), (200, 210), (200, 214)]
ORACLE_WINDOW = (37, 167)


@functools.lru_cache(maxsize=None)
def stream():
    from mused_amd import synth

    cols, _ = synth.metadata_stream(N, 1, missing=0.3)
    loc, tim, usr, tags = (cols[t].copy() for t in TYPES)
    usr = usr.astype(object)

    def invalid(rows):
        loc[rows] = np.nan
        tim[rows, 0] = 0.0
        usr[rows, 0] = ""
        for r in np.arange(N)[rows]:
            tags[r, 0] = ""   # what the reference's `data[:, 0] != ""` rejects ([] stays a valid, empty set)

    def valid(rows):
        for r in np.arange(N)[rows]:   # values of the row's own: no two made rows tie unless an edit below says so
            loc[r] = (47.0 + 0.001 * r, 9.0 - 0.002 * r)
            tim[r] = (1.25e9 + 977.5 * r, 1.2501e9 + 1201.25 * r)
            usr[r, 0] = f"made{r % 2}"
            tags[r, 0] = ["tag01", f"tag{10 + r % 7:02d}"]

    invalid(slice(200, 210))
    valid(slice(210, 214))
    valid(slice(35, 39))       # the rows the users / tags below are placed on hold a value in every column
    valid(slice(164, 170))
    valid(slice(60, 65))
    invalid(np.array([120, 159]))
    # ties: six rows share one location and straddle the end of (37, 167)
    loc[164:170] = (48.0, 11.0)
    # ties: identical tag sets, an empty set, a repeated tag
    for r in (60, 61, 62):
        tags[r, 0] = ["alpha", "beta"]
    tags[63, 0] = []
    tags[64, 0] = ["alpha", "alpha", "gamma"]
    # posting sub-ranges of (37, 167): a tag before, inside and after the window; a tag absent from it; a tag held by its
    # first and last row only
    for r in (10, 80, 300):
        tags[r, 0] = ["zz_span", "tag02"]
    for r in (5, 350):
        tags[r, 0] = ["zz_out"]
    for r in (37, 166):
        tags[r, 0] = ["zz_edge", "tag03"]
    # a user whose rows straddle the start of (37, 167), one straddling its end
    usr[35:39, 0] = "straddle_s"
    usr[165:169, 0] = "straddle_e"
    return {"location": loc, "time": tim, "username": usr.astype(str), "tags": tags}


@functools.lru_cache(maxsize=None)
def ties():
    from mused_amd import synth

    return synth.metadata_stream(N, 2, missing=0.3, integer_time=True)[0]


def host_valid(rows, t):
    """The per-window validity expression of matrix_operations._metadata_adjacency for type t."""
    rows = np.asarray(rows)
    if t == "location":
        return ~np.isnan(rows.astype(np.float64)).any(axis=1)
    if t == "time":
        return ~((rows[:, 0] == 0.0) | (rows[:, 1] == 0.0))
    return np.asarray(rows[:, 0] != "", dtype=bool)
