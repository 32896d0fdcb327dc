"""Fusion of modality adjacencies by an agreement threshold: the host side, plain NumPy (no torch, no device).

The rule (csrc/adj_fuse_table.hip and include/mused_hip.h use the same words):

    M modalities, 1 <= M <= 8.  Weights finite, fp64, > 0; without weights every weight is 1.0.
    A SUBSET s in [0, 2^M) has bit m set when modality m has the edge.
    Its SCORE is the fp64 sum, from 0.0, IN MODALITY ORDER, of w_m over the set bits: plain additions, nothing reassociated.
    The TABLE of (weights, tau) is the 256-bit truth table T:  T[s] = 1 iff s != 0 and score(s) >= tau.
    T[0] is always 0: no modality, no edge.
    tau must be finite, > 0 and <= score(2^M - 1), so the table always accepts at least the full subset.
    The fused matrix is the 0/1 matrix A[i, j] = T[s(i, j)]; its pattern is a subset of the OR of the modalities.

The table is 4 uint64 words: bit s of the table is bit s & 63 of word s >> 6.  `mused_adj_fuse_table` evaluates it on the device
without any floating point; `fuse_table_numpy` restates it on dense matrices.
"""
from __future__ import annotations

import numpy as np

MAX_PARTS = 8   # modalities of one fusion (csrc/adj_fuse_table.hip: FUSE_TABLE_MAX_M)


def _weights(weights, count=None):
    try:
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise ValueError(f"modality weights must be a sequence of numbers, got {weights!r}") from None
    if count is not None and len(w) != count:
        raise ValueError(f"{len(w)} modality weights for {count} modalities")
    if not 1 <= len(w) <= MAX_PARTS:
        raise ValueError(f"a fusion takes 1 .. {MAX_PARTS} modalities, got {len(w)}")
    for x in w:
        if not (np.isfinite(x) and x > 0.0):
            raise ValueError(f"modality weights must be finite and > 0, got {x!r}")
    return w


def subset_score(weights, s: int) -> float:
    """The score of subset s: the sum from 0.0, in modality order, of the weights of its set bits."""
    score = 0.0
    for m, w in enumerate(weights):
        if (s >> m) & 1:
            score = score + w
    return score


def check_threshold(weights, tau):
    """(weights as a list of floats, tau as a float) of a threshold fusion, or the ValueError of the rule: a weight that is not
    finite and > 0, fewer than 1 or more than 8 of them, a tau that is not finite, not > 0 or above the score of the full
    subset."""
    w = _weights(weights)
    try:
        t = float(tau)
    except (TypeError, ValueError):
        raise ValueError(f"the fusion threshold must be a number, got {tau!r}") from None
    if not (np.isfinite(t) and t > 0.0):
        raise ValueError(f"the fusion threshold must be finite and > 0, got {tau!r}")
    full = subset_score(w, (1 << len(w)) - 1)
    if t > full:
        raise ValueError(f"the fusion threshold {t!r} is above the score of all {len(w)} modalities, {full!r}: no edge could pass")
    return w, t


def threshold_table(weights, tau) -> np.ndarray:
    """The truth table of (weights, tau) as 4 uint64 words."""
    w, t = check_threshold(weights, tau)
    table = [0, 0, 0, 0]
    for s in range(1, 1 << len(w)):
        if subset_score(w, s) >= t:
            table[s >> 6] |= 1 << (s & 63)
    return np.array(table, dtype=np.uint64)


def check_table(table, M: int) -> np.ndarray:
    """`table` as 4 uint64 words; ValueError unless 1 <= M <= 8, bit 0 is clear and no bit at or above 2^M is set."""
    if not 1 <= int(M) <= MAX_PARTS:
        raise ValueError(f"a fusion takes 1 .. {MAX_PARTS} modalities, got {M}")
    t = np.ascontiguousarray(table, dtype=np.uint64)
    if t.shape != (4,):
        raise ValueError(f"a fusion table is 4 uint64 words, got shape {t.shape}")
    bits = table_bits(t)
    if bits[0]:
        raise ValueError("table bit 0 is set: no modality, no edge")
    if bits[1 << int(M):].any():
        raise ValueError(f"a table bit at or above 2^M = {1 << int(M)} is set")
    return t


def table_bits(table) -> np.ndarray:
    """The 256 bits of a table as a uint8 array indexed by subset."""
    t = np.ascontiguousarray(table, dtype=np.uint64)
    s = np.arange(256)
    return ((t[s >> 6] >> (s & 63).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def fuse_table_numpy(mats, table) -> np.ndarray:
    """The fused int64 0/1 matrix of dense modality matrices (nonzero = edge) under `table`: entry (i, j) is table bit
    s(i, j) = sum_m [mats[m][i, j] != 0] << m."""
    mats = [np.asarray(a) for a in mats]
    bits = table_bits(check_table(table, len(mats)))
    s = np.zeros(mats[0].shape, dtype=np.int64)
    for m, a in enumerate(mats):
        if a.shape != s.shape:
            raise ValueError("adjacency shapes differ")
        s |= (a != 0).astype(np.int64) << m
    return bits[s].astype(np.int64)
