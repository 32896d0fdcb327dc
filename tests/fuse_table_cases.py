"""Cases and restatements shared by the fusion-table tests (host and GPU): no torch, no device.

The rule under test (mused_amd/fusion.py): subset s has bit m set when modality m has the edge; its score is the fp64 sum from
0.0, in modality order, of the weights of its set bits; T[s] = 1 iff s != 0 and score(s) >= tau."""
import numpy as np

# (weights, tau): the threshold cases.  Equal weights with tau = 1, t, M are OR, "at least t", AND
WEIGHTED = (
    ((1.0, 0.5, 0.75), 1.25),            # = majority: 0.5 + 0.75 is exact
    ((1.0, 0.5, 0.75), 1.5),             # drops {1, 2}
    ((2.0 ** 53, 1.0, 1.0), 2.0 ** 53 + 2.0),   # 2^53 + 1 rounds back to 2^53: the full subset scores 2^53 and the threshold refuses
    ((1.0, 1.0, 2.0 ** 53), 2.0 ** 53 + 2.0),   # 1 + 1 first: the full subset scores 2^53 + 2
    ((0.1, 0.2, 0.3), 0.6000000000000001),      # the full subset scores 0.6000000000000001
    ((0.3, 0.2, 0.1), 0.6000000000000001),      # ... 0.6: the threshold is above the total, a ValueError
)


def threshold_cases():
    cases = []
    for M in range(1, 9):
        for t in range(1, M + 1):
            cases.append(((1.0,) * M, float(t)))
    cases += [c for c in WEIGHTED]
    cases += [((1.0, 0.5, 0.75, 2.0, 0.25), 2.25), ((1.0, 0.5, 0.75, 2.0, 0.25, 3.0, 1.5, 0.125), 4.0)]
    return cases


def scalar_scores(weights, order=None, high_bit=False):
    """score(s) for every subset, by the scalar loop.  `order`: the modalities in the order their weights are added (the
    rule: ascending); `high_bit`: modality m taken as bit M - 1 - m of s (the rule: bit m)."""
    M = len(weights)
    order = range(M) if order is None else order
    out = []
    for s in range(1 << M):
        score = 0.0
        for m in order:
            if (s >> ((M - 1 - m) if high_bit else m)) & 1:
                score = score + float(weights[m])
        out.append(score)
    return out


def scalar_table(weights, tau, strict=False, zero_bit=False, **kw):
    """The table by the scalar loop, as 4 uint64 words, or ValueError where the rule gives one.  strict / zero_bit / **kw: the
    named wrong variants (`>` instead of `>=`; T[0] = 1; see scalar_scores)."""
    M = len(weights)
    scores = scalar_scores(weights, **kw)
    if not (np.isfinite(tau) and tau > 0 and tau <= scores[-1]):
        raise ValueError("tau")
    words = [0, 0, 0, 0]
    for s in range(1 << M):
        on = (scores[s] > tau) if strict else (scores[s] >= tau)
        if s == 0:
            on = zero_bit
        if on:
            words[s >> 6] |= 1 << (s & 63)
    return np.array(words, dtype=np.uint64)


WRONG_VARIANTS = {
    "reversed modality order": lambda w, tau: scalar_table(w, tau, order=range(len(w) - 1, -1, -1)),
    "> instead of >=": lambda w, tau: scalar_table(w, tau, strict=True),
    "T[0] set": lambda w, tau: scalar_table(w, tau, zero_bit=True),
    "modality index as the high bit": lambda w, tau: scalar_table(w, tau, high_bit=True),
}


def table_of_bits(bits):
    """256 0/1 values -> 4 uint64 words."""
    words = [0, 0, 0, 0]
    for s, b in enumerate(bits):
        if b:
            words[s >> 6] |= 1 << (s & 63)
    return np.array(words, dtype=np.uint64)


def or_table(M):
    return table_of_bits([1 <= s < (1 << M) for s in range(256)])


def and_table(M):
    return table_of_bits([s == (1 << M) - 1 for s in range(256)])


def at_least_table(M, t):
    return table_of_bits([s < (1 << M) and bin(s).count("1") >= t for s in range(256)])


def majority_table(M):
    return at_least_table(M, M // 2 + 1)


def random_tables(M, count, seed):
    """Seeded random tables with bit 0 clear and nothing at or above 2^M."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        bits = np.zeros(256, dtype=np.uint8)
        bits[1:1 << M] = rng.integers(0, 2, (1 << M) - 1)
        out.append(table_of_bits(bits))
    return out


def all_tables(M):
    """Every table of M <= 3 modalities with bit 0 clear and some bit set: 2^(2^M - 1) - 1 of them (1, 7, 127)."""
    n_free = (1 << M) - 1
    return [table_of_bits([0] + [(v >> b) & 1 for b in range(n_free)]) for v in range(1, 1 << n_free)]


def make_masks(n, M, seed):
    """M boolean (n, n) matrices whose first min(n * n, 2^M) entries (row-major) run through the subset patterns 0, 1, 2, ...
    and whose other entries are random with densities from 0.2 to 0.6: with n * n >= 2^M every pattern occurs at some bit."""
    rng = np.random.default_rng(seed)
    mats = [rng.random((n, n)) < (0.2 + 0.4 * m / max(M - 1, 1)) for m in range(M)]
    head = min(n * n, 1 << M)
    for m in range(M):
        flat = mats[m].reshape(-1)
        flat[:head] = (np.arange(head) >> m) & 1
    return mats


def subset_index(mats):
    """s(i, j) = sum_m [mats[m][i, j] != 0] << m."""
    s = np.zeros(mats[0].shape, dtype=np.int64)
    for m, a in enumerate(mats):
        s |= (np.asarray(a) != 0).astype(np.int64) << m
    return s


def subsets_present(mats):
    return set(np.unique(subset_index(mats)).tolist())


def fuse_by_index(s, table):
    """fuse_table_numpy for inputs whose subset index is already known (many tables on the same inputs)."""
    t = np.ascontiguousarray(table, dtype=np.uint64)
    k = np.arange(256)
    bits = ((t[k >> 6] >> (k & 63).astype(np.uint64)) & np.uint64(1)).astype(np.int64)
    return bits[s]


def pack_mask(A, words=None):
    """Boolean (n, n) -> the device layout: (n, words) int64 holding uint64 words, bit j & 63 of word j >> 6 = A[i, j]."""
    n = A.shape[0]
    words = (n + 63) // 64 if words is None else words
    padded = np.zeros((n, words * 64), dtype=np.uint8)
    padded[:, :n] = A != 0
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(n, words).view(np.int64)


def unpack_mask(mask, n):
    """(n, words) int64 / uint64 -> boolean (n, words * 64): every stored bit, padding included."""
    m = np.ascontiguousarray(mask).view(np.uint8).reshape(mask.shape[0], -1)
    return np.unpackbits(m, axis=1, bitorder="little").astype(bool)
