"""Inputs shared by tests/test_adjacency_cases_host.py and tests/test_gpu_adjacency_edges.py: the case table of the adjacency
bitmask layer (csrc/adjacency.hip, mused_group_mask, mused_lists_to_mask) and a plain NumPy restatement of every operation on
boolean n x n matrices, with named wrong variants.

The device representation: an n x words array of uint64, bit (j & 63) of word (j >> 6) of row i set <=> A[i, j]; the row
pitch is `words` >= ceil(n / 64); every bit at a column >= n and every padding word is zero.

The restatements follow the device's loop structure where that structure is what can go wrong (the 1024-row blocks of the
degree scan, the 64-word groups of the CSR fill, the 64 x 64 tiles of the transpose), so that each VARIANT below is the
restatement with one of those steps left out.  tests/test_adjacency_cases_host.py checks the restatements against direct
boolean NumPy and that every variant breaks a case of the table: the table reaches the edges it claims."""
import functools

import numpy as np

NS = (1, 2, 63, 64, 65, 127, 128, 129, 333, 1023, 1024, 1025, 2049, 4097, 4160)
PATTERNS = ("empty", "full", "corner", "top_right", "random", "hubs", "asym")
PADS = (0, 3)
SCAN_BLOCK = 1024      # degree_scan_kernel: rows per trip of its one workgroup
CSR_GROUP = 64         # mask_to_csr_kernel: words per trip of a row's wave
TILE = 64              # mask_transpose_kernel: bits per tile side
VARIANTS = ("big_endian", "tail_bits_set", "scan_carry_dropped", "csr_carry_dropped", "partial_tile_skipped", "self_kept")


def words_for(n):
    return (n + 63) // 64


@functools.lru_cache(maxsize=None)
def pattern(n, name):
    """Boolean n x n matrix of a case (read-only)."""
    A = np.zeros((n, n), dtype=bool)
    if name == "empty":
        pass
    elif name == "full":                       # full off-diagonal: every degree n - 1
        A[:] = True
        np.fill_diagonal(A, False)
    elif name == "corner":                     # the last bit of the last word of the last row
        A[n - 1, n - 1] = True
    elif name == "top_right":
        A[0, n - 1] = True
    elif name == "random":
        A = np.random.default_rng([n, 7]).random((n, n)) < 0.07
    elif name == "hubs":                       # a few rows of degree n - 1 among empty rows
        for i in sorted({0, n // 2, n - 1}):
            A[i] = True
            A[i, i] = False
    elif name == "asym":                       # strictly upper triangular, arange-style: a transposed write shows
        lin = np.arange(n * n, dtype=np.int64).reshape(n, n)
        A = (lin % 3 == 0) & (lin % n > lin // n)
    else:
        raise KeyError(name)
    A = np.ascontiguousarray(A)
    A.setflags(write=False)
    return A


CASES = [(n, p) for n in NS for p in PATTERNS]


# ---- pack / unpack ---------------------------------------------------------------------------------------------------
def pack(A, words=None, variant=None):
    """n x words uint64 bitmask of a boolean matrix (padding words zero)."""
    A = np.asarray(A, dtype=bool)
    n, m = A.shape
    words = words_for(m) if words is None else words
    assert words >= words_for(m)
    out = np.zeros((n, words), dtype=np.uint64)
    for w in range(words_for(m)):                      # column j = 64 w + b -> bit b of word w
        cols = A[:, 64 * w:64 * w + 64].astype(np.uint64)
        b = np.arange(cols.shape[1], dtype=np.uint64)
        shift = (np.uint64(63) - b) if variant == "big_endian" else b
        out[:, w] = np.bitwise_or.reduce(cols << shift, axis=1)
    if variant == "tail_bits_set" and m & 63:
        out[:, (m - 1) >> 6] |= ~np.uint64(0) << np.uint64(m & 63)
    return out


def unpack(mask, n):
    """The first n columns of a bitmask as booleans; bits past n and padding words are not looked at."""
    mask = np.asarray(mask).view(np.uint64)
    out = np.zeros((mask.shape[0], n), dtype=bool)
    for w in range(words_for(n)):
        b = np.arange(min(64, n - 64 * w), dtype=np.uint64)
        out[:, 64 * w:64 * w + len(b)] = (mask[:, w:w + 1] >> b) & np.uint64(1)
    return out


def tail_is_clean(mask, n):
    """No bit at a column >= n, no bit in a padding word."""
    mask = np.asarray(mask).view(np.uint64)
    w = words_for(n)
    if mask[:, w:].any():
        return False
    if n & 63 and (mask[:, w - 1] >> np.uint64(n & 63)).any():
        return False
    return True


def popcount(mask):
    """Set bits per row, EVERY bit of every word at face value (what mask_degree_kernel counts)."""
    mask = np.ascontiguousarray(mask).view(np.uint64)
    return np.unpackbits(mask.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)


# ---- fuse ------------------------------------------------------------------------------------------------------------
def fuse(mats):
    out = np.array(mats[0], dtype=bool)
    for m in mats[1:]:
        out = np.logical_or(out, m)
    return out


# ---- degrees, exclusive rowptr, [max degree, nnz] -----------------------------------------------------------------------
def degrees(A, variant=None):
    """(deg[n], rowptr[n + 1], [max degree, nnz]) as int64, the scan in blocks of SCAN_BLOCK rows with a carry."""
    A = np.asarray(A, dtype=bool)
    n = A.shape[0]
    deg = np.array([int(np.count_nonzero(A[i])) for i in range(n)], dtype=np.int64)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    carry = 0
    for base in range(0, n, SCAN_BLOCK):
        blk = deg[base:base + SCAN_BLOCK]
        start = 0 if variant == "scan_carry_dropped" else carry
        run = start
        for t, v in enumerate(blk):
            rowptr[base + t] = run
            run += int(v)
        carry += int(blk.sum())
    rowptr[n] = carry
    return deg, rowptr, np.array([int(deg.max()), carry], dtype=np.int64)


# ---- ascending CSR -----------------------------------------------------------------------------------------------------
def csr(A, rowptr, variant=None, guard=1, fill=-1):
    """colidx (nnz + guard entries, the rest `fill`): row i's set columns ascending from rowptr[i], written per group of
    CSR_GROUP words with the running base carried from group to group."""
    A = np.asarray(A, dtype=bool)
    n = A.shape[0]
    col = np.full(int(rowptr[n]) + guard, fill, dtype=np.int64)
    span = 64 * CSR_GROUP
    for i in range(n):
        base = int(rowptr[i])
        for c0 in range(0, n, span):
            cols = c0 + np.flatnonzero(A[i, c0:c0 + span])
            col[base:base + len(cols)] = cols
            if variant != "csr_carry_dropped":
                base += len(cols)
    return col


# ---- transpose -----------------------------------------------------------------------------------------------------------
def transpose(A, variant=None):
    """A^T by TILE x TILE tiles (the last row and column of tiles are partial unless TILE divides n)."""
    A = np.asarray(A, dtype=bool)
    n = A.shape[0]
    out = np.zeros((n, n), dtype=bool)
    for r0 in range(0, n, TILE):
        for c0 in range(0, n, TILE):
            partial = r0 + TILE > n or c0 + TILE > n
            if variant == "partial_tile_skipped" and partial:
                continue
            blk = A[r0:r0 + TILE, c0:c0 + TILE]          # bit b of tile row a -> bit a of tile row b
            out[c0:c0 + blk.shape[1], r0:r0 + blk.shape[0]] = blk.T
    return out


# ---- dense import -----------------------------------------------------------------------------------------------------
def from_dense(D):
    """(boolean matrix, non-binary flag): nonzero -> edge, anything that is neither 0 nor 1 raises the flag.  -0.0 is zero;
    NaN compares unequal to both, so it is an edge and raises the flag."""
    D = np.asarray(D)
    nz = D != 0
    return nz, int(bool((nz & (D != 1)).any()))


DENSE_EDGES = (2, -1, 0.5, float("nan"))     # each raises the flag (0.5 and NaN: floating types only)


# ---- username relation -------------------------------------------------------------------------------------------------
def group_mask(ids, variant=None):
    """A[i, j] <=> ids[i] == ids[j] >= 0 and i != j."""
    ids = np.asarray(ids)
    n = len(ids)
    A = np.zeros((n, n), dtype=bool)
    for i in range(n):
        if ids[i] < 0:
            continue
        for j in range(n):
            if ids[j] == ids[i] and (j != i or variant == "self_kept"):
                A[i, j] = True
    return A


def group_ids(n, kind):
    if kind == "equal":
        return np.full(n, 5, dtype=np.int32)
    if kind == "distinct":
        return np.arange(n, dtype=np.int32)[::-1].copy()
    if kind == "mixed":                      # a few groups, a fifth of the rows without a name (-1)
        rng = np.random.default_rng([n, 11])
        ids = rng.integers(0, max(2, n // 9), n).astype(np.int32)
        ids[rng.random(n) < 0.2] = -1
        return ids
    raise KeyError(kind)


GROUP_NS = (1, 64, 65, 333)
GROUP_KINDS = ("equal", "distinct", "mixed")


# ---- neighbour lists -> mask -------------------------------------------------------------------------------------------
def lists_to_mask(idx, n, row_map=None, variant=None):
    """List row r (entries: list rows) becomes window row row_map[r] with the bits row_map[idx[r, j]], own column dropped;
    every other window row is empty.  Without a map: the identity."""
    idx = np.asarray(idx)
    A = np.zeros((n, n), dtype=bool)
    for r in range(idx.shape[0]):
        wr = int(row_map[r]) if row_map is not None else r
        for c in idx[r]:
            wc = int(row_map[c]) if row_map is not None else int(c)
            if wc != wr or variant == "self_kept":
                A[wr, wc] = True
    return A


def list_case(n, k, n_rows=None, seed=0):
    """(idx[n_rows, k] int32, row_map or None): in-range lists that contain their own row (column 0, where k > 0) and a
    repeated column (the last entry repeats the one before it, where k > 2); with n_rows the rows map to a random ascending
    subset of the n window rows."""
    rng = np.random.default_rng([n, k, seed, 0 if n_rows is None else n_rows + 1])
    m = n if n_rows is None else n_rows
    idx = rng.integers(0, max(m, 1), (m, k)).astype(np.int32)
    if k > 0 and m > 0:
        idx[:, 0] = np.arange(m)
    if k > 2:
        idx[:, k - 1] = idx[:, k - 2]
    row_map = None
    if n_rows is not None:
        row_map = np.sort(rng.choice(n, n_rows, replace=False)).astype(np.int32)
    return idx, row_map
