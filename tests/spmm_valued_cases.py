"""Case table and host restatements shared by the valued-SpMM and edge-value tests (no GPU here).

The rules under test:
  valued SpMM     Y[i, c] is accumulated over row i's list, in list order, from 0.0: acc = acc + (val[e] * Q[col[e], c]), the
                  product rounded before the add.
  edge values     val[e] = the fp64 sum from 0.0, in modality order, of w_m over the modalities whose bit (i, col[e]) is set;
                  for the lists of the transposed pattern the bit read is (col[e], i).
`restate` / `values_from_masks` are these rules in NumPy; the `wrong_*` functions are the variants a kernel could compute
instead.  tests/test_spmm_valued_host.py shows that each of them changes a case of the table, so the GPU tests, which compare
int64 bit patterns against the restatement on the same table, can tell them apart."""
from fractions import Fraction

import numpy as np

ROWS, WIDE = 0, 1
PATHS = {"rows": ROWS, "wide": WIDE}
# the grid of tests/test_gpu_spmm_paths.py: below, at and above the 4 rows of a workgroup, a ragged last workgroup
NS = (1, 6, 7, 8, 29, 257)
# empty rows, every remainder of the 4-entry step, steps of 1 .. 5 trips
DEGREES = (5, 0, 1, 2, 3, 4, 7, 8, 9, 23)
# a single lane, one / two / three loads of a 192-column trip of `wide` and a second trip, its second load on 1 and 31 lanes
RS = (2, 14, 16, 18, 126, 128, 130, 138, 190, 192, 194, 266)
# the cases small enough for exact rational arithmetic (the fused multiply-add variant)
SMALL = ((7, 2), (29, 14))


def make_lists(n):
    """Neighbour lists of n rows with the degrees of DEGREES in turn, ascending; a neighbour may repeat, and every third list
    of two or more names rows 0 and n - 1."""
    rng = np.random.default_rng(1000 + n)
    lists = []
    for i in range(n):
        d = DEGREES[i % len(DEGREES)]
        nb = np.sort(rng.choice(n, d, replace=d > n))
        if d >= 2 and i % 3 == 0:
            nb[0], nb[-1] = 0, n - 1
        if d >= 3 and i % 4 == 2:
            nb[1] = nb[2]
        lists.append(nb.astype(np.int32))
    return lists


def make_values(lists, seed):
    """One fp64 value per entry: magnitudes spread over 2^50, both signs, and in every list of five or more entries a +0.0,
    a -0.0 and a subnormal; every fifth row carries ONE value, 0.3, on all its entries (a row of a weighted fusion whose edges
    come from one modality)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, nb in enumerate(lists):
        d = len(nb)
        v = rng.standard_normal(d) * np.exp2(rng.integers(-25, 26, d).astype(np.float64))
        if i % 5 == 4:
            v[:] = 0.3
        elif d >= 5:
            v[1], v[2], v[3] = 0.0, -0.0, (3 + i) * 5e-324
        out.append(v)
    return out


def make_q(n, r, seed):
    """Rows of mixed size (the order of a sum matters) with -0.0 in every seventh entry of a row."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, r)) * np.exp(rng.uniform(-8.0, 8.0, (n, 1)))
    Q.reshape(-1)[3::7] = -0.0
    return Q


def restate(lists, vals, Q):
    """The rule: one element at a time, acc = acc + (v * q), each operation rounded to fp64."""
    want = np.zeros((len(lists), Q.shape[1]))
    for i, (nb, v) in enumerate(zip(lists, vals)):
        acc = np.zeros(Q.shape[1])
        for j, x in zip(nb, v):
            prod = x * Q[j]      # rounded product (NumPy does not fuse)
            acc = acc + prod     # rounded sum
        want[i] = acc
    return want


def _round_fraction(x):
    return float(x)   # Fraction -> float is correctly rounded (round to nearest even)


def wrong_fma(lists, vals, Q):
    """acc = fma(v, q, acc): one rounding per step (exact rational arithmetic, then one rounding)."""
    want = np.zeros((len(lists), Q.shape[1]))
    for i, (nb, v) in enumerate(zip(lists, vals)):
        for c in range(Q.shape[1]):
            acc = 0.0
            for j, x in zip(nb, v):
                acc = _round_fraction(Fraction(acc) + Fraction(float(x)) * Fraction(float(Q[j, c])))
            want[i, c] = acc
    return want


def wrong_reversed(lists, vals, Q):
    return restate([nb[::-1] for nb in lists], [v[::-1] for v in vals], Q)


def wrong_pairwise(lists, vals, Q):
    """Two partial sums, even and odd entries, added at the end (what two accumulators per lane would give)."""
    even = restate([nb[0::2] for nb in lists], [v[0::2] for v in vals], Q)
    odd = restate([nb[1::2] for nb in lists], [v[1::2] for v in vals], Q)
    return even + odd


def wrong_value_after_sum(lists, vals, Q):
    """The value applied after the sum: the rows of Q of a run of equal values are added first, then multiplied once."""
    want = np.zeros((len(lists), Q.shape[1]))
    for i, (nb, v) in enumerate(zip(lists, vals)):
        acc = np.zeros(Q.shape[1])
        e = 0
        while e < len(nb):
            f = e
            part = np.zeros(Q.shape[1])
            while f < len(nb) and v[f] == v[e] and np.signbit(v[f]) == np.signbit(v[e]):
                part = part + Q[nb[f]]
                f += 1
            acc = acc + v[e] * part
            e = f
        want[i] = acc
    return want


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- edge values of a weighted fusion -----------------------------------------------------------------------------------

def make_masks(n, M, seed):
    """M asymmetric boolean n x n masks, about 3 ones per row each, that share a common core (edges every modality has) --
    one is in row 0 -- and are not symmetric."""
    rng = np.random.default_rng(seed)
    core = rng.random((n, n)) < min(1.0, 2.0 / n)
    core[0, n // 2] = True
    masks = [core | (rng.random((n, n)) < min(1.0, 3.0 / n)) for _ in range(M)]
    return masks


def lists_of(pattern):
    """(rowptr int32, colidx int32) of a boolean matrix, columns ascending."""
    rows, cols = np.nonzero(pattern)
    rowptr = np.zeros(pattern.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=pattern.shape[0]), out=rowptr[1:])
    return rowptr, cols.astype(np.int32)


def _rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def values_from_masks(masks, weights, rowptr, colidx, transposed):
    """The rule: per entry, from 0.0, v = v + w_m for the modalities in order whose bit is set: (i, col), or (col, i) for the
    lists of the transposed pattern."""
    i = _rows_of(rowptr)
    ri, ci = (colidx, i) if transposed else (i, colidx)
    v = np.zeros(len(colidx))
    for A, w in zip(masks, weights):
        v = np.where(A[ri, ci], v + w, v)
    return v


def wrong_values_untransposed(masks, weights, rowptr, colidx, transposed):
    """The transposed lists valued from (i, col) instead of (col, i)."""
    return values_from_masks(masks, weights, rowptr, colidx, False)


def wrong_values_reversed_order(masks, weights, rowptr, colidx, transposed):
    return values_from_masks(masks[::-1], list(weights)[::-1], rowptr, colidx, transposed)


def pack_mask(A):
    """boolean n x n -> (n, ceil(n / 64)) int64 words, bit j of row i <=> A[i, j]."""
    n = A.shape[0]
    words = (n + 63) // 64
    padded = np.zeros((n, words * 64), dtype=np.uint8)
    padded[:, :n] = A
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(n, words).view(np.int64)


ORDER_WEIGHTS = ((2.0 ** 53, 1.0, 1.0), (1.0, 1.0, 2.0 ** 53))   # the modality order decides the last bit of the sum
