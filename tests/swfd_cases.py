"""Shared cases and helpers of the sliding-window sketch's edge tests (tests/test_swfd_cases_host.py on the CPU,
tests/test_gpu_swfd_edges.py on the device): seeded streams with a heavy burst, an instrumented copy of the
specification (oracle/swfd_oracle.py) that records how far every keep / dump / discard decision is from its threshold,
the parser of the exported state blob, and the comparison rule of tests/test_gpu_path.py::_compare.

TEST INFRASTRUCTURE ONLY: nothing here is imported by the package."""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

from oracle.swfd_oracle import REL_TOL, SeqBasedSWFD as Ora, _shrink, _Sketch

Case = namedtuple("Case", "N l d burst seed")

# name: N, l, d, burst (lo, hi, f), seed.  n = 4 N + 13 rows each.
CASES = {
    "l4": Case(96, 4, 12, (40, 70, 9.0), 11),
    "l3_odd": Case(70, 3, 5, (20, 45, 9.0), 12),              # odd l: the order-3l query plan is rounded up to even
    "l6_ragged_epoch": Case(100, 6, 24, (30, 60, 9.0), 13),   # N no multiple of l: a short block ends every epoch
    "l8": Case(90, 8, 20, (20, 50, 12.0), 14),
    "l2_d1": Case(50, 2, 1, (15, 30, 9.0), 15),
    "l8_d5": Case(64, 8, 5, (20, 40, 9.0), 16),               # d < l: every Gram matrix is rank deficient
    "N5_l8": Case(5, 8, 6, (7, 12, 9.0), 17),                 # N < l: every rotation is an epoch end
    "l1": Case(40, 1, 3, (10, 25, 9.0), 18),                  # the sketch is identically zero
    # the two below are used for one switch each (MUSED_SWFD_ORDERS / MUSED_SWFD_GRAM_SPLIT)
    "l128_d40": Case(300, 128, 40, (100, 200, 9.0), 19),
    "split_d100": Case(120, 8, 100, (30, 60, 9.0), 20),       # 4 k-chunks of 32 columns, the last one 4 wide
}
TABLE = ("l4", "l3_odd", "l6_ragged_epoch", "l8", "l2_d1", "l8_d5", "N5_l8", "l1")
BURST_CASES = ("l4", "l3_odd", "l6_ragged_epoch", "l8", "l2_d1", "l8_d5")


def stream(N, d, n, seed, burst):
    """n Gaussian rows of length d, the first min(3, d) columns heavy, rows burst[0] .. burst[1] multiplied by burst[2]:
    the burst makes the low levels overflow their snapshot rings, so that get() has to climb levels."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    k = min(3, d)
    X[:, :k] *= np.array([6.0, 4.0, 2.5])[:k]
    lo, hi, f = burst
    X[lo:hi] *= f
    return X


@functools.lru_cache(maxsize=None)
def case_stream(name):
    """(X, R) of a case: 4 N + 13 rows, R = the largest squared row norm.  Read only."""
    c = CASES[name]
    X = stream(c.N, c.d, 4 * c.N + 13, c.seed, c.burst)
    X.setflags(write=False)
    return X, float((X * X).sum(1).max())


def blocks(l, n):
    """Ragged block sizes in [1, 2 l + 2] that sum to n: appends end inside blocks, on rotation boundaries and across
    epoch ends."""
    rng = np.random.default_rng(5)
    out, t = [], 0
    while t < n:
        b = min(int(rng.integers(1, 2 * l + 3)), n - t)
        out.append(b)
        t += b
    return out


def case_blocks(name):
    c = CASES[name]
    return blocks(c.l, 4 * c.N + 13)


# ---- the instrumented specification ---------------------------------------------------------------------------------
class _ISketch(_Sketch):
    """A sketch of the specification that reports every rotation to its owner and carries the running maximum of lam0
    (the scale a device rotation is compared at) through the MAIN <- AUX swap."""

    def __init__(self, d, theta, cap, owner):
        super().__init__(d, theta, cap)
        self.owner = owner
        self.lam_max = 0.0

    def copy_from(self, other):
        super().copy_from(other)
        self.lam_max = other.lam_max

    def clear(self, d):
        super().clear(d)
        self.lam_max = 0.0

    def rotate(self, pending, t, N, ell):
        self.expire(t, N)
        M = np.vstack([self.K, pending]) if len(pending) else self.K
        s2, _, lam0, _ = _shrink(M, ell)
        st = self.owner.stats
        self.lam_max = max(self.lam_max, lam0)
        st["lam_max"] = max(st["lam_max"], lam0)
        tol, dumps = REL_TOL * lam0, 0
        for v in s2:
            if v > 0.0:
                st["discard_dist"] = min(st["discard_dist"], abs(v - tol) / lam0)
            if v > tol:
                st["theta_dist"] = min(st["theta_dist"], abs(v - self.theta) / self.theta)
                dumps += v >= self.theta
        if len(self.qt) + dumps > self.cap:
            st["evict_rotations"] += 1
        super().rotate(pending, t, N, ell)


class InstrumentedSWFD(Ora):
    """oracle.swfd_oracle.SeqBasedSWFD that records, over every rotation of every sketch: the largest lam0, the smallest
    relative distance |s2 - theta| / theta of a surviving direction from its dump threshold, the smallest
    |s2 - 1e-10 lam0| / lam0 of a positive s2, the rotations that evict from a full ring, and the rotation times."""

    def __init__(self, N, R, d, sketch_dim):
        super().__init__(N, R, d, sketch_dim)
        self.stats = {"lam_max": 0.0, "theta_dist": math.inf, "discard_dist": math.inf, "evict_rotations": 0}
        self.rotation_times = []
        cap = 2 * self.ell
        self.main = [_ISketch(self.d, th, cap, self) for th in self.theta]
        self.aux = [_ISketch(self.d, th, cap, self) for th in self.theta]

    def _rotate_all(self):
        self.rotation_times.append(self.i)
        super()._rotate_all()

    def epoch_start(self):
        return ((self.i - 1) // self.N) * self.N if self.i else 0

    def frozen(self):
        """MAIN levels the device stops rotating (csrc/swfd.hip, swfd_rep_kernel): below the top, not in the first epoch,
        a snapshot created in the current epoch already lost -- get() cannot select them before AUX replaces them."""
        if self.i <= self.N:
            return frozenset()
        e0 = self.epoch_start()
        return frozenset(j for j in range(self.L - 1) if self.main[j].dropped_t > e0)


def _snap_level(sk, d):
    return {"K": sk.K.copy(), "qv": np.array(sk.qv, dtype=np.float64).reshape(len(sk.qv), d), "qt": list(sk.qt),
            "dropped": sk.dropped_t, "lam_max": sk.lam_max}


@functools.lru_cache(maxsize=None)
def oracle_trace(name):
    """The specification run over the case's ragged blocks, once: (oracle, [state after every block]).  A state is
    {i, get, level, pending, frozen, epoch_start, halves: (MAIN levels, AUX levels)}.  Read only."""
    c = CASES[name]
    X, R = case_stream(name)
    ora = InstrumentedSWFD(N=c.N, R=R, d=c.d, sketch_dim=c.l)
    trace, t = [], 0
    for b in case_blocks(name):
        ora.fit(X[t:t + b])
        t += b
        trace.append({"i": ora.i, "get": ora.get(), "level": ora.select_level(), "pending": ora.pending.copy(),
                      "frozen": ora.frozen(), "epoch_start": ora.epoch_start(),
                      "halves": ([_snap_level(s, c.d) for s in ora.main], [_snap_level(s, c.d) for s in ora.aux])})
    return ora, trace


# ---- the exported state ------------------------------------------------------------------------------------------------
def parse_half(blob, L, l, d):
    """One exported half (mused_swfd_export_half) as a list of L levels {buf (2l, d), ring (2l, d), qt (2l,), nk, head,
    count, near, dropped}.  Layout: [bufs L*2l*d f64 | rings L*2l*d f64 | timestamps L*2l i64 | meta L*4 i32 | dropped L i64]."""
    raw = np.ascontiguousarray(np.asarray(blob, dtype=np.uint8)).tobytes()
    n2 = 2 * l
    sizes = [L * n2 * d * 8, L * n2 * d * 8, L * n2 * 8, L * 16, L * 8]
    assert len(raw) == sum(sizes), (len(raw), sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    part = [raw[offs[k]:offs[k + 1]] for k in range(5)]
    bufs = np.frombuffer(part[0], dtype=np.float64).reshape(L, n2, d)
    rings = np.frombuffer(part[1], dtype=np.float64).reshape(L, n2, d)
    qt = np.frombuffer(part[2], dtype=np.int64).reshape(L, n2)
    meta = np.frombuffer(part[3], dtype=np.int32).reshape(L, 4)
    dropped = np.frombuffer(part[4], dtype=np.int64)
    return [{"buf": bufs[j], "ring": rings[j], "qt": qt[j], "nk": int(meta[j, 0]), "head": int(meta[j, 1]),
             "count": int(meta[j, 2]), "near": int(meta[j, 3]), "dropped": int(dropped[j])} for j in range(L)]


def ring_slots(lv):
    """Slots of the live snapshots of a parsed level, oldest first."""
    cap = len(lv["qt"])
    return [(lv["head"] + q) % cap for q in range(lv["count"])]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def live_equal(a, b):
    """Two parsed levels hold the same sketch bit for bit: counters, the whole buffer, the live part of the ring (slots
    outside [head, head + count) keep whatever an earlier snapshot left there)."""
    if (a["nk"], a["count"], a["dropped"]) != (b["nk"], b["count"], b["dropped"]):
        return False
    sa, sb = ring_slots(a), ring_slots(b)
    return (same_bits(a["buf"], b["buf"]) and np.array_equal(a["qt"][sa], b["qt"][sb])
            and same_bits(a["ring"][sa], b["ring"][sb]))


# ---- device result against the specification ------------------------------------------------------------------------
def compare_get(dev, ora, tag):
    """tests/test_gpu_path.py::_compare with its numbers: level equal, sigma within 1e-8 sigma_1 (1e-6 relative above
    1e-3 sigma_1), B^T B and delta within 1e-8 sigma_1^2.  `dev`: a device sketch or its get() tuple, `ora` likewise.
    Returns the device tuple."""
    got = dev.get() if hasattr(dev, "get") else dev
    Bd, sd, ld, dd = got
    Bo, so, lo, do = ora.get() if hasattr(ora, "get") else ora
    assert ld == lo, f"{tag}: level {ld} vs {lo}"
    s0 = max(so[0], 1e-300)
    np.testing.assert_allclose(sd, so, rtol=0, atol=1e-8 * s0, err_msg=tag)
    big = so > 1e-3 * s0
    np.testing.assert_allclose(sd[big], so[big], rtol=1e-6, err_msg=tag)
    np.testing.assert_allclose(Bd.T @ Bd, Bo.T @ Bo, rtol=0, atol=1e-8 * s0 * s0, err_msg=tag)
    assert abs(dd - do) <= 1e-8 * s0 * s0, f"{tag}: delta {dd} vs {do}"
    return got
