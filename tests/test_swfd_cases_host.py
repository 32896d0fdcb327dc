"""tests/swfd_cases.py on the CPU: every case reaches what its table entry names, with the specification alone -- the
keep / dump / discard decisions are far from their thresholds (so the device cannot flip one by rounding), the burst cases
overflow their rings, climb levels and freeze MAIN levels, `l1` is identically zero and `N5_l8` rotates at epoch ends only;
the blob parser inverts the documented layout.  tests/test_gpu_swfd_edges.py relies on all of it (no GPU)."""
import numpy as np
import pytest

import swfd_cases as sc


@pytest.mark.parametrize("name", list(sc.CASES))
def test_decisions_are_far_from_their_thresholds(name):
    """100 x the comparison tolerance (1e-8) between every surviving direction and its dump threshold, and 1e-8 lam0
    between every positive shrunk energy and the discard rule."""
    ora, _ = sc.oracle_trace(name)
    st = ora.stats
    print(name, st)
    assert st["theta_dist"] >= 1e-6
    assert st["discard_dist"] >= 1e-8


@pytest.mark.parametrize("name", sc.BURST_CASES)
def test_burst_cases_evict_climb_and_freeze(name):
    c = sc.CASES[name]
    ora, trace = sc.oracle_trace(name)
    assert ora.stats["evict_rotations"] >= 1
    levels = {s["level"] for s in trace}
    print(name, "evictions", ora.stats["evict_rotations"], "levels", sorted(levels), "of", ora.L)
    assert 0 in levels and len(levels - {0}) >= 2
    later = [s for s in trace if s["i"] > c.N]
    assert any(s["frozen"] for s in later) and any(not s["frozen"] for s in later)
    # the rule, restated: below the top, a snapshot of the current epoch lost
    for s in later:
        assert s["frozen"] == {j for j in range(ora.L - 1) if s["halves"][0][j]["dropped"] > s["epoch_start"]}
    assert not any(s["frozen"] for s in trace if s["i"] <= c.N)


def test_blocks_end_everywhere():
    """The ragged blocks end inside blocks, on rotation boundaries and on epoch ends' both sides."""
    for name in sc.TABLE:
        c = sc.CASES[name]
        ends = np.cumsum(sc.case_blocks(name))
        assert ends[-1] == 4 * c.N + 13
        in_epoch = (ends - 1) % c.N + 1
        assert np.any(in_epoch % c.l == 0) or c.l > c.N
        assert np.any((in_epoch % c.l != 0) & (in_epoch != c.N)) or c.l == 1
        if c.N > 2 * c.l + 2:                                       # (a block is shorter than an epoch)
            assert len({int(e - 1) // c.N for e in ends}) == 5      # a block ends in every epoch


def test_l1_is_identically_zero():
    _, trace = sc.oracle_trace("l1")
    for s in trace:
        B, sig, lvl, delta = s["get"]
        assert not B.any() and not sig.any()


def test_n5_l8_rotates_at_epoch_ends_only():
    ora, _ = sc.oracle_trace("N5_l8")
    assert ora.rotation_times == list(range(5, ora.i + 1, 5))


def test_l128_d40_stays_on_level_zero():
    ora, trace = sc.oracle_trace("l128_d40")
    assert ora.stats["evict_rotations"] == 0 and {s["level"] for s in trace} == {0}


def test_split_case_has_a_narrow_last_chunk():
    """MUSED_SWFD_GRAM_SPLIT=4 at d = 100: the k-chunk is 32 columns (csrc/swfd.hip: ceil(d / split) rounded up to 16), every
    chunk starts below d and the last one holds 4 columns."""
    d, split = sc.CASES["split_d100"].d, 4
    kchunk = ((d + split - 1) // split + 15) // 16 * 16
    assert kchunk == 32 and (split - 1) * kchunk < d and d - (split - 1) * kchunk == 4


def test_parse_half_inverts_the_layout():
    L, l, d = 3, 2, 5
    rng = np.random.default_rng(0)
    bufs, rings = rng.standard_normal((L, 2 * l, d)), rng.standard_normal((L, 2 * l, d))
    qt = rng.integers(0, 1 << 40, (L, 2 * l))
    meta = rng.integers(0, 2 * l, (L, 4)).astype(np.int32)
    dropped = rng.integers(0, 1 << 40, L)
    blob = np.frombuffer(bufs.tobytes() + rings.tobytes() + qt.astype(np.int64).tobytes() + meta.tobytes()
                         + dropped.astype(np.int64).tobytes(), dtype=np.uint8)
    lv = sc.parse_half(blob, L, l, d)
    for j in range(L):
        assert np.array_equal(lv[j]["buf"], bufs[j]) and np.array_equal(lv[j]["ring"], rings[j])
        assert np.array_equal(lv[j]["qt"], qt[j]) and lv[j]["dropped"] == dropped[j]
        assert [lv[j]["nk"], lv[j]["head"], lv[j]["count"], lv[j]["near"]] == list(meta[j])
        assert sc.ring_slots(lv[j]) == [(meta[j, 1] + q) % (2 * l) for q in range(meta[j, 2])]
    with pytest.raises(AssertionError):
        sc.parse_half(blob[:-1], L, l, d)
