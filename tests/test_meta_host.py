"""Host side of the metadata corpus (mused_amd/meta.py): one encoding pass over a stream gives, for every window, what
the per-window host handling of matrix_operations._metadata_adjacency works out from the window's rows."""
import numpy as np
import pytest

import meta_cases as mc
from mused_amd import meta, synth

STREAMS = {"synth": lambda: synth.metadata_stream(400, 4, missing=0.3)[0], "made": mc.stream, "ties": mc.ties}


@pytest.fixture(scope="module", params=sorted(STREAMS))
def cols(request):
    return STREAMS[request.param]()


@pytest.fixture(scope="module")
def corpora(cols):
    return {t: meta.encode(cols[t], t) for t in mc.TYPES}


def test_shape_and_records(cols, corpora):
    for t, c in corpora.items():
        assert len(c) == mc.N and c.shape == cols[t].shape and c.kind == t and not c.host_only
        assert c.records is not None and len(c.records) == mc.N
        assert c.vrank.dtype == np.int32 and c.vrank.shape == (mc.N + 1,) and c.vrank[0] == 0
        w = c.window(37, 167)
        assert len(w) == 130 and w.shape == (130,) + cols[t].shape[1:]
        if t in ("location", "time"):
            assert np.array_equal(w.records, cols[t][37:167], equal_nan=True)
        else:
            assert np.array_equal(np.asarray(w.records, dtype=object), np.asarray(cols[t][37:167], dtype=object))


@pytest.mark.parametrize("s,e", mc.WINDOWS)
def test_validity_of_a_window_is_the_host_expression(cols, corpora, s, e):
    for t, c in corpora.items():
        valid = np.diff(c.vrank)[s:e].astype(bool)
        assert np.array_equal(valid, mc.host_valid(cols[t][s:e], t)), t
        assert c.vrank[e] - c.vrank[s] == valid.sum()
    c = corpora["location"]
    assert c.rec.dtype == np.float64 and np.array_equal(c.rec, cols["location"].astype(np.float64), equal_nan=True)
    assert np.array_equal(corpora["time"].rec, cols["time"].astype(np.float64))


@pytest.mark.parametrize("s,e", mc.WINDOWS)
def test_user_ids_agree_with_unique_inside_a_window(cols, corpora, s, e):
    c, rows = corpora["username"], cols["username"][s:e]
    uid = c.uid[s:e]
    assert c.uid.dtype == np.int32 and np.array_equal(uid < 0, rows[:, 0] == "")
    valid = np.where(rows[:, 0] != "")[0]
    if len(valid):
        _, ids = np.unique(rows[valid, 0].astype(str), return_inverse=True)
        assert np.array_equal(uid[valid][:, None] == uid[valid][None, :], ids[:, None] == ids[None, :])


def _sets(c, rows):
    return [set(c.tag[c.rowptr[r]:c.rowptr[r + 1]].tolist()) for r in rows]


@pytest.mark.parametrize("s,e", [w for w in mc.WINDOWS if w != (0, 400)])
def test_jaccard_scores_from_global_ids_equal_the_oracle(cols, corpora, s, e):
    from oracle import mo_oracle as omo

    c, rows = corpora["tags"], cols["tags"][s:e]
    valid = np.where(rows[:, 0] != "")[0]
    sets = _sets(c, s + valid)
    S = np.zeros((len(valid), len(valid)))
    for i, a in enumerate(sets):
        for j, b in enumerate(sets):
            if i == j:
                S[i, j] = 1.0
            elif a and b:
                S[i, j] = 0.0 - len(a & b) / (len(a) + len(b) - len(a & b))
    assert np.array_equal(S, omo.jaccard_scores(rows[valid, 0]))


def test_tag_csr_and_posting_lists(cols, corpora):
    c, col = corpora["tags"], cols["tags"][:, 0]
    assert all(a.dtype == np.int32 for a in (c.rowptr, c.tag, c.gpostptr, c.gpostrow))
    assert c.rowptr.shape == (mc.N + 1,) and c.gpostptr.shape == (c.V + 1,) and len(c.tag) == len(c.gpostrow) == c.nnz
    valid = np.diff(c.vrank).astype(bool)
    for r in range(mc.N):
        ids = c.tag[c.rowptr[r]:c.rowptr[r + 1]]
        assert np.all(np.diff(ids) > 0) and (len(ids) == 0 or (0 <= ids[0] and ids[-1] < c.V))
        want = len(set(col[r])) if valid[r] and col[r] else 0   # invalid rows and [] are empty in the CSR
        assert len(ids) == want
    holders = [np.flatnonzero([g in c.tag[c.rowptr[r]:c.rowptr[r + 1]] for r in range(mc.N)]) for g in range(c.V)]
    for g in range(c.V):
        post = c.gpostrow[c.gpostptr[g]:c.gpostptr[g + 1]]
        assert np.all(np.diff(post) > 0) and np.array_equal(post, holders[g])
        for s, e in mc.WINDOWS:   # a window's part of the list is one contiguous sub-range
            lo, hi = np.searchsorted(post, s), np.searchsorted(post, e)
            assert np.array_equal(post[lo:hi], holders[g][(holders[g] >= s) & (holders[g] < e)])


def test_hand_made_posting_cases():
    c, (s, e) = meta.encode(mc.stream()["tags"], "tags"), mc.ORACLE_WINDOW
    row_of = lambda name: [r for r in range(mc.N) if isinstance(c.records[r, 0], list) and name in c.records[r, 0]]
    ident = lambda name: int(next(g for g in c.tag[c.rowptr[row_of(name)[0]]:c.rowptr[row_of(name)[0] + 1]]
                                  if np.array_equal(c.gpostrow[c.gpostptr[g]:c.gpostptr[g + 1]], row_of(name))))
    part = lambda g: c.gpostrow[c.gpostptr[g]:c.gpostptr[g + 1]]
    inside = lambda g: [r for r in part(g) if s <= r < e]
    assert row_of("zz_span") == [10, 80, 300] and inside(ident("zz_span")) == [80]
    assert row_of("zz_out") == [5, 350] and inside(ident("zz_out")) == []
    assert row_of("zz_edge") == [s, e - 1] and inside(ident("zz_edge")) == [s, e - 1]
    assert len(_sets(c, [64])[0]) == 2 and _sets(c, [63]) == [set()] and _sets(c, [60]) == _sets(c, [61]) == _sets(c, [62])


def test_slicing():
    c = meta.encode(mc.stream()["time"], "time")
    w = c[50:300]
    assert (w.lo, w.hi) == (50, 300) and (w[10:20].lo, w[10:20].hi) == (60, 70)
    assert (w[10:20][3:].lo, w[10:20][3:].hi) == (63, 70) and (c[390:999].lo, c[390:999].hi) == (390, 400)
    assert np.array_equal(w[10:20].records, mc.stream()["time"][60:70])
    for bad in (slice(0, 10, 2), 5):
        with pytest.raises(TypeError):
            c[bad]
        with pytest.raises(TypeError):
            w[bad]
    for lo, hi in ((-1, 5), (5, 401), (7, 3)):
        with pytest.raises(IndexError):
            c.window(lo, hi)


def test_host_only_and_bad_arguments():
    cols = mc.stream()
    for t in mc.TYPES:
        c = meta.encode(cols[t], t, max_entries=100)
        assert c.host_only and len(c) == mc.N and len(c.window(3, 9).records) == 6
        with pytest.raises(ValueError):
            c.device_arrays("cuda")
    assert not meta.encode(cols["tags"][:50], "tags", max_entries=10 ** 4).host_only
    with pytest.raises(ValueError):
        meta.encode(cols["time"], "text")
    with pytest.raises(ValueError):
        meta.encode(cols["time"][:, 0], "time")
