"""The `*_ws_bytes` entries of the layouts that share common.h's workspace carver, against a restatement of each layout: the
arrays in their order, each rounded up to 256 bytes.  Equality is exact: a caller sizes its workspace by these values and every
array starts where the sum of the ones before it ends.  (Among the GPU tests because it loads the library; nothing is launched.)"""
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 128), (129, 3, 128), (600, 50, 128), (20000, 50, 4096), (2 ** 19, 1023, 65536)]
ROWS = [n for n, _, _ in SHAPES]


def A(x):
    return (x + 255) // 256 * 256


def _lib():
    from mused_amd import _lib

    return _lib.lib()


def delete_bytes(n, d, chunk):
    t, ldp = (n + 127) // 128, (d + 1) // 2 * 2
    return 9 * A(4 * n) + A(4 * t) + 256 + A(8 * n) + A(8 * chunk * ldp)


@pytest.mark.parametrize("n,d,chunk", SHAPES)
def test_incremental_dbscan(n, d, chunk):
    L = _lib()
    t, ldp = (n + 127) // 128, (d + 1) // 2 * 2
    assert L.mused_dbscan_incr_ws_bytes(n, d, chunk) == 4 * A(4 * n) + 2 * A(4 * t) + 256 + A(8 * chunk * ldp)
    assert L.mused_dbscan_incr_delete_ws_bytes(n, d, chunk) == delete_bytes(n, d, chunk)
    assert L.mused_dbscan_incr_delete_rows_ws_bytes(n, d, chunk) == delete_bytes(n, d, chunk) + 3 * A(4 * n) + A(4 * ((n + 1023) // 1024))


@pytest.mark.parametrize("n", ROWS)
def test_dbscan_and_emst(n):
    L = _lib()
    t = (n + 127) // 128
    # nrm; count, parent, root, rank; tile flags; info (16 bytes)
    assert L.mused_dbscan_ws_bytes(n) == A(8 * n) + 4 * A(4 * n) + A(4 * t) + 256
    # nrm, best, second, cbest, ckey (8 bytes each); bcol, bcol2, comp, parent; tile components; info (16 bytes); ctl (8 bytes)
    assert L.mused_emst_ws_bytes(n) == 5 * A(8 * n) + 4 * A(4 * n) + A(4 * t) + 256 + 256


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("cap", [1, 33, 257])
def test_knn_fused(n, cap):
    # norms, tau; count, taucol; the overflow word (256 bytes); candidate scores and columns
    assert _lib().mused_knn_fused_ws_bytes(n, cap) == 2 * A(8 * n) + 2 * A(4 * n) + 256 + A(8 * n * cap) + A(4 * n * cap)


@pytest.mark.parametrize("n,q", [(1, 1), (300, 129), (20000, 2000)])
@pytest.mark.parametrize("d", [1, 50])
def test_rows_find(n, q, d):
    total = n + q
    slots, nb = 2 * total + 1, (total + 1023) // 1024
    # table, first, firstq (one int per slot); two key / value pairs (one int per element); 256 counters per block of 1,024
    assert _lib().mused_rows_find_ws_bytes(n, q, d) == 3 * A(4 * slots) + 4 * A(4 * total) + A(4 * 256 * nb)


def tokenise_bytes(n, docs, slots, elem, cap, tile):
    # the lowered text; docptr; token starts per block of the scan; tok_start, tok_len, tok_slot; the table; occupied slots per
    # block of 256; ent_row; two key / value pairs of the sort; 256 counters per tile of 1,024 entries
    return (A(elem * n) + A(4 * (docs + 1)) + A(4 * ((n + tile - 1) // tile)) + 3 * A(4 * cap) + A(4 * slots)
            + A(4 * ((slots + 255) // 256)) + A(4 * cap) + 4 * A(4 * cap) + A(4 * 256 * ((cap + 1023) // 1024)))


@pytest.mark.parametrize("slots", [0, 1, 4099])
@pytest.mark.parametrize("n,docs", [(1, 1), (4097, 3), (10 ** 6, 2000)])
def test_tokenise(n, docs, slots):
    L = _lib()
    # bytes: a token takes three bytes or more, 4,096 bytes per block of the scan, by default two slots per possible token
    cap = n // 3 + 1
    assert L.mused_tokenise_ws_bytes(n, docs, slots) == tokenise_bytes(n, docs, slots or 2 * cap, 1, cap, 4096)
    # code points (4 bytes each): a token takes two or more, 2,048 per block
    cap = n // 2 + 1
    assert L.mused_tokenise_cp_ws_bytes(n, docs, slots) == tokenise_bytes(n, docs, slots or 2 * cap, 4, cap, 2048)
