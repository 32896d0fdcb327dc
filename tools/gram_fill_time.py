"""Times the Gram product of an FD rotation on sketch operands with a tail (csrc/gemm_f64.h), with and without the fill source
(tiles of pending rows copied from P P^T instead of computed), alternating, and the P P^T launch of a chunk of blocks on its
own; HIP events on a quiet GPU:
python tools/gram_fill_time.py [batch listed n2 d lanes blocks]     (default: the benchmark's 7-lane group, 196 115 256 1024 7 16)
The launch without the fill source is the one every rotation ran before round 11."""
import ctypes as C, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mused_amd import _lib
from mused_amd.engine import ptr, stream_ptr

batch, listed, n2, d, lanes, blocks = [int(a) for a in sys.argv[1:7]] if len(sys.argv) >= 7 else (196, 115, 256, 1024, 7, 16)
ell, per_lane = n2 // 2, batch // lanes
L = _lib.lib()
tail_fn = L.mused_debug_gemm_f64_batched_tail
tail_fn.restype = C.c_int
tail_fn.argtypes = ([C.c_int, C.c_int] + [C.c_void_p, C.c_long, C.c_long] * 3 + [C.c_int] * 4 + [C.c_void_p] * 3
                    + [C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p])
fill_fn = L.mused_debug_gemm_f64_batched_tail_fill
fill_fn.restype = C.c_int
fill_fn.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, C.c_void_p,
                    C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_int,
                    C.c_void_p]
rows_fn = L.mused_debug_gemm_gram_rows
rows_fn.restype = C.c_int
rows_fn.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_int, C.c_long, C.c_void_p, C.c_long, C.c_long] + [C.c_int] * 4 + [C.c_void_p]

torch.manual_seed(0)
A = torch.randn(batch, n2, d, dtype=torch.float64, device="cuda")
G = torch.empty(batch, n2, n2, dtype=torch.float64, device="cuda")
X = torch.randn(lanes, blocks * ell, d, dtype=torch.float32, device="cuda")          # the rows of a call, fp32 as the benchmark's
pend = X[:, :ell].to(torch.float64).contiguous()
zero = torch.zeros(d, dtype=torch.float64, device="cuda")
PP = torch.empty(blocks, lanes, ell, ell, dtype=torch.float64, device="cuda")
# kept rows as in the steady state of the benchmark stream: 116 .. 123 of them (244 .. 251 rows in use)
split = torch.zeros(batch * 4, dtype=torch.int32, device="cuda")
split[::4] = torch.randint(ell - 12, ell - 4, (batch,), dtype=torch.int32).cuda()
order = torch.randperm(batch)[:listed].tolist()
lst = torch.tensor([listed] + order + [0] * (batch - listed), dtype=torch.int32, device="cuda")


def chunk():
    _lib.check(rows_fn(ptr(X), _lib.F32, d, X.stride(0), lanes, ell * d, ptr(PP), ell, ell * ell, ell, d, blocks * lanes, 0, stream_ptr()))


def computed():
    _lib.check(tail_fn(1, 1, ptr(A), d, n2 * d, ptr(A), d, n2 * d, ptr(G), n2, n2 * n2, n2, n2, d, batch, ptr(lst), None, ptr(pend),
                       ell * d, per_lane, ptr(split), 4, ell, ptr(zero), 0, None, 0, 1, stream_ptr()))


def copied():
    _lib.check(fill_fn(ptr(A), d, n2 * d, ptr(G), n2, n2 * n2, n2, d, batch, ptr(lst), ptr(pend), ell * d, per_lane, ptr(split), 4,
                       ell, ptr(zero), 0, ptr(PP), ell * ell, ell, stream_ptr()))


def timed(run, reps=50):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        run()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3


chunk()
computed()
want = G.clone()
copied()
torch.cuda.synchronize()
print("bits equal:", bool(torch.equal(G.view(torch.int64)[order], want.view(torch.int64)[order])), flush=True)
for _ in range(10):
    computed(), copied(), chunk()
torch.cuda.synchronize()
tc, tf, tp = [], [], []
for _ in range(5):
    tc.append(timed(computed))
    tf.append(timed(copied))
    tp.append(timed(chunk, 10))
fmt = lambda t: " / ".join(f"{v:.1f}" for v in t)
print(f"Gram {listed} of {batch} x ({n2} x {d}), every tile computed: {fmt(tc)} us per launch (5 x 50 launches, alternating)")
print(f"the same with tiles of pending rows copied:              {fmt(tf)} us per launch; best {min(tf):.1f} / {min(tc):.1f} = "
      f"x{min(tf) / min(tc):.3f}")
print(f"P P^T of {blocks} blocks x {lanes} lanes ({ell} x {d}, fp32 rows):      {fmt(tp)} us per launch = "
      f"{min(tp) / blocks:.1f} us per block", flush=True)
