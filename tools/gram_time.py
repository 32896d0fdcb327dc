"""Times the Gram product of an FD rotation alone (symmetric batched launch of csrc/gemm_f64.h with a list), HIP events on a
quiet GPU: python tools/gram_time.py [batch listed n2 d]      (default: the benchmark's 7-lane group, 196 115 256 1024)
MUSED_GEMM_SYM_DIAG=0 python tools/gram_time.py               the diagonal tiles by the ordinary main loop"""
import ctypes as C, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mused_amd import _lib
from mused_amd.engine import ptr, stream_ptr

batch, listed, n2, d = [int(a) for a in sys.argv[1:5]] if len(sys.argv) >= 5 else (196, 115, 256, 1024)
fn = _lib.lib().mused_debug_gemm_f64_batched_active
fn.restype = C.c_int
fn.argtypes = [C.c_int, C.c_int] + [C.c_void_p, C.c_long, C.c_long] * 3 + [C.c_int] * 4 + [C.c_double] + [C.c_void_p] * 3
torch.manual_seed(0)
A = torch.randn(batch, n2, d, dtype=torch.float64, device="cuda")
G = torch.empty(batch, n2, n2, dtype=torch.float64, device="cuda")
order = torch.randperm(batch)[:listed].tolist()
lst = torch.tensor([listed] + order + [0] * (batch - listed), dtype=torch.int32, device="cuda")
run = lambda: _lib.check(fn(1, 1, ptr(A), d, n2 * d, ptr(A), d, n2 * d, ptr(G), n2, n2 * n2, n2, n2, d, batch, 1.0, ptr(lst),
                            None, stream_ptr()))
for _ in range(20):
    run()
torch.cuda.synchronize()
times = []
for _ in range(5):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(50):
        run()
    t1.record()
    torch.cuda.synchronize()
    times.append(t0.elapsed_time(t1) / 50 * 1e3)
flop = 2.0 * listed * n2 * n2 * d
print(f"Gram {listed} of {batch} x ({n2} x {d}): " + " / ".join(f"{t:.1f}" for t in times) + f" us per launch (5 x 50 launches); "
      f"best {min(times):.1f} us = {flop / min(times) / 1e6:.1f} TFLOP/s of the full product", flush=True)
