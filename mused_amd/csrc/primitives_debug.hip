// Test entries for the primitives the kernel files share: scan.h, block_scan.h, radix_sort.h, radix_select.h, union_find.h
// and wave_ops.h.  Each entry does nothing but call a primitive the way its consumers do and store what every thread
// received, so tests/test_gpu_primitives_shared.py can compare the primitive itself with an exact statement of it
// (tests/primitives_cases.py).  Not declared in include/mused_hip.h: the tests set the argument types themselves.
//
// Enqueue-only on the given stream.  No kernel here waits for another workgroup, and every store is guarded by the size
// of its buffer, so a wrong position from a primitive under test stays inside it.
#include "internal.h"
#include "radix_select.h"
#include "radix_sort.h"
#include "union_find.h"
#include "wave_ops.h"

namespace mused {

constexpr int DBG_WAVE_THREADS = 256;  // four waves: xchg16 / xchg32 read threadIdx.x, not a lane number
constexpr int DBG_WAVE_F64_OPS = 10;
constexpr int DBG_SCAN_MAX_CALLS = 8;

// out[op * 256 + t], op = 0 .. 9: the five DPP moves, xchg16, xchg32 (of a = in[t]); swap16_add, swap32_add (of a and
// b = in[256 + t]); wave_allsum (of a).  iout / uout: wave_incl_scan of iin[t] / uin[t]
__global__ __launch_bounds__(DBG_WAVE_THREADS) void dbg_wave_ops_kernel(const double* __restrict__ in, const int* __restrict__ iin,
                                                                       const unsigned long long* __restrict__ uin,
                                                                       double* __restrict__ out, int* __restrict__ iout,
                                                                       unsigned long long* __restrict__ uout) {
  const int t = threadIdx.x;
  const double a = in[t], b = in[DBG_WAVE_THREADS + t];
  double r[DBG_WAVE_F64_OPS];
  r[0] = dpp_mov_f64<DPP_QUAD_XOR1>(a);
  r[1] = dpp_mov_f64<DPP_QUAD_XOR2>(a);
  r[2] = dpp_mov_f64<DPP_ROW_HALF_MIRROR>(a);
  r[3] = dpp_mov_f64<DPP_ROW_MIRROR>(a);
  r[4] = dpp_mov_f64<DPP_ROW_ROR8>(a);
  r[5] = xchg16(a);
  r[6] = xchg32(a);
  r[7] = swap16_add(a, b);
  r[8] = swap32_add(a, b);
  r[9] = wave_allsum(a);
#pragma unroll
  for (int op = 0; op < DBG_WAVE_F64_OPS; ++op) out[op * DBG_WAVE_THREADS + t] = r[op];
  iout[t] = wave_incl_scan(iin[t]);
  uout[t] = wave_incl_scan(uin[t]);
}

// `calls` scans back to back on consecutive slices of `in`, one scratch, no barrier between them but the primitive's own
template <typename T>
__global__ __launch_bounds__(1024) void dbg_block_scan_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                              T* __restrict__ totals, int calls) {
  __shared__ T ws[16];
  const int t = threadIdx.x, nt = blockDim.x;
  T x[DBG_SCAN_MAX_CALLS], tot[DBG_SCAN_MAX_CALLS];
#pragma unroll
  for (int c = 0; c < DBG_SCAN_MAX_CALLS; ++c)
    if (c < calls) x[c] = block_excl_scan(in[c * nt + t], ws, tot[c]);
#pragma unroll
  for (int c = 0; c < DBG_SCAN_MAX_CALLS; ++c)
    if (c < calls) {
      out[c * nt + t] = x[c];
      totals[c * nt + t] = tot[c];
    }
}

__global__ __launch_bounds__(256) void dbg_lower_bound_kernel(const int* __restrict__ a, const int* __restrict__ lo,
                                                              const int* __restrict__ hi, const int* __restrict__ queries, int nq,
                                                              int* __restrict__ out) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q < nq) out[q] = lower_bound(a, lo[q], hi[q], queries[q]);
}

// workgroup b selects the kks[b]-th smallest of the m keys (a kk outside [1, m] leaves its outputs alone).  MODE 0: the
// keys are given; 1: they are f64_key of m doubles.  kmin / kmax as in pass 0 of select_k_kernel (csrc/knn.hip)
template <int MODE>
__global__ __launch_bounds__(SELECT_THREADS) void dbg_select_kernel(const unsigned long long* __restrict__ keys, int m,
                                                                   const int* __restrict__ kks,
                                                                   unsigned long long* __restrict__ out_thr,
                                                                   int* __restrict__ out_need_eq, int* __restrict__ out_eq_count) {
  __shared__ SelectLds lds;
  const int tid = threadIdx.x, kk = kks[blockIdx.x];
  if (kk < 1 || kk > m) return;  // (uniform)
  const double* scores = reinterpret_cast<const double*>(keys);
  auto key_at = [&](int i) -> unsigned long long { return MODE ? f64_key(scores[i]) : keys[i]; };
  unsigned long long kmin = ~0ull, kmax = 0ull;
  for (int i = tid; i < m; i += SELECT_THREADS) {
    const unsigned long long key = key_at(i);
    kmin = key < kmin ? key : kmin;
    kmax = key > kmax ? key : kmax;
  }
  const SelectThreshold th = block_select_threshold(lds, m, kk, key_at, kmin, kmax);
  if (tid == 0) {
    out_thr[blockIdx.x] = th.thr;
    out_need_eq[blockIdx.x] = th.need_eq;
    out_eq_count[blockIdx.x] = th.eq_count;
  }
}

__global__ __launch_bounds__(256) void dbg_uf_init_kernel(int* __restrict__ parent, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = i;
}

// one thread an edge (an edge with an end outside [0, n) is left alone)
__global__ __launch_bounds__(256) void dbg_uf_unite_kernel(int* parent, int n, const int* __restrict__ ea,
                                                           const int* __restrict__ eb, int m, int* __restrict__ joined_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  const int a = ea[e], b = eb[e];
  if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n) return;
  bool joined;
  db_unite(parent, a, b, &joined);
  joined_out[e] = joined ? 1 : 0;
}

__global__ __launch_bounds__(256) void dbg_uf_root_kernel(int* parent, int n, int* __restrict__ root_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) root_out[i] = db_find(parent, i);
}

struct DbgSortWs {
  int *key[2], *val[2], *hist;
};

static size_t dbg_sort_layout(int cap, char* base, DbgSortWs* w) {
  WsCarver c{base};
  DbgSortWs l;
  for (int i = 0; i < 2; ++i) {
    l.key[i] = c.take<int>((size_t)cap);
    l.val[i] = c.take<int>((size_t)cap);
  }
  l.hist = c.take<int>(256 * (size_t)cdiv(cap, RADIX_TILE));
  if (w) *w = l;
  return c.off;
}

}  // namespace mused

using namespace mused;

extern "C" {

// in: 512 fp64 (a = in[0 .. 256), b = in[256 .. 512)), iin: 256 int32, uin: 256 uint64; out: 10 x 256 fp64 (the order of
// dbg_wave_ops_kernel), iout: 256 int32, uout: 256 uint64.  One workgroup of 256 threads
int mused_debug_wave_ops(const double* in, const int* iin, const unsigned long long* uin, double* out, int* iout,
                         unsigned long long* uout, void* stream) {
  MUSED_REQUIRE(in && iin && uin && out && iout && uout, "mused_debug_wave_ops: null argument");
  hipLaunchKernelGGL(dbg_wave_ops_kernel, dim3(1), dim3(DBG_WAVE_THREADS), 0, (hipStream_t)stream, in, iin, uin, out, iout, uout);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// One workgroup of `threads` calls block_excl_scan `calls` times; in, out, totals: calls x threads words of int32
// (dtype 0) or uint64 (dtype 1).  out: the exclusive sums, totals: the total every thread received
int mused_debug_block_scan(const void* in, void* out, void* totals, int threads, int dtype, int calls, void* stream) {
  MUSED_REQUIRE(in && out && totals, "mused_debug_block_scan: null argument");
  MUSED_REQUIRE(threads >= 64 && threads <= 1024 && threads % 64 == 0 && (dtype == 0 || dtype == 1) && calls >= 1 &&
                    calls <= DBG_SCAN_MAX_CALLS,
                "mused_debug_block_scan: threads=%d (a multiple of 64 up to 1024), dtype=%d (0, 1), calls=%d (1 .. %d)", threads,
                dtype, calls, DBG_SCAN_MAX_CALLS);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    hipLaunchKernelGGL(dbg_block_scan_kernel<int>, dim3(1), dim3(threads), 0, st, (const int*)in, (int*)out, (int*)totals, calls);
  else
    hipLaunchKernelGGL(dbg_block_scan_kernel<unsigned long long>, dim3(1), dim3(threads), 0, st, (const unsigned long long*)in,
                       (unsigned long long*)out, (unsigned long long*)totals, calls);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// blockscan_kernel as its consumers launch it; total: null, a word of its own, or a + m
int mused_debug_blockscan(int* a, int m, int* total, void* stream) {
  MUSED_REQUIRE(a && m >= 0, "mused_debug_blockscan: bad arguments (m=%d)", m);
  hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, (hipStream_t)stream, a, m, total);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// out[q] = lower_bound(a, lo[q], hi[q], queries[q]); the caller keeps 0 <= lo[q] <= hi[q] <= the length of a
int mused_debug_lower_bound(const int* a, const int* lo, const int* hi, const int* queries, int nq, int* out, void* stream) {
  MUSED_REQUIRE(a && lo && hi && queries && out && nq >= 1, "mused_debug_lower_bound: bad arguments (nq=%d)", nq);
  hipLaunchKernelGGL(dbg_lower_bound_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, (hipStream_t)stream, a, lo, hi, queries, nq, out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

long mused_debug_radix_sort_ws_bytes(int cap) { return cap >= 1 ? (long)dbg_sort_layout(cap, nullptr, nullptr) : -1; }

// The callers' loop (csrc/tokenise.hip, csrc/rows_find.hip): `passes` passes with shift 8 p, no values on the first one, the
// pairs ping-ponging through the workspace and the last pass writing key_out, val_out and, where gather_src is set,
// gather_out[p] = gather_src[value].  The live count is count_ptr's word when that is set, count_value otherwise
int mused_debug_radix_sort(const int* key, int cap, int count_value, const int* count_ptr, int passes, const int* gather_src,
                           int* key_out, int* val_out, int* gather_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(key && key_out && val_out && ws && (!gather_src == !gather_out), "mused_debug_radix_sort: null argument");
  MUSED_REQUIRE(cap >= 1 && passes >= 1 && passes <= 4 && (count_ptr || (count_value >= 0 && count_value <= cap)),
                "mused_debug_radix_sort: cap=%d (>= 1), passes=%d (1 .. 4), count=%d (0 .. cap)", cap, passes, count_value);
  MUSED_REQUIRE(ws_bytes >= (long)dbg_sort_layout(cap, nullptr, nullptr), "mused_debug_radix_sort: workspace too small");
  DbgSortWs w;
  dbg_sort_layout(cap, (char*)ws, &w);
  const RadixCount count{count_value, count_ptr};
  const int* kin = key;
  const int* vin = nullptr;
  for (int p = 0; p < passes; ++p) {
    const bool last = p == passes - 1;
    int* kout = last ? key_out : w.key[p & 1];
    int* vout = last ? val_out : w.val[p & 1];
    const int rc = radix_sort_pass(kin, vin, cap, count, 8 * p, w.hist, kout, vout, last ? gather_src : nullptr,
                                   last ? gather_out : nullptr, (hipStream_t)stream);
    if (rc) return rc;
    kin = kout;
    vin = vout;
  }
  return MUSED_OK;
}

// Workgroup b: block_select_threshold for the kks[b]-th smallest (1-based) of m keys -> out_thr[b], out_need_eq[b],
// out_eq_count[b].  mode 0: keys are m uint64; mode 1: m fp64 scores, the keys are f64_key of them.  kks: nk int32
int mused_debug_radix_select(const void* keys, int m, int mode, const int* kks, int nk, unsigned long long* out_thr,
                             int* out_need_eq, int* out_eq_count, void* stream) {
  MUSED_REQUIRE(keys && kks && out_thr && out_need_eq && out_eq_count, "mused_debug_radix_select: null argument");
  MUSED_REQUIRE(m >= 1 && nk >= 1 && nk <= 65535 && (mode == 0 || mode == 1),
                "mused_debug_radix_select: m=%d (>= 1), nk=%d (1 .. 65535), mode=%d (0, 1)", m, nk, mode);
  const unsigned long long* k = (const unsigned long long*)keys;
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0)
    hipLaunchKernelGGL(dbg_select_kernel<0>, dim3(nk), dim3(SELECT_THREADS), 0, st, k, m, kks, out_thr, out_need_eq, out_eq_count);
  else
    hipLaunchKernelGGL(dbg_select_kernel<1>, dim3(nk), dim3(SELECT_THREADS), 0, st, k, m, kks, out_thr, out_need_eq, out_eq_count);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// parent[i] <- i; then one thread per edge: joined_out[e] <- whether db_unite(parent, ea[e], eb[e]) hooked a root itself;
// then root_out[i] <- db_find(parent, i).  parent, root_out: n int32; ea, eb, joined_out: m int32
int mused_debug_unite(int* parent, int n, const int* ea, const int* eb, int m, int* joined_out, int* root_out, void* stream) {
  MUSED_REQUIRE(parent && ea && eb && joined_out && root_out && n >= 1 && m >= 1, "mused_debug_unite: bad arguments (n=%d m=%d)",
                n, m);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dbg_uf_init_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, parent, n);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(dbg_uf_unite_kernel, dim3(cdiv(m, 256)), dim3(256), 0, st, parent, n, ea, eb, m, joined_out);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(dbg_uf_root_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, parent, n, root_out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
