// The WIDE Hungarian label chain: matched_t = match_clusters(matched_{t-1}, raw_t, "hungarian", min_overlap)
// (matrix_operations.py:155-233) for ANY int32 label values (the noise label -1, INT32_MIN, INT32_MAX) and up to
// MW_MAXC = 4,096 distinct labels a side -- what DBSCAN_incr produces and csrc/match_hung.hip (a 1,024-entry histogram of
// label values, P, N <= 256 in LDS) hands to the host.  The specification is hungarian.match_labels; the assignment is
// SciPy's linear_sum_assignment as hungarian.lsap states it, in integers.  Enqueue-only: seven launches per window, no host
// read or wait; a control block in the workspace carries P, N, the flag word and the "chain has ended" mark between them.
//
// Per window (pv = the previous matched window, nw = the raw labels, W rows):
//   1. mw_clear_kernel    the two hash sets, the row / column marks, the control block's per-window words
//   2. mw_insert_kernel   every label into the hash set of its side.  A slot is 64 bits: (1 << 32) | the label's bits, so
//                         every int32 is a label and 0 means empty.  No buffer depends on the RANGE of the values.
//   3. mw_sort_kernel     one workgroup per side: the distinct values out of the set, bitonic sort in LDS on the order
//                         preserving key (label ^ 0x80000000) -> np.unique's ascending values, P and N.  More than 4,096 of
//                         them: flag 8 (the insert stops filling a set once its count passed 4,096, so its size is fixed).
//   4. mw_zero_kernel     the nr x nc overlap counts (dense, at most 4,096 x 4,096 int32 of workspace)
//   5. mw_count_kernel    rank of every row's two labels by binary search, one integer atomicAdd per row into the counts
//                         (order independent); the add that makes a count reach min_overlap marks its row and its column.
//                         The counts are stored the way the solver reads them: TRANSPOSED when P > N, so that a solver row
//                         is contiguous either way.  The rank of the new label is kept per row for step 7.
//   6. mw_solve_kernel    one workgroup of 256 threads: the feasibility test (every row and column keeps a count >=
//                         min_overlap, else the window passes through), the assignment, the map new rank -> previous value,
//                         the info words, the end-of-chain mark
//   7. mw_relabel_kernel  a matched new label takes the previous value of its row, any other keeps its own
//
// Step 6, the solver (lsap.h) on the workgroup: thread t owns positions t, t + 256, ... of `remaining` and reads the counts
// of its columns from the global cost row.  Four waves, one per SIMD, two barriers per step: a scan of 4,096 positions is 16
// per thread, and at the usual few hundred to a thousand labels 2-5, where one wave would walk 64 per lane (every one an LDS
// read and a dependent global load) and 16 waves would only make the barrier dearer.  The solver's key bound needs
// W <= MW_MAX_W, which the entry enforces.
//
// Step budget: the solver takes about 2 min(P, N) steps on ordinary label pairs and min(P, N)^2 at worst; one workgroup
// must not run for seconds, so a window whose solve would take more than max_steps steps (0: 32 min(P, N)) is flagged.
//
// Flags (info word 4); the chain ends at the first flagged window, which is not written, nor are the ones behind it:
//   8 P or N beyond 4,096 (the info word of that side then holds 4,097);  16 the feasibility test passed but no complete
//   assignment exists (SciPy raises ValueError there);  32 the step budget is spent.  There is no range flag.
#include "internal.h"
#include "lsap.h"

namespace mused {

constexpr int MW_MAXC = 4096;              // largest P, N
constexpr int MW_HT = 16384;               // slots of a hash set (a power of two, 4 x MW_MAXC)
constexpr int MW_HT_BITS = 14;
constexpr int MW_INFO = 8;                 // ints of info_out per window
constexpr int MW_THREADS = 256;            // of the grid kernels and of the solver
constexpr int MW_SORT_THREADS = 1024;
constexpr int MW_FLAG_SIZE = 8;            // beside LSAP_FLAG_ASSIGN and LSAP_FLAG_STEPS
constexpr int MW_MAX_W = 1 << 20;
constexpr unsigned long long MW_NOKEY = ~0ull;
constexpr unsigned long long MW_OCC = 1ull << 32;

static_assert(MW_HT == 1 << MW_HT_BITS && MW_HT >= 4 * MW_MAXC, "hash set size");

struct WideCtl {
  int stop;        // the chain has ended: every later kernel of the call returns at once
  int flags;       // of the current window
  int count[2];    // distinct values seen by the insert (may overshoot 4,096 by the threads in flight)
  int P, N;
  int feasible;
  int pad;
};

// the workspace: every array starts on a multiple of 256 bytes
struct WideWs {
  WideCtl* ctl;
  unsigned long long* ht;   // 2 x MW_HT
  int* val;                 // 2 x MW_MAXC sorted distinct values: prev, new
  int* ok;                  // 2 x MW_MAXC: a row (prev rank) / a column (new rank) keeps a count >= min_overlap
  int* map_has;             // MW_MAXC: new rank -> matched?
  int* map_val;             // MW_MAXC: new rank -> the previous value it takes
  int* rank_n;              // W
  int* ov;                  // min(W, MW_MAXC)^2 overlap counts, solver orientation
};

constexpr size_t MW_CTL_BYTES = 256;   // the control block's share of the workspace, cleared by one memset per call
static_assert(sizeof(WideCtl) <= MW_CTL_BYTES, "the control block is the first 256 bytes");

// Carves the workspace of a call at window length W, the control block first; a null `ws` only sizes (*bytes).
static WideWs mw_carve(void* ws, int W, size_t* bytes) {
  WsCarver c{static_cast<char*>(ws)};
  const size_t m = W < MW_MAXC ? W : MW_MAXC;
  WideWs w;
  w.ctl = c.take<WideCtl>(1);
  w.ht = c.take<unsigned long long>(2 * MW_HT);
  w.val = c.take<int>(2 * MW_MAXC);
  w.ok = c.take<int>(2 * MW_MAXC);
  w.map_has = c.take<int>(MW_MAXC);
  w.map_val = c.take<int>(MW_MAXC);
  w.rank_n = c.take<int>(W);
  w.ov = c.take<int>(m * m);
  *bytes = c.off;
  return w;
}

__device__ __forceinline__ int mw_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- window 0 without a previous one: match_clusters returns the new labels as they are -----------------------------------
__global__ __launch_bounds__(MW_THREADS) void mw_copy_kernel(const int* __restrict__ nw, int* __restrict__ out, int W,
                                                             int* __restrict__ inf) {
  const int i = blockIdx.x * MW_THREADS + threadIdx.x;
  if (i < W) out[i] = nw[i];
  if (i < MW_INFO) inf[i] = i == 6;
}

// ---- 1 ----
__global__ __launch_bounds__(MW_THREADS) void mw_clear_kernel(WideWs w) {
  if (mw_ld(&w.ctl->stop)) return;
  const int g = blockIdx.x * MW_THREADS + threadIdx.x;   // grid: 2 MW_HT threads
  if (g < 2 * MW_HT) w.ht[g] = 0ull;
  if (g < 2 * MW_MAXC) w.ok[g] = 0;
  if (g < MW_MAXC) w.map_has[g] = 0;
  if (g == 0) {
    w.ctl->flags = 0;
    w.ctl->count[0] = w.ctl->count[1] = 0;
    w.ctl->P = w.ctl->N = 0;
    w.ctl->feasible = 0;
  }
}

// ---- 2 ----
__device__ __forceinline__ void mw_insert(unsigned long long* __restrict__ ht, int* __restrict__ count, int label) {
  const unsigned long long key = MW_OCC | (unsigned)label;
  unsigned h = ((unsigned)label * 2654435761u) >> (32 - MW_HT_BITS);
  for (int probe = 0; probe < MW_HT; ++probe) {   // bounded: a full set ends the walk, and so does a count past the limit
    unsigned long long cur = __hip_atomic_load(&ht[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return;
    if (mw_ld(count) > MW_MAXC) return;           // flag 8 is certain: nothing more is needed of this set
    if (cur == 0ull) {
      cur = atomicCAS(&ht[h], 0ull, key);
      if (cur == 0ull) {
        atomicAdd(count, 1);
        return;
      }
      if (cur == key) return;
    }
    h = (h + 1) & (MW_HT - 1);
  }
}

__global__ __launch_bounds__(MW_THREADS) void mw_insert_kernel(WideWs w, const int* __restrict__ pv, const int* __restrict__ nw,
                                                               int W) {
  if (mw_ld(&w.ctl->stop)) return;
  const int i = blockIdx.x * MW_THREADS + threadIdx.x;
  if (i >= W) return;
  mw_insert(w.ht, &w.ctl->count[0], pv[i]);
  mw_insert(w.ht + MW_HT, &w.ctl->count[1], nw[i]);
}

// ---- 3 ----  blockIdx.x = side
__global__ __launch_bounds__(MW_SORT_THREADS) void mw_sort_kernel(WideWs w) {
  __shared__ unsigned long long keys[MW_MAXC];
  __shared__ int fill;
  if (mw_ld(&w.ctl->stop)) return;
  const int side = blockIdx.x, t = threadIdx.x;
  const int cnt = w.ctl->count[side];
  if (cnt > MW_MAXC) {
    if (t == 0) {
      atomicOr(&w.ctl->flags, MW_FLAG_SIZE);
      (side ? w.ctl->N : w.ctl->P) = MW_MAXC + 1;
    }
    return;
  }
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;
  if (t == 0) fill = 0;
  for (int e = t; e < n2; e += MW_SORT_THREADS) keys[e] = MW_NOKEY;   // padding sorts behind every label
  __syncthreads();
  const unsigned long long* ht = w.ht + (long)side * MW_HT;
  for (int e = t; e < MW_HT; e += MW_SORT_THREADS) {
    const unsigned long long s = ht[e];
    if (s) {
      const int at = atomicAdd(&fill, 1);
      if (at < MW_MAXC) keys[at] = (unsigned long long)((unsigned)s ^ 0x80000000u);   // at < cnt <= MW_MAXC always
    }
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = t; e < n2; e += MW_SORT_THREADS) {
        const int x = e ^ j;
        if (x > e) {
          const unsigned long long a = keys[e], b = keys[x];
          const bool up = (e & k) == 0;
          if ((a > b) == up) {
            keys[e] = b;
            keys[x] = a;
          }
        }
      }
      __syncthreads();
    }
  int* val = w.val + side * MW_MAXC;
  for (int e = t; e < cnt; e += MW_SORT_THREADS) val[e] = (int)((unsigned)keys[e] ^ 0x80000000u);
  if (t == 0) (side ? w.ctl->N : w.ctl->P) = cnt;
}

// ---- 4 ----
__global__ __launch_bounds__(MW_THREADS) void mw_zero_kernel(WideWs w) {
  if (mw_ld(&w.ctl->stop) || w.ctl->flags) return;
  const long cells = (long)w.ctl->P * w.ctl->N;   // <= min(W, 4096)^2: inside the workspace
  for (long e = (long)blockIdx.x * MW_THREADS + threadIdx.x; e < cells; e += (long)gridDim.x * MW_THREADS) w.ov[e] = 0;
}

// ---- 5 ----
__device__ __forceinline__ int mw_rank(const int* __restrict__ val, int n, int x) {   // x is present: the set held it
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (val[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(MW_THREADS) void mw_count_kernel(WideWs w, const int* __restrict__ pv, const int* __restrict__ nw,
                                                              int W, int min_overlap) {
  if (mw_ld(&w.ctl->stop) || w.ctl->flags) return;
  const int i = blockIdx.x * MW_THREADS + threadIdx.x;
  if (i >= W) return;
  const int P = w.ctl->P, N = w.ctl->N;
  const int rp = mw_rank(w.val, P, pv[i]), rn = mw_rank(w.val + MW_MAXC, N, nw[i]);   // in [0, P), [0, N)
  w.rank_n[i] = rn;
  const long cell = P > N ? (long)rn * P + rp : (long)rp * N + rn;
  const int before = atomicAdd(&w.ov[cell], 1);
  if (before + 1 == min_overlap) {   // exactly one add per cell crosses the rule
    w.ok[rp] = 1;
    w.ok[MW_MAXC + rn] = 1;
  }
}

// ---- 6 ----
struct WideLds {
  LsapLds<MW_THREADS, MW_MAXC> ls;
  int bad;
};

__global__ __launch_bounds__(MW_THREADS) void mw_solve_kernel(WideWs w, int min_overlap, long max_steps, int* __restrict__ inf,
                                                              int* __restrict__ asg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mw_lds[];
  WideLds& s = *reinterpret_cast<WideLds*>(mw_lds);
  if (mw_ld(&w.ctl->stop)) return;
  const int t = threadIdx.x;
  const int P = w.ctl->P, N = w.ctl->N;
  int flags = w.ctl->flags, feasible = 0, steps = 0;
  if (!flags) {
    if (t == 0) s.bad = 0;
    __syncthreads();
    if (min_overlap > 0) {   // otherwise every count, zero included, is a finite cost
      for (int e = t; e < P; e += MW_THREADS)
        if (!w.ok[e]) s.bad = 1;
      for (int e = t; e < N; e += MW_THREADS)
        if (!w.ok[MW_MAXC + e]) s.bad = 1;
    }
    __syncthreads();
    feasible = !s.bad;
    if (feasible) {
      const bool tr = P > N;   // SciPy works on the transpose when there are more rows than columns
      const int nr = tr ? N : P, nc = tr ? P : N;
      const int* __restrict__ ov = w.ov;   // solver row i is contiguous: mw_count_kernel stored the transpose when P > N
      flags = lsap_solve<MW_THREADS, MW_MAXC, lsap_log2(MW_MAX_W)>(
          s.ls, nr, nc, min_overlap, [=](int i, int j) { return ov[(long)i * nc + j]; }, max_steps > 0 ? max_steps : 32l * nr,
          &steps);
      if (!flags)
        for (int r = t; r < nr; r += MW_THREADS) {
          const int c = s.ls.col4row[r];
          const int row = tr ? c : r, col = tr ? r : c;   // of the P x N matrix
          w.map_has[col] = 1;
          w.map_val[col] = w.val[row];
          if (asg) asg[row] = col;
        }
    }
  }
  if (t == 0) {
    inf[0] = P;
    inf[1] = N;
    inf[2] = steps;
    inf[3] = feasible;
    inf[4] = flags;
    inf[5] = 0;
    inf[6] = flags ? 0 : 1;
    inf[7] = 0;
    w.ctl->feasible = feasible;
    w.ctl->flags = flags;
    if (flags) w.ctl->stop = 1;
  }
}

// ---- 7 ----
__global__ __launch_bounds__(MW_THREADS) void mw_relabel_kernel(WideWs w, const int* __restrict__ nw, int* __restrict__ out,
                                                                int W) {
  if (mw_ld(&w.ctl->stop)) return;   // a flagged window is not written
  const int i = blockIdx.x * MW_THREADS + threadIdx.x;
  if (i >= W) return;
  int q = nw[i];
  if (w.ctl->feasible) {
    const int rn = w.rank_n[i];
    if (w.map_has[rn]) q = w.map_val[rn];
  }
  out[i] = q;
}

}  // namespace mused

using namespace mused;

extern "C" {

long mused_match_hung_wide_ws_bytes(int W) {
  if (W < 1 || W > MW_MAX_W) return -1;
  size_t bytes;
  mw_carve(nullptr, W, &bytes);
  return (long)bytes;
}

int mused_match_hung_wide_chain(const int* raw, int K_windows, int W, const int* prev0, int min_overlap, long max_steps,
                                int* matched_out, int* info_out, int* assign_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(raw && matched_out && info_out && ws && K_windows > 0, "mused_match_hung_wide_chain: bad arguments");
  MUSED_REQUIRE(W >= 1 && W <= MW_MAX_W, "mused_match_hung_wide_chain: W must lie in [1, 2^20] (the solver's key bound)");
  MUSED_REQUIRE((long)K_windows * W < (1l << 31) && K_windows < (1 << 18) && max_steps >= 0,
                "mused_match_hung_wide_chain: K_windows * W must stay below 2^31, K_windows below 2^18, max_steps >= 0");
  size_t need;
  const WideWs w = mw_carve(ws, W, &need);
  MUSED_REQUIRE(ws_bytes >= (long)need && ((size_t)ws & 255) == 0,
                "mused_match_hung_wide_chain: workspace too small or not 256-byte aligned");
  static LdsOptIn opt;
  const hipError_t aerr = allow_dynamic_lds(opt, reinterpret_cast<const void*>(mw_solve_kernel), sizeof(WideLds));
  MUSED_CHECK_HIP(aerr);
  hipStream_t st = (hipStream_t)stream;
  MUSED_CHECK_HIP(hipMemsetAsync(w.ctl, 0, MW_CTL_BYTES, st));
  MUSED_CHECK_HIP(hipMemsetAsync(info_out, 0, sizeof(int) * (size_t)K_windows * MW_INFO, st));
  if (assign_out) MUSED_CHECK_HIP(hipMemsetAsync(assign_out, 0xff, sizeof(int) * (size_t)K_windows * MW_MAXC, st));
  const int gw = cdiv(W, MW_THREADS);
  const long m = W < MW_MAXC ? W : MW_MAXC;
  const int gz = (int)(cdiv(m * m, MW_THREADS) < 2048 ? cdiv(m * m, MW_THREADS) : 2048);
  for (int tw = 0; tw < K_windows; ++tw) {
    const int* nw = raw + (long)tw * W;
    const int* pv = tw == 0 ? prev0 : matched_out + (long)(tw - 1) * W;
    int* out = matched_out + (long)tw * W;
    int* inf = info_out + (long)tw * MW_INFO;
    int* asg = assign_out ? assign_out + (long)tw * MW_MAXC : nullptr;
    if (pv == nullptr) {
      hipLaunchKernelGGL(mw_copy_kernel, dim3(gw), dim3(MW_THREADS), 0, st, nw, out, W, inf);
      MUSED_LAUNCH_CHECK();
      continue;
    }
    hipLaunchKernelGGL(mw_clear_kernel, dim3(2 * MW_HT / MW_THREADS), dim3(MW_THREADS), 0, st, w);
    hipLaunchKernelGGL(mw_insert_kernel, dim3(gw), dim3(MW_THREADS), 0, st, w, pv, nw, W);
    hipLaunchKernelGGL(mw_sort_kernel, dim3(2), dim3(MW_SORT_THREADS), 0, st, w);
    hipLaunchKernelGGL(mw_zero_kernel, dim3(gz), dim3(MW_THREADS), 0, st, w);
    hipLaunchKernelGGL(mw_count_kernel, dim3(gw), dim3(MW_THREADS), 0, st, w, pv, nw, W, min_overlap);
    hipLaunchKernelGGL(mw_solve_kernel, dim3(1), dim3(MW_THREADS), sizeof(WideLds), st, w, min_overlap, max_steps, inf, asg);
    hipLaunchKernelGGL(mw_relabel_kernel, dim3(gw), dim3(MW_THREADS), 0, st, w, nw, out, W);
    MUSED_LAUNCH_CHECK();
  }
  return MUSED_OK;
}

}  // extern "C"
