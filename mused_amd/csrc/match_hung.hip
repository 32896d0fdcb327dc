// The label chain of the Hungarian approaches (sSVDMC, sSVDMC_hung, SWFDMC, sSVDMC_mini) on the device:
// matched_t = match_clusters(matched_{t-1}, raw_t, "hungarian", min_overlap) (matrix_operations.py:155-185) for a whole run
// of windows in ONE launch of one workgroup, as the Sinkhorn chain of match.hip.  The assignment is SciPy's
// linear_sum_assignment restated step by step (the specification is mused_amd/hungarian.py, pinned to SciPy by the tests).
//
// Per window:
//   1. distinct sorted label values of prev / new, P and N of them            (match_labels.h, all 16 waves)
//   2. the P x N positional overlap counts                                     (match_labels.h, all 16 waves)
//   3. the min_overlap rule and the feasibility test; the counts go to LDS when P N <= HG_LDS_COST
//   4. the assignment: shortest augmenting paths, ONE wave, no workgroup barrier inside
//   5. new label of column col -> previous value of row row, relabel           (match_labels.h, all 16 waves)
//
// Step 4.  Everything is an integer: cost = -overlap, "inf" is the sentinel HG_INF, tested BEFORE anything is added to it
// (as inf behaves in IEEE arithmetic).  With integer costs SciPy's doubles hold the same integers exactly, so every
// comparison here is SciPy's.  The matrix is worked on transposed when P > N (nr <= nc).  One Dijkstra step scans the
// remaining columns: lane l owns positions l, l + 64, l + 128, l + 192 of `remaining` (LDS, SciPy's reversed initial order
// and its swap-removal, so a position means what it means in SciPy), updates sp / path of its columns and forms the key
//     ((sp + 2^52) << 9) | (assigned ? 256 + position : 255 - position)
// whose minimum over the wave is SciPy's choice: the lowest value; among equal values an unassigned column before an
// assigned one; among unassigned ones the LARGEST position, among assigned ones the SMALLEST.  One 64-bit min-reduction.
//
// The key fits.  Costs lie in [-W, 0] with W < 2^31; they are not shifted, so sp and minVal may be negative (SciPy's are).
// An unassigned column has v = 0, the row being inserted has u = 0 and matched edges are tight, so the duals telescope
// along an alternating path: the sp of a column when it is selected -- minVal of that step -- is the ORIGINAL cost of a
// path of at most 2 nr - 1 edges, |minVal| < 2^9 2^31 = 2^40.  Assigned rows keep cost - u_i - v_j >= 0, so minVal does not
// decrease over the steps of a row and the sp of every scanned column lies between the first and the last minVal.  The dual
// update therefore moves a u_i or v_j by less than 2^41 per row, |u|, |v| < 2^8 2^41 = 2^49 after all rows, and a finite
// sp = minVal + cost - u - v has |sp| < 2^40 + 2^31 + 2^50 < 2^52: 0 < sp + 2^52 < 2^53, the key stays below 2^62 and
// below the all-ones key of "no finite entry".
//
// Flags (info word 4), the chain ends at the first flagged window, which is not written:
//   MT_FLAG_RANGE 4 a label outside [0, 1024);  MT_FLAG_SIZE 8 P or N beyond 256;
//   HG_FLAG_ASSIGN 16 the feasibility test passed but no complete assignment exists (SciPy raises ValueError there)
#include "internal.h"
#include "match_labels.h"

namespace mused {

constexpr int HG_FLAG_ASSIGN = 16;
constexpr long long HG_INF = 0x7fffffffffffffffll;
constexpr unsigned long long HG_NOKEY = ~0ull;
constexpr long long HG_BIAS = 1ll << 52;
constexpr int HG_LDS_COST = 24 * 1024;   // overlap counts kept in LDS up to this many entries (150 x 150 fits)

struct HungLds {
  MatchTables tb;
  long long u[MT_MAXC], v[MT_MAXC], sp[MT_MAXC];
  int path[MT_MAXC], row4col[MT_MAXC], col4row[MT_MAXC], remaining[MT_MAXC];
  int SR[MT_MAXC], SC[MT_MAXC];
  int row_ok[MT_MAXC], col_ok[MT_MAXC], map_row[MT_MAXC];
  int infeasible, steps, solve_flags;
  int cost[HG_LDS_COST];
};

// the lanes of ONE wave exchange data through LDS: nothing to wait for in hardware (a wave's LDS operations complete in
// order), but the compiler must not move an access across the exchange
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long wave_allmin_u64(unsigned long long k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(k, o);
    k = other < k ? other : k;
  }
  return k;
}

// Step 4 on the calling wave (64 lanes, uniform control flow).  Solver row i, column j cost: -cnt[i * si + j * sj] when
// cnt >= min_overlap, else inf.  Leaves col4row[0 .. nr); returns 0 or HG_FLAG_ASSIGN, *steps_out = Dijkstra steps taken.
__device__ __forceinline__ int hung_solve(HungLds& s, int nr, int nc, int si, int sj, int min_overlap, const int* __restrict__ ov,
                                       bool in_lds, int* steps_out) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int p = l + 64 * c;
    s.u[p] = 0;
    s.v[p] = 0;
    s.col4row[p] = -1;
    s.row4col[p] = -1;
    s.path[p] = -1;
  }
  int steps = 0;
  for (int cur = 0; cur < nr; ++cur) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int p = l + 64 * c;
      s.remaining[p] = nc - 1 - p;   // the reversed order is SciPy's; positions >= nc are never read
      s.sp[p] = HG_INF;
      s.SR[p] = 0;
      s.SC[p] = 0;
    }
    wave_lds_sync();
    long long minVal = 0;
    int i = cur, nrem = nc, sink = -1;
    while (sink < 0) {
      ++steps;
      s.SR[i] = 1;
      const long long ui = s.u[i];
      unsigned long long key = HG_NOKEY;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int it = l + 64 * c;
        if (it < nrem) {
          const int j = s.remaining[it];
          const int e = i * si + j * sj;
          const int cnt = in_lds ? s.cost[e] : __hip_atomic_load(&ov[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          long long spj = s.sp[j];
          if (cnt >= min_overlap) {   // a finite cost: only then is anything added
            const long long r = minVal - (long long)cnt - ui - s.v[j];
            if (r < spj) {
              s.path[j] = i;
              s.sp[j] = r;
              spj = r;
            }
          }
          if (spj != HG_INF) {
            const unsigned tie = s.row4col[j] == -1 ? 255u - (unsigned)it : 256u + (unsigned)it;
            const unsigned long long k = ((unsigned long long)(spj + HG_BIAS) << 9) | tie;
            key = k < key ? k : key;
          }
        }
      }
      key = wave_allmin_u64(key);
      if (key == HG_NOKEY) {   // lowest == inf: no complete assignment
        *steps_out = steps;
        return HG_FLAG_ASSIGN;
      }
      minVal = (long long)(key >> 9) - HG_BIAS;
      const unsigned tie = (unsigned)key & 511u;
      const int index = tie & 256u ? (int)(tie & 255u) : 255 - (int)tie;
      wave_lds_sync();   // sp / path of this step are written before any lane goes on
      const int j = s.remaining[index];
      const int last = s.remaining[nrem - 1];
      const int owner = s.row4col[j];
      wave_lds_sync();   // every lane has read `remaining` before it changes
      --nrem;
      if (l == 0) {
        s.SC[j] = 1;
        s.remaining[index] = last;
      }
      wave_lds_sync();
      if (owner == -1) sink = j;
      else i = owner;
    }
    // dual updates, then the augmentation along `path` from the sink
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int p = l + 64 * c;
      if (p < nr) {
        if (p == cur) s.u[p] += minVal;
        else if (s.SR[p]) s.u[p] += minVal - s.sp[s.col4row[p]];
      }
      if (p < nc && s.SC[p]) s.v[p] -= minVal - s.sp[p];
    }
    wave_lds_sync();
    if (l == 0) {
      int j = sink;
      for (int n = 0; n < nr; ++n) {   // a path visits a row once: at most nr edges end at `cur`
        const int r = s.path[j];
        s.row4col[j] = r;
        const int t = s.col4row[r];
        s.col4row[r] = j;
        j = t;
        if (r == cur) break;
      }
    }
    wave_lds_sync();
  }
  *steps_out = steps;
  return 0;
}

__global__ __launch_bounds__(MT_THREADS) void match_hung_chain_kernel(const int* __restrict__ raw, int K_windows, int W,
                                                                      const int* __restrict__ prev0, int min_overlap,
                                                                      int* __restrict__ matched, int* __restrict__ info,
                                                                      int* __restrict__ assign_out, int* __restrict__ ov) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hg_lds[];
  HungLds& s = *reinterpret_cast<HungLds*>(hg_lds);
  const int t = threadIdx.x;
  int tw = 0;
  for (; tw < K_windows; ++tw) {
    const int* nw = raw + (long)tw * W;
    const int* pv = tw == 0 ? prev0 : matched + (long)(tw - 1) * W;
    int* out = matched + (long)tw * W;
    int* inf = info + tw * MT_INFO;
    int* asg = assign_out ? assign_out + (long)tw * MT_MAXC : nullptr;
    if (asg && t < MT_MAXC) asg[t] = -1;
    if (pv == nullptr) {   // no previous window: match_clusters returns the new labels as they are
      const int bad = mt_pass_through(s.tb, nw, out, W);
      if (t < MT_INFO) inf[t] = t == 6 ? !bad : (t == 4 && bad ? MT_FLAG_RANGE : 0);
      if (bad) break;
      continue;
    }
    if (t < MT_MAXC) {
      s.row_ok[t] = 0;
      s.col_ok[t] = 0;
      s.map_row[t] = -1;
    }
    if (t == 0) s.infeasible = s.steps = s.solve_flags = 0;
    int P, N;
    int flags = mt_label_tables(s.tb, pv, nw, W, &P, &N);
    int steps = 0, feasible = 0;
    if (!flags) {
      mt_overlap_counts(s.tb, pv, nw, W, P, N, ov);
      // step 3: every row and every column keeps a finite entry (matrix_operations.py:176-178)
      const bool in_lds = P * N <= HG_LDS_COST;
      for (int e = t; e < P * N; e += MT_THREADS) {
        const int cnt = __hip_atomic_load(&ov[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (in_lds) s.cost[e] = cnt;
        if (cnt >= min_overlap) {
          s.row_ok[e / N] = 1;
          s.col_ok[e % N] = 1;
        }
      }
      __syncthreads();
      if (t < MT_MAXC && ((t < P && !s.row_ok[t]) || (t < N && !s.col_ok[t]))) s.infeasible = 1;
      __syncthreads();
      feasible = !s.infeasible;
      if (feasible) {
        const bool tr = P > N;   // SciPy works on the transpose when there are more rows than columns
        const int nr = tr ? N : P;
        if (t < 64) {
          int st = 0;
          const int f = hung_solve(s, nr, tr ? P : N, tr ? 1 : N, tr ? N : 1, min_overlap, ov, in_lds, &st);
          if (t == 0) {
            s.steps = st;
            s.solve_flags = f;
          }
          if (!f) {
            for (int r = t; r < nr; r += 64) {
              const int c = s.col4row[r];
              const int row = tr ? c : r, col = tr ? r : c;   // of the P x N matrix
              s.map_row[col] = row;
              if (asg) asg[row] = col;
            }
          }
        }
        __syncthreads();   // the solving wave is done: map_row, steps and the flag are complete
        steps = s.steps;
        flags = s.solve_flags;
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
    }
    if (flags) break;   // uniform: the chain ends at the first flagged window
    mt_relabel(s.tb, nw, out, W, feasible ? s.map_row : nullptr);
  }
  // windows behind a flagged one were not run
  for (int e = t + (tw + 1) * MT_INFO; e < K_windows * MT_INFO; e += MT_THREADS) info[e] = 0;
  if (assign_out)
    for (long e = t + (long)(tw + 1) * MT_MAXC; e < (long)K_windows * MT_MAXC; e += MT_THREADS) assign_out[e] = -1;
}

}  // namespace mused

using namespace mused;

extern "C" {

long mused_match_hung_ws_bytes(void) { return 4l * MT_MAXC * MT_MAXC; }

int mused_match_hung_chain(const int* raw, int K_windows, int W, const int* prev0, int min_overlap, int* matched_out,
                           int* info_out, int* assign_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(raw && matched_out && info_out && ws && K_windows > 0 && W > 0, "mused_match_hung_chain: bad arguments");
  MUSED_REQUIRE((long)K_windows * W < (1l << 31) && K_windows < (1 << 24), "mused_match_hung_chain: K_windows * W must stay below 2^31");
  MUSED_REQUIRE(ws_bytes >= mused_match_hung_ws_bytes(), "mused_match_hung_chain: workspace too small");
  static LdsOptIn opt;
  const hipError_t aerr = allow_dynamic_lds(opt, reinterpret_cast<const void*>(match_hung_chain_kernel), sizeof(HungLds));
  MUSED_CHECK_HIP(aerr);
  hipLaunchKernelGGL(match_hung_chain_kernel, dim3(1), dim3(MT_THREADS), sizeof(HungLds), (hipStream_t)stream, raw, K_windows, W,
                     prev0, min_overlap, matched_out, info_out, assign_out, (int*)ws);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
