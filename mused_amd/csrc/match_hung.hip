// The label chain of the Hungarian approaches (sSVDMC, sSVDMC_hung, SWFDMC, sSVDMC_mini) on the device:
// matched_t = match_clusters(matched_{t-1}, raw_t, "hungarian", min_overlap) (matrix_operations.py:155-185) for a whole run
// of windows in ONE launch of one workgroup, as the Sinkhorn chain of match.hip.  The assignment is SciPy's
// linear_sum_assignment restated step by step (the specification is mused_amd/hungarian.py, pinned to SciPy by the tests).
//
// Per window:
//   1. distinct sorted label values of prev / new, P and N of them            (match_labels.h, all 16 waves)
//   2. the P x N positional overlap counts                                     (match_labels.h, all 16 waves)
//   3. the min_overlap rule and the feasibility test; the counts go to LDS when P N <= HG_LDS_COST
//   4. the assignment: shortest augmenting paths, ONE wave, no workgroup barrier inside (lsap.h: the other 15 waves wait
//      at the barrier behind it); the matrix is worked on transposed when P > N
//   5. new label of column col -> previous value of row row, relabel           (match_labels.h, all 16 waves)
//
// Flags (info word 4), the chain ends at the first flagged window, which is not written:
//   MT_FLAG_RANGE 4 a label outside [0, 1024);  MT_FLAG_SIZE 8 P or N beyond 256;
//   LSAP_FLAG_ASSIGN 16 the feasibility test passed but no complete assignment exists (SciPy raises ValueError there)
#include "internal.h"
#include "lsap.h"
#include "match_labels.h"

namespace mused {

constexpr int HG_LDS_COST = 24 * 1024;   // overlap counts kept in LDS up to this many entries (150 x 150 fits)
constexpr long HG_NO_BUDGET = 0x7fffffffffffffffl;   // a solve takes at most nr nc steps: never reached

constexpr int HG_STEPS = 0, HG_FLAGS = 1;   // what the solving wave leaves in the chain's two words

struct HungLds {
  ChainLds ch;
  LsapLds<64, MT_MAXC> ls;
  int cost[HG_LDS_COST];
};

__global__ __launch_bounds__(MT_THREADS) void match_hung_chain_kernel(const int* __restrict__ raw, int K_windows, int W,
                                                                      const int* __restrict__ prev0, int min_overlap,
                                                                      int* __restrict__ matched, int* __restrict__ info,
                                                                      int* __restrict__ assign_out, int* __restrict__ ov) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hg_lds[];
  HungLds& s = *reinterpret_cast<HungLds*>(hg_lds);
  const int t = threadIdx.x;
  // assign_out: -1 for every row of every window, here and once.  That covers the windows that pass through, the flagged
  // one and the ones behind it.  The solving wave stores the columns of a solved window later in program order and behind
  // workgroup barriers (the label passes of mt_chain have at least five before the solve), each of which waits for the
  // stores of every wave of the workgroup, so a column is never overwritten by this clear.
  if (assign_out)
    for (long e = t; e < (long)K_windows * MT_MAXC; e += MT_THREADS) assign_out[e] = -1;
  mt_chain(s.ch, raw, K_windows, W, prev0, matched, info, ov, [&](int tw, int P, int N) {
    // step 3: every row and every column keeps a finite entry
    const bool in_lds = P * N <= HG_LDS_COST;
    for (int e = t; e < P * N; e += MT_THREADS) {
      const int cnt = __hip_atomic_load(&ov[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (in_lds) s.cost[e] = cnt;
      if (cnt >= min_overlap) {
        s.ch.row_ok[e / N] = 1;
        s.ch.col_ok[e % N] = 1;
      }
    }
    if (!mt_feasible(s.ch, P, N)) return ChainSolved{0, 0, 0, 0};
    const bool tr = P > N;   // SciPy works on the transpose when there are more rows than columns
    const int nr = tr ? N : P, nc = tr ? P : N, si = tr ? 1 : N, sj = tr ? N : 1;
    if (t < 64) {
      int st = 0;
      const int f = lsap_solve<64, MT_MAXC, MT_LOG_MAX_W>(s.ls, nr, nc, min_overlap, [&](int i, int j) {
        const int e = i * si + j * sj;
        return in_lds ? s.cost[e] : __hip_atomic_load(&ov[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }, HG_NO_BUDGET, &st);
      if (t == 0) {
        s.ch.word[HG_STEPS] = st;
        s.ch.word[HG_FLAGS] = f;
      }
      if (!f) {
        int* asg = assign_out ? assign_out + (long)tw * MT_MAXC : nullptr;
        for (int r = t; r < nr; r += 64) {
          const int c = s.ls.col4row[r];
          const int row = tr ? c : r, col = tr ? r : c;   // of the P x N matrix
          s.ch.map_row[col] = row;
          if (asg) asg[row] = col;
        }
      }
    }
    __syncthreads();   // the solving wave is done: map_row, steps and the flag are complete
    return ChainSolved{s.ch.word[HG_STEPS], 1, s.ch.word[HG_FLAGS], 0};
  });
}

}  // namespace mused

using namespace mused;

extern "C" {

long mused_match_hung_ws_bytes(void) { return 4l * MT_MAXC * MT_MAXC; }

int mused_match_hung_chain(const int* raw, int K_windows, int W, const int* prev0, int min_overlap, int* matched_out,
                           int* info_out, int* assign_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(raw && matched_out && info_out && ws && K_windows > 0 && W > 0, "mused_match_hung_chain: bad arguments");
  MUSED_REQUIRE((long)K_windows * W < (1l << MT_LOG_MAX_W) && K_windows < (1 << 24),
                "mused_match_hung_chain: K_windows * W must stay below 2^31");
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
