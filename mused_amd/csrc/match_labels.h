// The passes of a label-chain window that do not depend on how the assignment is found, shared by the Sinkhorn chain
// (match.hip) and the Hungarian chain (match_hung.hip): the distinct label values of prev / new and their ranks, the
// P x N positional overlap counts, the relabel, and the loop over the windows of a launch with its info words (mt_chain).
// One workgroup of MT_THREADS threads calls every function here from uniform control flow.
#pragma once
#include "internal.h"

namespace mused {

constexpr int MT_THREADS = 1024;
constexpr int MT_WAVES = 16;
constexpr int MT_LABELS = 1024;   // label values the histogram covers (the project's MAX_CLUSTERS)
constexpr int MT_MAXC = 256;      // largest P, N
constexpr int MT_INFO = 8;        // ints of info_out per window
constexpr int MT_FLAG_RANGE = 4, MT_FLAG_SIZE = 8;
constexpr int MT_LOG_MAX_W = 31;  // the entries admit K_windows * W < 2^31 rows

static_assert(MT_THREADS == MT_LABELS, "one thread per label value in the rank pass");

struct MatchTables {
  int rank_p[MT_LABELS], rank_n[MT_LABELS];  // presence flag, then rank among the present values or -1
  int val_p[MT_MAXC];                        // sorted distinct values of prev
  int wcnt[2][MT_WAVES];
  int bad;
};

// A window without a previous one: match_clusters returns the new labels as they are.  Returns whether a label lies
// outside [0, 1024) (the caller's device copy does not hold the true value then).
__device__ __forceinline__ int mt_pass_through(MatchTables& tb, const int* __restrict__ nw, int* __restrict__ out, int W) {
  const int t = threadIdx.x;
  if (t == 0) tb.bad = 0;
  __syncthreads();
  for (int i = t; i < W; i += MT_THREADS) {
    const int q = nw[i];
    if ((unsigned)q >= (unsigned)MT_LABELS) tb.bad = 1;
    out[i] = q;
  }
  __threadfence();
  __syncthreads();
  const int bad = tb.bad;
  __syncthreads();   // the next window clears the mark
  return bad;
}

// Step 1: the sorted distinct values np.unique returns, P of prev and N of new (rank_p / rank_n / val_p).  Returns the
// flag word (MT_FLAG_RANGE, MT_FLAG_SIZE).  The first barrier in here also covers what the caller cleared before the call.
__device__ __forceinline__ int mt_label_tables(MatchTables& tb, const int* __restrict__ pv, const int* __restrict__ nw, int W,
                                               int* P_out, int* N_out) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const unsigned long long below = (1ull << l) - 1ull;
  tb.rank_p[t] = 0;
  tb.rank_n[t] = 0;
  if (t == 0) tb.bad = 0;
  __syncthreads();
  for (int i = t; i < W; i += MT_THREADS) {
    const int p = pv[i], q = nw[i];
    if ((unsigned)p >= (unsigned)MT_LABELS || (unsigned)q >= (unsigned)MT_LABELS) tb.bad = 1;
    else {
      tb.rank_p[p] = 1;
      tb.rank_n[q] = 1;
    }
  }
  __syncthreads();
  const bool fp = tb.rank_p[t] != 0, fn = tb.rank_n[t] != 0;
  const unsigned long long bp = __ballot(fp), bn = __ballot(fn);
  if (l == 0) {
    tb.wcnt[0][w] = __popcll(bp);
    tb.wcnt[1][w] = __popcll(bn);
  }
  __syncthreads();
  int P = 0, N = 0, offp = 0, offn = 0;
  for (int h = 0; h < MT_WAVES; ++h) {
    if (h == w) {
      offp = P;
      offn = N;
    }
    P += tb.wcnt[0][h];
    N += tb.wcnt[1][h];
  }
  const int rp = offp + __popcll(bp & below), rn = offn + __popcll(bn & below);
  tb.rank_p[t] = fp ? rp : -1;
  tb.rank_n[t] = fn ? rn : -1;
  if (fp && rp < MT_MAXC) tb.val_p[rp] = t;
  *P_out = P;
  *N_out = N;
  int flags = tb.bad ? MT_FLAG_RANGE : 0;
  if (P > MT_MAXC || N > MT_MAXC) flags |= MT_FLAG_SIZE;
  return flags;
}

// Step 2: ov[i * N + j] = rows whose prev label has rank i and whose new label has rank j (integer atomics on the
// workspace: order independent).  Complete and visible to the workgroup on return.
__device__ __forceinline__ void mt_overlap_counts(const MatchTables& tb, const int* __restrict__ pv, const int* __restrict__ nw,
                                                  int W, int P, int N, int* __restrict__ ov) {
  const int t = threadIdx.x;
  for (int e = t; e < P * N; e += MT_THREADS) ov[e] = 0;
  __threadfence();
  __syncthreads();
  for (int i = t; i < W; i += MT_THREADS) atomicAdd(&ov[tb.rank_p[pv[i]] * N + tb.rank_n[nw[i]]], 1);
  __threadfence();
  __syncthreads();
}

// Step 5: a new label whose column j has map_row[j] >= 0 takes the previous value of that row, any other keeps its own;
// map_row == nullptr (infeasible costs) passes the window through.  The caller's barrier has completed map_row.
__device__ __forceinline__ void mt_relabel(const MatchTables& tb, const int* __restrict__ nw, int* __restrict__ out, int W,
                                           const int* map_row) {
  for (int i = threadIdx.x; i < W; i += MT_THREADS) {
    const int q = nw[i];
    const int m = map_row ? map_row[tb.rank_n[q]] : -1;
    out[i] = m >= 0 ? tb.val_p[m] : q;
  }
  __threadfence();
  __syncthreads();   // the next window reads `out` and reuses the LDS tables
}

// ---- the chain: one workgroup walks the windows of a launch ----------------------------------------------------------------
// What both chain kernels keep in LDS besides their solver's state.
struct ChainLds {
  MatchTables tb;
  int row_ok[MT_MAXC], col_ok[MT_MAXC];   // step 3: the row / the column keeps a finite entry
  int map_row[MT_MAXC];                   // the solver's result: column j takes the previous value of row map_row[j], or -1
  int infeasible;
  int word[2];                            // the solver's own: zero when it is called
};

// Step 3's test, every row and every column keeps a finite entry (matrix_operations.py:176-178), on the marks the caller
// has written to row_ok / col_ok.
__device__ __forceinline__ bool mt_feasible(ChainLds& s, int P, int N) {
  const int t = threadIdx.x;
  __syncthreads();
  if (t < MT_MAXC && ((t < P && !s.row_ok[t]) || (t < N && !s.col_ok[t]))) s.infeasible = 1;
  __syncthreads();
  return !s.infeasible;
}

// What a solver reports of one window: info words 2 (its iteration or step count), 3, 4 and 5.
struct ChainSolved {
  int count, feasible, flags, word5;
};

// The chain matched_t = match(matched_{t-1}, raw_t), t = 0 .. K_windows - 1, and its contract with the host (_match_chain in
// matrix_operations.py reads words 3, 4 and 6; the wide chain of match_wide.hip writes the same eight words):
//   info[t] = { P, N, the solver's count, feasible, flags, the solver's word, done = !flags, 0 }
// A window without a previous one passes through.  The chain ends at the first flagged window, which is not written; the
// info of the windows behind it is zero.  solve(tw, P, N) is called by every thread once the label tables and the overlap
// counts ov[i * N + j] of window tw stand, with row_ok / col_ok / word zero and map_row -1; it returns a ChainSolved,
// uniform over the workgroup, and -- when that is feasible and unflagged -- map_row filled, behind a workgroup barrier.
template <typename Solve>
__device__ __forceinline__ void mt_chain(ChainLds& s, const int* __restrict__ raw, int K_windows, int W,
                                         const int* __restrict__ prev0, int* __restrict__ matched, int* __restrict__ info,
                                         int* __restrict__ ov, Solve solve) {
  const int t = threadIdx.x;
  int tw = 0;
  for (; tw < K_windows; ++tw) {
    const int* nw = raw + (long)tw * W;
    const int* pv = tw == 0 ? prev0 : matched + (long)(tw - 1) * W;
    int* out = matched + (long)tw * W;
    int* inf = info + tw * MT_INFO;
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
    if (t == 0) s.infeasible = s.word[0] = s.word[1] = 0;
    int P, N;
    ChainSolved r = {0, 0, mt_label_tables(s.tb, pv, nw, W, &P, &N), 0};
    if (!r.flags) {
      mt_overlap_counts(s.tb, pv, nw, W, P, N, ov);
      r = solve(tw, P, N);
    }
    if (t == 0) {
      inf[0] = P;
      inf[1] = N;
      inf[2] = r.count;
      inf[3] = r.feasible;
      inf[4] = r.flags;
      inf[5] = r.word5;
      inf[6] = r.flags ? 0 : 1;
      inf[7] = 0;
    }
    if (r.flags) break;   // uniform
    mt_relabel(s.tb, nw, out, W, r.feasible ? s.map_row : nullptr);
  }
  for (int e = t + (tw + 1) * MT_INFO; e < K_windows * MT_INFO; e += MT_THREADS) info[e] = 0;
}

}  // namespace mused
