// The passes of a label-chain window that do not depend on how the assignment is found, shared by the Sinkhorn chain
// (match.hip) and the Hungarian chain (match_hung.hip): the distinct label values of prev / new and their ranks, the
// P x N positional overlap counts, and the relabel.  One workgroup of MT_THREADS threads calls every function here
// from uniform control flow.
#pragma once
#include "internal.h"

namespace mused {

constexpr int MT_THREADS = 1024;
constexpr int MT_WAVES = 16;
constexpr int MT_LABELS = 1024;   // label values the histogram covers (the project's MAX_CLUSTERS)
constexpr int MT_MAXC = 256;      // largest P, N
constexpr int MT_INFO = 8;        // ints of info_out per window
constexpr int MT_FLAG_RANGE = 4, MT_FLAG_SIZE = 8;

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

}  // namespace mused
