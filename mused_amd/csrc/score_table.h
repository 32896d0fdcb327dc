// The contingency table of two label arrays in one workgroup of SC_THREADS threads, shared by score.hip (the reference's
// seven numbers) and score_partitions.hip (the partition scores): (1) presence bits of both sides in LDS, label values
// -1 .. 65534 at offset 1; (2) ranks = per-word prefix counts plus a popcount below the bit, computed where needed; (3) the
// T x P counts, in LDS while T * P <= SC_LDS_CELLS, else in global memory (cleared by the caller), with integer atomics:
// equal cells of the 256 rows a wave holds are combined first.
#pragma once
#include "internal.h"

namespace mused {

constexpr int SC_THREADS = 1024;
constexpr int SC_WAVES = 16;
constexpr int SC_WORDS = 1024;         // 64-bit presence words per side: 65,536 label values
constexpr int SC_MAXC = 4096;          // largest T, P
constexpr int SC_LDS_CELLS = 24576;    // largest table kept in LDS (96 KiB)
constexpr int SC_OUT = 8, SC_INFO = 8; // doubles of out, ints of info per segment
constexpr int SC_FLAG_RANGE = 4, SC_FLAG_SIZE = 8;   // the label chains' flag values (match_labels.h)
constexpr int SC_SUMS = 9;

static_assert(SC_THREADS == SC_WORDS, "one thread per presence word in the rank pass");

struct ScoreLds {
  unsigned long long bm[2][SC_WORDS];   // presence of value v at bit v + 1: [0] true, [1] predicted
  int pre[2][SC_WORDS];                 // set bits in the words before this one
  int rs[SC_MAXC], cs[SC_MAXC];         // row and column sums
  int wtot[2][SC_WAVES];
  double red[SC_SUMS][SC_WAVES];
  unsigned long long iacc[2];           // sum |t - c|, agreeing rows
  int inter, pe, bad;
  int tab[SC_LDS_CELLS];
};
static_assert(sizeof(ScoreLds) <= 160 * 1024, "one workgroup's LDS");

// Four consecutive labels of both sides (rows 4 q .. 4 q + 3 of the segment); returns how many exist.
__device__ __forceinline__ int sc_load4(const int* __restrict__ tr, const int* __restrict__ pr, long q, long n, bool vec, int* a,
                                        int* b) {
  const long i = q << 2;
  if (i >= n) return 0;
  if (vec && i + 3 < n) {
    const int4 x = *reinterpret_cast<const int4*>(tr + i), y = *reinterpret_cast<const int4*>(pr + i);
    a[0] = x.x, a[1] = x.y, a[2] = x.z, a[3] = x.w;
    b[0] = y.x, b[1] = y.y, b[2] = y.z, b[3] = y.w;
    return 4;
  }
  const int c = (int)(n - i < 4 ? n - i : 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = j < c ? tr[i + j] : 0;
    b[j] = j < c ? pr[i + j] : 0;
  }
  return c;
}

__device__ __forceinline__ int sc_rank(const ScoreLds& s, int side, int v) {
  const unsigned x = (unsigned)v + 1u;
  return s.pre[side][x >> 6] + __popcll(s.bm[side][x >> 6] & ((1ull << (x & 63)) - 1ull));
}

template <bool LDS>
__device__ __forceinline__ void sc_add(ScoreLds& s, int* __restrict__ gtab, int cell, int v) {
  if (LDS) atomicAdd(&s.tab[cell], v);
  else atomicAdd(&gtab[cell], v);
}

template <bool LDS>
__device__ __forceinline__ int sc_cell(const ScoreLds& s, const int* gtab, int e) {
  return LDS ? s.tab[e] : __hip_atomic_load(&gtab[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Steps 1 and 2 for the workgroup's segment: clears the accumulators, sets the presence bits and the per-word prefix
// counts.  Returns T and P; s.bad tells a label outside [-1, 65534].  `pre` is complete after the caller's next barrier.
__device__ __forceinline__ void sc_presence_ranks(ScoreLds& s, const int* __restrict__ tr, const int* __restrict__ pr, long seg_len,
                                                  int vec, int& T, int& P) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  s.bm[0][t] = 0;
  s.bm[1][t] = 0;
  for (int i = t; i < SC_MAXC; i += SC_THREADS) s.rs[i] = s.cs[i] = 0;
  if (t == 0) {
    s.iacc[0] = s.iacc[1] = 0;
    s.inter = s.pe = s.bad = 0;
  }
  __syncthreads();
  // step 1: presence
  const long nq = (seg_len + 3) >> 2;
  for (long q = t; q < nq; q += SC_THREADS) {
    int a[4], b[4];
    const int cnt = sc_load4(tr, pr, q, seg_len, vec != 0, a, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // constant indices: a and b stay in registers
      if (j >= cnt) continue;
      const unsigned x = (unsigned)a[j] + 1u, y = (unsigned)b[j] + 1u;
      if (x >= 65536u || y >= 65536u) {
        s.bad = 1;
        continue;
      }
      const unsigned long long mx = 1ull << (x & 63), my = 1ull << (y & 63);
      if (!(s.bm[0][x >> 6] & mx)) atomicOr(&s.bm[0][x >> 6], mx);   // the plain read only spares repeated atomics
      if (!(s.bm[1][y >> 6] & my)) atomicOr(&s.bm[1][y >> 6], my);
    }
  }
  __syncthreads();
  // step 2: exclusive prefix counts of the words
  const unsigned long long wt = s.bm[0][t], wp = s.bm[1][t];
  const int ct = __popcll(wt), cp = __popcll(wp), cu = __popcll(wt & wp);
  int it = ct, ip = cp;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int vt = __shfl_up(it, o), vp = __shfl_up(ip, o);
    if (l >= o) {
      it += vt;
      ip += vp;
    }
  }
  if (l == 63) {
    s.wtot[0][w] = it;
    s.wtot[1][w] = ip;
  }
  if (cu) atomicAdd(&s.inter, cu);
  __syncthreads();
  int offt = 0, offp = 0;
  T = 0, P = 0;
  for (int h = 0; h < SC_WAVES; ++h) {
    if (h == w) {
      offt = T;
      offp = P;
    }
    T += s.wtot[0][h];
    P += s.wtot[1][h];
  }
  s.pre[0][t] = offt + it - ct;
  s.pre[1][t] = offp + ip - cp;
}

// Step 3.  A wave holds up to 256 rows per pass.  Twice, the cell of its first row still uncounted is taken, every row
// of the wave in that cell is counted by ballot and ONE add is issued; what is left after that adds itself.  (Binary
// labels at noise rate 0.95: 19 of 20 rows share a cell, and two rounds leave 1 row in 400.)
template <bool LDS>
__device__ __forceinline__ void sc_counts(ScoreLds& s, const int* __restrict__ tr, const int* __restrict__ pr, long n, bool vec,
                                          int P, int* __restrict__ gtab) {
  const int t = threadIdx.x, l = t & 63;
  const long nq = (n + 3) >> 2;
  unsigned long long dsum = 0, agree = 0;
  for (long base = 0; base < nq; base += SC_THREADS) {   // uniform trip count: the ballots below need every lane
    int a[4], b[4], c[4];
    bool act[4];
    const int cnt = sc_load4(tr, pr, base + t, n, vec, a, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      act[j] = j < cnt;
      c[j] = 0;
      if (act[j]) {
        c[j] = sc_rank(s, 0, a[j]) * P + sc_rank(s, 1, b[j]);
        const long d = (long)a[j] - (long)b[j];
        dsum += (unsigned long long)(d < 0 ? -d : d);
        agree += a[j] == b[j];
      }
    }
    for (int r = 0; r < 2; ++r) {
      const unsigned long long b0 = __ballot(act[0]), b1 = __ballot(act[1]), b2 = __ballot(act[2]), b3 = __ballot(act[3]);
      if (!(b0 | b1 | b2 | b3)) break;
      const int js = b0 ? 0 : b1 ? 1 : b2 ? 2 : 3;
      const unsigned long long bj = js == 0 ? b0 : js == 1 ? b1 : js == 2 ? b2 : b3;
      const int leader = __ffsll((long long)bj) - 1;
      const int lc = __shfl(js == 0 ? c[0] : js == 1 ? c[1] : js == 2 ? c[2] : c[3], leader);
      int total = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool hit = act[j] && c[j] == lc;
        total += __popcll(__ballot(hit));
        act[j] = act[j] && !hit;
      }
      if (l == leader) sc_add<LDS>(s, gtab, lc, total);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (act[j]) sc_add<LDS>(s, gtab, c[j], 1);
  }
  atomicAdd(&s.iacc[0], dsum);   // integers: exact in any order
  atomicAdd(&s.iacc[1], agree);
}

// Step 3 for an unflagged segment (T * P cells fit gtab): clears the table where it lives, counts, and returns whether that
// is LDS.  The table is complete for every thread on return.
__device__ __forceinline__ bool sc_build_table(ScoreLds& s, const int* __restrict__ tr, const int* __restrict__ pr, long seg_len,
                                               int vec, int T, int P, int* __restrict__ gtab) {
  const int t = threadIdx.x;
  // step 3: counts
  const int cells = T * P;
  const bool in_lds = cells <= SC_LDS_CELLS;
  if (in_lds) {
    for (int e = t; e < cells; e += SC_THREADS) s.tab[e] = 0;
  } else {
    for (int e = t; e < cells; e += SC_THREADS) gtab[e] = 0;
    __threadfence();
  }
  __syncthreads();   // also completes `pre`
  if (in_lds) sc_counts<true>(s, tr, pr, seg_len, vec != 0, P, gtab);
  else sc_counts<false>(s, tr, pr, seg_len, vec != 0, P, gtab);
  __threadfence();
  __syncthreads();
  return in_lds;
}

}  // namespace mused
