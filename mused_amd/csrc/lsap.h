// SciPy's linear_sum_assignment (shortest augmenting paths) on integer overlap counts, for the Hungarian label chains: one
// wave inside the chain kernel of match_hung.hip, one workgroup of 256 threads in match_wide.hip.  The specification is
// hungarian.lsap, pinned to SciPy by the tests.
//
// Solver row i, column j costs -count(i, j) when count(i, j) >= min_overlap, else inf; nr <= nc (the callers hand over the
// transpose when P > N, as SciPy does).  Everything is an integer: "inf" is the sentinel LSAP_INF, tested BEFORE anything
// is added to it (as inf behaves in IEEE arithmetic), and with integer costs SciPy's doubles hold the same integers exactly,
// so every comparison here is SciPy's.  Costs are not shifted: sp and minVal may be negative, as SciPy's are.
//
// `remaining` keeps SciPy's reversed initial order and its swap-removal, so a position means what it means in SciPy.  The
// removed column is parked behind position nrem, which SciPy never reads again: positions [nrem, nc) are exactly the
// scanned columns SC and their owners the scanned rows SR, so neither set needs an array.  One Dijkstra step: thread t owns
// positions t, t + THREADS, ... of `remaining`, updates sp / path of its columns and forms one 64-bit key
//     ((sp + 2^BIAS_BITS) << TIE_BITS) | (assigned ? CAP + position : CAP - 1 - position)
// whose minimum over the threads is SciPy's choice: the lowest value; among equal values an unassigned column before an
// assigned one; among unassigned ones the LARGEST position, among assigned ones the SMALLEST.
//
// The key fits.  Let CAP = 2^c and let the caller admit windows of at most 2^w rows, so that costs lie in [-2^w, 0].  An
// unassigned column has v = 0, the row being inserted has u = 0 and matched edges are tight, so the duals telescope along an
// alternating path: the sp of a column when it is selected -- minVal of that step -- is the ORIGINAL cost of a path of at
// most 2 nr - 1 < 2^(c+1) edges, |minVal| < 2^(w+c+1).  Assigned rows keep cost - u_i - v_j >= 0, so minVal does not
// decrease over the steps of a row and the sp of every scanned column lies between the first and the last minVal.  The dual
// update therefore moves a u_i or v_j by less than 2^(w+c+2) per row, |u|, |v| < 2^(w+2c+2) after all 2^c rows, and a finite
// sp = minVal + cost - u - v has |sp| < 2^(w+c+1) + 2^w + 2^(w+2c+3) < 2^(w+2c+4) = 2^BIAS_BITS.  So 0 < sp + 2^BIAS_BITS <
// 2^(w+2c+5), and with the c + 1 tie bits the key stays below 2^(w+3c+6): 61 bits for (w, c) = (31, 8), 62 for (20, 12),
// below 2^63 and below the all-ones key of "no finite entry".  The static_asserts of lsap_solve hold an instantiation to it.
#pragma once
#include "internal.h"
#include "wave_ops.h"

namespace mused {

constexpr int LSAP_FLAG_ASSIGN = 16;   // the lowest key is inf: no complete assignment (SciPy raises ValueError there)
constexpr int LSAP_FLAG_STEPS = 32;    // the step budget is spent
constexpr long long LSAP_INF = 0x7fffffffffffffffll;
constexpr unsigned long long LSAP_NOKEY = ~0ull;
constexpr unsigned LSAP_NONE = 0xffffu;   // "no row / no column" in the uint16 tables

constexpr int lsap_log2(long x) { return x <= 1 ? 0 : 1 + lsap_log2(x >> 1); }

template <int THREADS, int CAP>
struct LsapLds {
  long long u[CAP], v[CAP], sp[CAP];
  unsigned short remaining[CAP], path[CAP], row4col[CAP], col4row[CAP];
  unsigned long long wmin[THREADS / 64];   // the exchange between the waves of a workgroup: each wave's minimum,
  int sel_j, sel_owner;                    // the selected column and its owner
};

// The threads of the solver meet.  ONE wave exchanges data through LDS without a workgroup barrier -- the other waves of its
// workgroup may be waiting at one behind the solver: nothing to wait for in hardware (a wave's LDS operations complete in
// order), but the compiler must not move an access across the exchange.
template <int THREADS>
__device__ __forceinline__ void lsap_sync() {
  if constexpr (THREADS == 64) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// Run by THREADS threads (threadIdx.x in [0, THREADS): one wave, or the whole workgroup) from uniform control flow.
// CAP: the largest nc.  LOG_W: log2 of the largest window the caller admits.  Leaves s.col4row[0 .. nr); returns 0,
// LSAP_FLAG_ASSIGN or -- before step max_steps + 1 -- LSAP_FLAG_STEPS; *steps_out = Dijkstra steps taken.
template <int THREADS, int CAP, int LOG_W, typename Count>
__device__ __forceinline__ int lsap_solve(LsapLds<THREADS, CAP>& s, int nr, int nc, int min_overlap, Count count, long max_steps,
                                          int* steps_out) {
  constexpr int LOG_C = lsap_log2(CAP), TIE_BITS = LOG_C + 1, BIAS_BITS = LOG_W + 2 * LOG_C + 4;
  constexpr long long BIAS = 1ll << BIAS_BITS;
  static_assert(THREADS % 64 == 0 && CAP == 1 << LOG_C && CAP % THREADS == 0, "whole waves, a power-of-two capacity");
  static_assert(CAP < (int)LSAP_NONE, "uint16 tables");
  static_assert((BIAS_BITS + 1) + TIE_BITS < 63, "|sp| < 2^(w + 2c + 4): the key must stay below 2^63");
  const int t = threadIdx.x;
  for (int p = t; p < nc; p += THREADS) {
    s.u[p] = 0;
    s.v[p] = 0;
    s.col4row[p] = LSAP_NONE;
    s.row4col[p] = LSAP_NONE;
    s.path[p] = LSAP_NONE;
  }
  long steps = 0;
  for (int cur = 0; cur < nr; ++cur) {
    for (int p = t; p < nc; p += THREADS) {
      s.remaining[p] = (unsigned short)(nc - 1 - p);   // the reversed order is SciPy's
      s.sp[p] = LSAP_INF;
    }
    lsap_sync<THREADS>();
    long long minVal = 0;
    int i = cur, nrem = nc, sink = -1;
    while (sink < 0) {
      if (steps >= max_steps) {
        *steps_out = (int)steps;
        return LSAP_FLAG_STEPS;
      }
      ++steps;
      const long long ui = s.u[i];
      unsigned long long key = LSAP_NOKEY;
      for (int it = t; it < nrem; it += THREADS) {
        const int j = s.remaining[it];
        const int cnt = count(i, j);
        long long spj = s.sp[j];
        if (cnt >= min_overlap) {   // a finite cost: only then is anything added
          const long long r = minVal - (long long)cnt - ui - s.v[j];
          if (r < spj) {
            s.path[j] = (unsigned short)i;
            s.sp[j] = r;
            spj = r;
          }
        }
        if (spj != LSAP_INF) {
          const unsigned tie = s.row4col[j] == LSAP_NONE ? (unsigned)(CAP - 1 - it) : (unsigned)(CAP + it);
          const unsigned long long k = ((unsigned long long)(spj + BIAS) << TIE_BITS) | tie;
          key = k < key ? k : key;
        }
      }
      key = wave_allmin_u64(key);
      if constexpr (THREADS > 64) {
        if ((t & 63) == 0) s.wmin[t >> 6] = key;
        __syncthreads();
#pragma unroll
        for (int wv = 0; wv < THREADS / 64; ++wv) key = s.wmin[wv] < key ? s.wmin[wv] : key;
      } else {
        lsap_sync<THREADS>();   // sp / path of this step are written, `remaining` is read, before any lane goes on
      }
      if (key == LSAP_NOKEY) {   // lowest == inf: no complete assignment
        *steps_out = (int)steps;
        return LSAP_FLAG_ASSIGN;
      }
      minVal = (long long)(key >> TIE_BITS) - BIAS;
      const int tie = (int)(key & (unsigned long long)(2 * CAP - 1));
      const int index = tie >= CAP ? tie - CAP : CAP - 1 - tie;
      --nrem;
      // the chosen column j is parked behind nrem; every thread learns j and its owner
      int j, owner;
      if constexpr (THREADS > 64) {   // from the thread that owns the chosen position
        if ((index & (THREADS - 1)) == t) {
          const int jj = s.remaining[index];
          s.remaining[index] = s.remaining[nrem];
          s.remaining[nrem] = (unsigned short)jj;
          s.sel_j = jj;
          s.sel_owner = s.row4col[jj];
        }
        __syncthreads();
        j = s.sel_j;
        owner = s.sel_owner;
      } else {   // one wave: every lane reads them itself, which spares the write-read round trip through LDS
        j = s.remaining[index];
        owner = s.row4col[j];
        const int last = s.remaining[nrem];
        lsap_sync<THREADS>();   // every lane has read `remaining` before it changes
        if (t == 0) {
          s.remaining[index] = (unsigned short)last;
          s.remaining[nrem] = (unsigned short)j;
        }
        lsap_sync<THREADS>();
      }
      if (owner == (int)LSAP_NONE) sink = j;
      else i = owner;
    }
    // dual updates over the scanned columns remaining[nrem .. nc) and their owners (the scanned rows other than cur:
    // col4row[row] == j), then the augmentation from the sink.  The sink has sp == minVal and no owner: its thread moves
    // u[cur], so that every update of a row is one pass of the same loop
    for (int p = nrem + t; p < nc; p += THREADS) {
      const int j = s.remaining[p];
      const int own = s.row4col[j];
      const long long d = minVal - s.sp[j];
      s.v[j] -= d;
      s.u[j == sink ? cur : own] += j == sink ? minVal : d;
    }
    lsap_sync<THREADS>();
    if (t == 0) {
      int j = sink;
      for (int n = 0; n < nr; ++n) {   // a path visits a row once: at most nr edges end at `cur`
        const int r = s.path[j];
        s.row4col[j] = (unsigned short)r;
        const int nx = s.col4row[r];
        s.col4row[r] = (unsigned short)j;
        j = nx;
        if (r == cur) break;
      }
    }
    lsap_sync<THREADS>();
  }
  *steps_out = (int)steps;
  return 0;
}

}  // namespace mused
