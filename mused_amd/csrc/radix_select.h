// Exact radix select by one 1024-thread workgroup: the kk-th smallest (key, position) pair among m order-preserving 64-bit
// keys.  Shared by select_k_kernel (csrc/knn.hip: one row of scores) and chunk_select_kernel (csrc/meta_stream.hip: a running
// list and a chunk).  Bits above the highest bit in which the smallest and the largest key differ are skipped; each pass
// histograms one digit (<= 8 bits) of the still-undecided keys in LDS; when the bin that holds the kk-th key has shrunk to
// <= 256 keys the rest is finished by ranking those candidates against each other by (key, position).
#pragma once
#include "scan.h"

namespace mused {

constexpr int SELECT_THREADS = 1024;
constexpr int SELECT_WAVES = SELECT_THREADS / 64;

// the static LDS of a selecting kernel; `ws` is the callers' scratch for block_excl_scan in their emit loops
struct SelectLds {
  unsigned long long cand_key[256];  // its first 2 * SELECT_WAVES words also carry the min / max reduction, long before
  unsigned long long prefix, maskbits;
  int hist[256];
  int cand_idx[256];
  int ws[SELECT_WAVES];
  int remaining, shift, done, ncand, eqcount;
};

struct SelectThreshold {
  unsigned long long thr;  // the kk-th smallest key
  int need_eq;             // how many keys == thr are selected (smallest positions first)
  int eq_count;            // how many keys == thr there are, or -1 where the passes ran out of bits before a ranking
};

// key_at(i), i in [0, m): the keys; kmin / kmax: this thread's share of their minimum and maximum (~0ull / 0 for no key).
// Needs 1 <= kk <= m.  Called by all 1024 threads; ends behind a barrier
template <class KeyAt>
__device__ __forceinline__ SelectThreshold block_select_threshold(SelectLds& s, int m, int kk, KeyAt key_at,
                                                                   unsigned long long kmin, unsigned long long kmax) {
  const int tid = threadIdx.x;
  unsigned long long* red = s.cand_key;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long a = __shfl_xor(kmin, o), b = __shfl_xor(kmax, o);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = kmin;
    red[SELECT_WAVES + (tid >> 6)] = kmax;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long mn = red[0], mx = red[SELECT_WAVES];
    for (int i = 1; i < SELECT_WAVES; ++i) {
      mn = red[i] < mn ? red[i] : mn;
      mx = red[SELECT_WAVES + i] > mx ? red[SELECT_WAVES + i] : mx;
    }
    const unsigned long long diff = mn ^ mx;
    s.remaining = kk;
    if (diff == 0) {  // all keys equal: threshold = that key, every needed element is "equal"
      s.prefix = mn;
      s.maskbits = ~0ull;
      s.shift = -1;
    } else {
      const int top = 64 - __clzll(diff);  // bits [top, 64) are common
      s.maskbits = (top >= 64) ? 0ull : (~0ull << top);
      s.prefix = mn & s.maskbits;
      s.shift = top;  // the next digit covers [max(0, top - 8), top)
    }
    s.done = 0;
    s.ncand = 0;
  }
  __syncthreads();

  while (true) {
    const int top = s.shift;
    if (top <= 0 || s.done) break;
    const int lo = top >= 8 ? top - 8 : 0;
    const int width = top - lo;
    const unsigned long long pmask = s.maskbits, prefix = s.prefix;
    for (int i = tid; i < 256; i += SELECT_THREADS) s.hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += SELECT_THREADS) {
      const unsigned long long key = key_at(i);
      if ((key & pmask) == prefix) atomicAdd(&s.hist[(int)((key >> lo) & ((1u << width) - 1))], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int rem = s.remaining, cum = 0, dsel = 0;
      const int nb = 1 << width;
      for (int b = 0; b < nb; ++b) {
        if (cum + s.hist[b] >= rem) { dsel = b; break; }
        cum += s.hist[b];
      }
      s.remaining = rem - cum;
      s.prefix = prefix | ((unsigned long long)dsel << lo);
      s.maskbits = pmask | ((((unsigned long long)1 << width) - 1) << lo);
      s.shift = lo;
      if (s.hist[dsel] <= 256 && lo > 0) s.done = 1;  // finish by ranking the bin's members
    }
    __syncthreads();
  }

  const bool ranked = s.done;
  if (ranked) {
    // gather the undecided bin (<= 256 keys) with an LDS atomic append; the order does not matter, the ranking below is by
    // (key, position)
    const unsigned long long pmask = s.maskbits, prefix = s.prefix;
    for (int i = tid; i < m; i += SELECT_THREADS) {
      const unsigned long long key = key_at(i);
      if ((key & pmask) == prefix) {
        const int pos = atomicAdd(&s.ncand, 1);
        s.cand_key[pos] = key;
        s.cand_idx[pos] = i;
      }
    }
    __syncthreads();
    const int nc = s.ncand, rem = s.remaining;  // the rem-th smallest (1-based) of the candidates
    if (tid < nc) {
      const unsigned long long mk = s.cand_key[tid];
      const int mi = s.cand_idx[tid];
      int rank = 0, eq_before = 0, eq_all = 0;
      for (int j = 0; j < nc; ++j) {
        const unsigned long long kj = s.cand_key[j];
        const bool same = (kj == mk);
        const bool before = same && s.cand_idx[j] < mi;
        rank += (kj < mk) || before;
        eq_before += before;
        eq_all += same;
      }
      if (rank == rem - 1) {
        s.prefix = mk;
        s.remaining = eq_before + 1;
        s.eqcount = eq_all;
      }
    }
  }
  __syncthreads();
  return SelectThreshold{s.prefix, s.remaining, ranked ? s.eqcount : -1};
}

}  // namespace mused
