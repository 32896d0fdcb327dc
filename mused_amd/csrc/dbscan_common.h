// What csrc/dbscan.hip and csrc/dbscan_incr.hip share: the constants of their state arrays and the kernel that numbers the
// clusters by ascending root.
#pragma once
#include "common.h"

namespace mused {

constexpr int DB_NONE = 0x7fffffff;        // root of a row that no cluster has reached
constexpr int DB_HAS_CORE = 1, DB_HAS_NONCORE = 2;
constexpr int DB_HAS_REBUILD = 4;         // (csrc/dbscan_incr.hip, a delete: the tile holds a row whose component is rebuilt)
constexpr long DB_MAX_ROWS = 1l << 19;     // 4096 row tiles: the tile grid, 4096 * 2049 workgroups of 256 threads, stays below the
                                           // 2^32 threads one launch may hold (reached near 740,000 rows)

// rank[i] = number of roots (core rows with root[i] == i) below i; one workgroup walks the rows in chunks of 1024 consecutive
// ones (coalesced): wave ballots give the position inside a wave, the 16 wave totals and a running carry the rest
constexpr int DB_RANK_THREADS = 1024;
static __global__ __launch_bounds__(DB_RANK_THREADS) void dbscan_rank_kernel(const int* __restrict__ root, int* __restrict__ rank,
                                                                              int* __restrict__ info, int n) {
  __shared__ int wtot[DB_RANK_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += DB_RANK_THREADS) {
    const int i = base + t;
    const bool is_root = i < n && root[i] == i;
    const unsigned long long bal = __ballot(is_root);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < DB_RANK_THREADS / 64; ++w) {
      const int c = wtot[w];
      total += c;
      before += w < wave ? c : 0;
    }
    if (i < n) rank[i] = carry + before + __popcll(bal & ((1ull << lane) - 1ull));
    carry += total;
    __syncthreads();  // wtot is rewritten by the next chunk
  }
  if (t == 0) info[1] = carry;
}

}  // namespace mused
