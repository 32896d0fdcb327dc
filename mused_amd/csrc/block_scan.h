// The scan of an array by ONE workgroup, in chunks of 1024 consecutive entries (coalesced): the block counts of a compaction
// (csrc/dbscan_incr.hip, csrc/tokenise.hip) and the histograms of a radix pass (radix_sort.h).  Each .hip is compiled on its
// own, so the kernel is static.
#pragma once
#include "scan.h"

namespace mused {

constexpr int BLOCKSCAN_THREADS = 1024;
// a[0 .. m) <- its exclusive prefix sums; *total <- the sum unless total is null (it may be a + m)
static __global__ __launch_bounds__(BLOCKSCAN_THREADS) void blockscan_kernel(int* __restrict__ a, int m, int* total) {
  __shared__ int ws[16];
  int carry = 0;
  for (int base = 0; base < m; base += BLOCKSCAN_THREADS) {
    const int i = base + threadIdx.x;
    const int v = i < m ? a[i] : 0;
    int tot;
    const int x = carry + block_excl_scan(v, ws, tot);
    if (i < m) a[i] = x;
    carry += tot;
  }
  if (total && threadIdx.x == 0) *total = carry;
}

}  // namespace mused
