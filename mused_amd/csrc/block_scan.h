// a[0 .. m) <- its exclusive prefix sums, by ONE workgroup: shared by csrc/dbscan_incr.hip (the block totals of a keep mask) and
// csrc/rows_find.hip (the histograms of a radix pass).  Chunks of 1024 consecutive entries (coalesced): shuffles scan a wave,
// the 16 wave totals and a running carry give the rest.
#pragma once
#include "common.h"

namespace mused {

constexpr int BLOCKSCAN_THREADS = 1024;
static __global__ __launch_bounds__(BLOCKSCAN_THREADS) void blockscan_kernel(int* __restrict__ a, int m) {
  __shared__ int wtot[BLOCKSCAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int carry = 0;
  for (int base = 0; base < m; base += BLOCKSCAN_THREADS) {
    const int i = base + t;
    const int v = i < m ? a[i] : 0;
    int x = v;  // inclusive over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o);
      x += lane >= o ? y : 0;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < BLOCKSCAN_THREADS / 64; ++w) {
      const int c = wtot[w];
      total += c;
      before += w < wave ? c : 0;
    }
    if (i < m) a[i] = carry + before + x - v;
    carry += total;
    __syncthreads();  // wtot is rewritten by the next chunk
  }
}

}  // namespace mused
