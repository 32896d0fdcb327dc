// The prefix sums and the binary search the kernel files share:
//   wave_incl_scan    inclusive sum over the 64 lanes, by shuffles
//   block_excl_scan   exclusive sum over a workgroup: shuffles scan a wave, the wave totals in LDS give the rest
//   lower_bound       on an ascending int array
#pragma once
#include "common.h"

namespace mused {

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

// Exclusive prefix sum of v over the workgroup, T = int or unsigned long long; total <- the sum, in every thread.  The
// workgroup is any multiple of 64 threads up to 1024 and all of them call; ws: 16 words of LDS.  Waves 0 .. 14 leave their
// sums in ws[0 .. 15); a thread adds those of the waves before its own (a 16th wave's sum is nobody's, and words past the
// last wave are read and never selected); the last thread's inclusive sum is the total and travels in ws[15].  Two barriers:
// every read of ws[0 .. 15) lies between them, and ws[15] is written between them and read behind the second, so the next
// call may follow at once
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* ws /*[16]*/, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T x = wave_incl_scan(v);
  if (lane == 63 && w < 15) ws[w] = x;
  __syncthreads();
  T base = 0;
#pragma unroll
  for (int i = 0; i < 15; ++i) base += (i < w) ? ws[i] : 0;
  if (threadIdx.x == blockDim.x - 1) ws[15] = base + x;
  __syncthreads();
  total = ws[15];
  return base + x - v;
}

// first position p in [lo, hi) with a[p] >= v (hi if none)
__device__ __forceinline__ int lower_bound(const int* __restrict__ a, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace mused
