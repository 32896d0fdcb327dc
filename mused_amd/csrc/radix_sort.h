// One pass of a stable LSD radix sort of (key, value) pairs of ints, 8 bits of the key a pass: shared by csrc/tokenise.hip
// (entries by term) and csrc/rows_find.hip (elements by group).  A histogram per tile of 1024 entries (one wave a tile), one
// exclusive scan of the digit-major table (block_scan.h), then the scatter in tile order with the ranks inside a chunk of 64
// from ballots: entries of one digit keep their order.  The callers loop over the passes; their pass counts follow their keys.
// Key range: p passes order the pairs by the low 8 p bits of the keys, as unsigned numbers.  So with fewer than four passes
// the keys are non-negative and below 2^(8 p) (tokenise.hip's term ids, rows_find.hip's slots); four passes order all 32 bits
// as one unsigned word, which is why silhouette.hip flips the sign bit of its labels first.
#pragma once
#include "block_scan.h"

namespace mused {

constexpr int RADIX_TILE = 1024;  // entries per wave

// The live count of a sort whose grid covers an upper bound: a value, or read on the device when `ptr` is set
struct RadixCount {
  int value;
  const int* ptr;
  __device__ __forceinline__ int get() const { return ptr ? *ptr : value; }
};

__device__ __forceinline__ int radix_digit(int key, int shift) { return (key >> shift) & 255; }

// hist[digit * nb + tile] <- entries of the tile with that digit
static __global__ __launch_bounds__(64) void radix_hist_kernel(const int* __restrict__ key, RadixCount count, int shift,
                                                              int* __restrict__ hist, int nb) {
  __shared__ int c[256];
  const int lane = threadIdx.x, n = count.get();
  for (int j = lane; j < 256; j += 64) c[j] = 0;
  __syncthreads();
  const long t0 = (long)blockIdx.x * RADIX_TILE;
  for (int q = 0; q < RADIX_TILE; q += 64) {
    const long i = t0 + q + lane;
    if (i < n) atomicAdd(&c[radix_digit(key[i], shift)], 1);
  }
  __syncthreads();
  for (int j = lane; j < 256; j += 64) hist[(long)j * nb + blockIdx.x] = c[j];
}

// hist scanned (digit-major): entry i of tile b goes to hist[digit][b] + its rank among the tile's earlier entries of the
// digit.  val == nullptr: the entry is its own index (the first pass).  gather_out set: gather_out[p] = gather_src[value] too
static __global__ __launch_bounds__(64) void radix_scatter_kernel(const int* __restrict__ key, const int* __restrict__ val,
                                                                 RadixCount count, int shift, const int* __restrict__ hist,
                                                                 int nb, int* __restrict__ key_out, int* __restrict__ val_out,
                                                                 const int* __restrict__ gather_src,
                                                                 int* __restrict__ gather_out) {
  __shared__ int run[256];
  const int lane = threadIdx.x, n = count.get();
  for (int j = lane; j < 256; j += 64) run[j] = hist[(long)j * nb + blockIdx.x];
  __syncthreads();
  const long t0 = (long)blockIdx.x * RADIX_TILE;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int q = 0; q < RADIX_TILE; q += 64) {
    const long i = t0 + q + lane;
    const bool live = i < n;
    const int k = live ? key[i] : 0;
    const int dg = radix_digit(k, shift);
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (dg >> bit) & 1;
      const unsigned long long m = __ballot(live && on);
      peers &= on ? m : ~m;
    }
    const int ahead = __popcll(peers & below);
    const int p = live ? run[dg] + ahead : 0;
    __syncthreads();
    if (live && ahead == 0) run[dg] += __popcll(peers);  // one lane per digit present in the chunk
    __syncthreads();
    if (live && (unsigned)p < (unsigned)n) {
      const int v = val ? val[i] : (int)i;
      key_out[p] = k;
      val_out[p] = v;
      if (gather_out) gather_out[p] = gather_src[v];
    }
  }
}

// one pass over at most `cap` entries: (key, val) -> (key_out, val_out) by the digit at `shift`; hist: 256 * cdiv(cap, RADIX_TILE)
static int radix_sort_pass(const int* key, const int* val, int cap, RadixCount count, int shift, int* hist, int* key_out,
                           int* val_out, const int* gather_src, int* gather_out, hipStream_t st) {
  const int nb = cdiv(cap, RADIX_TILE);
  hipLaunchKernelGGL(radix_hist_kernel, dim3(nb), dim3(64), 0, st, key, count, shift, hist, nb);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, st, hist, 256 * nb, (int*)nullptr);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(radix_scatter_kernel, dim3(nb), dim3(64), 0, st, key, val, count, shift, hist, nb, key_out, val_out,
                     gather_src, gather_out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // namespace mused
