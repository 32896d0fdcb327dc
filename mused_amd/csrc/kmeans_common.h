// The arithmetic every k-means path takes from one place, so that labels stay bit-identical between mused_kmeans_lloyd,
// mused_kmeans_lloyd_wide (csrc/kmeans.hip) and mused_mbkm_step / mused_kmeans_assign (csrc/minibatch.hip):
//   km_take / km_lane_min    first minimum of csq_j - 2 x . c_j: strict < per thread, lexicographic (distance, j) across lanes
//   km_stream_tiles          tile sizes of the streamed E-step kernels (kmw_assign_kernel, mbkm_assign_kernel) within an
//                            LDS budget; allow_dynamic_lds (internal.h) raises a kernel's limit to one
//   km_norm2 / km_csq_kernel |c_j|^2 as one fma chain over c = 0 .. d - 1
//   km_finish                tail of a Lloyd M step: total squared shift (fixed tree), centre norms, stop rule
#pragma once
#include "internal.h"

namespace mused {

constexpr int KM_CHUNK = 256;  // threads of an E-step workgroup; rows of an M-step chunk

struct KmInfo {
  int iters;      // Lloyd iterations run
  int done;       // 0 running, 1 strict convergence (labels repeated), 2 centre shift <= tol
  int empty;      // a cluster lost all its rows
  int changed;    // scratch: some label differs from the previous iteration
};

constexpr int KM_NO_LABEL = 0x7fffffff;             // (best, lab) holds no candidate yet
constexpr double KM_NO_DIST = 1.7976931348623157e308;

// Candidate (dist, j) of a thread whose candidates come in ascending j: strict <, the first minimum wins, as in sklearn.
__device__ __forceinline__ void km_take(double& best, int& lab, double dist, int j) {
  if (lab == KM_NO_LABEL || dist < best) {
    best = dist;
    lab = j;
  }
}

// The pt (a power of two <= 64) adjacent lanes that share a row agree on the lexicographic (distance, j) minimum of their
// (best, lab); lanes without a candidate do not count.  Unrolls where pt is a constant.
__device__ __forceinline__ void km_lane_min(double& best, int& lab, int pt) {
  for (int o = 1; o < pt; o <<= 1) {
    const double ob = __shfl_xor(best, o);
    const int ol = __shfl_xor(lab, o);
    if (ol != KM_NO_LABEL && (lab == KM_NO_LABEL || ob < best || (ob == best && ol < lab))) {
      best = ob;
      lab = ol;
    }
  }
}

__device__ __forceinline__ double km_norm2(const double* c, int d) {
  double s = 0.0;
  for (int i = 0; i < d; ++i) s = fma(c[i], c[i], s);
  return s;
}

static __global__ void km_csq_kernel(const double* __restrict__ C, int k, int d, double* __restrict__ csq) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < k) csq[j] = km_norm2(C + (long)j * d, d);
}

// Tiles of a streamed E-step kernel within `budget` doubles of LDS: TR rows (32, else 16) and KT centres (a multiple of
// PT = 256 / TR, or all k).
static inline bool km_stream_tiles(size_t budget, int d, int k, int* TR, int* KT) {
  const int cap = (int)(budget / (d + 1));
  for (int tr : {32, 16}) {
    const int pt = KM_CHUNK / tr;
    int kt = cap - tr;
    if (kt >= k) kt = k;
    else kt = (kt / pt) * pt;
    if (kt >= 1 && (kt >= pt || kt == k)) {
      *TR = tr;
      *KT = kt;
      return true;
    }
  }
  return false;
}

// Tail of a Lloyd M step in one workgroup of 1024 threads, after the centres C are written.  `acc` is this thread's share
// of the squared shift (elements e = t, t + 1024, ... in order); the shares are added by a fixed tree, the centre norms
// follow, and thread 0 applies the stop rule.
__device__ __forceinline__ void km_finish(double acc, const double* C, int k, int d, double* csq, double tol, int first_iter,
                                          KmInfo* info) {
  __shared__ double red[1024];
  const int t = threadIdx.x;
  red[t] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  for (int j = t; j < k; j += 1024) csq[j] = km_norm2(C + (long)j * d, d);
  if (t == 0) {
    info->iters += 1;
    if (!first_iter && info->changed == 0) info->done = 1;       // labels repeated: strict convergence
    else if (red[0] <= tol) info->done = 2;                       // centres stopped moving
    info->changed = 0;
  }
}

}  // namespace mused
