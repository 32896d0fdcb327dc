// What the kernels that decide something per pair of rows share (dbscan_tile_kernel, dbscan_incr_tile_kernel,
// emst_tile_kernel, sil_tile_kernel, kd_tile_kernel, knn_band_kernel): each leaves a 128 x 128 tile of x_i . x_j in the accumulators of
// gemm_tile_mainloop (gemm_f64.h) and then looks at every entry.  The deciding part is each file's own; here are
//   pair_slot / pair_tile / pair_grid   which tile a workgroup takes when every unordered pair of row tiles is visited once
//   patch_lanes / patch_row / patch_col where the entries of a thread's accumulators lie in the tile, and which lanes share a
//                                       row or a column of it
//   pair_launch                    the launch of a kernel's VEC or plain instance, behind its dynamic-LDS opt-in
//   col_slices                          how a full-square schedule cuts its column tiles below 256 row tiles
//   self_product_args                   GemmArgs of X X^T
//   norm_not_finite / norms_finite_kernel, pair_tau_coeff / ulp4   the guards around a comparison of squared distances
// A wrong formula here gives no error: it gives results that are wrong for the pairs of particular tiles only.
#pragma once
#include "gemm_f64.h"

namespace mused {

// ---- which tile ---------------------------------------------------------------------------------------------------------
// Tile (I, (I + delta) mod tiles), delta in [0, tiles / 2]: every unordered pair of row tiles once.  A launch covers n_delta
// consecutive distances; 64 consecutive workgroups (one XCD's share) touch 8 A row-panels and 15 B row-panels.
static inline int pair_grid(int tiles, int n_delta) { return cdiv(tiles, 8) * 8 * n_delta; }
static inline int pair_grid(int tiles) { return pair_grid(tiles, tiles / 2 + 1); }  // all distances in one launch

// step 1: this workgroup's row tile (counted from the first one of the launch) and its distance (from the launch's first)
__device__ __forceinline__ void pair_slot(int n_delta, int& I, int& dk) {
  const int e = xcd_remap(blockIdx.x, gridDim.x);
  const int per_group = 8 * n_delta;
  const int ig = e / per_group, rem = e - ig * per_group;
  dk = rem >> 3;
  I = ig * 8 + (rem & 7);
}

// step 2: the column tile J of row tile I at distance delta <= tiles / 2; false: no tile (the grid's padding, or the second
// visit of an antipodal pair).  A tile with delta != 0 holds one orientation of its pairs and serves both; a diagonal tile
// holds both orientations itself
__device__ __forceinline__ bool pair_tile(int I, int delta, int tiles, int& J) {
  if (I >= tiles) return false;
  if (2 * delta == tiles && I >= tiles / 2) return false;  // even tile count: the antipodal pairs once
  J = I + delta;
  if (J >= tiles) J -= tiles;
  return true;
}

// ---- where a thread's entries lie ---------------------------------------------------------------------------------------
// Wave (wr, wc) of the 2 x 2 holds a 64 x 64 patch of the tile.  acc[i][j][r] of its lane (kq, li) is the entry
//   (patch_row(m0, wr, kq) + 16 i + 4 r,  patch_col(n0, wc, li) + 16 j)         i, j, r in [0, 4)
// so the 16 lanes that share kq hold the 64 columns of a row between them (__shfl_xor by 1, 2, 4, 8; the lane with li == 0
// writes for them) and the 4 lanes that share li the 64 rows of a column (__shfl_xor by 16, 32; the lane with kq == 0).
// The helpers stop here on purpose: with i, j, r, the reductions or the li == 0 / kq == 0 tests behind a function the
// compiler allocates registers and schedules the epilogues of dbscan_tile_kernel differently.
__device__ __forceinline__ void patch_lanes(int& lane, int& wr, int& wc, int& kq, int& li) {
  lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  wr = wave >> 1, wc = wave & 1, kq = lane >> 4, li = lane & 15;
}
__device__ __forceinline__ int patch_row(int m0, int wr, int kq) { return m0 + wr * 64 + kq; }
__device__ __forceinline__ int patch_col(int n0, int wc, int li) { return n0 + wc * 64 + li; }

// ---- host ---------------------------------------------------------------------------------------------------------------
// Full-square schedules (sil_tile_kernel, kd_tile_kernel: a workgroup owns a row tile and walks column tiles): column slices
// for `tiles` row tiles.  1 from 256 tiles on (the row tiles alone fill the GPU), else as many runs of whole column tiles as
// bring the grid to about 512 workgroups, at most 16
constexpr int MAX_COL_SLICES = 16;
static inline int col_slices(int tiles) {
  if (tiles >= 256) return 1;
  const int s = 512 / tiles < tiles ? 512 / tiles : tiles;
  return s < MAX_COL_SLICES ? s : MAX_COL_SLICES;
}

// X X^T for n rows of length d
static inline GemmArgs self_product_args(const void* X, long ld, long n, int d) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = X; g.B = X; g.lda = ld; g.ldb = ld; g.M = (int)n; g.N = (int)n; g.K = d;
  return g;
}

// One launch of a tile kernel of GEMM_THREADS threads with lds_bytes of dynamic LDS: its VEC instance (16-byte loads legal:
// vec_ok) or the plain one, each behind its own opt-in (allow_dynamic_lds, internal.h)
template <auto KVEC, auto KPLAIN, class... Args>
static int pair_launch(bool vec, int grid, size_t lds_bytes, hipStream_t st, Args... args) {
  static LdsOptIn opt[2];
  const hipError_t err = allow_dynamic_lds(opt[vec ? 1 : 0], vec ? (const void*)KVEC : (const void*)KPLAIN, lds_bytes);
  MUSED_CHECK_HIP(err);
  if (vec) hipLaunchKernelGGL(KVEC, dim3(grid), dim3(GEMM_THREADS), lds_bytes, st, args...);
  else hipLaunchKernelGGL(KPLAIN, dim3(grid), dim3(GEMM_THREADS), lds_bytes, st, args...);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// ---- guards -------------------------------------------------------------------------------------------------------------
// NaN or inf (an overflowing norm of finite values included)
__device__ __forceinline__ bool norm_not_finite(double v) { return !(fabs(v) <= 1.7976931348623157e308); }

// some nrm[0 .. n) is not finite -> *flag |= bit.  256 threads a workgroup.  (A launch of its own behind the kernel that
// clears the flag, so that the flag is not cleared behind it.)
static __global__ __launch_bounds__(256) void norms_finite_kernel(const double* __restrict__ nrm, int n, int* __restrict__ flag,
                                                                  int bit) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool bad = norm_not_finite(i < n ? nrm[i] : 0.0);
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, bit);
}

// Any evaluation of d2(x, y) in d dimensions, here or in scikit-learn, lies within (d + 8) 2^-52 (|x|^2 + |y|^2) of the exact
// value (derivation: mused_amd/dbscan.py tau_coefficient, which returns the same 2 (d + 8)): two evaluations
// further apart than pair_tau_coeff(d) (|x|^2 + |y|^2) lie on the same side of a threshold.
static inline double pair_tau_coeff(int d) { return 2.0 * (d + 8) * 2.220446049250313e-16; }
// 4 ulp of v >= 0 (an ulp is at most v * 2^-52; subnormal v: the smallest subnormal)
__host__ __device__ __forceinline__ double ulp4(double v) { return 4.0 * fmax(v * 2.220446049250313e-16, 4.9406564584124654e-324); }

}  // namespace mused
