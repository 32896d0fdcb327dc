// One fp64 value per entry of CSR neighbour lists, for the valued eigenstep (spmm_valued.hip).  Two sources:
//   masks   weighted fusion S = sum_m w_m A_m of M <= 8 modality bitmasks whose OR gave the lists:
//           val[e] = the fp64 sum, from 0.0, IN MODALITY ORDER, of w_m over the modalities whose bit (i, col[e]) is set --
//           plain additions, nothing reassociated, so that the host restates it bit for bit.
//   dense   any square matrix (F32 / F64 / I64) whose nonzeros gave the lists: val[e] = (double)dense[i, col[e]].
// `transposed`: the lists are those of the transposed pattern (row i lists the j with an entry (j, i)): the value is read at
// (col[e], i).  One wave per row, lanes over the row's entries.  A value that is not finite raises bit 0 of *nonfinite.
// The source description (pointers, weights) reaches the kernels by value (the stand-alone entries) or from device memory
// (an eigenstep handle: its recorded graph must stay valid when masks and weights change from call to call).
// GUARD (the handle's kernels): the eigenstep behind them squares its panels twice (Gram of A^T A Q) and several of its
// kernels pick a row by comparing magnitudes (LU pivot, svd_flip): a NaN there is an index nobody wrote.  So no value that
// could make one enters the chain: a value that is not finite (bit 0), or whose magnitude lies outside
// [2^-200, 2^200] (bit 1: beyond it the chain over- or underflows for n up to 2^17), is flagged and STORED AS 1.0 -- the call's
// result is invalid and says so, and every kernel behind runs on finite numbers.
#include "internal.h"

#pragma clang fp contract(off)

namespace mused {

constexpr double ADJ_VAL_MAX = 1.6069380442589903e60;   // 2^200
constexpr double ADJ_VAL_MIN = 6.223015277861142e-61;   // 2^-200

template <bool GUARD>
__device__ __forceinline__ double adj_val_checked(double v, int* __restrict__ flag) {
  if (!isfinite(v)) {
    if (flag) atomicOr(flag, 1);
    return GUARD ? 1.0 : v;
  }
  if (GUARD && v != 0.0 && !(fabs(v) <= ADJ_VAL_MAX && fabs(v) >= ADJ_VAL_MIN)) {
    if (flag) atomicOr(flag, 2);
    return 1.0;
  }
  return v;
}

template <bool GUARD>
__device__ __forceinline__ void csr_values_masks_row(const AdjValSrc& s, int n, int words, const int* __restrict__ rowptr,
                                                     const int* __restrict__ colidx, int transposed,
                                                     double* __restrict__ vals, int* __restrict__ nonfinite) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const int beg = rowptr[row], end = rowptr[row + 1];
  for (int e = beg + lane; e < end; e += 64) {
    const int j = colidx[e];
    const int ri = transposed ? j : row, ci = transposed ? row : j;
    const long word = (long)ri * words + (ci >> 6);
    double v = 0.0;
#pragma unroll
    for (int m = 0; m < ADJ_VAL_MAX_M; ++m)
      if (m < s.M && ((reinterpret_cast<const unsigned long long*>(s.p[m])[word] >> (ci & 63)) & 1ull)) v = v + s.w[m];
    vals[e] = adj_val_checked<GUARD>(v, nonfinite);
  }
}

template <bool GUARD>
__device__ __forceinline__ void csr_values_dense_row(const AdjValSrc& s, int n, const int* __restrict__ rowptr,
                                                     const int* __restrict__ colidx, int transposed,
                                                     double* __restrict__ vals, int* __restrict__ nonfinite) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const int beg = rowptr[row], end = rowptr[row + 1];
  for (int e = beg + lane; e < end; e += 64) {
    const int j = colidx[e];
    const long at = transposed ? (long)j * s.ld + row : (long)row * s.ld + j;
    double v;
    if (s.dtype == MUSED_F64) v = reinterpret_cast<const double*>(s.p[0])[at];
    else if (s.dtype == MUSED_F32) v = (double)reinterpret_cast<const float*>(s.p[0])[at];
    else v = (double)reinterpret_cast<const long long*>(s.p[0])[at];
    vals[e] = adj_val_checked<GUARD>(v, nonfinite);
  }
}

__global__ void csr_values_masks_kernel(AdjValSrc s, int n, int words, const int* __restrict__ rowptr,
                                        const int* __restrict__ colidx, int transposed, double* __restrict__ vals,
                                        int* __restrict__ nonfinite) {
  csr_values_masks_row<false>(s, n, words, rowptr, colidx, transposed, vals, nonfinite);
}

__global__ void csr_values_masks_dev_kernel(const AdjValSrc* __restrict__ s, int n, int words, const int* __restrict__ rowptr,
                                            const int* __restrict__ colidx, int transposed, double* __restrict__ vals,
                                            int* __restrict__ nonfinite) {
  csr_values_masks_row<true>(*s, n, words, rowptr, colidx, transposed, vals, nonfinite);
}

__global__ void csr_values_dense_kernel(AdjValSrc s, int n, const int* __restrict__ rowptr, const int* __restrict__ colidx,
                                        int transposed, double* __restrict__ vals, int* __restrict__ nonfinite) {
  csr_values_dense_row<false>(s, n, rowptr, colidx, transposed, vals, nonfinite);
}

__global__ void csr_values_dense_dev_kernel(const AdjValSrc* __restrict__ s, int n, const int* __restrict__ rowptr,
                                            const int* __restrict__ colidx, int transposed, double* __restrict__ vals,
                                            int* __restrict__ nonfinite) {
  csr_values_dense_row<true>(*s, n, rowptr, colidx, transposed, vals, nonfinite);
}

__global__ void adj_val_src_store_kernel(AdjValSrc s, AdjValSrc* __restrict__ dst) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *dst = s;
}

// masks / weights as the C entries take them (HOST arrays) -> the kernels' description; MUSED_ERR_ARG on anything the
// weighted fusion does not define: M outside 1 .. 8, a null mask, a weight that is not finite and > 0
int adj_val_src_masks(const unsigned long long* const* masks, const double* weights, int M, AdjValSrc* out, const char* who) {
  MUSED_REQUIRE(masks && weights, "%s: null pointer", who);
  MUSED_REQUIRE(M >= 1 && M <= ADJ_VAL_MAX_M, "%s: M = %d modalities outside 1 .. %d", who, M, ADJ_VAL_MAX_M);
  memset(out, 0, sizeof(*out));
  for (int m = 0; m < M; ++m) {
    MUSED_REQUIRE(masks[m], "%s: mask %d is null", who, m);
    MUSED_REQUIRE(weights[m] > 0.0 && weights[m] <= 1.7976931348623157e308, "%s: weight %d = %g is not finite and > 0", who, m,
                  weights[m]);
    out->p[m] = masks[m];
    out->w[m] = weights[m];
  }
  out->M = M;
  return MUSED_OK;
}

int adj_val_src_dense(const void* dense, int dtype, int n, long ld, AdjValSrc* out, const char* who) {
  MUSED_REQUIRE(dense, "%s: null pointer", who);
  MUSED_REQUIRE(ld >= n, "%s: ld = %ld below n = %d", who, ld, n);
  if (dtype != MUSED_F32 && dtype != MUSED_F64 && dtype != MUSED_I64) {
    set_error("%s: unsupported dtype %d", who, dtype);
    return MUSED_ERR_UNSUPPORTED;
  }
  memset(out, 0, sizeof(*out));
  out->p[0] = dense;
  out->dtype = dtype;
  out->ld = ld;
  return MUSED_OK;
}

int adj_val_src_store(const AdjValSrc& src, AdjValSrc* dst, hipStream_t st) {
  hipLaunchKernelGGL(adj_val_src_store_kernel, dim3(1), dim3(64), 0, st, src, dst);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

int adj_csr_values_dev(const AdjValSrc* src_dev, bool dense, int n, int words, const int* rowptr, const int* colidx,
                       int transposed, double* vals, int* nonfinite, hipStream_t st) {
  if (dense)
    hipLaunchKernelGGL(csr_values_dense_dev_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, src_dev, n, rowptr, colidx, transposed,
                       vals, nonfinite);
  else
    hipLaunchKernelGGL(csr_values_masks_dev_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, src_dev, n, words, rowptr, colidx,
                       transposed, vals, nonfinite);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // namespace mused

using namespace mused;

extern "C" {

int mused_adj_csr_values(const unsigned long long* const* masks, const double* weights, int M, int n, int words,
                         const int* rowptr, const int* colidx, int transposed, double* vals, void* stream) {
  AdjValSrc src;
  int rc;
  if ((rc = adj_val_src_masks(masks, weights, M, &src, "mused_adj_csr_values"))) return rc;
  MUSED_REQUIRE(rowptr && colidx && vals, "mused_adj_csr_values: null pointer");
  MUSED_REQUIRE(n > 0 && words >= (n + 63) / 64 && (transposed == 0 || transposed == 1),
                "mused_adj_csr_values: bad sizes n=%d words=%d transposed=%d", n, words, transposed);
  hipLaunchKernelGGL(csr_values_masks_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, src, n, words, rowptr, colidx,
                     transposed, vals, (int*)nullptr);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

int mused_adj_csr_values_dense(const void* dense, int dtype, int n, long ld, const int* rowptr, const int* colidx,
                               int transposed, double* vals, int* nonfinite, void* stream) {
  MUSED_REQUIRE(rowptr && colidx && vals && nonfinite, "mused_adj_csr_values_dense: null pointer");
  MUSED_REQUIRE(n > 0 && (transposed == 0 || transposed == 1), "mused_adj_csr_values_dense: bad sizes n=%d transposed=%d", n,
                transposed);
  AdjValSrc src;
  int rc;
  if ((rc = adj_val_src_dense(dense, dtype, n, ld, &src, "mused_adj_csr_values_dense"))) return rc;
  hipLaunchKernelGGL(csr_values_dense_kernel, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, src, n, rowptr, colidx,
                     transposed, vals, nonfinite);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
