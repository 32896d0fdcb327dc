// Y = S * Q for a real matrix S given as CSR neighbour lists with one fp64 value per entry (the weighted fusion
// S = sum_m w_m A_m of the modality masks, or any square matrix: adj_values.hip) and a dense row-major Q (n x r, fp64):
//   Y[i, c] = sum_{e in list(i)} val[e] * Q[col[e], c].
// The valued twin of spmm.hip, behind the same shape rule and switches (spmm_path) and with the same trip structure:
//   rows    one wave per output row, lanes across the columns, 8-byte loads, two entries per trip.
//   wide    a lane owns a column PAIR (16-byte loads), four entries per trip, indices AND values read with scalar loads (they are
//           wave-uniform: the values take no vector registers), those of the next trip in flight behind the row loads of this one.
// The rule both follow: every Y[i, c] is accumulated by ONE lane over row i's list, in list order, from
// 0.0, each step  acc = acc + (val[e] * Q[col[e], c])  with the product rounded before it is added -- no fused multiply-add
// (this file's `fp contract(off)`), so that the result can be restated in NumPy bit for bit and the two kernels agree bit for
// bit.  With every value 1.0 the product is exact and the result is that of mused_spmm_binary, bit for bit.
// col_sign: as in spmm.hip (a zero sum is stored as +0.0).
#include "spmm_common.h"

#pragma clang fp contract(off)

namespace mused {

__global__ void spmm_valued_kernel(const int* __restrict__ rowptr, const int* __restrict__ colidx,
                                   const double* __restrict__ vals, int n, const double* __restrict__ Q, long ldq, int r,
                                   double* __restrict__ Y, long ldy, const double* __restrict__ col_sign) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const int beg = rowptr[row], end = rowptr[row + 1];
  for (int c0 = 0; c0 < r; c0 += 192) {
    const int ca = c0 + lane, cb = ca + 64, cc = ca + 128;
    const bool ha = ca < r, hb = cb < r, hc = cc < r;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int e = beg;
    for (; e + 2 <= end; e += 2) {
      const double* q0 = Q + (long)colidx[e] * ldq;
      const double* q1 = Q + (long)colidx[e + 1] * ldq;
      const double v0 = vals[e], v1 = vals[e + 1];
      const double x0 = ha ? q0[ca] : 0.0, x1 = hb ? q0[cb] : 0.0, x2 = hc ? q0[cc] : 0.0;
      const double y0 = ha ? q1[ca] : 0.0, y1 = hb ? q1[cb] : 0.0, y2 = hc ? q1[cc] : 0.0;
      a0 = a0 + v0 * x0; a1 = a1 + v0 * x1; a2 = a2 + v0 * x2;
      a0 = a0 + v1 * y0; a1 = a1 + v1 * y1; a2 = a2 + v1 * y2;
    }
    if (e < end) {
      const double* q0 = Q + (long)colidx[e] * ldq;
      const double v0 = vals[e];
      if (ha) a0 = a0 + v0 * q0[ca];
      if (hb) a1 = a1 + v0 * q0[cb];
      if (hc) a2 = a2 + v0 * q0[cc];
    }
    if (col_sign) {
      if (ha) a0 = spmm_signed(col_sign[ca], a0);
      if (hb) a1 = spmm_signed(col_sign[cb], a1);
      if (hc) a2 = spmm_signed(col_sign[cc], a2);
    }
    double* y = Y + (long)row * ldy;
    if (ha) y[ca] = a0;
    if (hb) y[cb] = a1;
    if (hc) y[cc] = a2;
  }
}

// acc += v * x on both halves of the pairs a (columns ca, ca + 1) and b (cb, cb + 1): four rounded products, four rounded adds
__device__ __forceinline__ void spmm_valued_step(double2& a, double2& b, double v, double2 x, double2 z) {
  a.x = a.x + v * x.x; a.y = a.y + v * x.y;
  b.x = b.x + v * z.x; b.y = b.y + v * z.y;
}

// One wave per output row; a trip covers 192 columns as in spmm_wide_kernel.  The list and its values are wave-uniform.
template <bool Y16>
__global__ __launch_bounds__(256) void spmm_valued_wide_kernel(const int* __restrict__ rowptr, const int* __restrict__ colidx,
                                                               const double* __restrict__ vals, int n,
                                                               const double* __restrict__ Q, long ldq, int r,
                                                               double* __restrict__ Y, long ldy,
                                                               const double* __restrict__ col_sign) {
  const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const int beg = rowptr[row], end = rowptr[row + 1];
  for (int c0 = 0; c0 < r; c0 += 192) {
    const int ca = c0 + 2 * lane, cb = ca + 128;
    const bool ha = ca < r, hb = lane < 32 && cb < r;
    const double2 zero = make_double2(0.0, 0.0);
    double2 a = zero, b = zero;
    int e = beg;
    int j0 = 0, j1 = 0, j2 = 0, j3 = 0;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    if (e + 4 <= end) {
      j0 = colidx[e]; j1 = colidx[e + 1]; j2 = colidx[e + 2]; j3 = colidx[e + 3];
      v0 = vals[e]; v1 = vals[e + 1]; v2 = vals[e + 2]; v3 = vals[e + 3];
    }
    while (e + 4 <= end) {
      const double* q0 = Q + (long)j0 * ldq;
      const double* q1 = Q + (long)j1 * ldq;
      const double* q2 = Q + (long)j2 * ldq;
      const double* q3 = Q + (long)j3 * ldq;
      const double w0 = v0, w1 = v1, w2 = v2, w3 = v3;
      const double2 x0 = ha ? spmm_load_pair(q0 + ca) : zero, x1 = ha ? spmm_load_pair(q1 + ca) : zero;
      const double2 x2 = ha ? spmm_load_pair(q2 + ca) : zero, x3 = ha ? spmm_load_pair(q3 + ca) : zero;
      const double2 z0 = hb ? spmm_load_pair(q0 + cb) : zero, z1 = hb ? spmm_load_pair(q1 + cb) : zero;
      const double2 z2 = hb ? spmm_load_pair(q2 + cb) : zero, z3 = hb ? spmm_load_pair(q3 + cb) : zero;
      e += 4;
      if (e + 4 <= end) {
        j0 = colidx[e]; j1 = colidx[e + 1]; j2 = colidx[e + 2]; j3 = colidx[e + 3];
        v0 = vals[e]; v1 = vals[e + 1]; v2 = vals[e + 2]; v3 = vals[e + 3];
      }
      spmm_valued_step(a, b, w0, x0, z0);
      spmm_valued_step(a, b, w1, x1, z1);
      spmm_valued_step(a, b, w2, x2, z2);
      spmm_valued_step(a, b, w3, x3, z3);
    }
    const int m = end - e;  // 0 .. 3 entries left
    if (m > 0) {
      const int e1 = m > 1 ? e + 1 : e, e2 = m > 2 ? e + 2 : e;
      const double* q0 = Q + (long)colidx[e] * ldq;
      const double* q1 = Q + (long)colidx[e1] * ldq;
      const double* q2 = Q + (long)colidx[e2] * ldq;
      const double w0 = vals[e], w1 = vals[e1], w2 = vals[e2];
      const double2 x0 = ha ? spmm_load_pair(q0 + ca) : zero, x1 = ha ? spmm_load_pair(q1 + ca) : zero;
      const double2 x2 = ha ? spmm_load_pair(q2 + ca) : zero;
      const double2 z0 = hb ? spmm_load_pair(q0 + cb) : zero, z1 = hb ? spmm_load_pair(q1 + cb) : zero;
      const double2 z2 = hb ? spmm_load_pair(q2 + cb) : zero;
      spmm_valued_step(a, b, w0, x0, z0);
      if (m > 1) spmm_valued_step(a, b, w1, x1, z1);
      if (m > 2) spmm_valued_step(a, b, w2, x2, z2);
    }
    double* y = Y + (long)row * ldy;
    if (ha) spmm_store_pair<Y16>(y, ca, a, col_sign);
    if (hb) spmm_store_pair<Y16>(y, cb, b, col_sign);
  }
}

// The binary dispatcher's shape rule and its switches (MUSED_SPMM, mused_spmm_force_path); the default is `wide` wherever the
// shape can take it: measured faster than `rows` on A and A^T at (n, r) = (10^4, 138) AND at (2,000, 60), below the 4 MB
// that decide for the binary kernels.
static int spmm_valued_path(int r, long ldq, int q_align) {
  if ((r & 1) || (ldq & 1) || (q_align & 15)) return SPMM_ROWS;  // (spmm_path's shape rule)
  return spmm_forced_path() == SPMM_ROWS ? SPMM_ROWS : SPMM_WIDE;
}

int spmm_valued(const int* rowptr, const int* colidx, const double* vals, int n, const double* Q, long ldq, int r, double* Y,
                long ldy, hipStream_t stream, const double* col_sign) {
  const int q_align = (int)((uintptr_t)Q & 15), y_align = (int)((uintptr_t)Y & 15);
  const bool y16 = !(ldy & 1) && !y_align;
  if (spmm_valued_path(r, ldq, q_align) == SPMM_WIDE)
    hipLaunchKernelGGL(y16 ? spmm_valued_wide_kernel<true> : spmm_valued_wide_kernel<false>, dim3(cdiv(n, 4)), dim3(256), 0,
                       stream, rowptr, colidx, vals, n, Q, ldq, r, Y, ldy, col_sign);
  else
    hipLaunchKernelGGL(spmm_valued_kernel, dim3(cdiv(n, 4)), dim3(256), 0, stream, rowptr, colidx, vals, n, Q, ldq, r, Y, ldy,
                       col_sign);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // namespace mused

extern "C" int mused_spmm_valued(const int* rowptr, const int* colidx, const double* vals, int n, const double* Q, long ldq,
                                 int r, double* Y, long ldy, void* stream) {
  MUSED_REQUIRE(rowptr && colidx && vals && Q && Y && n > 0 && r > 0 && ldq >= r && ldy >= r,
                "mused_spmm_valued: bad arguments");
  return mused::spmm_valued(rowptr, colidx, vals, n, Q, ldq, r, Y, ldy, (hipStream_t)stream, nullptr);
}
