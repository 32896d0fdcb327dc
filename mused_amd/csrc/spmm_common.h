// What the binary (spmm.hip) and the valued (spmm_valued.hip) eigenstep products share: the kernel names of the dispatcher,
// the sign-in-store rule and the 16-byte pair accesses of `wide`.
#pragma once
#include "common.h"

namespace mused {

enum { SPMM_ROWS = 0, SPMM_WIDE = 1 };

__device__ __forceinline__ double spmm_signed(double s, double v) {
  const double x = s * v;
  return x == 0.0 ? 0.0 : x;
}

// the pair (c, c + 1) of one output row: c even, c + 1 < r.  Y16: y + c is 16-byte aligned (a template argument, not a flag:
// behind a run-time flag the compiler merges the two forms into 8-byte stores)
template <bool Y16>
__device__ __forceinline__ void spmm_store_pair(double* __restrict__ y, int c, double2 a, const double* __restrict__ col_sign) {
  if (col_sign) {
    a.x = spmm_signed(col_sign[c], a.x);
    a.y = spmm_signed(col_sign[c + 1], a.y);
  }
  if (Y16) {
    *reinterpret_cast<double2*>(y + c) = a;
  } else {
    y[c] = a.x;
    y[c + 1] = a.y;
  }
}

__device__ __forceinline__ double2 spmm_load_pair(const double* __restrict__ q) {
  return *reinterpret_cast<const double2*>(q);
}

// Which kernel a binary call gets (spmm.hip: shape rule, MUSED_SPMM / mused_spmm_force_path, the measured default).
int spmm_path(int n, int r, long ldq, long ldy, int q_align, int y_align);
// MUSED_SPMM / mused_spmm_force_path: SPMM_ROWS, SPMM_WIDE, or -1 for the default of the kernel family
int spmm_forced_path();

}  // namespace mused
