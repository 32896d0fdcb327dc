// Y = A * Q for a 0/1 adjacency A given as CSR neighbour lists (ascending columns) and a
// dense row-major Q (n x r, fp64): Y[i, :] = sum_{j in nbr(i)} Q[j, :].
// This is the `A @ Q` / `A.T @ Q` of sklearn's randomized range finder
// (sklearn:utils/extmath.py:349-355) specialised to the binary fused adjacency that
// matrix_operations.py:143-147 is always called with.  Gather-bound (Q stays L2 / Infinity-Cache
// resident: n*r*8 = 11 MB at n = 10^4, r = 138).  Every Y[i, c] is summed by ONE lane, in list
// order, starting from 0.0, whichever kernel runs: results are bitwise reproducible and do not
// depend on the kernel, the grid or the placement of its workgroups.
//
// Two kernels behind one dispatcher (spmm_path):
//   rows    one wave per output row, lanes across the columns, 8-byte loads, two neighbours per trip.  Takes every shape,
//           pitch and alignment.
//   wide    one wave per output row, a lane owns a column PAIR (16-byte loads), four neighbours per trip, the list read with
//           scalar loads, the indices of the next trip in flight behind the row loads of this one.  Needs r even and
//           Q + j * ldq 16-byte aligned for every j.
// (A third, `panels` -- the columns in 8 panels, one per XCD, so that an XCD gathers from a slice of Q that fits its L2 --
// was measured beside them and not kept: DESIGN section 4s.)
// col_sign (optional, r doubles of +-1): Y[i, c] = col_sign[c] * sum.  A sign commutes exactly with a floating-point sum
// (negation is exact, rounding is symmetric); a zero sum is stored as +0.0, which is what summing the negated terms from
// 0.0 gives: the bits are those of spmm(A, Q * diag(col_sign)).
#include <atomic>
#include <stdlib.h>

#include "spmm_common.h"

namespace mused {

__global__ void spmm_binary_kernel(const int* __restrict__ rowptr, const int* __restrict__ colidx, int n,
                                   const double* __restrict__ Q, long ldq, int r, double* __restrict__ Y,
                                   long ldy, const double* __restrict__ col_sign) {
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
      const double x0 = ha ? q0[ca] : 0.0, x1 = hb ? q0[cb] : 0.0, x2 = hc ? q0[cc] : 0.0;
      const double y0 = ha ? q1[ca] : 0.0, y1 = hb ? q1[cb] : 0.0, y2 = hc ? q1[cc] : 0.0;
      a0 += x0; a1 += x1; a2 += x2;
      a0 += y0; a1 += y1; a2 += y2;
    }
    if (e < end) {
      const double* q0 = Q + (long)colidx[e] * ldq;
      if (ha) a0 += q0[ca];
      if (hb) a1 += q0[cb];
      if (hc) a2 += q0[cc];
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

// One wave per output row.  A trip covers 192 columns: lane l the pair at 2 l of the first 128 and, for l < 32, the pair at
// 128 + 2 l.  The list is wave-uniform (scalar loads); four neighbours per step, their eight row loads and the indices of
// the next step issued before the first add.
template <bool Y16>
__global__ __launch_bounds__(256) void spmm_wide_kernel(const int* __restrict__ rowptr, const int* __restrict__ colidx, int n,
                                                        const double* __restrict__ Q, long ldq, int r, double* __restrict__ Y,
                                                        long ldy, const double* __restrict__ col_sign) {
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
    if (e + 4 <= end) { j0 = colidx[e]; j1 = colidx[e + 1]; j2 = colidx[e + 2]; j3 = colidx[e + 3]; }
    while (e + 4 <= end) {
      const double* q0 = Q + (long)j0 * ldq;
      const double* q1 = Q + (long)j1 * ldq;
      const double* q2 = Q + (long)j2 * ldq;
      const double* q3 = Q + (long)j3 * ldq;
      const double2 x0 = ha ? spmm_load_pair(q0 + ca) : zero, x1 = ha ? spmm_load_pair(q1 + ca) : zero;
      const double2 x2 = ha ? spmm_load_pair(q2 + ca) : zero, x3 = ha ? spmm_load_pair(q3 + ca) : zero;
      const double2 z0 = hb ? spmm_load_pair(q0 + cb) : zero, z1 = hb ? spmm_load_pair(q1 + cb) : zero;
      const double2 z2 = hb ? spmm_load_pair(q2 + cb) : zero, z3 = hb ? spmm_load_pair(q3 + cb) : zero;
      e += 4;
      if (e + 4 <= end) { j0 = colidx[e]; j1 = colidx[e + 1]; j2 = colidx[e + 2]; j3 = colidx[e + 3]; }
      a.x += x0.x; a.y += x0.y; b.x += z0.x; b.y += z0.y;
      a.x += x1.x; a.y += x1.y; b.x += z1.x; b.y += z1.y;
      a.x += x2.x; a.y += x2.y; b.x += z2.x; b.y += z2.y;
      a.x += x3.x; a.y += x3.y; b.x += z3.x; b.y += z3.y;
    }
    const int m = end - e;  // 0 .. 3 neighbours left
    if (m > 0) {
      const double* q0 = Q + (long)colidx[e] * ldq;
      const double* q1 = Q + (long)colidx[m > 1 ? e + 1 : e] * ldq;
      const double* q2 = Q + (long)colidx[m > 2 ? e + 2 : e] * ldq;
      const double2 x0 = ha ? spmm_load_pair(q0 + ca) : zero, x1 = ha ? spmm_load_pair(q1 + ca) : zero;
      const double2 x2 = ha ? spmm_load_pair(q2 + ca) : zero;
      const double2 z0 = hb ? spmm_load_pair(q0 + cb) : zero, z1 = hb ? spmm_load_pair(q1 + cb) : zero;
      const double2 z2 = hb ? spmm_load_pair(q2 + cb) : zero;
      a.x += x0.x; a.y += x0.y; b.x += z0.x; b.y += z0.y;
      if (m > 1) { a.x += x1.x; a.y += x1.y; b.x += z1.x; b.y += z1.y; }
      if (m > 2) { a.x += x2.x; a.y += x2.y; b.x += z2.x; b.y += z2.y; }
    }
    double* y = Y + (long)row * ldy;
    if (ha) spmm_store_pair<Y16>(y, ca, a, col_sign);
    if (hb) spmm_store_pair<Y16>(y, cb, b, col_sign);
  }
}

// MUSED_SPMM=rows|wide (diagnostic, read once) or mused_spmm_force_path; -1: the measured default per shape
static std::atomic<int> g_spmm_forced{-2};  // -2: the environment has not been read

int spmm_forced_path() {
  int f = g_spmm_forced.load(std::memory_order_relaxed);
  if (f == -2) {
    const char* e = getenv("MUSED_SPMM");
    f = -1;
    if (e && !strcmp(e, "rows")) f = SPMM_ROWS;
    else if (e && !strcmp(e, "wide")) f = SPMM_WIDE;
    int expect = -2;
    if (!g_spmm_forced.compare_exchange_strong(expect, f)) f = expect;
  }
  return f;
}

// The measured choice per shape class.  A panel Q that fits one XCD's L2 (the reference's default
// parameters: n = 2,000, r = 60) keeps `rows`: the launch takes 10 - 40 us either way and nothing shows in the pipeline.
constexpr long SPMM_L2_BYTES = 4l << 20;

static int spmm_default_path(int n, int r) { return (long)n * r * 8 > SPMM_L2_BYTES ? SPMM_WIDE : SPMM_ROWS; }

// Which kernel a call gets.  q_align / y_align: the base pointers of Q and Y modulo 16 bytes.
int spmm_path(int n, int r, long ldq, long ldy, int q_align, int y_align) {
  (void)ldy; (void)y_align;  // (they only choose the width of the stores inside `wide`)
  if ((r & 1) || (ldq & 1) || (q_align & 15)) return SPMM_ROWS;
  const int want = spmm_forced_path();
  return want < 0 ? spmm_default_path(n, r) : want;
}

int spmm_binary(const int* rowptr, const int* colidx, int n, const double* Q, long ldq, int r, double* Y, long ldy,
                hipStream_t stream, const double* col_sign) {
  const int q_align = (int)((uintptr_t)Q & 15), y_align = (int)((uintptr_t)Y & 15);
  const bool y16 = !(ldy & 1) && !y_align;
  if (spmm_path(n, r, ldq, ldy, q_align, y_align) == SPMM_WIDE)
    hipLaunchKernelGGL(y16 ? spmm_wide_kernel<true> : spmm_wide_kernel<false>, dim3(cdiv(n, 4)), dim3(256), 0, stream, rowptr,
                       colidx, n, Q, ldq, r, Y, ldy, col_sign);
  else
    hipLaunchKernelGGL(spmm_binary_kernel, dim3(cdiv(n, 4)), dim3(256), 0, stream, rowptr, colidx, n, Q, ldq, r, Y, ldy,
                       col_sign);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // namespace mused

extern "C" int mused_spmm_binary(const int* rowptr, const int* colidx, int n, const double* Q, long ldq, int r,
                                 double* Y, long ldy, void* stream) {
  MUSED_REQUIRE(rowptr && colidx && Q && Y && n > 0 && r > 0 && ldq >= r && ldy >= r, "mused_spmm_binary: bad arguments");
  return mused::spmm_binary(rowptr, colidx, n, Q, ldq, r, Y, ldy, (hipStream_t)stream, nullptr);
}

// The kernel mused_spmm_binary runs for these arguments: 0 rows, 1 wide (q_align, y_align: base pointers mod 16).
extern "C" int mused_spmm_binary_path(int n, int r, long ldq, long ldy, int q_align, int y_align) {
  return mused::spmm_path(n, r, ldq, ldy, q_align, y_align);
}

// Test-facing: force a kernel for the shapes that can take it (0 rows, 1 wide), as MUSED_SPMM does; -1 returns to
// the measured default.  An eigenstep handle records its kernels when it first runs a shape: force before that.
extern "C" int mused_spmm_force_path(int path) {
  MUSED_REQUIRE(path >= -1 && path <= mused::SPMM_WIDE, "mused_spmm_force_path: path %d outside -1 .. 1", path);
  mused::g_spmm_forced.store(path, std::memory_order_relaxed);
  return MUSED_OK;
}
