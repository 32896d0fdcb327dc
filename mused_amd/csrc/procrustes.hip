// Orthogonal Procrustes on the device (specification: mused_amd/procrustes.py): the orthogonal R that best carries the rows of
// A (m x r) onto the rows of B (m x r), R = polar factor of M = A^T B, and the product E R of a whole window with it.
//
//   mused_procrustes        M = A^T B by the library's split-K GEMM (tiny r x r output, long K = m; partials summed in split
//                           order), then procrustes_svd_kernel
//   mused_svd_jacobi_small  procrustes_svd_kernel alone: W = M V and the column norms (for tests)
//   mused_procrustes_apply  out = E R for all n rows, fused with |A R - B|^2, |B|^2, |A - B|^2 over the first m rows
//
// procrustes_svd_kernel.  One workgroup of 16 waves.  M lives in LDS column by column, column j at j * P with P = r | 1: the
// Jacobi reads and writes whole columns (contiguous: conflict free at any pitch), the products behind it read one row of many
// columns at once (stride P doubles: an odd pitch keeps the 64-bank stride of P = 128 away).  One-sided (Hestenes) Jacobi on
// the columns: a sweep is the n2 - 1 steps of the round-robin schedule (n2 = r rounded up to even; with r odd the pair that
// holds column r is the step's bye), the n2 / 2 disjoint pairs of a step are dealt to the waves, a wave owns its pair's two
// columns (rows l and l + 64 in lane l), takes the three dot products by wave reductions and rotates when
// (w_p.w_q)^2 > 2^-100 (w_p.w_p)(w_q.w_q).  Steps are separated by LDS-only barriers.  A sweep in which no wave rotated --
// every wave's ballot, exchanged through one LDS word a wave -- is the last; at most 30 sweeps.  Then sigma_j = |w_j|,
// U = W / sigma, T = (U^T M) / sigma (= V^T; M is read again from global memory), R0 = U T, one Newton-Schulz step
// R = 1/2 R0 (3 I - R0^T R0).  The three intermediate r x r matrices pass through global scratch (the workgroup's own L1; LDS
// holds one matrix at r = 128).  Every sum has a fixed order: two calls give the same bits.
//
// procrustes_apply_kernel.  R in LDS; a workgroup walks 16-row tiles of E (staged in LDS, each wave 4 rows, lane l columns
// l and l + 64), keeps its three sums in registers and leaves them as one partial; procrustes_sums_kernel adds the partials
// in index order.  No floating-point atomic.
#include "trd_common.h"

namespace mused {

constexpr int PR_MAX_R = 128;
constexpr int PR_THREADS = 1024, PR_WAVES = PR_THREADS / 64;
constexpr int PR_MAX_SWEEPS = 30;                                             // (mused_amd.procrustes.MAX_SWEEPS)
constexpr int PR_FLAG_NONFINITE = 2, PR_FLAG_ILLCOND = 4, PR_FLAG_NOCONV = 8;  // (mused_amd.procrustes.FLAG_*)
constexpr double PR_ROT_THRESHOLD = 7.888609052210118e-31;                    // 2^-100
constexpr double PR_ILLCOND_RATIO = 6.103515625e-05;                          // 2^-14
constexpr int PR_KCHUNK = 256;                                                // rows of A, B per split of the cross product
constexpr int PR_ROWS_PER_THREAD = PR_MAX_R / (PR_THREADS / PR_MAX_R);        // 16: the panel products' rows a thread
constexpr int PR_APPLY_THREADS = 256, PR_APPLY_ROWS = 16, PR_APPLY_MAX_WG = 1024;

__host__ __device__ constexpr int pr_pitch(int r) { return r | 1; }
static size_t pr_svd_lds_bytes(int r) { return (size_t)r * pr_pitch(r) * 8; }
static size_t pr_apply_lds_bytes(int r) { return (size_t)(r + PR_APPLY_ROWS) * pr_pitch(r) * 8; }

struct PrWs {
  double* part;     // [PR_APPLY_MAX_WG][3]: mused_procrustes_apply's partial sums (FIRST: that entry takes the same workspace)
  double* M;        // [r][r]
  double* scratch;  // [3][r][r]: T, R0, H
  double* partial;  // [splits][r][r]
};

static size_t pr_layout(long m, int r, char* base, PrWs* ws) {
  PrWs sizing;
  PrWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  w.part = c.take<double>(3 * PR_APPLY_MAX_WG);
  w.M = c.take<double>((size_t)r * r);
  w.scratch = c.take<double>(3 * (size_t)r * r);
  w.partial = c.take<double>((size_t)cdiv(m, PR_KCHUNK) * r * r);
  return c.off;
}

static bool pr_shape_ok(long m, int r) { return m >= 1 && m < (1l << 30) && r >= 1 && r <= PR_MAX_R; }

struct PrSvdArgs {
  const double* M;  // r x r, row-major, pitch ldm
  long ldm;
  int r;
  double* W_out;      // r x r row-major: M V (null: not wanted)
  double* sigma_out;  // r column norms of W, in column order (null: not wanted)
  double* R_out;      // r x r row-major (null: the SVD alone)
  double* scratch;    // 3 r^2 doubles (with R_out)
  double* out_f64;    // {scale, sigma_max, sigma_min, 0} (with R_out)
  int* info;          // {flags, sweeps, 0, 0}
};

// One r x r product of the kernel's tail: thread (g, k) = (t / 128, t % 128) computes column k of the rows g, g + 8, ... of
// out[row][k] = sum_x left(row, x) * right(x, k).  left() reads LDS at an address the wave shares (a broadcast), right() is
// the thread's own column: one load a term for 16 multiply-adds.
template <typename FL, typename FR, typename FO>
__device__ __forceinline__ void pr_panel(int r, FL left, FR right, FO store) {
  const int k = threadIdx.x & (PR_MAX_R - 1), g = threadIdx.x >> 7;
  if (k >= r) return;  // (no barrier inside)
  double acc[PR_ROWS_PER_THREAD];
#pragma unroll
  for (int j = 0; j < PR_ROWS_PER_THREAD; ++j) acc[j] = 0.0;
  for (int x = 0; x < r; ++x) {
    const double rv = right(x, k);
#pragma unroll
    for (int j = 0; j < PR_ROWS_PER_THREAD; ++j) {
      const int row = g + 8 * j;
      if (row < r) acc[j] = fma(left(row, x), rv, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < PR_ROWS_PER_THREAD; ++j) {
    const int row = g + 8 * j;
    if (row < r) store(row, k, acc[j]);
  }
}

__global__ __launch_bounds__(PR_THREADS) void procrustes_svd_kernel(const PrSvdArgs a) {
  extern __shared__ __attribute__((aligned(16))) double Wl[];  // r columns of P doubles
  __shared__ double sig[PR_MAX_R];
  __shared__ int wrot[PR_WAVES];
  const int r = a.r, P = pr_pitch(r), rr = r * r;
  const int t = threadIdx.x, w = __builtin_amdgcn_readfirstlane(t >> 6), l = t & 63;

  int bad = 0;
  for (int e = t; e < rr; e += PR_THREADS) {
    const int i = e / r, j = e - i * r;
    const double v = a.M[(long)i * a.ldm + j];
    bad |= !(fabs(v) <= 1.7976931348623157e308);
    Wl[j * P + i] = v;
  }
  if (__syncthreads_or(bad)) {  // (uniform) nothing is computed
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (t < 4) {
      a.info[t] = t == 0 ? PR_FLAG_NONFINITE : 0;
      if (a.out_f64) a.out_f64[t] = t == 3 ? 0.0 : nan;
    }
    return;
  }

  // ---- the sweeps ----
  const int n2 = r + (r & 1), nm = n2 - 1, half = n2 >> 1;
  const bool h0 = l < r, h1 = l + 64 < r;
  int sweeps = 0;
  bool again = true;
  while (again && sweeps < PR_MAX_SWEEPS) {
    ++sweeps;
    bool rot = false;
    for (int s = 0; s < nm; ++s) {
      for (int k = w; k < half; k += PR_WAVES) {  // (k, hence the pair, is the wave's: no divergence below)
        int x = s + k, y = s - k;                 // (s + k) mod nm, (s - k) mod nm: k < half <= nm
        x = x >= nm ? x - nm : x;
        y = y < 0 ? y + nm : y;
        if (k == 0) x = s, y = nm;
        const int p = min(x, y), q = max(x, y);
        if (q >= r) continue;  // the bye of an odd r
        double* cp = Wl + p * P;
        double* cq = Wl + q * P;
        const double x0 = h0 ? cp[l] : 0.0, x1 = h1 ? cp[l + 64] : 0.0;
        const double y0 = h0 ? cq[l] : 0.0, y1 = h1 ? cq[l + 64] : 0.0;
        const double aa = wave_allsum(fma(x1, x1, x0 * x0));
        const double bb = wave_allsum(fma(y1, y1, y0 * y0));
        const double cc = wave_allsum(fma(x1, y1, x0 * y0));
        // (the sums are the same bits in every lane: the branch is the wave's.  A branch-free variant with the wave's four
        // pairs side by side was measured slower -- 2.9 against 1.3 ms at r = 50, equal at r = 128: the step is bound by the
        // number of vector instructions, which every lane spends on the same rotation, not by their latency)
        if (cc * cc > PR_ROT_THRESHOLD * aa * bb) {
          rot = true;
          const double zeta = (bb - aa) / (2.0 * cc);
          const double tt = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
          if (h0) {
            cp[l] = cs * x0 - sn * y0;
            cq[l] = sn * x0 + cs * y0;
          }
          if (h1) {
            cp[l + 64] = cs * x1 - sn * y1;
            cq[l + 64] = sn * x1 + cs * y1;
          }
        }
      }
      lds_barrier();  // the next step pairs these columns with others
    }
    // Did any wave rotate?  A word a wave; a wave writes its word again only behind the next sweep's first step barrier,
    // which no wave passes before every wave has read the words here.
    const bool wave_rot = __ballot(rot) != 0ull;
    if (l == 0) wrot[w] = wave_rot ? 1 : 0;
    lds_barrier();
    int any = 0;
#pragma unroll
    for (int i = 0; i < PR_WAVES; ++i) any |= wrot[i];
    again = any != 0;
  }

  // ---- sigma_j = |w_j| ----
  for (int j = w; j < r; j += PR_WAVES) {
    const double x0 = h0 ? Wl[j * P + l] : 0.0, x1 = h1 ? Wl[j * P + l + 64] : 0.0;
    const double s2 = wave_allsum(fma(x1, x1, x0 * x0));
    if (l == 0) sig[j] = sqrt(s2);
  }
  __syncthreads();
  double smax = 0.0, smin = 1.7976931348623157e308, scale = 0.0;  // (every thread: the same loop, the same bits)
  for (int j = 0; j < r; ++j) {
    const double sj = sig[j];
    smax = fmax(smax, sj);
    smin = fmin(smin, sj);
    scale += sj;
  }
  int flags = again ? PR_FLAG_NOCONV : 0;
  if (!(smax > 0.0) || smin <= PR_ILLCOND_RATIO * smax) flags |= PR_FLAG_ILLCOND;
  if (t < 4) a.info[t] = t == 0 ? flags : (t == 1 ? sweeps : 0);
  if (a.W_out)
    for (int e = t; e < rr; e += PR_THREADS) {
      const int i = e / r, j = e - i * r;
      a.W_out[e] = Wl[j * P + i];
    }
  if (a.sigma_out && t < r) a.sigma_out[t] = sig[t];
  if (!a.R_out) return;
  if (t == 0) {
    a.out_f64[0] = scale;
    a.out_f64[1] = smax;
    a.out_f64[2] = smin;
    a.out_f64[3] = 0.0;
  }

  // ---- R0 = U (U^T M / sigma), R = 1/2 R0 (3 I - R0^T R0) ----
  double* Tg = a.scratch;
  double* R0g = Tg + rr;
  double* Hg = R0g + rr;
  for (int e = t; e < rr; e += PR_THREADS) {  // U = W / sigma (a zero column stays zero: flagged above)
    const int j = e / r, i = e - j * r;
    const double sj = sig[j];
    Wl[j * P + i] = Wl[j * P + i] / (sj > 0.0 ? sj : 1.0);
  }
  __syncthreads();
  // T[j][k] = (sum_i U[i][j] M[i][k]) / sigma_j
  pr_panel(
      r, [&](int j, int i) { return Wl[j * P + i]; }, [&](int i, int k) { return a.M[(long)i * a.ldm + k]; },
      [&](int j, int k, double v) { Tg[j * r + k] = v / (sig[j] > 0.0 ? sig[j] : 1.0); });
  __threadfence_block();
  __syncthreads();  // (global stores of this workgroup, read by this workgroup)
  // R0[i][k] = sum_j U[i][j] T[j][k]
  pr_panel(
      r, [&](int i, int j) { return Wl[j * P + i]; }, [&](int j, int k) { return Tg[j * r + k]; },
      [&](int i, int k, double v) { R0g[i * r + k] = v; });
  __threadfence_block();
  __syncthreads();  // U has been read: its place takes R0, row i at i * P
  for (int e = t; e < rr; e += PR_THREADS) {
    const int i = e / r, k = e - i * r;
    Wl[i * P + k] = R0g[e];
  }
  __syncthreads();
  // H[a][b] = 1/2 (3 [a == b] - sum_i R0[i][a] R0[i][b])
  pr_panel(
      r, [&](int ca, int i) { return Wl[i * P + ca]; }, [&](int i, int cb) { return Wl[i * P + cb]; },
      [&](int ca, int cb, double v) { Hg[ca * r + cb] = 0.5 * ((ca == cb ? 3.0 : 0.0) - v); });
  __threadfence_block();
  __syncthreads();
  // R[i][b] = sum_a R0[i][a] H[a][b]
  pr_panel(
      r, [&](int i, int ca) { return Wl[i * P + ca]; }, [&](int ca, int cb) { return Hg[ca * r + cb]; },
      [&](int i, int cb, double v) { a.R_out[i * r + cb] = v; });
}

struct PrApplyArgs {
  const double* E;  // n x r, pitch lde
  long lde;
  int n, r;
  const double* R;  // r x r row-major
  double* out;      // n x r, pitch ldo
  long ldo;
  const double* Bref;  // m x r, pitch ldb (null: no sums)
  long ldb;
  int m;
  double* part;  // [gridDim.x][3]
};

__global__ __launch_bounds__(PR_APPLY_THREADS) void procrustes_apply_kernel(const PrApplyArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double wsum[PR_APPLY_THREADS / 64][3];
  const int r = a.r, P = pr_pitch(r);
  double* Rl = sm;           // row j of R at j * P
  double* Es = sm + r * P;   // row i of the tile at i * P
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const bool h0 = l < r, h1 = l + 64 < r;
  for (int e = t; e < r * r; e += PR_APPLY_THREADS) {
    const int j = e / r, k = e - j * r;
    Rl[j * P + k] = a.R[e];
  }
  double s_res = 0.0, s_b = 0.0, s_un = 0.0;
  const int tiles = (a.n + PR_APPLY_ROWS - 1) / PR_APPLY_ROWS;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int i0 = tile * PR_APPLY_ROWS;
    __syncthreads();  // R is staged / the tile before has been read
    for (int e = t; e < PR_APPLY_ROWS * r; e += PR_APPLY_THREADS) {
      const int i = e / r, k = e - i * r;
      Es[i * P + k] = i0 + i < a.n ? a.E[(long)(i0 + i) * a.lde + k] : 0.0;
    }
    __syncthreads();
    double acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = 0.0;
    const double* er = Es + (4 * w) * P;
    for (int j = 0; j < r; ++j) {
      const double r0 = h0 ? Rl[j * P + l] : 0.0, r1 = h1 ? Rl[j * P + l + 64] : 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double ev = er[i * P + j];
        acc[i][0] = fma(ev, r0, acc[i][0]);
        acc[i][1] = fma(ev, r1, acc[i][1]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = i0 + 4 * w + i;
      if (row >= a.n) continue;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int k = l + 64 * c;
        if (k >= r) continue;
        a.out[(long)row * a.ldo + k] = acc[i][c];
        if (a.Bref && row < a.m) {
          const double bv = a.Bref[(long)row * a.ldb + k], ev = er[i * P + k];
          const double dr = acc[i][c] - bv, du = ev - bv;
          s_res = fma(dr, dr, s_res);
          s_b = fma(bv, bv, s_b);
          s_un = fma(du, du, s_un);
        }
      }
    }
  }
  s_res = wave_allsum(s_res);
  s_b = wave_allsum(s_b);
  s_un = wave_allsum(s_un);
  if (l == 0) {
    wsum[w][0] = s_res;
    wsum[w][1] = s_b;
    wsum[w][2] = s_un;
  }
  __syncthreads();
  if (t < 3) {
    double s = 0.0;
    for (int ww = 0; ww < PR_APPLY_THREADS / 64; ++ww) s += wsum[ww][t];
    a.part[blockIdx.x * 3 + t] = s;
  }
}

// sums[c] = part[0][c] + part[1][c] + ...: lane l adds the partials l, l + 64, ... in that order, then the wave's tree
__global__ __launch_bounds__(64) void procrustes_sums_kernel(const double* __restrict__ part, int count, double* __restrict__ sums) {
  const int l = threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = l; i < count; i += 64)
    for (int c = 0; c < 3; ++c) s[c] += part[i * 3 + c];
  for (int c = 0; c < 3; ++c) s[c] = wave_allsum(s[c]);
  if (l < 3) sums[l] = l == 0 ? s[0] : (l == 1 ? s[1] : s[2]);
}

static int pr_svd_launch(const PrSvdArgs& a, hipStream_t st) {
  static LdsOptIn opt;
  MUSED_CHECK_HIP(allow_dynamic_lds(opt, reinterpret_cast<const void*>(procrustes_svd_kernel), pr_svd_lds_bytes(PR_MAX_R)));
  hipLaunchKernelGGL(procrustes_svd_kernel, dim3(1), dim3(PR_THREADS), pr_svd_lds_bytes(a.r), st, a);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// do [p, p + (rows - 1) ld + r) and [q, ...) share a double?
static bool pr_overlap(const double* p, long ldp, const double* q, long ldq, long rows, int r) {
  const double* pe = p + (rows - 1) * ldp + r;
  const double* qe = q + (rows - 1) * ldq + r;
  return p < qe && q < pe;
}

}  // namespace mused

using namespace mused;

extern "C" {

// bytes of workspace mused_procrustes needs (-1: m < 1, m >= 2^30 or r outside [1, 128])
long mused_procrustes_ws_bytes(long m, int r) {
  if (!pr_shape_ok(m, r)) return -1;
  return (long)pr_layout(m, r, nullptr, nullptr);
}

int mused_procrustes(const double* A, long lda, const double* B, long ldb, long m, int r, double* R_out, double* out_f64,
                     int* info_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(A && B && R_out && out_f64 && info_out && ws, "mused_procrustes: null argument");
  if (r > PR_MAX_R) {  // before any launch: the caller's host path takes it
    set_error("mused_procrustes: r = %d exceeds %d columns (one matrix in one CU's LDS)", r, PR_MAX_R);
    return MUSED_ERR_UNSUPPORTED;
  }
  MUSED_REQUIRE(pr_shape_ok(m, r) && lda >= r && ldb >= r, "mused_procrustes: bad shape (m=%ld r=%d lda=%ld ldb=%ld)", m, r, lda, ldb);
  MUSED_REQUIRE(ws_bytes >= (long)pr_layout(m, r, nullptr, nullptr), "mused_procrustes: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  PrWs w;
  pr_layout(m, r, (char*)ws, &w);
  const int nsplit = cdiv(m, PR_KCHUNK);
  int rc;
  // A and B are stored [K = m][r]: neither operand is K-contiguous
  if ((rc = gemm_f64_splitk(false, false, A, lda, B, ldb, w.partial, r, r, (int)m, PR_KCHUNK, nsplit, st))) return rc;
  if ((rc = gemm_splitk_reduce(w.partial, nsplit, (long)r * r, w.M, st))) return rc;
  const PrSvdArgs a{w.M, r, r, nullptr, nullptr, R_out, w.scratch, out_f64, info_out};
  return pr_svd_launch(a, st);
}

int mused_svd_jacobi_small(const double* M, long ldm, int r, double* W_out, double* sigma_out, int* info_out, void* stream) {
  MUSED_REQUIRE(M && W_out && sigma_out && info_out, "mused_svd_jacobi_small: null argument");
  if (r > PR_MAX_R) {
    set_error("mused_svd_jacobi_small: r = %d exceeds %d columns", r, PR_MAX_R);
    return MUSED_ERR_UNSUPPORTED;
  }
  MUSED_REQUIRE(r >= 1 && ldm >= r, "mused_svd_jacobi_small: bad shape (r=%d ldm=%ld)", r, ldm);
  const PrSvdArgs a{M, ldm, r, W_out, sigma_out, nullptr, nullptr, nullptr, info_out};
  return pr_svd_launch(a, (hipStream_t)stream);
}

int mused_procrustes_apply(const double* E, long lde, long n, int r, const double* R, double* out, long ldo, const double* Bref,
                           long ldb, long m, double* sums_out, void* ws, void* stream) {
  MUSED_REQUIRE(E && R && out && ws, "mused_procrustes_apply: null argument");
  if (r > PR_MAX_R) {
    set_error("mused_procrustes_apply: r = %d exceeds %d columns", r, PR_MAX_R);
    return MUSED_ERR_UNSUPPORTED;
  }
  MUSED_REQUIRE(n >= 1 && n < (1l << 30) && r >= 1 && lde >= r && ldo >= r, "mused_procrustes_apply: bad shape (n=%ld r=%d lde=%ld ldo=%ld)",
                n, r, lde, ldo);
  MUSED_REQUIRE(!Bref || (sums_out && m >= 1 && m <= n && ldb >= r), "mused_procrustes_apply: bad reference rows (m=%ld ldb=%ld)", m, ldb);
  MUSED_REQUIRE(!pr_overlap(E, lde, out, ldo, n, r), "mused_procrustes_apply: out must not alias E");
  hipStream_t st = (hipStream_t)stream;
  static LdsOptIn opt;
  MUSED_CHECK_HIP(allow_dynamic_lds(opt, reinterpret_cast<const void*>(procrustes_apply_kernel), pr_apply_lds_bytes(PR_MAX_R)));
  const int tiles = cdiv(n, PR_APPLY_ROWS), grid = tiles < PR_APPLY_MAX_WG ? tiles : PR_APPLY_MAX_WG;
  const PrApplyArgs a{E, lde, (int)n, r, R, out, ldo, Bref, ldb, Bref ? (int)m : 0, (double*)ws};
  hipLaunchKernelGGL(procrustes_apply_kernel, dim3(grid), dim3(PR_APPLY_THREADS), pr_apply_lds_bytes(r), st, a);
  if (Bref) hipLaunchKernelGGL(procrustes_sums_kernel, dim3(1), dim3(64), 0, st, (const double*)ws, grid, sums_out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
