// Plain fp64 GEMM launchers on top of gemm_f64.h + library-wide error string.
#include <stdarg.h>

#include "gemm_f64.h"
#include "internal.h"

namespace mused {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

const char* last_error() { return g_err; }

int gemm_f64_prepare_all() {
  int rc = 0;
#define PREP(a, b, v) rc |= gemm_f64_prepare_t<double, double, a, b, v, EpiStore>()
  PREP(true, true, true); PREP(true, true, false); PREP(true, false, true); PREP(true, false, false);
  PREP(false, true, true); PREP(false, true, false); PREP(false, false, true); PREP(false, false, false);
#undef PREP
#define PREP(a, b, v) rc |= gemm_f64_prepare_t<double, double, a, b, v, EpiStore, true>()
  PREP(true, true, true); PREP(true, true, false); PREP(true, false, true); PREP(true, false, false);
#undef PREP
  rc |= gemm_f64_prepare_t<double, double, true, true, true, EpiStore, false, true>();
  rc |= gemm_f64_prepare_t<double, double, true, true, false, EpiStore, false, true>();
  rc |= gemm_f64_prepare_t<float, float, true, true, true, EpiStore, false, true>();
  rc |= gemm_f64_prepare_t<float, float, true, true, false, EpiStore, false, true>();
  return rc ? MUSED_ERR_HIP : MUSED_OK;
}

// The operands a tail applies to (see GemmTail), checked; vec: whether the tail rows keep the 16-byte loads.
static int gemm_set_tail(GemmArgs& g, const GemmTail& t, bool a_kc, bool b_kc, long ld, bool& vec) {
  MUSED_REQUIRE(t.rows && t.split && t.zero_row && t.per_lane >= 1 && t.pend >= 0, "gemm_f64: bad tail");
  MUSED_REQUIRE(a_kc && (!b_kc || g.sym), "gemm_f64: a tail needs a Gram launch or a K-rows operand B");
  g.tail = t.rows; g.tail_stride = t.lane_stride; g.tail_per = t.per_lane;
  g.tail_split = t.split; g.tail_split_stride = t.split_stride; g.tail_pend = t.pend; g.tail_zero = t.zero_row;
  if (g.sym && t.plain_diag) g.sym = 3;
  if (t.fill) {
    MUSED_REQUIRE(g.sym && !g.bsplit && !g.splitk && t.fill_ld >= t.pend, "gemm_f64: a fill source needs a Gram launch that is not split over K");
    g.fill = t.fill; g.fill_stride = t.fill_stride; g.fill_ld = t.fill_ld;
  }
  vec = vec && vec_ok<double>(t.rows, ld, t.lane_stride) && vec_ok<double>(t.zero_row, ld, 0);
  return MUSED_OK;
}

int gemm_f64(bool a_kc, bool b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
             long strideB, double* C, long ldc, long strideC, int M, int N, int K, int batch, double alpha,
             hipStream_t stream, const int* rep, const int* list, const int* kact, const GemmTail* tail) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = B; g.lda = lda; g.ldb = ldb; g.strideA = strideA; g.strideB = strideB;
  g.M = M; g.N = N; g.K = K; g.splitk = 0; g.kchunk = 0;
  g.rep = rep; g.list = list; g.kact = kact;
  // Gram products (A A^T: same operand, same layout, square result): tiles on or above the diagonal + mirrored stores
  g.sym = (A == B && a_kc == b_kc && lda == ldb && strideA == strideB && M == N) ? 1 : 0;
  EpiStore epi{C, ldc, strideC, alpha};
  bool vec = vec_ok<double>(A, lda, strideA) && vec_ok<double>(B, ldb, strideB);
  if (tail) {
    int rc;
    if ((rc = gemm_set_tail(g, *tail, a_kc, b_kc, ldb, vec))) return rc;
    if (b_kc) return gemm_f64_launch_t<double, double, true, true, EpiStore, true>(g, batch, epi, vec, stream);
    return gemm_f64_launch_t<double, double, true, false, EpiStore, true>(g, batch, epi, vec, stream);
  }
  if (a_kc && b_kc) return gemm_f64_launch_t<double, double, true, true>(g, batch, epi, vec, stream);
  if (a_kc && !b_kc) return gemm_f64_launch_t<double, double, true, false>(g, batch, epi, vec, stream);
  if (!a_kc && b_kc) return gemm_f64_launch_t<double, double, false, true>(g, batch, epi, vec, stream);
  return gemm_f64_launch_t<double, double, false, false>(g, batch, epi, vec, stream);
}

int gemm_gram_rows(const void* A, bool f32, long lda, long strideA, int per_group, long group_stride, double* C, long ldc,
                   long strideC, int M, int K, int batch, int plain_diag, hipStream_t stream) {
  MUSED_REQUIRE(per_group >= 1 && ldc >= M, "gemm_gram_rows: bad arguments");
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = A; g.lda = lda; g.ldb = lda; g.strideA = strideA; g.strideB = strideA;
  g.M = M; g.N = M; g.K = K;
  g.sym = plain_diag ? 3 : 1;
  g.grp_per = per_group; g.grp_stride = group_stride;
  EpiStore epi{C, ldc, strideC, 1.0};
  if (f32) {
    const bool vec = vec_ok<float>(A, lda, strideA) && group_stride % 4 == 0;
    return gemm_f64_launch_t<float, float, true, true, EpiStore, false, true>(g, batch, epi, vec, stream);
  }
  const bool vec = vec_ok<double>(A, lda, strideA) && group_stride % 2 == 0;
  return gemm_f64_launch_t<double, double, true, true, EpiStore, false, true>(g, batch, epi, vec, stream);
}

int gemm_f64_splitk(bool a_kc, bool b_kc, const double* A, long lda, const double* B, long ldb, double* partial,
                    int M, int N, int K, int kchunk, int nsplit, hipStream_t stream) {
  MUSED_REQUIRE(kchunk > 0 && kchunk % GEMM_BK == 0 && nsplit >= 1 && (long)kchunk * nsplit >= K,
                "gemm_f64_splitk: bad kchunk %d x %d for K=%d", kchunk, nsplit, K);
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = B; g.lda = lda; g.ldb = ldb;
  g.M = M; g.N = N; g.K = K; g.splitk = 1; g.kchunk = kchunk;
  EpiStore epi{partial, (long)N, (long)M * N, 1.0};
  const bool vec = vec_ok<double>(A, lda, 0) && vec_ok<double>(B, ldb, 0);
  if (a_kc && b_kc) return gemm_f64_launch_t<double, double, true, true>(g, nsplit, epi, vec, stream);
  if (a_kc && !b_kc) return gemm_f64_launch_t<double, double, true, false>(g, nsplit, epi, vec, stream);
  if (!a_kc && b_kc) return gemm_f64_launch_t<double, double, false, true>(g, nsplit, epi, vec, stream);
  return gemm_f64_launch_t<double, double, false, false>(g, nsplit, epi, vec, stream);
}

__global__ void splitk_reduce_kernel(const double* __restrict__ partial, int nsplit, long count,
                                     double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  double s = 0.0;
  for (int z = 0; z < nsplit; ++z) s += partial[(long)z * count + i];  // fixed order: reproducible
  out[i] = s;
}

// Batched split-K: partial[(z * nsplit + sp)] (M x N each, ld = N) = opA(A[z]) opB(B[z]) over k in [sp * kchunk, (sp + 1) * kchunk);
// entries with rep[z] != z are skipped.  Sum with gemm_batched_splitk_reduce (fixed split order: results do not depend on the
// batch).  For products whose K loop is long and whose tiles do not fill the GPU (sketch Gram matrices at d = 10,000).
int gemm_f64_batched_splitk(bool a_kc, bool b_kc, const double* A, long lda, long strideA, const double* B, long ldb, long strideB,
                            double* partial, int M, int N, int K, int batch, int kchunk, int nsplit, hipStream_t stream,
                            const int* rep, const int* list, const GemmTail* tail) {
  MUSED_REQUIRE(kchunk > 0 && kchunk % GEMM_BK == 0 && nsplit >= 1 && (long)kchunk * nsplit >= K,
                "gemm_f64_batched_splitk: bad kchunk %d x %d for K=%d", kchunk, nsplit, K);
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = B; g.lda = lda; g.ldb = ldb; g.strideA = strideA; g.strideB = strideB;
  g.M = M; g.N = N; g.K = K; g.splitk = 0; g.kchunk = kchunk; g.bsplit = nsplit;
  g.rep = rep; g.list = list;
  g.sym = (A == B && a_kc == b_kc && lda == ldb && strideA == strideB && M == N) ? 1 : 0;
  EpiStore epi{partial, (long)N, (long)M * N, 1.0};
  bool vec = vec_ok<double>(A, lda, strideA) && vec_ok<double>(B, ldb, strideB);
  if (tail) {
    int rc;
    if ((rc = gemm_set_tail(g, *tail, a_kc, b_kc, ldb, vec))) return rc;
    if (b_kc) return gemm_f64_launch_t<double, double, true, true, EpiStore, true>(g, batch * nsplit, epi, vec, stream);
    return gemm_f64_launch_t<double, double, true, false, EpiStore, true>(g, batch * nsplit, epi, vec, stream);
  }
  if (a_kc && b_kc) return gemm_f64_launch_t<double, double, true, true>(g, batch * nsplit, epi, vec, stream);
  if (a_kc && !b_kc) return gemm_f64_launch_t<double, double, true, false>(g, batch * nsplit, epi, vec, stream);
  if (!a_kc && b_kc) return gemm_f64_launch_t<double, double, false, true>(g, batch * nsplit, epi, vec, stream);
  return gemm_f64_launch_t<double, double, false, false>(g, batch * nsplit, epi, vec, stream);
}

__global__ void batched_splitk_reduce_kernel(const double* __restrict__ partial, int nsplit, long count, double* __restrict__ out,
                                             const int* __restrict__ rep, const int* __restrict__ list) {
  int z = blockIdx.y;
  if (list) {
    if (z >= list[0]) return;
    z = list[1 + z];
  } else if (rep && rep[z] != z) return;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const double* p = partial + (long)z * nsplit * count + i;
  double s = 0.0;
  for (int sp = 0; sp < nsplit; ++sp) s += p[(long)sp * count];  // fixed order: reproducible
  out[(long)z * count + i] = s;
}

int gemm_batched_splitk_reduce(const double* partial, int nsplit, long count, double* out, int batch, const int* rep,
                               hipStream_t stream, const int* list) {
  hipLaunchKernelGGL(batched_splitk_reduce_kernel, dim3(cdiv(count, 256), batch), dim3(256), 0, stream, partial, nsplit, count, out,
                     rep, list);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

int gemm_splitk_reduce(const double* partial, int nsplit, long count, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(cdiv(count, 256)), dim3(256), 0, stream, partial, nsplit, count,
                     out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // namespace mused

extern "C" {

const char* mused_last_error(void) { return mused::last_error(); }

int mused_version(void) { return 100; }

// Async device-to-device copy on `stream` (host code that only has raw pointers uses this).
int mused_memcpy_d2d(void* dst, const void* src, long bytes, void* stream) {
  MUSED_REQUIRE(dst && src && bytes >= 0, "mused_memcpy_d2d: bad arguments");
  MUSED_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MUSED_OK;
}

// Test/diagnostic entry: C = alpha * op(A) op(B), fp64.
int mused_gemm_f64(int a_kc, int b_kc, const double* A, long lda, const double* B, long ldb, double* C, long ldc,
                   int M, int N, int K, double alpha, void* stream) {
  return mused::gemm_f64(a_kc != 0, b_kc != 0, A, lda, 0, B, ldb, 0, C, ldc, 0, M, N, K, 1, alpha,
                         (hipStream_t)stream);
}

int mused_gemm_f64_batched(int a_kc, int b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
                           long strideB, double* C, long ldc, long strideC, int M, int N, int K, int batch,
                           double alpha, void* stream) {
  return mused::gemm_f64(a_kc != 0, b_kc != 0, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, M, N, K, batch,
                         alpha, (hipStream_t)stream);
}

// Test/diagnostic entries for the launch modes the library uses internally (split-K, duplicate skipping).
int mused_gemm_f64_batched_rep(int a_kc, int b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
                               long strideB, double* C, long ldc, long strideC, int M, int N, int K, int batch,
                               double alpha, const int* rep, void* stream) {
  return mused::gemm_f64(a_kc != 0, b_kc != 0, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, M, N, K, batch,
                         alpha, (hipStream_t)stream, rep);
}

// The same with a compacted list (list[0] = count, list[1 ..] = entries; see GemmArgs) and / or a K bound per entry.
int mused_debug_gemm_f64_batched_active(int a_kc, int b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
                                        long strideB, double* C, long ldc, long strideC, int M, int N, int K, int batch,
                                        double alpha, const int* list, const int* kact, void* stream) {
  return mused::gemm_f64(a_kc != 0, b_kc != 0, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, M, N, K, batch,
                         alpha, (hipStream_t)stream, nullptr, list, kact);
}

// The same with a second row segment (GemmTail in internal.h) for the operands built from sketch buffers; nsplit > 1: the
// batched split-K launch and its reduction (partial: batch x nsplit x M x N doubles), kact then unused.
int mused_debug_gemm_f64_batched_tail(int a_kc, int b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
                                      long strideB, double* C, long ldc, long strideC, int M, int N, int K, int batch,
                                      const int* list, const int* kact, const double* tail, long tail_stride, int per_lane,
                                      const int* split, int split_stride, int pend, const double* zero_row, int plain_diag, double* partial,
                                      int kchunk,
                                      int nsplit, void* stream) {
  MUSED_REQUIRE(A && B && C && tail && split && batch >= 1, "mused_debug_gemm_f64_batched_tail: bad arguments");
  const mused::GemmTail t{tail, tail_stride, per_lane, split, split_stride, pend, zero_row, plain_diag};
  if (nsplit <= 1)
    return mused::gemm_f64(a_kc != 0, b_kc != 0, A, lda, strideA, B, ldb, strideB, C, ldc, strideC, M, N, K, batch, 1.0,
                           (hipStream_t)stream, nullptr, list, kact, &t);
  MUSED_REQUIRE(partial && ldc == N && strideC == (long)M * N, "mused_debug_gemm_f64_batched_tail: split-K writes a dense C");
  int rc = mused::gemm_f64_batched_splitk(a_kc != 0, b_kc != 0, A, lda, strideA, B, ldb, strideB, partial, M, N, K, batch, kchunk,
                                          nsplit, (hipStream_t)stream, nullptr, list, &t);
  if (rc != MUSED_OK) return rc;
  return mused::gemm_batched_splitk_reduce(partial, nsplit, (long)M * N, C, batch, nullptr, (hipStream_t)stream, list);
}

// The Gram launch with a tail and a fill source (GemmTail::fill): tiles of tail rows and zero rows are copied from P P^T.
int mused_debug_gemm_f64_batched_tail_fill(const double* A, long lda, long strideA, double* C, long ldc, long strideC, int n, int K,
                                           int batch, const int* list, const double* tail, long tail_stride, int per_lane,
                                           const int* split, int split_stride, int pend, const double* zero_row, int plain_diag,
                                           const double* fill, long fill_stride, int fill_ld, void* stream) {
  MUSED_REQUIRE(A && C && tail && split && fill && batch >= 1, "mused_debug_gemm_f64_batched_tail_fill: bad arguments");
  const mused::GemmTail t{tail, tail_stride, per_lane, split, split_stride, pend, zero_row, plain_diag, fill, fill_stride, fill_ld};
  return mused::gemm_f64(true, true, A, lda, strideA, A, lda, strideA, C, ldc, strideC, n, n, K, batch, 1.0, (hipStream_t)stream,
                         nullptr, list, nullptr, &t);
}

// P P^T of row blocks read in place (gemm_gram_rows; dtype MUSED_F32 or MUSED_F64).
int mused_debug_gemm_gram_rows(const void* A, int dtype, long lda, long strideA, int per_group, long group_stride, double* C,
                               long ldc, long strideC, int M, int K, int batch, int plain_diag, void* stream) {
  MUSED_REQUIRE(A && C && batch >= 1 && (dtype == MUSED_F32 || dtype == MUSED_F64), "mused_debug_gemm_gram_rows: bad arguments");
  return mused::gemm_gram_rows(A, dtype == MUSED_F32, lda, strideA, per_group, group_stride, C, ldc, strideC, M, K, batch,
                               plain_diag, (hipStream_t)stream);
}

int mused_gemm_f64_splitk(int a_kc, int b_kc, const double* A, long lda, const double* B, long ldb, double* partial,
                          double* C, int M, int N, int K, int kchunk, int nsplit, void* stream) {
  MUSED_REQUIRE(A && B && partial && C && M >= 0 && N >= 0 && K >= 0, "mused_gemm_f64_splitk: bad arguments");
  int rc = mused::gemm_f64_splitk(a_kc != 0, b_kc != 0, A, lda, B, ldb, partial, M, N, K, kchunk, nsplit,
                                  (hipStream_t)stream);
  if (rc != MUSED_OK || M == 0 || N == 0) return rc;
  return mused::gemm_splitk_reduce(partial, nsplit, (long)M * N, C, (hipStream_t)stream);
}

int mused_gemm_f64_batched_splitk(int a_kc, int b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
                                  long strideB, double* partial, double* C, int M, int N, int K, int batch, int kchunk,
                                  int nsplit, const int* rep, void* stream) {
  MUSED_REQUIRE(A && B && partial && C && M >= 0 && N >= 0 && K >= 0 && batch >= 1,
                "mused_gemm_f64_batched_splitk: bad arguments");
  int rc = mused::gemm_f64_batched_splitk(a_kc != 0, b_kc != 0, A, lda, strideA, B, ldb, strideB, partial, M, N, K, batch,
                                          kchunk, nsplit, (hipStream_t)stream, rep);
  if (rc != MUSED_OK || M == 0 || N == 0) return rc;
  return mused::gemm_batched_splitk_reduce(partial, nsplit, (long)M * N, C, batch, rep, (hipStream_t)stream);
}

}  // extern "C"
