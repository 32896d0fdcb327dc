// Host-side entry points shared between translation units of libmused_hip.
#pragma once
#include "common.h"

#include <atomic>
#include <mutex>

// knn.hip (a C entry, include/mused_hip.h): out[i] = |x_i|^2, for the kernels that turn a tile of dot products into distances
extern "C" int mused_row_sq_norms(const void* X, int dtype, long n, int d, long ld, double* out, void* stream);

namespace mused {

// knn.hip: per-row selection of the k smallest scores computed on the fly (no n x n score matrix), see select_k_kernel
int select_from_records(const double* rec, int n, int kind, int k, int* out_idx, unsigned long long* out_mask,
                        int mask_words, hipStream_t stream);
int select_from_tag_sets(const int* rowptr, const int* tags, const int* postptr, const int* postrow, int n, int k,
                         int* out_idx, unsigned long long* out_mask, int mask_words, hipStream_t stream);
int select_max_fused_rows(bool tag_sets);
// the same selections for rows [s, e) of arrays that cover a whole stream, bitmask in window coordinates (meta_window.hip)
int select_window_records(const double* rec, const int* vrank, int s, int e, int kind, int k, unsigned long long* out_mask,
                          int mask_words, hipStream_t stream);
int select_window_tag_sets(const int* rowptr, const int* tags, const int* postptr, const int* postrow, const int* vrank, int s,
                           int e, int k, unsigned long long* out_mask, int mask_words, hipStream_t stream);

// One process-wide lock around every stream capture of this library AND around the calls that create or release HIP
// resources next to one (handle / plan creation and destruction: hipMalloc, hipFree, hipGraph(Exec)Destroy,
// hipStreamCreate / Destroy, allow_dynamic_lds below).  Round 2 locked only Begin..EndCapture; a handle re-created on one host
// thread then ran those calls beside another thread's capture (gpurun_out/r2_gputest23.log; tools/repro_capture_threads.hip
// asks the runtime which of them a ThreadLocal capture survives).  Recursive: creation paths nest (rsvd -> eig plan).
std::recursive_mutex& capture_mutex();
using CaptureLock = std::lock_guard<std::recursive_mutex>;

// The dynamic-LDS opt-in of one kernel instance (more than 64 KiB needs it once per kernel): the library's only call of
// hipFuncSetAttribute.  One LdsOptIn, static, per kernel instance.  A launch that finds `done` set takes no lock: it never
// waits behind another thread's capture.  The first caller takes capture_mutex() -- the ONLY lock involved -- checks again,
// sets the attribute, keeps the error (sticky) and publishes `done`.  No std::call_once around or inside: the prepare
// functions are reached both from plan creation, capture_mutex() held, and lazily from a solve, without it; with the mutex
// taken inside a once, thread B would sit in the once waiting for the mutex while thread A, holding the mutex, waits at the
// same once.  Here a caller that holds the mutex nests (recursive), one that does not waits for it and nothing else.
struct LdsOptIn {
  std::atomic<bool> done{false};
  hipError_t err = hipSuccess;
};
inline hipError_t allow_dynamic_lds(LdsOptIn& s, const void* kernel, size_t bytes) {
  if (!s.done.load(std::memory_order_acquire)) {
    CaptureLock lock(capture_mutex());
    if (!s.done.load(std::memory_order_relaxed)) {
      s.err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      s.done.store(true, std::memory_order_release);
    }
  }
  return s.err;
}
// several kernels behind one entry: the first failure wins, the kernels behind it are left alone
inline hipError_t allow_dynamic_lds(hipError_t before, LdsOptIn& s, const void* kernel, size_t bytes) {
  return before != hipSuccess ? before : allow_dynamic_lds(s, kernel, bytes);
}


// C[z] = alpha * opA(A[z]) * opB(B[z]); fp64 in / fp64 out, MFMA f64 16x16x4.
//   a_kc: A stored [M][K] (true) or [K][M] (false);  b_kc: B stored [N][K] (true) or [K][N] (false).
// A second row segment for operands built from sketch buffers (GemmArgs::tail in gemm_f64.h): with nk = split[z * split_stride],
// row r of entry z is the operand's row r below nk, row r - nk of rows + (z / per_lane) * lane_stride (the operand's pitch) below
// nk + pend, and +0.0 from there on (read from zero_row: as many doubles of +0.0 as an operand row is long).  It applies to both operands of a Gram launch (A == B, both K-contiguous) and to the
// K-rows operand B of an (a_kc, !b_kc) launch; other launches refuse it.
struct GemmTail {
  const double* rows;
  long lane_stride;
  int per_lane;
  const int* split;
  int split_stride;
  int pend;
  const double* zero_row;
  int plain_diag;  // 1: the diagonal tiles of this (Gram) launch run the ordinary main loop, as under MUSED_GEMM_SYM_DIAG=0 (tests)
  // optional, Gram launches that are not split over K: P P^T of every lane's tail rows (lane at fill + lane * fill_stride, leading
  // dimension fill_ld >= pend), from gemm_gram_rows on those rows.  Tiles that hold only tail rows and zero rows are copied
  // from it instead of computed (GemmArgs::fill): the same bits for finite operands.
  const double* fill;
  long fill_stride;
  int fill_ld;
};
int gemm_f64(bool a_kc, bool b_kc, const double* A, long lda, long strideA, const double* B, long ldb,
             long strideB, double* C, long ldc, long strideC, int M, int N, int K, int batch, double alpha,
             hipStream_t stream, const int* rep = nullptr, const int* list = nullptr, const int* kact = nullptr,
             const GemmTail* tail = nullptr);
// Gram products of row blocks read in place, fp32 (widened exactly) or fp64 rows: C[z] = P_z P_z^T (M x M, K = the row length) for
// z = group * per_group + e, P_z = the M rows at A + e * strideA + group * group_stride (elements), row pitch lda.  The tile
// order, K order and MFMA sequence of the symmetric launch of gemm_f64 (plain_diag as in GemmTail).
int gemm_gram_rows(const void* A, bool f32, long lda, long strideA, int per_group, long group_stride, double* C, long ldc,
                   long strideC, int M, int K, int batch, int plain_diag, hipStream_t stream);
// rep (device, batch ints, optional): entry z is computed only when rep[z] == z (duplicates are skipped)
// list (device, 1 + batch ints, optional, instead of rep): the entries to compute, compacted -- list[0] of them, list[1 ..];
//   workgroup z of the batch takes entry list[1 + z], so the workgroups with nothing to do are dispatched last
// kact (device, batch ints, optional): entry z multiplies over k < kact[z] (a multiple of 16 keeps the vector loads) -- both operands must be exact
//   zeros from there on, the result is then bit-identical to the full product

// batched split-K (see gemm_f64.hip): partial results per (entry, split), then the fixed-order sum
int gemm_f64_batched_splitk(bool a_kc, bool b_kc, const double* A, long lda, long strideA, const double* B, long ldb, long strideB,
                            double* partial, int M, int N, int K, int batch, int kchunk, int nsplit, hipStream_t stream,
                            const int* rep = nullptr, const int* list = nullptr, const GemmTail* tail = nullptr);
int gemm_batched_splitk_reduce(const double* partial, int nsplit, long count, double* out, int batch, const int* rep,
                               hipStream_t stream, const int* list = nullptr);
// Sets the dynamic-LDS attribute of every plain GEMM instantiation (call before stream capture).
int gemm_f64_prepare_all();

// Split-K variant for short-and-wide products (tiny M x N, long K): partial[z] for
// z < nsplit (each M x N, ld = N), then reduce with gemm_splitk_reduce.
int gemm_f64_splitk(bool a_kc, bool b_kc, const double* A, long lda, const double* B, long ldb, double* partial,
                    int M, int N, int K, int kchunk, int nsplit, hipStream_t stream);
int gemm_splitk_reduce(const double* partial, int nsplit, long count, double* out, hipStream_t stream);

// Y (n x r) <- P*L (first min(n,r) columns) ; pivstep: n + ceil(n/16) ints, prow: ws_f64_len doubles, at least
// r + ceil(n/16); with 4 (r + n) the blocked path runs (n <= 10240)
int lu_permute_l(double* Y, int n, int r, long ld, int* pivstep, double* prow, long ws_f64_len, hipStream_t st);
// Q (n x r) <- economic Householder Q of Y (destroyed); tau: r doubles, wpart: ceil(n/512)*r + 2 n doubles
// run_if (optional, device int): the whole chain is a no-op unless *run_if != 0 (fallback of the Cholesky-QR path)
int qr_economic(double* Y, int n, int r, long ldy, double* Q, long ldq, double* tau, double* wpart, hipStream_t st,
                const int* run_if = nullptr);
// Y = A Q for binary CSR A; col_sign (optional, r doubles of +-1): Y = A Q diag(col_sign), bit for bit
int spmm_binary(const int* rowptr, const int* colidx, int n, const double* Q, long ldq, int r, double* Y, long ldy,
                hipStream_t stream, const double* col_sign = nullptr);

// Y = S Q for CSR lists with one fp64 value per entry (spmm_valued.hip): acc = acc + (val * q), product rounded first, in
// list order from 0.0; the kernel choice and col_sign as for spmm_binary
int spmm_valued(const int* rowptr, const int* colidx, const double* vals, int n, const double* Q, long ldq, int r, double* Y,
                long ldy, hipStream_t stream, const double* col_sign = nullptr);

// adj_values.hip: where the values of CSR lists come from.  M >= 1: the weighted sum of M bitmasks p[0 .. M - 1] (weights w);
// M == 0: the dense matrix p[0] (dtype, row pitch ld)
constexpr int ADJ_VAL_MAX_M = 8;
struct AdjValSrc {
  const void* p[ADJ_VAL_MAX_M];
  double w[ADJ_VAL_MAX_M];
  long ld;
  int M, dtype;
};
// the C entries' HOST arrays / dense arguments, checked (MUSED_ERR_ARG, MUSED_ERR_UNSUPPORTED) -> *out; `who` names the entry
int adj_val_src_masks(const unsigned long long* const* masks, const double* weights, int M, AdjValSrc* out, const char* who);
int adj_val_src_dense(const void* dense, int dtype, int n, long ld, AdjValSrc* out, const char* who);
// *dst (device) = src, stream-ordered (the description travels in the launch, not through host memory)
int adj_val_src_store(const AdjValSrc& src, AdjValSrc* dst, hipStream_t st);
// vals[e] for every entry of the lists, the description read from DEVICE memory at run time (safe to record in a graph);
// a value that is not finite (bit 0 of *flag) or outside [2^-200, 2^200] in magnitude (bit 1) is flagged and stored as 1.0:
// nothing that could become a NaN inside the eigenstep reaches it (adj_values.hip, GUARD)
int adj_csr_values_dev(const AdjValSrc* src_dev, bool dense, int n, int words, const int* rowptr, const int* colidx,
                       int transposed, double* vals, int* flag, hipStream_t st);

// bitmask -> (deg, rowptr, colidx ascending); stats[0] = max degree, stats[1] = nnz; entries beyond
// `cap` (if cap > 0) are dropped and *overflow set.
int adj_csr_from_mask(const unsigned long long* mask, int n, int words, int* deg, int* rowptr, int* colidx,
                      int* stats, long cap, int* overflow, hipStream_t st);
int zero_ints(int* p, long n, hipStream_t st);
int adj_transpose(const unsigned long long* mask, int n, int words, unsigned long long* out, hipStream_t st);

// eig.hip: batched symmetric eigensolver for even orders up to 1024, fp64.  A plan fixes (order, batch, sweep cap) and, once,
// at creation, which kernels solve it: a one-sided block Jacobi (one persistent work-queue launch, or a hipGraph of
// launch-per-round sweeps), optionally behind a direct solver for the leading eigenpairs (trd.hip / trdx.hip) whose rejects
// the Jacobi takes.  The result lives in the plan as columns lam_j u_j (eig_plan_columns); eigenvectors are extracted on request.
struct EigPlan;
constexpr int EIG_PLAN_FIXED_SWEEPS = 1;  // always `sweeps` sweeps (no convergence flags)
constexpr int EIG_PLAN_NO_SORT = 2;       // no column sorting: column j of the result descends from column j of the input
constexpr int EIG_PLAN_TOP_HALF = 4;      // the caller reads only the n / 2 largest eigenpairs (FD rotation): orders a direct
                                          // solver covers go to it, the Jacobi takes what its certificate rejects
constexpr int EIG_PLAN_TOP_NEED = 8;      // the caller reads the `need` largest eigenpairs, ALL of which must be certified (eigenstep)
constexpr int EIG_PLAN_TOP_FD = 16;       // as TOP_HALF with an explicit `need` (sketch query: the l largest of 3 l or 4 l)
// own_graph: capture the Jacobi's launches into a private hipGraph (false when the caller captures a larger pipeline that
//   contains this solve).  MUSED_EIG_TRD, MUSED_EIG_QUEUE, MUSED_EIG_QUEUE_TIMEOUT_TICKS and MUSED_NO_GRAPH are read here, once
//   per call, and by no solve.  On failure nothing is left allocated and *out is not written.
// rep (device, batch ints, optional, read at every solve): matrix b is solved only when rep[b] == b
// err_out (device int, optional): OR-ed with 1 by a solve of the persistent work-queue solver that gave up waiting
//   (timeout: the matrices are left partially rotated and the results of that solve are invalid)
int eig_plan_create(int n, int batch, int sweeps, bool own_graph, EigPlan** out, const int* rep = nullptr, int flags = 0,
                    int* err_out = nullptr, int need = 0, const int* list = nullptr, const int* offs = nullptr);
// list (device, 1 + batch ints, optional, read at every solve; plans whose direct solver is trd.hip, ignored by the others):
//   list[0] = how many matrices have rep[b] == b, list[1 ..] = which; the solver's workgroups take their matrix from it
// offs (device, batch ints, optional, read at every solve; order 256 with trd.hip only): matrix b is zero from row and column
//   256 - offs[b] on and is solved at that order
void eig_plan_destroy(EigPlan* p);
// (batch x n x n) device buffer the caller fills with the symmetric matrices before eig_plan_run_inplace
double* eig_plan_input(EigPlan* p);
// Solves what eig_plan_input holds.  evals (batch x n, unsorted) and V (batch x n x n, column j <-> eigenvalue j) are
// extracted when evals is not null; allow_graph: replay the plan's private graph, if it has one.
int eig_plan_run_inplace(EigPlan* p, double* evals, double* V, hipStream_t stream, bool allow_graph);
// The same on a copy of G (batch x n x n, symmetric)
int eig_plan_run(EigPlan* p, const double* G, double* evals, double* V, hipStream_t stream);
// The result of the last solve as the solver leaves it: cols[(b * ld + j) * ld + a] = lam_j u_j[a], lam[b * ld + j] = eigenvalue j
struct EigColumns {
  const double *cols, *lam;
  int ld;
};
EigColumns eig_plan_columns(EigPlan* p);
bool eig_plan_direct_solver(EigPlan* p);  // the plan runs a direct solver (trd.hip / trdx.hip) with the Jacobi as its fallback
// Live timing (HIP events around every solve between profile(on) and a blocking read).  Plans without a direct solver:
// summed ms of the Jacobi, its launch rounds and the bytes one of them moves.  Plans with one: summed ms of the direct
// solver alone, its launches, the matrices it solved over all of them and the ms of its first kernel.
int eig_plan_profile(EigPlan* p, bool on);
int eig_plan_profile_read(EigPlan* p, double* total_ms, long* launches, double* bytes_per_launch);
int eig_plan_profile_read_direct(EigPlan* p, double* total_ms, long* launches, double* matrices_solved,
                                 double* tridiag_ms = nullptr);

// trd.hip: direct solver for orders <= 256, the `need` <= 128 largest eigenpairs (tridiagonalisation + multisection +
// twisted factorisation + back-transformation); matrices column-major with leading dimension ldn (n <= ldn <= 256)
size_t trd_workspace_doubles(int batch);
int trd_prepare();
bool trd_supports(int n, int ldn, int need);
// the order-256 tridiagonalisation alone (the blocked solver's tail): see trd.hip
long trd_tail_ws_per();
long trd_tail_off_hs();
long trd_tail_off_tg();
int trd_tail_launch(const double* G, const int* rep, double* ws, int batch, hipStream_t st);
int trd_solve(double* Gc, int n, int ldn, int need, bool cert_all, int batch, const int* rep, int* done, double* ws,
              hipStream_t st, long long* dbg_clk = nullptr, unsigned long long* work = nullptr, hipEvent_t after_a = nullptr,
              double* lam_out = nullptr,  // lam_out (batch x ldn, optional): eigenvalues of the solved matrices (zeros behind them)
              const int* list = nullptr,  // list (1 + batch ints, optional): the matrices to solve, compacted
              const int* offs = nullptr); // offs (batch ints, optional, n = ldn = 256): 256 - the order matrix b is solved at

// trdx.hip: blocked direct solver for padded orders 320, 384, 448, 512 (need rounded up to 32 <= order / 2)
bool trdx_supports(int ldn, int need);
size_t trdx_workspace_doubles(int ldn, int batch);
int trdx_prepare(int ldn);
int trdx_solve(double* Gc, int ldn, int need, bool cert_all, int batch, const int* rep, int* done, int* act, int* jrep,
               int* nrej, double* ws, hipStream_t st, unsigned long long* work = nullptr, hipEvent_t after_a = nullptr,
               long long* prof = nullptr,   // prof (device, batch x 4, diagnostic): s_memtime ticks per phase of kernel A
               double* lam_out = nullptr);  // lam_out (batch x ldn, optional): eigenvalues of the solved matrices

}  // namespace mused
