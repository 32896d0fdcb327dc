// The "text" modality's per-window TF-IDF (matrix_operations.py:91-110: TfidfVectorizer().fit_transform, then the
// normalisation cosine_similarity applies once more) from the integer arrays of a corpus that was tokenised once
// (mused_amd/text.py).  The rule, statement by statement: mused_amd/tfidf.py; scikit-learn's values bit for bit.
//
// Four launches on one stream; launch order is the only synchronisation between workgroups (nobody waits on anybody,
// nothing is accumulated through atomics -- the one atomicOr raises an error flag):
//   terms   one thread per GLOBAL term: two binary searches of its posting slice give the slice [start, start + df) that
//           falls into the window and the 64-bit key (first window row - s) << 32 | position of the term's first occurrence
//           in that row -- the order in which CountVectorizer numbers its vocabulary (absent terms: df = 0)
//   scan    one workgroup: exclusive scans over the V terms of df (-> the window's posting pointers) and of df > 0 (-> the
//           window column id: the rank among the present terms, alphabetical like scikit-learn's) in one 64-bit pass
//   rows    one wave per document: keys to LDS, rank by counting smaller keys (the keys of a row are distinct) = the stored
//           order of the row; cnt * idf[df] in that order; both L2 normalisations as sequential chains (sum from 0 in
//           stored order, multiply and add unfused, rows with sum 0 left alone, sqrt, divide: inplace_csr_row_normalize_l2);
//           then every entry finds its posting slot -- the position of its row in the term's window slice, one binary
//           search -- and writes (document, twice-normalised value) there: lists ascending by document, as
//           mused_sparse_cosine_knn requires
//   dense   (mused_tfidf_dense, once V_w is known) the once-normalised values scattered into a zeroed n x V_w matrix
// The idf table comes from the host (NumPy's log; the device never calls log).
#include "common.h"
#include "internal.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace mused {

constexpr int TFIDF_MAX_ROW_TERMS = 1024;  // keys, values and ranks of one row in LDS: 20 KiB at the cap
constexpr int TF_SCAN_THREADS = 1024;
constexpr int TF_FLAG_ROW = 1;             // the window is not what the caller sized for: documents, entries, row length

struct TfCorpus {
  const int *rowptr, *term, *cnt, *pos, *vrank, *vrow, *gpostptr, *gpostrow, *gpostent;
};

__global__ __launch_bounds__(256) void tfidf_terms_kernel(TfCorpus c, int n_terms, int s, int e, int* __restrict__ df,
                                                         unsigned long long* __restrict__ key, int* __restrict__ start) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_terms) return;
  const int p1 = c.gpostptr[t + 1];
  const int lo = lower_bound(c.gpostrow, c.gpostptr[t], p1, s);
  const int hi = lower_bound(c.gpostrow, lo, p1, e);
  df[t] = hi - lo;
  start[t] = lo;
  key[t] = hi > lo ? ((unsigned long long)(unsigned)(c.gpostrow[lo] - s) << 32) | (unsigned)c.pos[c.gpostent[lo]] : ~0ull;
}

// s + v * v as a multiply and an add, each rounded.  Written out under this file's `fp contract(off)`:
// __dadd_rn(s, __dmul_rn(v, v)) does not do here -- the header's inline bodies are compiled under the default contraction
// mode and fuse into one v_fmac_f64 once inlined.
__device__ __forceinline__ double tf_add_square(double s, double v) {
  const double q = v * v;
  return s + q;
}

// df < 2^31 summed and at most 2^31 flags: the two sums share a 64-bit word without a carry between them
__global__ __launch_bounds__(TF_SCAN_THREADS) void tfidf_scan_kernel(const int* __restrict__ df, int n_terms,
                                                                    int* __restrict__ postptr, int* __restrict__ colid,
                                                                    int* __restrict__ info) {
  __shared__ unsigned long long ws[TF_SCAN_THREADS / 64];
  unsigned long long carry = 0;
  for (int base = 0; base < n_terms; base += TF_SCAN_THREADS) {
    const int t = base + threadIdx.x;
    const int d = t < n_terms ? df[t] : 0;
    unsigned long long total;
    const unsigned long long x = carry + block_excl_scan(((unsigned long long)d << 32) | (d > 0 ? 1u : 0u), ws, total);
    if (t < n_terms) {
      postptr[t] = (int)(x >> 32);
      colid[t] = (int)(x & 0xffffffffu);
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    postptr[n_terms] = (int)(carry >> 32);
    info[0] = (int)(carry & 0xffffffffu);  // V_w
    info[2] = (int)(carry >> 32);          // entries of the window
  }
}

__global__ __launch_bounds__(64) void tfidf_rows_kernel(TfCorpus c, int s, int e, int n_docs, int nnz_w, int cap,
                                                       const double* __restrict__ idf, const int* __restrict__ df,
                                                       const unsigned long long* __restrict__ key,
                                                       const int* __restrict__ start, const int* __restrict__ colid,
                                                       const int* __restrict__ postptr, int* __restrict__ out_rowptr,
                                                       int* __restrict__ out_term, int* __restrict__ out_col,
                                                       double* __restrict__ out_val, double* __restrict__ out_val2,
                                                       int* __restrict__ out_postrow, double* __restrict__ out_postval,
                                                       int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long tf_smem[];
  unsigned long long* keys = tf_smem;                      // [cap]
  double* val = reinterpret_cast<double*>(tf_smem + cap);  // [cap], stored order
  int* rk = reinterpret_cast<int*>(tf_smem + 2 * cap);     // [cap]: stored position of native entry i
  const int r = blockIdx.x, lane = threadIdx.x;
  const int v0 = c.vrank[s];
  if (c.vrank[e] - v0 != n_docs) {  // the idf table and the outputs were sized for n_docs documents
    if (r == 0 && lane == 0) atomicOr(&info[1], TF_FLAG_ROW);
    return;
  }
  const int row = c.vrow[v0 + r];
  // invalid rows are empty, so rowptr[s] is where the window's first document starts
  const int base = c.rowptr[s], a0 = c.rowptr[row], a1 = c.rowptr[row + 1];
  const int L = a1 - a0, o0 = a0 - base;
  if (lane == 0) {
    if (r == 0) out_rowptr[0] = 0;
    out_rowptr[r + 1] = a1 - base;
  }
  if (L > cap || o0 < 0 || a1 - base > nnz_w) {
    if (lane == 0) atomicOr(&info[1], TF_FLAG_ROW);
    return;
  }
  for (int i = lane; i < L; i += 64) keys[i] = key[c.term[a0 + i]];
  __syncthreads();
  for (int i = lane; i < L; i += 64) {
    const unsigned long long ki = keys[i];
    int p = 0;
    for (int j = 0; j < L; ++j) p += keys[j] < ki;
    const int t = c.term[a0 + i];
    rk[i] = p;
    val[p] = __dmul_rn((double)c.cnt[a0 + i], idf[df[t]]);
    out_term[o0 + p] = t;
    out_col[o0 + p] = colid[t];
  }
  __syncthreads();
  // every lane walks the whole row (LDS broadcasts): the same chain in all of them, nothing to hand around
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    double sum = 0.0;
    for (int p = 0; p < L; ++p) {
      const double v = val[p];
      sum = tf_add_square(sum, v);
    }
    __syncthreads();
    const double nrm = __dsqrt_rn(sum);
    double* out = pass == 0 ? out_val : out_val2;
    for (int p = lane; p < L; p += 64) {
      const double v = sum != 0.0 ? __ddiv_rn(val[p], nrm) : val[p];
      val[p] = v;
      out[o0 + p] = v;
    }
    __syncthreads();
  }
  for (int i = lane; i < L; i += 64) {
    const int t = c.term[a0 + i];
    const int st = start[t], d = df[t];
    const int q = lower_bound(c.gpostrow, st, st + d, row) - st;
    const int slot = postptr[t] + q;
    if (q < d && slot < nnz_w) {
      out_postrow[slot] = r;
      out_postval[slot] = val[rk[i]];
    }
  }
}

__global__ __launch_bounds__(64) void tfidf_dense_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const double* __restrict__ val, int n_cols,
                                                        double* __restrict__ out, long ld) {
  const int r = blockIdx.x;
  const int a1 = rowptr[r + 1];
  for (int p = rowptr[r] + threadIdx.x; p < a1; p += 64) {
    const int cidx = col[p];
    if (cidx >= 0 && cidx < n_cols) out[(long)r * ld + cidx] = val[p];
  }
}

static long tfidf_ws_bytes(long n_terms) {
  const long v = (n_terms + 1) / 2 * 2;  // int arrays of an even length keep the keys 8-byte aligned
  return 8 * v + 3 * 4 * v;              // key | df | start | colid
}

}  // namespace mused

using namespace mused;

extern "C" {

long mused_tfidf_ws_bytes(long n_terms) { return n_terms >= 1 && n_terms < (1l << 31) ? tfidf_ws_bytes(n_terms) : -1; }

int mused_tfidf_window(const int* rowptr, const int* term, const int* cnt, const int* pos, const int* vrank, const int* vrow,
                       const int* gpostptr, const int* gpostrow, const int* gpostent, int n_rows, int n_terms,
                       int max_row_terms, int s, int e, int n_docs, int nnz_w, const double* idf, int* out_rowptr,
                       int* out_term, int* out_col, double* out_val, double* out_val2, int* out_postptr, int* out_postrow,
                       double* out_postval, int* info, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(rowptr && term && cnt && pos && vrank && vrow && gpostptr && gpostrow && gpostent && idf,
                "mused_tfidf_window: a corpus array or the idf table is missing");
  MUSED_REQUIRE(n_rows >= 1 && n_terms >= 1 && 0 <= s && s < e && e <= n_rows && n_docs >= 1 && n_docs <= e - s && nnz_w >= 1,
                "mused_tfidf_window: bad window (rows=%d terms=%d s=%d e=%d docs=%d entries=%d)", n_rows, n_terms, s, e,
                n_docs, nnz_w);
  MUSED_REQUIRE(max_row_terms >= 1 && max_row_terms <= TFIDF_MAX_ROW_TERMS,
                "mused_tfidf_window: rows of up to %d terms (the kernel ranks at most %d in LDS)", max_row_terms,
                TFIDF_MAX_ROW_TERMS);
  MUSED_REQUIRE(out_rowptr && out_term && out_col && out_val && out_val2 && out_postptr && out_postrow && out_postval && info,
                "mused_tfidf_window: an output is missing");
  MUSED_REQUIRE(ws && ws_bytes >= tfidf_ws_bytes(n_terms) && ((uintptr_t)ws & 7) == 0,
                "mused_tfidf_window: workspace of %ld bytes, need %ld (8-byte aligned)", ws_bytes, tfidf_ws_bytes(n_terms));
  hipStream_t st = (hipStream_t)stream;
  const long v = ((long)n_terms + 1) / 2 * 2;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(ws);
  int* df = reinterpret_cast<int*>(key + v);
  int* start = df + v;
  int* colid = start + v;
  TfCorpus c{rowptr, term, cnt, pos, vrank, vrow, gpostptr, gpostrow, gpostent};
  MUSED_CHECK_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int), st));
  hipLaunchKernelGGL(tfidf_terms_kernel, dim3(cdiv(n_terms, 256)), dim3(256), 0, st, c, n_terms, s, e, df, key, start);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tfidf_scan_kernel, dim3(1), dim3(TF_SCAN_THREADS), 0, st, df, n_terms, out_postptr, colid, info);
  MUSED_LAUNCH_CHECK();
  const int cap = (max_row_terms + 63) / 64 * 64;
  hipLaunchKernelGGL(tfidf_rows_kernel, dim3(n_docs), dim3(64), (size_t)cap * 20, st, c, s, e, n_docs, nnz_w, cap, idf, df, key,
                     start, colid, out_postptr, out_rowptr, out_term, out_col, out_val, out_val2, out_postrow, out_postval,
                     info);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

int mused_tfidf_dense(const int* w_rowptr, const int* w_col, const double* w_val, int n_docs, int n_cols, double* out,
                      long ld, void* stream) {
  MUSED_REQUIRE(w_rowptr && w_col && w_val && out && n_docs >= 1 && n_cols >= 1 && ld >= n_cols,
                "mused_tfidf_dense: bad arguments (docs=%d cols=%d ld=%ld)", n_docs, n_cols, ld);
  hipStream_t st = (hipStream_t)stream;
  MUSED_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)n_docs * ld * sizeof(double), st));
  hipLaunchKernelGGL(tfidf_dense_kernel, dim3(n_docs), dim3(64), 0, st, w_rowptr, w_col, w_val, n_cols, out, ld);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
