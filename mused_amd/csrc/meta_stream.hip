// Batch-scale selection (the reference's process_batch_data, main.py:132-167: one "window" of the whole subset, up to
// 150,000 rows by default): the k smallest (score, column) pairs per row over ALL n columns, for scores computed on the fly,
// with no n x n matrix and no limit of one row of scores in LDS.
//
// One 1024-thread workgroup per row walks the columns in chunks [c0, c1) of at most `chunk` columns.  LDS holds the row's
// running list (the k smallest pairs of the columns seen so far, ascending column order) followed by the keys of the chunk;
// an exact radix select over that concatenation keeps the k smallest by (key, position).  Every column of the running list
// is smaller than every column of the chunk, so position order IS column order and ties go to the smaller column exactly as
// in select_k_kernel (knn.hip).  By induction the final list is the k smallest of the whole row: the same neighbour lists as
// mused_record_knn / mused_jaccard_knn wherever those apply.  No global scratch.
//
// Score sources (the arithmetic of meta_scores.h / knn.hip, operation by operation, no fused multiply-add):
//   HAVERSINE, TIME  n x 2 records
//   JACCARD          tag sets as CSR + posting lists (rows ascending); each list is cut to the chunk by binary search
//   SPCOS            the L2-normalised TF-IDF rows as CSR (entries in the order scikit-learn stores them) + per-term posting
//                    lists with values: score = 0 - sum_t x_it x_jt, the sum over row i's entries in STORED order starting
//                    from 0 -- the order of SciPy's csr_matmat behind cosine_similarity on sparse input, so the similarities
//                    equal the reference's text_sim bit for bit (matrix_operations.py:104-108)
#include "common.h"
#include "internal.h"
#include "meta_scores.h"
#include "radix_select.h"

#pragma clang fp contract(off)

namespace mused {

constexpr int CS_THREADS = SELECT_THREADS;
constexpr int CS_MAX_K = 1024;
constexpr int CS_MAX_CHUNK = 16384;
constexpr int CS_LDS_DYN = 152 * 1024;  // dynamic LDS: (k + chunk) keys + k columns; the static arrays take ~4.5 KB more

enum { CS_HAVERSINE = 1, CS_TIME = 2, CS_JACCARD = 3, CS_SPCOS = 4 };

struct ChunkSource {
  const double* rec;      // HAVERSINE / TIME: n x 2 records
  const int* rowptr;      // JACCARD / SPCOS: rows as CSR (tag ids / term ids) ...
  const int* cols;
  const double* vals;     // SPCOS: the row's values
  const int* postptr;     // ... and the posting lists of the tags / terms (rows ascending)
  const int* postrow;
  const double* postval;  // SPCOS: the values of the posting entries
};

template <int SRC>
__global__ __launch_bounds__(CS_THREADS) void chunk_select_kernel(int n, int k, int chunk, ChunkSource src,
                                                                 int* __restrict__ out_idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long cs_smem[];
  __shared__ SelectLds lds;

  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  unsigned long long* keys = cs_smem;                           // [k + chunk]: running list, then the chunk
  int* run_col = reinterpret_cast<int*>(cs_smem + k + chunk);  // [k]: columns of the running list

  [[maybe_unused]] double r0 = 0.0, r1 = 0.0;
  [[maybe_unused]] int t0 = 0, t1 = 0;
  if constexpr (SRC == CS_HAVERSINE || SRC == CS_TIME) {
    r0 = src.rec[2 * (long)row];
    r1 = src.rec[2 * (long)row + 1];
  } else {
    t0 = src.rowptr[row];
    t1 = src.rowptr[row + 1];
  }

  int kc = 0;  // entries in the running list
  for (int c0 = 0; c0 < n; c0 += chunk) {
    const int len = min(n - c0, chunk), c1 = c0 + len;
    unsigned long long* ck = keys + kc;
    if constexpr (SRC == CS_JACCARD || SRC == CS_SPCOS) {
      // intersection counts / dot products of this row with the chunk's rows, by walking the posting lists of the row's
      // tags / terms in stored order (rows inside one list are distinct: no atomics, a barrier between lists)
      for (int j = tid; j < len; j += CS_THREADS) ck[j] = 0ull;  // 0 = integer 0 = +0.0
      __syncthreads();
      for (int t = t0; t < t1; ++t) {
        const int term = src.cols[t];
        const int p1 = src.postptr[term + 1];
        const int lo = lower_bound(src.postrow, src.postptr[term], p1, c0);
        const int hi = lower_bound(src.postrow, lo, p1, c1);
        if constexpr (SRC == CS_JACCARD) {
          for (int q = lo + tid; q < hi; q += CS_THREADS) ck[src.postrow[q] - c0] += 1ull;
        } else {
          const double v = src.vals[t];
          for (int q = lo + tid; q < hi; q += CS_THREADS) {
            double* acc = reinterpret_cast<double*>(ck + (src.postrow[q] - c0));
            // a product and a sum, each rounded, written out under this file's `fp contract(off)`: __dadd_rn(*acc,
            // __dmul_rn(...)) fuses into one v_fmac_f64 once the header's inline bodies are inlined (tfidf.hip)
            const double prod = v * src.postval[q];
            *acc = *acc + prod;
          }
        }
        __syncthreads();
      }
    }
    for (int j = tid; j < len; j += CS_THREADS) {
      const int i = c0 + j;
      double s;
      if constexpr (SRC == CS_HAVERSINE) {
        s = haversine_km(r0, r1, src.rec[2 * (long)i], src.rec[2 * (long)i + 1]);
      } else if constexpr (SRC == CS_TIME) {
        s = time_l1(r0, r1, src.rec[2 * (long)i], src.rec[2 * (long)i + 1]);
      } else if constexpr (SRC == CS_JACCARD) {
        const int li = t1 - t0, lj = src.rowptr[i + 1] - src.rowptr[i];
        s = 0.0;
        if (li > 0 && lj > 0) {
          const int in = (int)ck[j];
          s = 0.0 - (double)in / (double)(li + lj - in);
        }
        if (i == row) s = 1.0;
      } else {
        s = 0.0 - __longlong_as_double((long long)ck[j]);
      }
      ck[j] = f64_key(s);
    }
    __syncthreads();

    const int m = kc + len;
    const int kk = min(k, m);
    unsigned long long thr = ~0ull;
    int need_eq = m;  // m <= k: every entry is kept
    if (m > k) {
      // the kk-th smallest (key, position) among keys[0, m)
      unsigned long long kmin = ~0ull, kmax = 0ull;
      for (int i = tid; i < m; i += CS_THREADS) {
        const unsigned long long key = keys[i];
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
      }
      const SelectThreshold th = block_select_threshold(lds, m, kk, [&](int i) { return keys[i]; }, kmin, kmax);
      thr = th.thr;
      need_eq = th.need_eq;
    }

    // ---- keep: keys < thr plus the first need_eq keys == thr in position (= column) order, compacted in place ----
    // every read of a batch precedes the barriers of its scans and a write goes to a position <= the one it came from
    int eq_seen = 0, emitted = 0;
    for (int base = 0; base < m; base += CS_THREADS) {
      const int i = base + tid;
      unsigned long long key = ~0ull;
      int col = 0, is_lt = 0, is_eq = 0;
      if (i < m) {
        key = keys[i];
        col = i < kc ? run_col[i] : c0 + (i - kc);
        is_lt = key < thr;
        is_eq = key == thr;
      }
      int tot_eq;
      const int eq_pos = block_excl_scan(is_eq, lds.ws, tot_eq);
      const int sel = is_lt || (is_eq && (eq_seen + eq_pos) < need_eq);
      int tot_sel;
      const int pos = block_excl_scan(sel, lds.ws, tot_sel);
      if (sel) {
        keys[emitted + pos] = key;
        run_col[emitted + pos] = col;
      }
      eq_seen += tot_eq;
      emitted += tot_sel;
    }
    kc = kk;
    __syncthreads();
  }
  for (int p = tid; p < k; p += CS_THREADS) out_idx[(long)row * k + p] = run_col[p];
}

// ---- neighbour lists -> adjacency bitmask rows in window coordinates --------------------------------------------------
// One workgroup per list row r: window row w = map[r] (r without a map), bits map[idx[r][j]] except w itself, built in LDS
// and written as whole words.  Rows no list maps to are left to the caller's zero fill.
__global__ __launch_bounds__(256) void lists_to_mask_kernel(const int* __restrict__ idx, int k, const int* __restrict__ map,
                                                            int words, unsigned long long* __restrict__ mask) {
  extern __shared__ __attribute__((aligned(16))) unsigned int lm_bits[];  // [2 * words]
  const int r = blockIdx.x;
  for (int w = threadIdx.x; w < 2 * words; w += 256) lm_bits[w] = 0u;
  __syncthreads();
  const int wr = map ? map[r] : r;
  for (int j = threadIdx.x; j < k; j += 256) {
    const int c = idx[(long)r * k + j];
    const int wc = map ? map[c] : c;
    if (wc != wr) atomicOr(&lm_bits[wc >> 5], 1u << (wc & 31));
  }
  __syncthreads();
  const unsigned long long* b64 = reinterpret_cast<const unsigned long long*>(lm_bits);
  for (int w = threadIdx.x; w < words; w += 256) mask[(long)wr * words + w] = b64[w];
}

constexpr int LM_MAX_WORDS = 8192;  // 64 KiB of LDS: n <= 524,288

int lists_to_mask(const int* idx, int n_rows, int k, const int* map, int n, unsigned long long* mask, int words,
                  hipStream_t st) {
  if (map) MUSED_CHECK_HIP(hipMemsetAsync(mask, 0, (size_t)n * words * 8, st));
  if (n_rows == 0) return MUSED_OK;
  hipLaunchKernelGGL(lists_to_mask_kernel, dim3(n_rows), dim3(256), (size_t)words * 8, st, idx, k, map, words, mask);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

int chunk_lds_bytes(int k, int chunk) { return (k + chunk) * 8 + k * 4; }

// the largest chunk (<= CS_MAX_CHUNK) whose keys fit the LDS next to a running list of k entries
int chunk_for(int k, int chunk) {
  int c = (CS_LDS_DYN - 12 * k) / 8;
  if (c > CS_MAX_CHUNK) c = CS_MAX_CHUNK;
  if (chunk > 0 && chunk < c) c = chunk;
  return c;
}

template <int SRC>
static int chunk_select_launch(int n, int k, int chunk, const ChunkSource& src, int* out_idx, unsigned long long* out_mask,
                               int mask_words, hipStream_t st) {
  static LdsOptIn opt;
  const hipError_t attr_rc = allow_dynamic_lds(opt, reinterpret_cast<const void*>(chunk_select_kernel<SRC>), CS_LDS_DYN);
  MUSED_CHECK_HIP(attr_rc);
  const int c = chunk_for(k, chunk);
  hipLaunchKernelGGL(chunk_select_kernel<SRC>, dim3(n), dim3(CS_THREADS), (size_t)chunk_lds_bytes(k, c), st, n, k, c, src,
                     out_idx);
  MUSED_LAUNCH_CHECK();
  if (out_mask) return lists_to_mask(out_idx, n, k, nullptr, n, out_mask, mask_words, st);
  return MUSED_OK;
}

}  // namespace mused

using namespace mused;

extern "C" {

int mused_record_knn_chunked(const double* rec, int n, int kind, int k, int chunk, int* out_idx,
                             unsigned long long* out_mask, int mask_words, void* stream) {
  MUSED_REQUIRE(rec && out_idx && n > 0 && (kind == 0 || kind == 1) && k >= 1 && k <= n && k <= CS_MAX_K && chunk >= 0,
                "mused_record_knn_chunked: bad arguments (n=%d kind=%d k=%d chunk=%d)", n, kind, k, chunk);
  MUSED_REQUIRE(!out_mask || (mask_words >= (n + 63) / 64 && mask_words <= LM_MAX_WORDS),
                "mused_record_knn_chunked: mask_words %d (n=%d)", mask_words, n);
  ChunkSource src{};
  src.rec = rec;
  if (kind == 0) return chunk_select_launch<CS_HAVERSINE>(n, k, chunk, src, out_idx, out_mask, mask_words, (hipStream_t)stream);
  return chunk_select_launch<CS_TIME>(n, k, chunk, src, out_idx, out_mask, mask_words, (hipStream_t)stream);
}

int mused_jaccard_knn_chunked(const int* rowptr, const int* tags, const int* postptr, const int* postrow, int n, int n_tags,
                              int k, int chunk, int* out_idx, unsigned long long* out_mask, int mask_words, void* stream) {
  MUSED_REQUIRE(rowptr && postptr && out_idx && n > 0 && n_tags >= 0 && k >= 1 && k <= n && k <= CS_MAX_K && chunk >= 0,
                "mused_jaccard_knn_chunked: bad arguments (n=%d k=%d chunk=%d)", n, k, chunk);
  MUSED_REQUIRE(!out_mask || (mask_words >= (n + 63) / 64 && mask_words <= LM_MAX_WORDS),
                "mused_jaccard_knn_chunked: mask_words %d (n=%d)", mask_words, n);
  ChunkSource src{};
  src.rowptr = rowptr; src.cols = tags; src.postptr = postptr; src.postrow = postrow;
  return chunk_select_launch<CS_JACCARD>(n, k, chunk, src, out_idx, out_mask, mask_words, (hipStream_t)stream);
}

int mused_sparse_cosine_knn(const int* rowptr, const int* terms, const double* vals, const int* postptr, const int* postrow,
                            const double* postval, int n, int n_terms, int k, int chunk, int* out_idx,
                            unsigned long long* out_mask, int mask_words, void* stream) {
  MUSED_REQUIRE(rowptr && postptr && out_idx && n > 0 && n_terms >= 0 && k >= 1 && k <= n && k <= CS_MAX_K && chunk >= 0,
                "mused_sparse_cosine_knn: bad arguments (n=%d k=%d chunk=%d)", n, k, chunk);
  MUSED_REQUIRE(!out_mask || (mask_words >= (n + 63) / 64 && mask_words <= LM_MAX_WORDS),
                "mused_sparse_cosine_knn: mask_words %d (n=%d)", mask_words, n);
  ChunkSource src{};
  src.rowptr = rowptr; src.cols = terms; src.vals = vals; src.postptr = postptr; src.postrow = postrow; src.postval = postval;
  return chunk_select_launch<CS_SPCOS>(n, k, chunk, src, out_idx, out_mask, mask_words, (hipStream_t)stream);
}

int mused_lists_to_mask(const int* idx, int n_rows, int k, const int* row_map, int n, unsigned long long* out_mask,
                        int mask_words, void* stream) {
  MUSED_REQUIRE(out_mask && n > 0 && n_rows >= 0 && n_rows <= n && k >= 0 && (idx || n_rows == 0 || k == 0),
                "mused_lists_to_mask: bad arguments (n_rows=%d n=%d k=%d)", n_rows, n, k);
  MUSED_REQUIRE(row_map || n_rows == n, "mused_lists_to_mask: without a row map the lists must cover all %d rows", n);
  MUSED_REQUIRE(mask_words >= (n + 63) / 64 && mask_words <= LM_MAX_WORDS, "mused_lists_to_mask: mask_words %d (n=%d)",
                mask_words, n);
  return lists_to_mask(idx, n_rows, k, row_map, n, out_mask, mask_words, (hipStream_t)stream);
}

}  // extern "C"
