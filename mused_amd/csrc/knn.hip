// a1/a2 of SURVEY section 8: pairwise scores (squared-L2 or negated cosine) by fp64
// MFMA GEMM with a fused epilogue, then per-row selection of the k smallest scores.
//
// Reference behaviour reproduced (matrix_operations.py:112-119 via sklearn's
// EuclideanArgKmin; :101-108 via cosine_similarity + argsort):
//   l2     : score(i,j) = max(0, |x_i|^2 - 2 x_i.x_j + |x_j|^2), fp64
//   cosine : score(i,j) = -(x_i.x_j) / (max(|x_i|,!0) * max(|x_j|,!0)), fp64
//   neighbours of i = the k rows of smallest score, ties at the k-th value towards
//   the smaller index (sklearn's heap keeps the earlier candidate on ties).
#include "gemm_f64.h"
#include "internal.h"
#include "meta_scores.h"
#include "radix_select.h"

namespace mused {

// ---- row squared norms (HBM-bound: one wave per row, 16-B loads) ------------
// One lane's share of a row's sum.  The norm is a function of the row's values, d and T alone: lane L adds the V = 16 /
// sizeof(T) columns of every 64th 16-byte group (their squares summed first), then the columns behind the last whole group
// at stride 64, whether the row starts on a 16-byte line (ALIGNED: one 16-byte load per group) or not (V element loads of
// the same columns).  The arithmetic is the same text for both, so duplicate rows get the same bits wherever they lie and
// the scores built on the norms tie exactly (selection then goes by column).
template <typename T, bool ALIGNED>
__device__ __forceinline__ double row_sqnorm_lane(const T* __restrict__ p, int d, int lane) {
  constexpr int V = 16 / sizeof(T);
  double s = 0.0;
  for (int c = lane * V; c + V <= d; c += 64 * V) {
    if constexpr (sizeof(T) == 4) {
      float4 v;
      if constexpr (ALIGNED) v = *reinterpret_cast<const float4*>(p + c);
      else v = make_float4(p[c], p[c + 1], p[c + 2], p[c + 3]);
      s += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    } else {
      double2 v;
      if constexpr (ALIGNED) v = *reinterpret_cast<const double2*>(p + c);
      else v = make_double2(p[c], p[c + 1]);
      s += v.x * v.x + v.y * v.y;
    }
  }
  // tail columns (d not a multiple of V), from the first uncovered column
  for (int t = (d / V) * V + lane; t < d; t += 64) s += (double)p[t] * (double)p[t];
  return s;
}

template <typename T>
__global__ void row_sqnorm_kernel(const T* __restrict__ X, long n, int d, long ld, double* __restrict__ out) {
  const long row = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const T* p = X + row * ld;
  const bool vec = ((uintptr_t)p % 16 == 0);  // wave-uniform: one row per wave
  double s = vec ? row_sqnorm_lane<T, true>(p, d, lane) : row_sqnorm_lane<T, false>(p, d, lane);
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

__global__ void inv_norm_kernel(const double* __restrict__ sq, long n, double* __restrict__ inv) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double nr = sqrt(sq[i]);
  inv[i] = (nr == 0.0) ? 1.0 : 1.0 / nr;  // sklearn normalize(): zero norms replaced by 1
}

int inv_norms_launch(double* norms, long n, hipStream_t st) {
  hipLaunchKernelGGL(inv_norm_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, norms, n, norms);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// ---- epilogues ---------------------------------------------------------------
struct EpiSqL2 {
  double* S;
  long ld;
  const double* nrm;  // squared norms
  __device__ __forceinline__ void operator()(int, int row, int col, double v) const {
    S[(long)row * ld + col] = value(row, col, v);
  }
  __device__ __forceinline__ double value(int row, int col, double v) const {
    const double dd = nrm[row] - 2.0 * v + nrm[col];
    return dd > 0.0 ? dd : 0.0;
  }
  __device__ __forceinline__ void put(int, int row, int col, double val) const { S[(long)row * ld + col] = val; }
};

struct EpiNegCos {
  double* S;
  long ld;
  const double* inv;  // 1 / norm
  __device__ __forceinline__ void operator()(int, int row, int col, double v) const {
    S[(long)row * ld + col] = value(row, col, v);
  }
  // 0.0 - x, not -x: a zero dot product gives +0.0 whatever its sign, so that equal similarities are equal KEYS for the
  // selection too (ties then go to the smaller column, as everywhere else)
  __device__ __forceinline__ double value(int row, int col, double v) const { return 0.0 - (v * inv[row] * inv[col]); }
  __device__ __forceinline__ void put(int, int row, int col, double val) const { S[(long)row * ld + col] = val; }
};

template <typename T>
static int scores_launch(const T* X, long n, int d, long ld, int metric, double* norms, double* S,
                         hipStream_t stream) {
  hipLaunchKernelGGL(row_sqnorm_kernel<T>, dim3(cdiv(n, 4)), dim3(256), 0, stream, X, n, d, ld, norms);
  MUSED_LAUNCH_CHECK();
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = X; g.B = X; g.lda = ld; g.ldb = ld; g.M = (int)n; g.N = (int)n; g.K = d;
  // X X^T: the squared-distance / cosine epilogues are symmetric in (row, col) -> upper tiles only, mirrored stores
  static const int sym = [] {
    const char* sy = getenv("MUSED_SCORES_SYM");
    return (sy && sy[0] == '0') ? 0 : 1;
  }();
  g.sym = sym;
  const bool vec = vec_ok<T>(X, ld, 0);
  if (metric == 0) {
    EpiSqL2 epi{S, n, norms};
    return gemm_f64_launch_t<T, T, true, true>(g, 1, epi, vec, stream);
  }
  hipLaunchKernelGGL(inv_norm_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, norms, n, norms);
  MUSED_LAUNCH_CHECK();
  EpiNegCos epi{S, n, norms};
  return gemm_f64_launch_t<T, T, true, true>(g, 1, epi, vec, stream);
}

// ---- k-smallest selection -------------------------------------------------------
// One 1024-thread workgroup per row.  Exact radix select on order-preserving 64-bit
// keys (radix_select.h).  Selected columns are emitted in ascending column order
// (block prefix sums) -> deterministic output.
constexpr int SEL_THREADS = SELECT_THREADS;
constexpr int SEL_MAX_LDS_KEYS = 16384;  // 128 KiB of keys cached in LDS; longer rows re-read global
constexpr int SEL_MAX_JACCARD_ROWS = 15000;  // keys + 16-bit intersection counters of one row: 150 KB of the 160 KB

// Where a row of scores comes from.  SRC_MATRIX: row `row` of S (the classic path).  The others compute the row on the
// fly (rows of at most SEL_MAX_LDS_KEYS scores, kept as keys in LDS) -- the metadata modality types of meta.hip without
// an n x n score matrix: SRC_HAVERSINE / SRC_TIME from n x 2 records, SRC_JACCARD from tag sets (CSR + posting lists).
// SRC_*_WIN: the same scores for rows [win_s, win_e) of arrays that cover a whole STREAM (csrc/meta_window.hip): n is the
// window length and every row, column and mask bit is a window coordinate; a row is valid iff vrank steps at it.  Invalid
// rows keep their position with the largest key, so they are never among the min(k, valid rows) smallest, and write an
// empty mask row.
enum { SRC_MATRIX = 0, SRC_HAVERSINE = 1, SRC_TIME = 2, SRC_JACCARD = 3, SRC_HAVERSINE_WIN = 4, SRC_TIME_WIN = 5,
       SRC_JACCARD_WIN = 6 };
constexpr bool src_windowed(int src) { return src >= SRC_HAVERSINE_WIN; }
constexpr bool src_tag_sets(int src) { return src == SRC_JACCARD || src == SRC_JACCARD_WIN; }
struct SelSource {
  const double* rec;     // SRC_HAVERSINE / SRC_TIME: n x 2 records
  const int* rowptr;     // SRC_JACCARD: tag sets as CSR ...
  const int* tags;
  const int* postptr;    // ... and the posting lists of the tags
  const int* postrow;
  const int* vrank;      // SRC_*_WIN: prefix count of valid rows over the stream ...
  int win_s, win_e;      // ... and the window's rows
};

template <int SRC>
__global__ __launch_bounds__(SEL_THREADS) void select_k_kernel(const double* __restrict__ S, long ld, int n, int k,
                                                             int* __restrict__ out_idx /* n x k or null */,
                                                             unsigned long long* __restrict__ out_mask, int mask_words,
                                                             SelSource src) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sel_smem[];
  __shared__ SelectLds lds;

  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const double* srow = SRC == SRC_MATRIX ? S + (long)row * ld : nullptr;
  const bool cached = (SRC != SRC_MATRIX) || (n <= SEL_MAX_LDS_KEYS);
  unsigned long long* keys = sel_smem;  // [n] when cached

  [[maybe_unused]] unsigned short* inter = reinterpret_cast<unsigned short*>(sel_smem + n);  // SRC_JACCARD: behind the keys
  [[maybe_unused]] double r0 = 0.0, r1 = 0.0;
  [[maybe_unused]] int li = 0;
  [[maybe_unused]] int ws0 = 0;  // SRC_*_WIN: stream row of window row 0
  if constexpr (src_windowed(SRC)) {
    ws0 = src.win_s;
    if (src.vrank[ws0 + row + 1] == src.vrank[ws0 + row]) {  // an invalid row: no neighbours (the whole workgroup leaves)
      for (int w = tid; w < mask_words; w += SEL_THREADS) out_mask[(long)row * mask_words + w] = 0ull;
      return;
    }
    const int n_valid = src.vrank[src.win_e] - src.vrank[ws0];
    k = k < n_valid ? k : n_valid;
  }
  if constexpr (SRC == SRC_HAVERSINE || SRC == SRC_TIME) {
    r0 = src.rec[2 * (long)row];
    r1 = src.rec[2 * (long)row + 1];
  }
  if constexpr (SRC == SRC_HAVERSINE_WIN || SRC == SRC_TIME_WIN) {
    r0 = src.rec[2 * (long)(ws0 + row)];
    r1 = src.rec[2 * (long)(ws0 + row) + 1];
  }
  if constexpr (SRC == SRC_JACCARD) {
    // intersection sizes of this row's tag set with every row's: walk the posting lists of its tags (rows inside a
    // list are distinct: no atomics, a barrier between lists) -- jaccard_scores_kernel of meta.hip
    for (int j = tid; j < n; j += SEL_THREADS) inter[j] = 0;
    __syncthreads();
    const int t0 = src.rowptr[row], t1 = src.rowptr[row + 1];
    li = t1 - t0;
    for (int t = t0; t < t1; ++t) {
      const int tag = src.tags[t];
      const int p1 = src.postptr[tag + 1];
      for (int q = src.postptr[tag] + tid; q < p1; q += SEL_THREADS) inter[src.postrow[q]] += 1;
      __syncthreads();
    }
  }
  if constexpr (SRC == SRC_JACCARD_WIN) {
    // the same counters, indexed by window row, from the part of every posting list that lies in [win_s, win_e): rows
    // ascend inside a list, so that part starts at the lower bound of win_s (one lane searches, the others read it from
    // LDS; two slots, so one barrier per list separates both the slots' reuse and the lists' additions) and ends at the
    // first row >= win_e
    __shared__ int s_lb[2];
    const int we = src.win_e;
    for (int j = tid; j < n; j += SEL_THREADS) inter[j] = 0;
    const int t0 = src.rowptr[ws0 + row], t1 = src.rowptr[ws0 + row + 1];
    li = t1 - t0;
    for (int t = t0; t < t1; ++t) {
      const int tag = src.tags[t];
      const int p1 = src.postptr[tag + 1];
      if (tid == 0) s_lb[(t - t0) & 1] = lower_bound(src.postrow, src.postptr[tag], p1, ws0);
      __syncthreads();
      for (int q = s_lb[(t - t0) & 1] + tid; q < p1; q += SEL_THREADS) {
        const int r = src.postrow[q];
        if (r >= we) break;
        inter[r - ws0] += 1;
      }
    }
    __syncthreads();
  }
  auto score_at = [&](int i) -> double {
    if constexpr (SRC == SRC_MATRIX) return srow[i];
    if constexpr (SRC == SRC_HAVERSINE) return haversine_km(r0, r1, src.rec[2 * (long)i], src.rec[2 * (long)i + 1]);
    if constexpr (SRC == SRC_TIME) return time_l1(r0, r1, src.rec[2 * (long)i], src.rec[2 * (long)i + 1]);
    if constexpr (SRC == SRC_JACCARD) {
      if (i == row) return 1.0;
      const int lj = src.rowptr[i + 1] - src.rowptr[i];
      if (li == 0 || lj == 0) return 0.0;
      const int in = inter[i];
      return 0.0 - (double)in / (double)(li + lj - in);
    }
    if constexpr (SRC == SRC_HAVERSINE_WIN)
      return haversine_km(r0, r1, src.rec[2 * (long)(ws0 + i)], src.rec[2 * (long)(ws0 + i) + 1]);
    if constexpr (SRC == SRC_TIME_WIN) return time_l1(r0, r1, src.rec[2 * (long)(ws0 + i)], src.rec[2 * (long)(ws0 + i) + 1]);
    if constexpr (SRC == SRC_JACCARD_WIN) {
      if (i == row) return 1.0;
      const int lj = src.rowptr[ws0 + i + 1] - src.rowptr[ws0 + i];
      if (li == 0 || lj == 0) return 0.0;
      const int in = inter[i];
      return 0.0 - (double)in / (double)(li + lj - in);
    }
    return 0.0;
  };
  auto fresh_key = [&](int i) -> unsigned long long {
    if constexpr (src_windowed(SRC)) {
      if (src.vrank[ws0 + i + 1] == src.vrank[ws0 + i]) return ~0ull;  // above every score's key
    }
    return f64_key(score_at(i));
  };

  // pass 0: keys, min, max
  unsigned long long kmin = ~0ull, kmax = 0ull;
  for (int i = tid; i < n; i += SEL_THREADS) {
    const unsigned long long key = fresh_key(i);
    if (cached) keys[i] = key;
    kmin = key < kmin ? key : kmin;
    kmax = key > kmax ? key : kmax;
  }
  auto key_at = [&](int i) -> unsigned long long { return cached ? keys[i] : f64_key(srow[i]); };
  const SelectThreshold th = block_select_threshold(lds, n, k, key_at, kmin, kmax);
  const unsigned long long thr = th.thr;  // k-th smallest key
  const int need_eq = th.need_eq;         // how many keys == thr are selected (smallest indices first)

  // emit: keys < thr, plus the first need_eq keys == thr in index order
  unsigned long long* mrow = out_mask ? out_mask + (long)row * mask_words : nullptr;
  // LDS bitmask staging reuses hist/cand arrays is awkward for large n; write mask words with
  // wave ballots instead: each group of 64 consecutive columns is one word owned by one wave.
  if (!out_idx && th.eq_count == need_eq) {
    // common case: every key equal to the threshold is selected (no tie is cut) and only the bitmask
    // is wanted -> one ballot per 64 columns, no prefix sums, no barriers
    for (int base = 0; base < n; base += SEL_THREADS) {
      const int i = base + tid;
      const bool sel = (i < n) && (key_at(i) <= thr) && (i != row);
      const unsigned long long bal = __ballot(sel);
      const int word = i >> 6;
      if ((tid & 63) == 0 && word < mask_words) mrow[word] = bal;
    }
    const int first_free = ((n + SEL_THREADS - 1) / SEL_THREADS) * (SEL_THREADS / 64);
    for (int w = first_free + tid; w < mask_words; w += SEL_THREADS) mrow[w] = 0ull;
    return;
  }
  int eq_seen = 0, emitted = 0;
  for (int base = 0; base < n; base += SEL_THREADS) {
    const int i = base + tid;
    unsigned long long key = ~0ull;
    int is_lt = 0, is_eq = 0;
    if (i < n) {
      key = key_at(i);
      is_lt = key < thr;
      is_eq = key == thr;
    }
    int tot_eq;
    const int eq_pos = block_excl_scan(is_eq, lds.ws, tot_eq);
    const int sel = is_lt || (is_eq && (eq_seen + eq_pos) < need_eq);
    int tot_sel;
    const int pos = block_excl_scan(sel, lds.ws, tot_sel);
    if (sel && out_idx) out_idx[(long)row * k + emitted + pos] = i;
    if (mrow) {
      const unsigned long long bal = __ballot(sel && i != row);  // self edge dropped (matrix_operations.py:128)
      const int word = i >> 6;  // base is a multiple of 64 -> each wave covers exactly one word
      if ((tid & 63) == 0 && word < mask_words) mrow[word] = bal;
    }
    eq_seen += tot_eq;
    emitted += tot_sel;
  }
  // zero any mask words past the last processed column group
  if (mrow) {
    const int first_free = ((n + SEL_THREADS - 1) / SEL_THREADS) * (SEL_THREADS / 64);
    for (int w = first_free + tid; w < mask_words; w += SEL_THREADS) mrow[w] = 0ull;
  }
}

template <int SRC>
static int select_launch_src(const double* S, long ld, int n, int k, int* out_idx, unsigned long long* out_mask,
                             int mask_words, const SelSource& src, hipStream_t stream) {
  // keys of the row (cached case) + the 16-bit intersection counters of SRC_JACCARD behind them
  const size_t lds = ((SRC != SRC_MATRIX || n <= SEL_MAX_LDS_KEYS) ? (size_t)n * 8 : 0) + (src_tag_sets(SRC) ? (size_t)n * 2 + 8 : 0);
  static LdsOptIn opt;
  const hipError_t attr_rc = allow_dynamic_lds(opt, reinterpret_cast<const void*>(select_k_kernel<SRC>),
                                               src_tag_sets(SRC) ? SEL_MAX_JACCARD_ROWS * 10 + 64 : SEL_MAX_LDS_KEYS * 8);
  MUSED_CHECK_HIP(attr_rc);
  hipLaunchKernelGGL(select_k_kernel<SRC>, dim3(n), dim3(SEL_THREADS), lds, stream, S, ld, n, k, out_idx, out_mask,
                     mask_words, src);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

static int select_launch(const double* S, long ld, int n, int k, int* out_idx, unsigned long long* out_mask,
                         int mask_words, hipStream_t stream) {
  return select_launch_src<SRC_MATRIX>(S, ld, n, k, out_idx, out_mask, mask_words, SelSource{}, stream);
}

// selection straight from the records / tag sets (rows of at most SEL_MAX_LDS_KEYS scores): meta.hip's C entry points
int select_from_records(const double* rec, int n, int kind, int k, int* out_idx, unsigned long long* out_mask,
                        int mask_words, hipStream_t stream) {
  SelSource src{};
  src.rec = rec;
  if (kind == 0) return select_launch_src<SRC_HAVERSINE>(nullptr, 0, n, k, out_idx, out_mask, mask_words, src, stream);
  return select_launch_src<SRC_TIME>(nullptr, 0, n, k, out_idx, out_mask, mask_words, src, stream);
}
int select_from_tag_sets(const int* rowptr, const int* tags, const int* postptr, const int* postrow, int n, int k,
                         int* out_idx, unsigned long long* out_mask, int mask_words, hipStream_t stream) {
  SelSource src{};
  src.rowptr = rowptr; src.tags = tags; src.postptr = postptr; src.postrow = postrow;
  return select_launch_src<SRC_JACCARD>(nullptr, 0, n, k, out_idx, out_mask, mask_words, src, stream);
}
// the same for rows [s, e) of stream-wide arrays, in window coordinates (csrc/meta_window.hip); k is capped by the window's
// valid rows on the device
int select_window_records(const double* rec, const int* vrank, int s, int e, int kind, int k, unsigned long long* out_mask,
                          int mask_words, hipStream_t stream) {
  SelSource src{};
  src.rec = rec; src.vrank = vrank; src.win_s = s; src.win_e = e;
  if (kind == 0) return select_launch_src<SRC_HAVERSINE_WIN>(nullptr, 0, e - s, k, nullptr, out_mask, mask_words, src, stream);
  return select_launch_src<SRC_TIME_WIN>(nullptr, 0, e - s, k, nullptr, out_mask, mask_words, src, stream);
}
int select_window_tag_sets(const int* rowptr, const int* tags, const int* postptr, const int* postrow, const int* vrank, int s,
                           int e, int k, unsigned long long* out_mask, int mask_words, hipStream_t stream) {
  SelSource src{};
  src.rowptr = rowptr; src.tags = tags; src.postptr = postptr; src.postrow = postrow;
  src.vrank = vrank; src.win_s = s; src.win_e = e;
  return select_launch_src<SRC_JACCARD_WIN>(nullptr, 0, e - s, k, nullptr, out_mask, mask_words, src, stream);
}
int select_max_fused_rows(bool tag_sets) { return tag_sets ? SEL_MAX_JACCARD_ROWS : SEL_MAX_LDS_KEYS; }

}  // namespace mused

using namespace mused;

extern "C" {

// Replaces: `np.linalg.norm(...)**2` style row norms (main.py:61) and the norm stage of
// sklearn's Euclidean/cosine kernels.  out[i] = sum_j X[i,j]^2 in fp64.
int mused_row_sq_norms(const void* X, int dtype, long n, int d, long ld, double* out, void* stream) {
  MUSED_REQUIRE(X && out && n >= 0 && d > 0 && ld >= d, "mused_row_sq_norms: bad arguments");
  if (n == 0) return MUSED_OK;
  if (dtype == MUSED_F32)
    hipLaunchKernelGGL(row_sqnorm_kernel<float>, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)X, n, d, ld, out);
  else if (dtype == MUSED_F64)
    hipLaunchKernelGGL(row_sqnorm_kernel<double>, dim3(cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const double*)X, n, d, ld, out);
  else {
    set_error("mused_row_sq_norms: unsupported dtype %d", dtype);
    return MUSED_ERR_UNSUPPORTED;
  }
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// Pairwise score matrix S (n x n fp64, ld = n).  metric 0 = squared L2, 1 = negated cosine.
// `norms` is an n-double workspace (squared norms for l2, 1/norm for cosine on return).
int mused_pairwise_scores(const void* X, int dtype, long n, int d, long ld, int metric, double* norms, double* S,
                          void* stream) {
  MUSED_REQUIRE(X && norms && S && n > 0 && d > 0 && ld >= d, "mused_pairwise_scores: bad arguments");
  MUSED_REQUIRE(metric == 0 || metric == 1, "mused_pairwise_scores: metric must be 0 (l2) or 1 (cosine)");
  MUSED_REQUIRE(n < (1l << 31), "mused_pairwise_scores: n too large");
  if (dtype == MUSED_F32) return scores_launch<float>((const float*)X, n, d, ld, metric, norms, S, (hipStream_t)stream);
  if (dtype == MUSED_F64) return scores_launch<double>((const double*)X, n, d, ld, metric, norms, S, (hipStream_t)stream);
  set_error("mused_pairwise_scores: unsupported dtype %d", dtype);
  return MUSED_ERR_UNSUPPORTED;
}

// Per row, the k smallest entries of S (ties -> smaller column).  out_idx (n x k int32,
// ascending column order) and/or out_mask (n x mask_words uint64 bitmask with the row's
// own column cleared) may be null.
int mused_select_k_smallest(const double* S, long ld, int n, int k, int* out_idx, unsigned long long* out_mask,
                            int mask_words, void* stream) {
  MUSED_REQUIRE(S && n > 0 && k >= 1 && k <= n && ld >= n, "mused_select_k_smallest: need 1 <= k <= n (k=%d n=%d)", k, n);
  MUSED_REQUIRE(!out_mask || mask_words >= (n + 63) / 64, "mused_select_k_smallest: mask_words too small");
  return select_launch(S, ld, n, k, out_idx, out_mask, mask_words, (hipStream_t)stream);
}

// Replaces sklearn NearestNeighbors(...).kneighbors (matrix_operations.py:118-119) and the
// cosine + argsort top-k of :106-108 for dense rows: scores + selection in one call.
// ws_scores: n*n doubles, ws_norms: n doubles (caller-allocated workspaces).
int mused_knn_topk(const void* X, int dtype, long n, int d, long ld, int k, int metric, double* ws_scores,
                   double* ws_norms, int* out_idx, unsigned long long* out_mask, int mask_words, void* stream) {
  int rc = mused_pairwise_scores(X, dtype, n, d, ld, metric, ws_norms, ws_scores, stream);
  if (rc) return rc;
  return mused_select_k_smallest(ws_scores, n, (int)n, k, out_idx, out_mask, mask_words, stream);
}

}  // extern "C"
