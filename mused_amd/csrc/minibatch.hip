// The arithmetic of scikit-learn's MiniBatchKMeans.partial_fit (main.py:82-86, approach "sSVDMC_mini": one clusterer for
// the whole stream, partial_fit(reduced).predict(reduced) per window) on the device.  What couples the result to NumPy's
// MT19937 stream -- k-means++ on the first batch, the reassignment decision, the rows picked for reassigned centres --
// stays on the host (mused_amd/cluster.py) and acts on a host copy of the k counts; what runs here is
//
//   E step      labels_i = argmin_j ( |c_j|^2 - 2 x_i . c_j ), first minimum on ties      (_k_means_lloyd.pyx _update_chunk_dense)
//   update      per cluster c with wsum > 0 rows:  c <- c * counts[c];  c += x_i for its rows IN SAMPLE ORDER;
//               counts[c] += wsum;  c *= 1 / counts[c]                                     (_k_means_minibatch.pyx update_center_dense)
//   reassign    centres[dst] <- X[src], counts <- host vector                               (_kmeans.py _mini_batch_step :1643-1673)
//
// The update is deterministic per cluster (no atomics, no order that depends on the schedule), so the centres and counts
// equal scikit-learn's bit for bit whenever the labels agree.  The E step takes the centre norms (km_csq_kernel)
// and its tiles (km_stream_tiles, within this file's budget) from kmeans_common.h; mbkm_assign_kernel is the wide Lloyd
// entry's kmw_assign_kernel (csrc/kmeans.hip) without the stop flags, on X with its pitch ld.  fp64 throughout; k <= 1024,
// d <= 512, no k * d bound: the centres travel through LDS in tiles.
#include "kmeans_common.h"

namespace mused {

constexpr int MB_THREADS = 256;
constexpr int MB_ASSIGN_LDS_DOUBLES = 17920;  // 140 KiB: row tile + centre tile of the assign kernel
constexpr int MB_UPDATE_LDS_DOUBLES = 7168;   // 56 KiB: rows staged by the update kernel (stays under the 64 KiB default)
constexpr int MB_LIST = 1024;                 // labels scanned per pass of the update kernel

// E step.  A workgroup owns TR rows (staged in LDS, pitch d + 1) and walks the centres in tiles of KT (LDS, pitch d + 1);
// PT = 256 / TR adjacent lanes share a row and take centres part, part + PT, ... of every tile, two at a time (two
// independent chains: the sum of each dot product is still sequential over c).  Candidates of one thread come in
// ascending j, so strict < keeps the first minimum; the PT threads then agree on the lexicographic (distance, j) minimum:
// km_take and km_lane_min (kmeans_common.h) written out, as in kmw_assign_kernel (csrc/kmeans.hip), whose copy this is.
__global__ __launch_bounds__(MB_THREADS) void mbkm_assign_kernel(const double* __restrict__ X, long ld, int n, int d, int k,
                                                                 const double* __restrict__ C, const double* __restrict__ csq,
                                                                 int* __restrict__ labels, int TR, int KT) {
  extern __shared__ __attribute__((aligned(16))) double mb_lds[];
  const int dp = d + 1, PT = MB_THREADS / TR;
  double* xs = mb_lds;                  // [TR][dp]
  double* cs = mb_lds + (long)TR * dp;  // [KT][dp]
  const int t = threadIdx.x, r0 = blockIdx.x * TR;
  const int nr = min(TR, n - r0);
  for (int e = t; e < nr * d; e += MB_THREADS) {
    const int r = e / d, c = e - r * d;
    xs[(long)r * dp + c] = X[(long)(r0 + r) * ld + c];
  }
  const int row = t / PT, part = t % PT;
  const double* x = xs + (long)row * dp;
  double best = KM_NO_DIST;
  int lab = KM_NO_LABEL;
  for (int j0 = 0; j0 < k; j0 += KT) {
    const int kt = min(KT, k - j0);
    __syncthreads();  // the row tile is staged / the previous centre tile is consumed
    for (int e = t; e < kt * d; e += MB_THREADS) {
      const int jj = e / d, c = e - jj * d;
      cs[(long)jj * dp + c] = C[(long)(j0 + jj) * d + c];
    }
    __syncthreads();
    if (row >= nr) continue;
    int jj = part;
    for (; jj + PT < kt; jj += 2 * PT) {
      const double* ca = cs + (long)jj * dp;
      const double* cb = cs + (long)(jj + PT) * dp;
      double da = 0.0, db = 0.0;
      for (int c = 0; c < d; ++c) {
        da = fma(x[c], ca[c], da);
        db = fma(x[c], cb[c], db);
      }
      const double dista = csq[j0 + jj] - 2.0 * da;
      if (lab == KM_NO_LABEL || dista < best) {  // strict <: the first minimum wins, as in sklearn
        best = dista;
        lab = j0 + jj;
      }
      const double distb = csq[j0 + jj + PT] - 2.0 * db;
      if (distb < best) {
        best = distb;
        lab = j0 + jj + PT;
      }
    }
    if (jj < kt) {
      const double* ca = cs + (long)jj * dp;
      double da = 0.0;
      for (int c = 0; c < d; ++c) da = fma(x[c], ca[c], da);
      const double dista = csq[j0 + jj] - 2.0 * da;
      if (lab == KM_NO_LABEL || dista < best) {
        best = dista;
        lab = j0 + jj;
      }
    }
  }
  for (int o = 1; o < PT; o <<= 1) {  // the PT threads of a row are adjacent lanes of one wave (PT <= 16)
    const double ob = __shfl_xor(best, o);
    const int ol = __shfl_xor(lab, o);
    if (ol != KM_NO_LABEL && (lab == KM_NO_LABEL || ob < best || (ob == best && ol < lab))) {
      best = ob;
      lab = ol;
    }
  }
  if (part == 0 && row < nr) labels[r0 + row] = lab;
}

// Ordered centre update: one workgroup per cluster j.  Passes over MB_LIST labels build the ordered list of the pass's
// rows labelled j (wave ballots + prefix counts); the rows are staged through LDS, S at a time, and thread t adds them to
// features t and t + 256 in list order.  Explicit _rn intrinsics: no contraction of c * counts + x into one fma.
__global__ __launch_bounds__(MB_THREADS) void mbkm_update_kernel(const double* __restrict__ X, long ld, int n, int d,
                                                                 const int* __restrict__ labels, double* __restrict__ C,
                                                                 double* __restrict__ counts, int S) {
  extern __shared__ __attribute__((aligned(16))) double mb_rows[];  // [S][d]
  __shared__ int list[MB_LIST];
  __shared__ int wcnt[MB_LIST / 64];
  const int j = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const double cnt_old = counts[j];
  double* cj = C + (long)j * d;
  double acc0 = 0.0, acc1 = 0.0;
  if (t < d) acc0 = __dmul_rn(cj[t], cnt_old);
  if (t + MB_THREADS < d) acc1 = __dmul_rn(cj[t + MB_THREADS], cnt_old);
  int total = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = 0; base < n; base += MB_LIST) {
    // sub-pass q covers rows base + 256 q + t; list position = rows of earlier (sub-pass, wave) groups + lanes below
    unsigned long long bal[MB_LIST / MB_THREADS];
#pragma unroll
    for (int q = 0; q < MB_LIST / MB_THREADS; ++q) {
      const int r = base + q * MB_THREADS + t;
      bal[q] = __ballot(r < n && labels[r] == j);
      if (lane == 0) wcnt[q * (MB_THREADS / 64) + w] = __popcll(bal[q]);
    }
    __syncthreads();
    int off = 0, m = 0;
    for (int g = 0; g < MB_LIST / 64; ++g) m += wcnt[g];
#pragma unroll
    for (int q = 0; q < MB_LIST / MB_THREADS; ++q) {
      const int g = q * (MB_THREADS / 64) + w;
      if ((bal[q] >> lane) & 1ull) {
        off = 0;
        for (int h = 0; h < g; ++h) off += wcnt[h];
        list[off + __popcll(bal[q] & below)] = base + q * MB_THREADS + t;
      }
    }
    __syncthreads();
    for (int s0 = 0; s0 < m; s0 += S) {
      const int ns = min(S, m - s0);
      for (int e = t; e < ns * d; e += MB_THREADS) {
        const int r = e / d, c = e - r * d;
        mb_rows[(long)r * d + c] = X[(long)list[s0 + r] * ld + c];
      }
      __syncthreads();
      if (t < d)
        for (int r = 0; r < ns; ++r) acc0 = __dadd_rn(acc0, mb_rows[(long)r * d + t]);
      if (t + MB_THREADS < d)
        for (int r = 0; r < ns; ++r) acc1 = __dadd_rn(acc1, mb_rows[(long)r * d + t + MB_THREADS]);
      __syncthreads();
    }
    total += m;
  }
  if (total == 0) return;  // no row in this batch: centre and count unchanged
  const double cnt_new = __dadd_rn(cnt_old, (double)total);
  const double alpha = __ddiv_rn(1.0, cnt_new);
  if (t < d) cj[t] = __dmul_rn(acc0, alpha);
  if (t + MB_THREADS < d) cj[t + MB_THREADS] = __dmul_rn(acc1, alpha);
  if (t == 0) counts[j] = cnt_new;
}

// centres[dst[b]] <- X[src[b]] (workgroup b < m); workgroup m writes the counts.  Pairs outside [0, n) x [0, k) are skipped.
__global__ __launch_bounds__(MB_THREADS) void mbkm_reassign_kernel(const double* __restrict__ X, long ld, int n, int d, int k,
                                                                   const int* __restrict__ src, const int* __restrict__ dst,
                                                                   int m, const double* __restrict__ new_counts,
                                                                   double* __restrict__ C, double* __restrict__ counts) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (b < m) {
    const int s = src[b], g = dst[b];
    if (s < 0 || s >= n || g < 0 || g >= k) return;
    for (int c = t; c < d; c += MB_THREADS) C[(long)g * d + c] = X[(long)s * ld + c];
  } else {
    for (int jj = t; jj < k; jj += MB_THREADS) counts[jj] = new_counts[jj];
  }
}

// centre norms into csq, then the E step
static int assign_launch(const double* X, long ld, int n, int d, int k, const double* C, double* csq, int* labels,
                         hipStream_t st) {
  int TR = 0, KT = 0;
  MUSED_REQUIRE(km_stream_tiles(MB_ASSIGN_LDS_DOUBLES, d, k, &TR, &KT), "minibatch assign: no tile fits d = %d", d);
  static LdsOptIn opt;
  const hipError_t aerr = allow_dynamic_lds(opt, reinterpret_cast<const void*>(mbkm_assign_kernel), 8 * MB_ASSIGN_LDS_DOUBLES);
  MUSED_CHECK_HIP(aerr);
  hipLaunchKernelGGL(km_csq_kernel, dim3(cdiv(k, 64)), dim3(64), 0, st, C, k, d, csq);
  const size_t lds = 8 * (size_t)(TR + KT) * (d + 1);
  hipLaunchKernelGGL(mbkm_assign_kernel, dim3(cdiv(n, TR)), dim3(MB_THREADS), lds, st, X, ld, n, d, k, C, csq, labels, TR, KT);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // namespace mused

using namespace mused;

extern "C" {

// workspace bytes for mused_mbkm_step / mused_kmeans_assign (the k centre norms)
long mused_mbkm_ws_bytes(int n, int d, int k) {
  if (n <= 0 || d <= 0 || k <= 0) return -1;
  return 8l * k + 256;
}

int mused_kmeans_assign(const double* X, long ld, int n, int d, int k, const double* centers, int* labels, void* ws,
                        long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && centers && labels && ws && n > 0 && d > 0 && k > 0 && ld >= d, "mused_kmeans_assign: bad arguments");
  MUSED_REQUIRE(k <= 1024 && d <= 512, "mused_kmeans_assign: k <= 1024 and d <= 512 (got k = %d, d = %d)", k, d);
  MUSED_REQUIRE(ws_bytes >= mused_mbkm_ws_bytes(n, d, k), "mused_kmeans_assign: workspace too small");
  return assign_launch(X, ld, n, d, k, centers, (double*)ws, labels, (hipStream_t)stream);
}

int mused_mbkm_step(const double* X, long ld, int n, int d, int k, double* centers, double* counts, int* labels, void* ws,
                    long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && centers && counts && labels && ws && n > 0 && d > 0 && k > 0 && ld >= d, "mused_mbkm_step: bad arguments");
  MUSED_REQUIRE(k <= 1024 && d <= 512, "mused_mbkm_step: k <= 1024 and d <= 512 (got k = %d, d = %d)", k, d);
  MUSED_REQUIRE(ws_bytes >= mused_mbkm_ws_bytes(n, d, k), "mused_mbkm_step: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int rc = assign_launch(X, ld, n, d, k, centers, (double*)ws, labels, st);
  if (rc != MUSED_OK) return rc;
  const int S = MB_UPDATE_LDS_DOUBLES / d;
  hipLaunchKernelGGL(mbkm_update_kernel, dim3(k), dim3(MB_THREADS), 8 * (size_t)S * d, st, X, ld, n, d, labels, centers,
                     counts, S);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

int mused_mbkm_reassign(const double* X, long ld, int n, int d, int k, const int* src_rows, const int* dst_centers, int m,
                        const double* new_counts, double* centers, double* counts, void* stream) {
  MUSED_REQUIRE(X && centers && counts && new_counts && n > 0 && d > 0 && k > 0 && ld >= d && m >= 0 && m <= k &&
                    (m == 0 || (src_rows && dst_centers)),
                "mused_mbkm_reassign: bad arguments");
  hipLaunchKernelGGL(mbkm_reassign_kernel, dim3(m + 1), dim3(MB_THREADS), 0, (hipStream_t)stream, X, ld, n, d, k, src_rows,
                     dst_centers, m, new_counts, centers, counts);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
