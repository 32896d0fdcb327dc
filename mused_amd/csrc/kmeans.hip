// the assign / update iterations of perform_clustering (matrix_operations.py:149-153 =
// sklearn KMeans(n_clusters, random_state=seed): k-means++ seeding, n_init = 1, Lloyd, max_iter = 300, tol = 1e-4) on
// the device.  The seeds are an input: mused_kmeans_seed (csrc/kmeanspp.hip) computes them on the device from the draws
// the host takes from RandomState(seed) up front, or -- MUSED_KMEANS_SEED=host, and any window whose seeding the device
// flags as decided within rounding -- sklearn's own kmeans_plusplus computes them on the host; what runs here is
// sklearn:cluster/_kmeans.py `_kmeans_single_lloyd` (:586-720) / `_k_means_lloyd.pyx` `lloyd_iter_chunked_dense`:
//
//   repeat (<= max_iter):
//     E step   labels_i = argmin_j ( |c_j|^2 - 2 x_i . c_j ),  first minimum on ties        (_k_means_lloyd.pyx _update_chunk_dense)
//     M step   c_j <- mean of the rows labelled j;  shift = sum_j |c_j_new - c_j|^2
//     stop     if labels == labels of the previous iteration (strict convergence)  else if shift <= tol
//   if not strictly converged: one more E step with the final centres                     (_kmeans.py:709-720)
//
// Floating point: fp64 throughout like sklearn; sums are taken in a FIXED order (rows of a 256-row chunk in sequence,
// chunks in sequence), so results are reproducible run to run -- sklearn's own sums depend on its thread count, and
// labels are only sensitive to that for rows within rounding of a cell boundary (tests: bit-identical labels on every
// golden window and on the 20-window benchmark stream).  An empty cluster (sklearn relocates its centre,
// _k_means_common.pyx `_relocate_empty_clusters_dense`) is not handled here: it raises info[2] and the host falls back to
// scikit-learn for that window.
//
// Two entries: mused_kmeans_lloyd keeps all k centres and the k x d sums of a chunk in LDS (k * d <= 8192);
// mused_kmeans_lloyd_wide works in tiles for any k <= 1024, d <= 512 and returns the same bits.  Both run km_lloyd_run,
// the one host driver (workspace from km_carve), with their own E-step and M-step launches, and both take from
// kmeans_common.h what decides a label or a stop: the first-minimum rule (km_take, km_lane_min), the centre norms
// (km_csq_kernel, km_norm2), the shift tree with the stop rule (km_finish) and the tile choice of the streamed E step
// (km_stream_tiles), which csrc/minibatch.hip uses too.
#include <stdlib.h>

#include "kmeans_common.h"

namespace mused {

__global__ void km_center_kernel(const double* __restrict__ X, long ldx, const double* __restrict__ mean, int n, int d,
                                 double* __restrict__ Xc) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)n * d) return;
  const int r = (int)(gid / d), c = (int)(gid - (long)r * d);
  Xc[gid] = X[(long)r * ldx + c] - mean[c];
}

// pcnt[j] <- rows of a chunk (labels sL[0 .. rows) in LDS) with label j; k may exceed the 256 threads
__device__ __forceinline__ void km_chunk_counts(const int* sL, int rows, int k, int* __restrict__ pcnt) {
  for (int j = threadIdx.x; j < k; j += KM_CHUNK) {
    int cnt = 0;
    for (int r = 0; r < rows; ++r) cnt += (sL[r] == j);
    pcnt[j] = cnt;
  }
}

// E step for one chunk of 256 rows + the chunk's partial sums of the M step.  LDS: centres [k][d], sums [k][d], labels.
__global__ __launch_bounds__(KM_CHUNK) void km_assign_kernel(const double* __restrict__ Xc, int n, int d, int k,
                                                            const double* __restrict__ C, const double* __restrict__ csq,
                                                            int* __restrict__ labels, const int* __restrict__ labels_old,
                                                            double* __restrict__ psum, int* __restrict__ pcnt,
                                                            KmInfo* __restrict__ info, int want_sums) {
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  if (info->done) return;  // converged in an earlier iteration of this batch of launches
  double* sC = km_lds;                  // [k][d]
  double* sS = km_lds + (long)k * d;    // [k][d]
  int* sL = reinterpret_cast<int*>(sS + (long)k * d);  // [KM_CHUNK]
  const int t = threadIdx.x, r0 = blockIdx.x * KM_CHUNK;
  for (int e = t; e < k * d; e += KM_CHUNK) {
    sC[e] = C[e];
    sS[e] = 0.0;
  }
  __syncthreads();
  const int row = r0 + t;
  double best = KM_NO_DIST;
  int lab = KM_NO_LABEL;  // stays so for a thread past the last row: sL[t] is not read there
  if (row < n) {
    const double* x = Xc + (long)row * d;
    for (int j = 0; j < k; ++j) {
      double dot = 0.0;
      for (int c = 0; c < d; ++c) dot = fma(x[c], sC[(long)j * d + c], dot);
      km_take(best, lab, csq[j] - 2.0 * dot, j);
    }
    labels[row] = lab;
    if (labels_old && labels_old[row] != lab) info->changed = 1;  // benign race: everybody writes 1
  }
  sL[t] = lab;
  __syncthreads();
  if (!want_sums) return;
  // M step partials: thread c owns column c and walks the chunk's rows in order (deterministic)
  const int rows = min(KM_CHUNK, n - r0);
  for (int c = t; c < d; c += KM_CHUNK) {
    for (int r = 0; r < rows; ++r) {
      const int j = sL[r];
      sS[(long)j * d + c] += Xc[(long)(r0 + r) * d + c];
    }
  }
  km_chunk_counts(sL, rows, k, pcnt + (long)blockIdx.x * k);
  __syncthreads();
  for (int e = t; e < k * d; e += KM_CHUNK) psum[(long)blockIdx.x * k * d + e] = sS[e];
}

// The same E step + M-step partials with the chunk's rows staged through LDS.  The kernel above gives every thread a row
// and reads it from global memory once per centre (64 cache lines per load instruction, the row fetched k times: DESIGN.md).
// Here a 256-row chunk travels as 256 / TR sub-tiles of TR rows, loaded coalesced into LDS (pitch d + 1); PT = 256 / TR
// threads share a row (centres j = part, part + PT, ...: every dot product still runs over c = 0 .. d - 1 in sequence)
// and agree on the first minimum by km_lane_min; the M-step partials add the rows of the chunk in the same order as
// before, from LDS.  Results are bit-identical to the kernel above (same sums in the same order).
template <int TR>
__global__ __launch_bounds__(KM_CHUNK) void km_assign_tiled_kernel(const double* __restrict__ Xc, int n, int d, int k,
                                                                  const double* __restrict__ C, const double* __restrict__ csq,
                                                                  int* __restrict__ labels, const int* __restrict__ labels_old,
                                                                  double* __restrict__ psum, int* __restrict__ pcnt,
                                                                  KmInfo* __restrict__ info, int want_sums) {
  constexpr int PT = KM_CHUNK / TR;
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  if (info->done) return;  // converged in an earlier iteration of this batch of launches
  const int dp = d + 1;
  double* sC = km_lds;                       // [k][dp]
  double* sS = sC + (long)k * dp;            // [k][d]
  double* xs = sS + (long)k * d;             // [TR][dp]
  int* sL = reinterpret_cast<int*>(xs + (long)TR * dp);  // [KM_CHUNK]
  const int t = threadIdx.x, r0 = blockIdx.x * KM_CHUNK;
  for (int e = t; e < k * d; e += KM_CHUNK) {
    const int j = e / d, c = e - j * d;
    sC[(long)j * dp + c] = C[e];
    sS[e] = 0.0;
  }
  const int rows = min(KM_CHUNK, n - r0);
  const int row = t / PT, part = t % PT;
  for (int sub = 0; sub * TR < rows; ++sub) {
    const int rb = r0 + sub * TR, nr = min(TR, n - rb);
    __syncthreads();  // the centres are staged / the previous sub-tile is consumed
    for (int e = t; e < nr * d; e += KM_CHUNK) {
      const int r = e / d, c = e - r * d;
      xs[(long)r * dp + c] = Xc[(long)(rb + r) * d + c];
    }
    __syncthreads();
    double best = KM_NO_DIST;
    int lab = KM_NO_LABEL;
    if (row < nr) {
      const double* x = xs + (long)row * dp;
      for (int j = part; j < k; j += PT) {
        const double* cj = sC + (long)j * dp;
        double dot = 0.0;
        for (int c = 0; c < d; ++c) dot = fma(x[c], cj[c], dot);
        km_take(best, lab, csq[j] - 2.0 * dot, j);
      }
    }
    km_lane_min(best, lab, PT);  // the PT threads of a row are adjacent lanes
    if (part == 0 && row < nr) {
      labels[rb + row] = lab;
      if (labels_old && labels_old[rb + row] != lab) info->changed = 1;  // benign race: everybody writes 1
      sL[sub * TR + row] = lab;
    }
    __syncthreads();
    if (want_sums) {  // M-step partials: thread c owns column c and walks the sub-tile's rows in order (deterministic)
      for (int c = t; c < d; c += KM_CHUNK)
        for (int r = 0; r < nr; ++r) sS[(long)sL[sub * TR + r] * d + c] += xs[(long)r * dp + c];
    }
  }
  if (!want_sums) return;
  __syncthreads();
  km_chunk_counts(sL, rows, k, pcnt + (long)blockIdx.x * k);
  for (int e = t; e < k * d; e += KM_CHUNK) psum[(long)blockIdx.x * k * d + e] = sS[e];
}

// M step: centres from the chunk partials (chunks in order), total squared shift, stopping rule.  One workgroup.
__global__ __launch_bounds__(1024) void km_update_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt,
                                                        int nchunk, int k, int d, double* __restrict__ C,
                                                        double* __restrict__ csq, double tol, int first_iter,
                                                        KmInfo* __restrict__ info) {
  __shared__ int s_cnt[1024];
  if (info->done) return;
  const int t = threadIdx.x;
  for (int j = t; j < k; j += 1024) {
    int cnt = 0;
    for (int ch = 0; ch < nchunk; ++ch) cnt += pcnt[(long)ch * k + j];
    s_cnt[j] = cnt;
    if (cnt == 0) info->empty = 1;
  }
  __syncthreads();
  double acc = 0.0;  // this thread's share of the squared shift, elements in a fixed order
  for (int e = t; e < k * d; e += 1024) {
    const int j = e / d;
    double s = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) s += psum[(long)ch * k * d + e];
    // sklearn averages by multiplying with the reciprocal (_k_means_common.pyx _average_centers: alpha = 1.0 / weight)
    const double nw = s_cnt[j] > 0 ? s * (1.0 / (double)s_cnt[j]) : C[e];
    const double df = nw - C[e];
    acc = fma(df, df, acc);
    C[e] = nw;
  }
  km_finish(acc, C, k, d, csq, tol, first_iter, info);
}

// LDS bytes of km_assign_tiled_kernel<tr>: centres [k][d + 1], sums [k][d], rows [tr][d + 1], labels
static size_t km_tiled_lds(int tr, int d, int k) {
  return 8 * ((size_t)k * (d + 1) + (size_t)k * d + (size_t)tr * (d + 1)) + 4 * KM_CHUNK + 16;
}
constexpr size_t KM_LDS_MAX = 156 * 1024;

// The E/M-step kernel of a call: the staged variant with the largest sub-tile (64 / 32 / 16 rows) whose LDS need fits;
// 0 = the row-per-thread kernel (also with MUSED_KMEANS_ASSIGN=p, read once).
static int km_assign_rows(int d, int k) {
  static const bool plain_only = [] {
    const char* e = getenv("MUSED_KMEANS_ASSIGN");
    return e && e[0] == 'p';
  }();
  if (plain_only) return 0;
  for (int tr = 64; tr >= 16; tr >>= 1)
    if (km_tiled_lds(tr, d, k) <= KM_LDS_MAX) return tr;
  return 0;
}

// ---- any k x d (k <= 1024, d <= 512): mused_kmeans_lloyd_wide ---------------------------------------------------------
// The kernels above keep all k centres and a k x d block of sums in LDS, hence k * d <= 8192.  Here the iteration is three
// steps that each hold a tile: the E step streams the centres through LDS (kmw_assign_kernel), the M-step
// partials take a column tile of the sums per workgroup, and the centre sums are spread over workgroups.  Every sum keeps
// the order of the kernels above -- a dot product runs over c = 0 .. d - 1, the rows of a 256-row chunk are added in row
// order from 0.0, the chunks in chunk order, the shift as the per-thread sums e = t, t + 1024, ... into km_finish's tree
// -- so labels, info and the centres' bits equal mused_kmeans_lloyd's wherever both accept the shape.
constexpr size_t KMW_ASSIGN_LDS_DOUBLES = 19456;  // 152 KiB: row tile + centre tile of the E step

// E step.  A workgroup owns TR rows (LDS, pitch d + 1) and walks the centres in tiles of KT (LDS, pitch d + 1); PT = 256 / TR
// adjacent lanes share a row and take centres part, part + PT, ... of every tile, two at a time (two independent chains: each
// dot product is still sequential over c).  Candidates of one thread come in ascending j, so strict < keeps the first
// minimum; the PT lanes then agree on the lexicographic (distance, j) minimum.  The two rules are km_take and km_lane_min
// (kmeans_common.h) written out, and mbkm_assign_kernel (csrc/minibatch.hip) is this kernel without the Lloyd flags on
// pitched rows: one template for both, and calls of the helpers here, measured 3 to 9 % slower.
__global__ __launch_bounds__(KM_CHUNK) void kmw_assign_kernel(const double* __restrict__ Xc, int n, int d, int k,
                                                             const double* __restrict__ C, const double* __restrict__ csq,
                                                             int* __restrict__ labels, const int* __restrict__ labels_old,
                                                             KmInfo* __restrict__ info, int TR, int KT) {
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  if (info->done) return;  // converged in an earlier iteration of this batch of launches
  const int dp = d + 1, PT = KM_CHUNK / TR;
  double* xs = km_lds;                  // [TR][dp]
  double* cs = km_lds + (long)TR * dp;  // [KT][dp]
  const int t = threadIdx.x;
  const long r0 = (long)blockIdx.x * TR;
  const int nr = (int)min((long)TR, n - r0);
  for (int e = t; e < nr * d; e += KM_CHUNK) {
    const int r = e / d, c = e - r * d;
    xs[(long)r * dp + c] = Xc[(r0 + r) * d + c];
  }
  const int row = t / PT, part = t % PT;
  const double* x = xs + (long)row * dp;
  double best = KM_NO_DIST;
  int lab = KM_NO_LABEL;
  for (int j0 = 0; j0 < k; j0 += KT) {
    const int kt = min(KT, k - j0);
    __syncthreads();  // the row tile is staged / the previous centre tile is consumed
    for (int e = t; e < kt * d; e += KM_CHUNK) {
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
  if (part == 0 && row < nr) {
    labels[r0 + row] = lab;
    if (labels_old && labels_old[r0 + row] != lab) info->changed = 1;  // benign race: everybody writes 1
  }
}

// M-step partials of one 256-row chunk (blockIdx.x) and one tile of DT columns (blockIdx.y).  LDS: sums [k][DT], labels.
// The 256 threads are 256 / DT groups of DT columns; group g owns the clusters j = g mod 256 / DT, and every thread walks the
// chunk's rows in order, so the sum of a (cluster, column) is taken as km_assign_kernel takes it.
__global__ __launch_bounds__(KM_CHUNK) void kmw_partial_kernel(const double* __restrict__ Xc, int n, int d, int k,
                                                              const int* __restrict__ labels, double* __restrict__ psum,
                                                              int* __restrict__ pcnt, const KmInfo* __restrict__ info, int DT) {
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  if (info->done) return;
  double* sS = km_lds;                                      // [k][DT]
  int* sL = reinterpret_cast<int*>(sS + (long)k * DT);      // [KM_CHUNK]
  const int t = threadIdx.x, c0 = blockIdx.y * DT;
  const long r0 = (long)blockIdx.x * KM_CHUNK;
  const int rows = (int)min((long)KM_CHUNK, n - r0);
  const int gmask = KM_CHUNK / DT - 1, c = t % DT, g = t / DT;  // DT is a power of two
  for (int e = t; e < k * DT; e += KM_CHUNK) sS[e] = 0.0;
  sL[t] = t < rows ? labels[r0 + t] : -1;
  __syncthreads();
  if (c0 + c < d) {
    const double* x = Xc + r0 * d + c0 + c;
    for (int r = 0; r < rows; ++r) {
      const int j = sL[r];
      if ((j & gmask) == g && (unsigned)j < (unsigned)k) sS[(long)j * DT + c] += x[(long)r * d];
    }
  }
  if (blockIdx.y == 0) km_chunk_counts(sL, rows, k, pcnt + (long)blockIdx.x * k);
  __syncthreads();
  for (int e = t; e < k * DT; e += KM_CHUNK) {
    const int j = e / DT, cc = e - j * DT;
    if (c0 + cc < d) psum[((long)blockIdx.x * k + j) * d + c0 + cc] = sS[e];
  }
}

// M step, first half: element e of the centres from the chunk partials (chunks in order) -- km_update_kernel's arithmetic
// with one thread per element over as many workgroups as k * d asks for.  shift[e] = new - old for the second half.
__global__ __launch_bounds__(256) void kmw_centres_kernel(const double* __restrict__ psum, const int* __restrict__ pcnt,
                                                         int nchunk, int k, int d, double* __restrict__ C,
                                                         double* __restrict__ shift, KmInfo* __restrict__ info) {
  if (info->done) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= k * d) return;
  const int j = e / d;
  int cnt = 0;
  for (int ch = 0; ch < nchunk; ++ch) cnt += pcnt[(long)ch * k + j];
  if (cnt == 0) info->empty = 1;
  double s = 0.0;
  for (int ch = 0; ch < nchunk; ++ch) s += psum[(long)ch * k * d + e];
  const double nw = cnt > 0 ? s * (1.0 / (double)cnt) : C[e];
  shift[e] = nw - C[e];
  C[e] = nw;
}

// M step, second half: the total squared shift in km_update_kernel's order, then km_finish as there.
__global__ __launch_bounds__(1024) void kmw_finish_kernel(const double* __restrict__ shift, int k, int d,
                                                         const double* __restrict__ C, double* __restrict__ csq, double tol,
                                                         int first_iter, KmInfo* __restrict__ info) {
  if (info->done) return;
  double acc = 0.0;  // this thread's share of the squared shift, elements in a fixed order
  for (int e = threadIdx.x; e < k * d; e += 1024) acc = fma(shift[e], shift[e], acc);
  km_finish(acc, C, k, d, csq, tol, first_iter, info);
}

// Tiles of the wide kernels: TR rows and KT centres of the E step within its budget (km_stream_tiles); DT columns
// (64 / 32 / 16) of the M-step partials: the widest whose k x DT sums stay within 64 KiB (several workgroups per CU), 16
// beyond that (128 KiB at k = 1024), and no wider than d needs.
static size_t kmw_partial_lds(int dt, int k) { return 8 * (size_t)k * dt + 4 * KM_CHUNK + 16; }
static bool kmw_tiles(int d, int k, int* TR, int* KT, int* DT) {
  if (d <= 0 || k <= 0 || d > 512 || k > 1024) return false;
  if (!km_stream_tiles(KMW_ASSIGN_LDS_DOUBLES, d, k, TR, KT)) return false;
  int dt = 16;
  for (int w : {64, 32})
    if (8 * (size_t)k * w <= 64 * 1024) {
      dt = w;
      break;
    }
  while (dt > 16 && dt / 2 >= d) dt /= 2;
  *DT = dt;
  return kmw_partial_lds(dt, k) <= KM_LDS_MAX;
}

// The workspace of both entries; `shift` (k x d) only in the wide one.  The bytes count 8 n for the n labels of lab2 and
// 4096 on top, which covers the carver's rounding (seven arrays).
struct KmWs {
  double *Xc, *psum, *shift, *csq;
  int *pcnt, *lab2;
  KmInfo* info;
};
static long km_ws_bytes(int n, int d, int k, bool wide) {
  const long nchunk = cdiv(n, KM_CHUNK);
  return 8l * n * d + 8l * nchunk * k * d + (wide ? 8l * k * d : 0) + 4l * nchunk * k + 8l * k + 8l * n + 4096;
}
static KmWs km_carve(void* ws, int n, int d, int k, bool wide) {
  const size_t nchunk = cdiv(n, KM_CHUNK), kd = (size_t)k * d;
  WsCarver c{(char*)ws};
  KmWs w;
  w.Xc = c.take<double>((size_t)n * d);
  w.psum = c.take<double>(nchunk * kd);
  w.shift = wide ? c.take<double>(kd) : nullptr;
  w.csq = c.take<double>(k);
  w.pcnt = c.take<int>(nchunk * k);
  w.lab2 = c.take<int>(n);
  w.info = c.take<KmInfo>(1);
  return w;
}

// The Lloyd iterations of both entries, after their argument checks.  estep(labels, labels_old or null, want_sums) queues
// the E step of an iteration and, with want_sums, the M-step partials; mstep(first_iter) queues the rest of the M step,
// which ends in km_finish.  BLOCKING: reads KmInfo every four iterations.
template <typename EStep, typename MStep>
static int km_lloyd_run(const double* X, long ld, int n, int d, int k, const double* mean, double* centers, int max_iter,
                        int* labels_out, int* info_out, const KmWs& w, hipStream_t st, EStep estep, MStep mstep) {
  MUSED_CHECK_HIP(hipMemsetAsync(w.info, 0, sizeof(KmInfo), st));
  hipLaunchKernelGGL(km_center_kernel, dim3(cdiv((long)n * d, 256)), dim3(256), 0, st, X, ld, mean, n, d, w.Xc);
  hipLaunchKernelGGL(km_csq_kernel, dim3(cdiv(k, 64)), dim3(64), 0, st, centers, k, d, w.csq);
  KmInfo h = {};
  int* cur = labels_out;
  int* old = w.lab2;
  int it = 0;
  while (it < max_iter && !h.done) {
    const int batch = (max_iter - it) < 4 ? (max_iter - it) : 4;  // iterations between two reads of the stopping flag
    for (int b = 0; b < batch; ++b, ++it) {
      estep(cur, it > 0 ? old : (const int*)nullptr, 1);
      mstep(it == 0 ? 1 : 0);
      int* tmp = cur; cur = old; old = tmp;  // `old` now holds the labels of the iteration just queued
    }
    MUSED_LAUNCH_CHECK();
    MUSED_CHECK_HIP(hipMemcpyAsync(&h, w.info, sizeof(h), hipMemcpyDeviceToHost, st));
    MUSED_CHECK_HIP(hipStreamSynchronize(st));
    if (h.empty) break;
  }
  // labels of the last iteration that RAN are in one of the two buffers: iterations queued after convergence returned at
  // once, so parity of h.iters tells which.  Iteration i (0-based) wrote labels_out when i is even.
  int* last = ((h.iters - 1) % 2 == 0) ? labels_out : w.lab2;
  if (h.done != 1 && !h.empty) {
    // not strictly converged: labels must match the final centres (one more E step, no update)
    MUSED_CHECK_HIP(hipMemsetAsync(&w.info->done, 0, sizeof(int), st));
    estep(labels_out, (const int*)nullptr, 0);
    MUSED_LAUNCH_CHECK();
  } else if (last != labels_out) {
    MUSED_CHECK_HIP(hipMemcpyAsync(labels_out, last, 4l * n, hipMemcpyDeviceToDevice, st));
  }
  MUSED_CHECK_HIP(hipStreamSynchronize(st));
  info_out[0] = h.iters; info_out[1] = h.done; info_out[2] = h.empty; info_out[3] = 0;
  return MUSED_OK;
}

}  // namespace mused

using namespace mused;

extern "C" {

// workspace bytes for mused_kmeans_lloyd_wide; -1 for a shape it rejects
long mused_kmeans_wide_ws_bytes(int n, int d, int k) {
  return n <= 0 || d <= 0 || k <= 0 || k > 1024 || d > 512 || k > n ? -1 : km_ws_bytes(n, d, k, true);
}

// diagnostic: out[0..2] = {rows per tile, centres per tile of the E step, columns per tile of the M-step partials} that
// mused_kmeans_lloyd_wide launches for (d, k).  LDS: 8 (out[0] + out[1]) (d + 1) and 8 k out[2] + 1040 bytes.
int mused_kmeans_wide_tiles(int d, int k, int* out) {
  MUSED_REQUIRE(out, "mused_kmeans_wide_tiles: bad arguments");
  MUSED_REQUIRE(kmw_tiles(d, k, out, out + 1, out + 2), "mused_kmeans_wide_tiles: k <= 1024 and d <= 512 (got k = %d, d = %d)", k, d);
  return MUSED_OK;
}

// mused_kmeans_lloyd for any k x d within k <= 1024, d <= 512: the same arguments, contract and -- where both accept the
// shape -- bits.  ws: mused_kmeans_wide_ws_bytes(n, d, k) bytes.  BLOCKING.
int mused_kmeans_lloyd_wide(const double* X, long ld, int n, int d, int k, const double* mean, double* centers, double tol,
                            int max_iter, int* labels_out, int* info_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && mean && centers && labels_out && info_out && ws && n > 0 && d > 0 && k > 0 && k <= n && ld >= d,
                "mused_kmeans_lloyd_wide: bad arguments");
  MUSED_REQUIRE(k <= 1024 && d <= 512, "mused_kmeans_lloyd_wide: k <= 1024 and d <= 512 (got k = %d, d = %d)", k, d);
  MUSED_REQUIRE(ws_bytes >= mused_kmeans_wide_ws_bytes(n, d, k), "mused_kmeans_lloyd_wide: workspace too small");
  int TR = 0, KT = 0, DT = 0;
  MUSED_REQUIRE(kmw_tiles(d, k, &TR, &KT, &DT), "mused_kmeans_lloyd_wide: no tile fits d = %d, k = %d", d, k);
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = cdiv(n, KM_CHUNK);
  const KmWs w = km_carve(ws, n, d, k, true);
  static LdsOptIn opt[2];
  hipError_t aerr = allow_dynamic_lds(opt[0], reinterpret_cast<const void*>(kmw_assign_kernel), 8 * KMW_ASSIGN_LDS_DOUBLES);
  aerr = allow_dynamic_lds(aerr, opt[1], reinterpret_cast<const void*>(kmw_partial_kernel), KM_LDS_MAX);
  MUSED_CHECK_HIP(aerr);
  const size_t lds_e = 8 * (size_t)(TR + KT) * (d + 1), lds_m = kmw_partial_lds(DT, k);
  return km_lloyd_run(
      X, ld, n, d, k, mean, centers, max_iter, labels_out, info_out, w, st,
      [&](int* cur, const int* old, int want) {
        hipLaunchKernelGGL(kmw_assign_kernel, dim3(cdiv(n, TR)), dim3(KM_CHUNK), lds_e, st, w.Xc, n, d, k, centers, w.csq, cur,
                           old, w.info, TR, KT);
        if (want)
          hipLaunchKernelGGL(kmw_partial_kernel, dim3(nchunk, cdiv(d, DT)), dim3(KM_CHUNK), lds_m, st, w.Xc, n, d, k, cur,
                             w.psum, w.pcnt, w.info, DT);
      },
      [&](int first_iter) {
        hipLaunchKernelGGL(kmw_centres_kernel, dim3(cdiv(k * d, 256)), dim3(256), 0, st, w.psum, w.pcnt, nchunk, k, d, centers,
                           w.shift, w.info);
        hipLaunchKernelGGL(kmw_finish_kernel, dim3(1), dim3(1024), 0, st, w.shift, k, d, centers, w.csq, tol, first_iter,
                           w.info);
      });
}

// workspace bytes for mused_kmeans_lloyd
long mused_kmeans_ws_bytes(int n, int d, int k) {
  return n <= 0 || d <= 0 || k <= 0 ? -1 : km_ws_bytes(n, d, k, false);
}

// diagnostic: the sub-tile rows mused_kmeans_lloyd launches its E/M step with for (d, k): 64 / 32 / 16, 0 = row per thread
int mused_kmeans_assign_rows(int d, int k) {
  if (d <= 0 || k <= 0 || (long)k * d > 8192 || k > 1024) return -1;
  return km_assign_rows(d, k);
}

// Replaces the Lloyd iterations of KMeans(n_clusters = k, random_state = seed).fit_predict(X)
// (matrix_operations.py:149-153); arguments and contract: include/mused_hip.h.  tol comes by value: a caller that
// computed it on the device reads it first.  BLOCKING (reads its stopping flag every few iterations).  k * d <= 8192.
int mused_kmeans_lloyd(const double* X, long ld, int n, int d, int k, const double* mean, double* centers, double tol,
                       int max_iter, int* labels_out, int* info_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && mean && centers && labels_out && info_out && ws && n > 0 && d > 0 && k > 0 && k <= n && ld >= d,
                "mused_kmeans_lloyd: bad arguments");
  MUSED_REQUIRE((long)k * d <= 8192 && k <= 1024, "mused_kmeans_lloyd: k * d must be <= 8192");
  MUSED_REQUIRE(ws_bytes >= mused_kmeans_ws_bytes(n, d, k), "mused_kmeans_lloyd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nchunk = cdiv(n, KM_CHUNK);
  const KmWs w = km_carve(ws, n, d, k, false);
  const int tr = km_assign_rows(d, k);
  const size_t lds = tr ? km_tiled_lds(tr, d, k) : 8 * 2 * (size_t)k * d + 4 * (KM_CHUNK + (size_t)k) + 16;
  static LdsOptIn opt[4];
  hipError_t aerr = allow_dynamic_lds(opt[0], reinterpret_cast<const void*>(km_assign_kernel), 8 * 2 * 8192 + 4 * (KM_CHUNK + 1024) + 16);
  aerr = allow_dynamic_lds(aerr, opt[1], reinterpret_cast<const void*>(km_assign_tiled_kernel<64>), KM_LDS_MAX);
  aerr = allow_dynamic_lds(aerr, opt[2], reinterpret_cast<const void*>(km_assign_tiled_kernel<32>), KM_LDS_MAX);
  aerr = allow_dynamic_lds(aerr, opt[3], reinterpret_cast<const void*>(km_assign_tiled_kernel<16>), KM_LDS_MAX);
  MUSED_CHECK_HIP(aerr);
  // the fused E step + M-step partials of this (d, k): all four kernels take the same arguments
  const auto assign = tr == 64   ? km_assign_tiled_kernel<64>
                      : tr == 32 ? km_assign_tiled_kernel<32>
                      : tr == 16 ? km_assign_tiled_kernel<16>
                                 : km_assign_kernel;
  return km_lloyd_run(
      X, ld, n, d, k, mean, centers, max_iter, labels_out, info_out, w, st,
      [&](int* cur, const int* old, int want) {
        hipLaunchKernelGGL(assign, dim3(nchunk), dim3(KM_CHUNK), lds, st, w.Xc, n, d, k, centers, w.csq, cur, old, w.psum,
                           w.pcnt, w.info, want);
      },
      [&](int first_iter) {
        hipLaunchKernelGGL(km_update_kernel, dim3(1), dim3(1024), 0, st, w.psum, w.pcnt, nchunk, k, d, centers, w.csq, tol,
                           first_iter, w.info);
      });
}

}  // extern "C"
