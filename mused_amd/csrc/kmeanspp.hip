// The head of perform_clustering (matrix_operations.py:149-153 = sklearn KMeans(n_clusters, random_state=seed)) on the
// device: what KMeans.fit does BEFORE its Lloyd iterations (csrc/kmeans.hip).
//
//   mused_kmeans_moments   tol = mean(var(X, 0)) * 1e-4 and the column means (sklearn:cluster/_kmeans.py `_tolerance`,
//                          `fit`: X -= X.mean(axis=0)), with NumPy's own steps so that the means have NumPy's bits
//   mused_kmeans_seed      `_kmeans_plusplus` on the centred rows
//
// What couples k-means++ to NumPy's MT19937 stream is one `choice` for the first centre and one
// `uniform(size=n_local_trials)` per further centre; neither the number nor the order of the draws depends on the data, so the
// host draws them all up front (matrix_operations.kmeanspp_draws) and hands them over: `first` and U ((k - 1) x trials).
// Per added centre c (sklearn `_kmeans_plusplus`):
//
//   cum        = cumsum(closest_dist_sq)
//   cand[l]    = min(searchsorted(cum, U[c - 1][l] * current_pot), n - 1)
//   dist[l][i] = max(0, -2 x_cand[l] . x_i + |x_cand[l]|^2 + |x_i|^2)
//   dmin[l][i] = min(closest_dist_sq[i], dist[l][i]);  pot[l] = sum_i dmin[l][i]
//   best       = argmin_l pot[l] (first minimum);  centre c = row cand[best], closest_dist_sq = dmin[best], current_pot = pot[best]
//
// Two launches per step, no host synchronisation and no workgroup waiting for another:
//   kpp_dist_kernel   (grid over 64-row blocks) the L candidate rows against all rows: dmin and the block's share of pot
//   kpp_step_kernel   (ONE workgroup) closes the step just computed (pot from the block shares, argmin, centre) and opens
//                     the next one: the block shares of dmin[best] ARE the 64-row sums of the new closest_dist_sq, so the
//                     scan runs over the blocks and each search ends inside one block of 64 rows -- no pass over n
// dmin alternates between two buffers: closest_dist_sq of a step is row `best` of the previous step's buffer, read in
// place; it is copied out once, at the end.
//
// Floating point: fp64, every sum in a FIXED order (two runs give the same bits), dot products as fma chains over the
// columns in order like the Lloyd E step.  The sums are NOT taken in scikit-learn's order (np.cumsum, BLAS), so a decision
// can differ from scikit-learn's where it hangs on the last bits.  With S = sum_i |x_i|^2,
//   E = 4 (d + 8) 2^-52 (S + n max_i |x_i|^2)
// bounds the absolute error of a potential or a scan value under either order; info[0] is raised when a searched value
// lies within 2 E of an end of the interval it fell into, or the best potential lies within 2 E of the best potential of a
// candidate with ANOTHER row index.  The host then seeds that window with scikit-learn itself.
#include "internal.h"

namespace mused {

constexpr int KPP_MAX_TRIALS = 8;
constexpr int KPP_ROWS = 64;    // rows per workgroup of kpp_dist_kernel = rows of one block share
constexpr int KPP_TILE = 64;    // rows x columns of one LDS tile
constexpr int KPP_STEP_THREADS = 1024;

struct KppState {
  double E;             // the rounding bound above
  double pot;           // current_pot
  int cand[KPP_MAX_TRIALS];  // candidate rows of the step in flight
  int info[2];          // {ambiguity flag, steps done}
  int best;             // row of the previous step's dmin buffer that is closest_dist_sq now
  int pad;
};

// ---- moments --------------------------------------------------------------------------------------------------------
// One workgroup, a column per lane, rows in sequence: np.add.reduce(X, axis=0) adds row after row, so does np.var's sum of
// the squared deviations, and the chain over the rows is sequential by construction.  What can be hidden is the memory
// latency behind it: all 1024 threads fetch the next tile of rows (coalesced across the columns) into registers while the
// column lanes add up the current one from LDS.  Columns in groups of 512.  Contraction is off in this kernel: NumPy
// rounds the square before it adds it, an fma would not.
constexpr int KPP_MOM_THREADS = 1024;
constexpr int KPP_MOM_PER = 6;                                  // tile elements per thread
constexpr int KPP_MOM_TILE = KPP_MOM_THREADS * KPP_MOM_PER;     // 48 KB of LDS
constexpr int KPP_MOM_COLS = 512;

// sum over the rows, in row order, of x (SQ = false) or of (x - m)^2 (SQ = true) for column c0 + t of a group of cw columns
template <bool SQ>
__device__ __forceinline__ double kpp_column_chain(const double* __restrict__ X, long ld, int n, int c0, int cw, double m,
                                                   double* __restrict__ tile) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  const int R = KPP_MOM_TILE / cw;  // rows per tile
  int er[KPP_MOM_PER], ec[KPP_MOM_PER];
#pragma unroll
  for (int j = 0; j < KPP_MOM_PER; ++j) {
    const int e = t + j * KPP_MOM_THREADS;
    er[j] = e / cw;
    ec[j] = e - er[j] * cw;
  }
  double v[KPP_MOM_PER];
  auto fetch = [&](int r0) {
#pragma unroll
    for (int j = 0; j < KPP_MOM_PER; ++j)
      v[j] = (er[j] < R && r0 + er[j] < n) ? X[(long)(r0 + er[j]) * ld + c0 + ec[j]] : 0.0;
  };
  fetch(0);
  double s = 0.0;
  for (int r0 = 0; r0 < n; r0 += R) {
    __syncthreads();  // the previous tile is consumed
#pragma unroll
    for (int j = 0; j < KPP_MOM_PER; ++j) tile[t + j * KPP_MOM_THREADS] = v[j];
    __syncthreads();
    if (r0 + R < n) fetch(r0 + R);  // in flight during the chain below
    if (t < cw) {
      const int nr = min(R, n - r0);
      auto add = [&](double x) {
        if (SQ) {
          const double df = x - m;
          s += df * df;
        } else {
          s += x;
        }
      };
      int r = 0;
      for (; r + 16 <= nr; r += 16) {  // the LDS reads of 16 rows are issued ahead of the adds that wait for them
        double x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = tile[(r + j) * cw + t];
#pragma unroll
        for (int j = 0; j < 16; ++j) add(x[j]);
      }
      for (; r < nr; ++r) add(tile[r * cw + t]);
    }
  }
  return s;
}

__global__ __launch_bounds__(KPP_MOM_THREADS) void kpp_moments_kernel(const double* __restrict__ X, long ld, int n, int d,
                                                                     double* __restrict__ mean_out, double* __restrict__ tol_out) {
#pragma clang fp contract(off)
  __shared__ double tile[KPP_MOM_TILE];
  __shared__ double red[KPP_MOM_COLS];
  const int t = threadIdx.x;
  double vsum = 0.0;  // the variances of this thread's columns, in order
  for (int c0 = 0; c0 < d; c0 += KPP_MOM_COLS) {
    const int cw = min(KPP_MOM_COLS, d - c0);
    const double m = kpp_column_chain<false>(X, ld, n, c0, cw, 0.0, tile) / (double)n;
    if (t < cw) mean_out[c0 + t] = m;
    const double q = kpp_column_chain<true>(X, ld, n, c0, cw, m, tile);
    if (t < cw) vsum += q / (double)n;
  }
  if (t < KPP_MOM_COLS) red[t] = vsum;
  __syncthreads();
  for (int o = KPP_MOM_COLS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) tol_out[0] = (red[0] / (double)d) * 1e-4;
}

// ---- seeding --------------------------------------------------------------------------------------------------------
// Xc = X - mean and |Xc_i|^2; one wave per row, lanes stride the columns, butterfly sum (fixed order).
__global__ __launch_bounds__(256) void kpp_center_kernel(const double* __restrict__ X, long ld, const double* __restrict__ mean,
                                                        int n, int d, double* __restrict__ Xc, double* __restrict__ xsq) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;  // whole waves leave together
  double s = 0.0;
  for (int c = lane; c < d; c += 64) {
    const double v = X[(long)row * ld + c] - mean[c];
    Xc[(long)row * d + c] = v;
    s = fma(v, v, s);
  }
  s = wave_sum(s);
  if (lane == 0) xsq[row] = s;
}

// E from the row norms, the first centre, and the state of a fresh run.  One workgroup.
__global__ __launch_bounds__(KPP_STEP_THREADS) void kpp_setup_kernel(const double* __restrict__ xsq, int n, int d, int first,
                                                                   KppState* __restrict__ stt) {
  __shared__ double rs[KPP_STEP_THREADS], rm[KPP_STEP_THREADS];
  const int t = threadIdx.x;
  double s = 0.0, m = 0.0;
  for (int i = t; i < n; i += KPP_STEP_THREADS) {
    s += xsq[i];
    m = fmax(m, xsq[i]);
  }
  rs[t] = s;
  rm[t] = m;
  __syncthreads();
  for (int o = KPP_STEP_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) {
      rs[t] += rs[t + o];
      rm[t] = fmax(rm[t], rm[t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
    stt->E = 4.0 * (double)(d + 8) * 0x1p-52 * (rs[0] + (double)n * rm[0]);
    stt->pot = 0.0;
    for (int l = 0; l < KPP_MAX_TRIALS; ++l) stt->cand[l] = first;
    stt->info[0] = 0;
    stt->info[1] = 0;
    stt->best = 0;
  }
}

// dmin[l][i] = min(closest[i], dist(cand[l], i)) for the L candidates of the state, closest = dmin_prev[best] (init: no
// closest yet, L = 1), and
// ppot[l][block] = the block's rows of dmin[l] added up.  64 rows per workgroup (one LDS tile); wave w owns the
// candidates w and w + 4, its lanes the tile's rows.  Rows and candidate rows pass through LDS 64 columns at a time (loads
// coalesced, pitch 65: lanes read different banks); every dot product still runs over c = 0 .. d - 1 in sequence.
__global__ __launch_bounds__(256) void kpp_dist_kernel(const double* __restrict__ Xc, const double* __restrict__ xsq, int n, int d,
                                                      int L, int init, const double* __restrict__ dmin_prev,
                                                      const KppState* __restrict__ stt, double* __restrict__ dmin,
                                                      double* __restrict__ ppot, int nblk) {
  __shared__ double xs[KPP_TILE * (KPP_TILE + 1)];
  __shared__ double sc[KPP_MAX_TRIALS * KPP_TILE];
  __shared__ int s_cand[KPP_MAX_TRIALS];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  if (t < KPP_MAX_TRIALS) s_cand[t] = stt->cand[t];
  __syncthreads();
  const double* closest = dmin_prev + (long)stt->best * n;
  const int l0 = w, l1 = w + 4;
  const bool has0 = l0 < L, has1 = l1 < L;
  double acc0 = 0.0, acc1 = 0.0;
  const long r0 = (long)blockIdx.x * KPP_ROWS;
  for (int sub = 0; sub < KPP_ROWS / KPP_TILE; ++sub) {
    const long rb = r0 + (long)sub * KPP_TILE;
    if (rb >= n) break;  // uniform over the workgroup
    const int nr = (int)min((long)KPP_TILE, (long)n - rb);
    double dot0 = 0.0, dot1 = 0.0;
    for (int cb = 0; cb < d; cb += KPP_TILE) {
      const int cw = min(KPP_TILE, d - cb);
      __syncthreads();  // the previous tile is consumed
      for (int e = t; e < KPP_TILE * KPP_TILE; e += 256) {
        const int r = e >> 6, c = e & 63;
        if (r < nr && c < cw) xs[r * (KPP_TILE + 1) + c] = Xc[(rb + r) * d + cb + c];
      }
      for (int e = t; e < L * KPP_TILE; e += 256) {
        const int l = e >> 6, c = e & 63;
        if (c < cw) sc[e] = Xc[(long)s_cand[l] * d + cb + c];
      }
      __syncthreads();
      if (lane < nr) {
        const double* x = xs + lane * (KPP_TILE + 1);
        if (has1) {
#pragma unroll 8
          for (int c = 0; c < cw; ++c) {
            dot0 = fma(x[c], sc[l0 * KPP_TILE + c], dot0);
            dot1 = fma(x[c], sc[l1 * KPP_TILE + c], dot1);
          }
        } else if (has0) {
#pragma unroll 8
          for (int c = 0; c < cw; ++c) dot0 = fma(x[c], sc[l0 * KPP_TILE + c], dot0);
        }
      }
    }
    double m0 = 0.0, m1 = 0.0;
    if (lane < nr) {
      const long i = rb + lane;
      const double xi = xsq[i];
      const double cl = init ? 0.0 : closest[i];
      if (has0) {  // sklearn: distances = -2 X Y^T; += |x_cand|^2; += |x_i|^2; maximum(., 0)
        m0 = fmax((-2.0 * dot0 + xsq[s_cand[l0]]) + xi, 0.0);
        if (!init) m0 = fmin(cl, m0);
        dmin[(long)l0 * n + i] = m0;
      }
      if (has1) {
        m1 = fmax((-2.0 * dot1 + xsq[s_cand[l1]]) + xi, 0.0);
        m1 = fmin(cl, m1);
        dmin[(long)l1 * n + i] = m1;
      }
    }
    acc0 += wave_sum(m0);  // rows beyond n add 0.0
    acc1 += wave_sum(m1);
  }
  if (lane == 0) {
    if (has0) ppot[(long)l0 * nblk + blockIdx.x] = acc0;
    if (has1) ppot[(long)l1 * nblk + blockIdx.x] = acc1;
  }
}

// Closes step `c` (its L candidates are in dmin / ppot) and, unless it was the last one, opens step c + 1.  One workgroup.
//   close: pot[l] = sum of the block shares (lanes stride the blocks, butterfly); first minimum; margin to the best
//          candidate with another row index; centre c and its row index
//   open:  running sums of closest_dist_sq = dmin[best] in two levels.  Over the blocks: thread t owns the blocks
//          [t * ch, (t + 1) * ch), chunk sums, scan over the threads, then a second walk that finds, per trial, the first
//          block whose running sum reaches U * pot.  Inside that block: its 64 rows in sequence from the block's start value.
__global__ __launch_bounds__(KPP_STEP_THREADS) void kpp_step_kernel(const double* __restrict__ Xc, int n, int d, int c, int L,
                                                                  int Lnext, const double* __restrict__ Unext,
                                                                  const double* __restrict__ dmin, const double* __restrict__ ppot,
                                                                  int nblk, double* __restrict__ centers_out,
                                                                  int* __restrict__ indices_out, KppState* __restrict__ stt,
                                                                  int* __restrict__ info_dev) {
  __shared__ double s_pot[KPP_MAX_TRIALS];
  __shared__ double s_scan[KPP_STEP_THREADS];
  __shared__ double s_tgt[KPP_MAX_TRIALS], s_lo[KPP_MAX_TRIALS];
  __shared__ double s_rows[KPP_MAX_TRIALS][KPP_ROWS];
  __shared__ int s_blk[KPP_MAX_TRIALS], s_cand[KPP_MAX_TRIALS], s_amb[KPP_MAX_TRIALS];
  __shared__ int s_best, s_row, s_flag;
  constexpr int NONE = 0x7fffffff;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  if (w < L) {
    double s = 0.0;
    for (int b = lane; b < nblk; b += 64) s += ppot[(long)w * nblk + b];
    s = wave_sum(s);
    if (lane == 0) s_pot[w] = s;
  }
  __syncthreads();
  if (t == 0) {
    int best = 0;
    for (int l = 1; l < L; ++l)
      if (s_pot[l] < s_pot[best]) best = l;  // strict <: np.argmin takes the first minimum
    const double E2 = 2.0 * stt->E;
    int flag = 0;
    for (int l = 0; l < L; ++l)
      if (stt->cand[l] != stt->cand[best] && s_pot[l] - s_pot[best] <= E2) flag = 1;
    s_best = best;
    s_row = stt->cand[best];
    s_flag = flag;
    stt->pot = s_pot[best];
    stt->best = best;
    indices_out[c] = s_row;
  }
  __syncthreads();
  const int row = s_row;
  const double pot = s_pot[s_best];
  for (int e = t; e < d; e += KPP_STEP_THREADS) centers_out[(long)c * d + e] = Xc[(long)row * d + e];
  if (Lnext == 0) {  // the last centre
    if (t == 0) {
      stt->info[0] |= s_flag;
      stt->info[1] = c + 1;
      info_dev[0] = stt->info[0];
      info_dev[1] = c + 1;
    }
    return;
  }
  // ---- level 1: the blocks
  const double* bs = ppot + (long)s_best * nblk;
  const int ch = (nblk + KPP_STEP_THREADS - 1) / KPP_STEP_THREADS;
  const int b0 = min(nblk, t * ch), b1 = min(nblk, b0 + ch);
  double cs = 0.0;
  for (int b = b0; b < b1; ++b) cs += bs[b];
  s_scan[t] = cs;
  if (t < KPP_MAX_TRIALS) {
    s_tgt[t] = t < Lnext ? Unext[t] * pot : 0.0;  // rand_vals = uniform(size = L) * current_pot
    s_blk[t] = NONE;
  }
  __syncthreads();
  for (int o = 1; o < KPP_STEP_THREADS; o <<= 1) {  // inclusive scan over the chunk sums
    const double add = t >= o ? s_scan[t - o] : 0.0;
    __syncthreads();
    s_scan[t] += add;
    __syncthreads();
  }
  double run = t > 0 ? s_scan[t - 1] : 0.0;
  int fblk[KPP_MAX_TRIALS];
  double flo[KPP_MAX_TRIALS];
#pragma unroll
  for (int l = 0; l < KPP_MAX_TRIALS; ++l) {
    fblk[l] = NONE;
    flo[l] = 0.0;
  }
  for (int b = b0; b < b1; ++b) {
    const double before = run;
    run += bs[b];
#pragma unroll
    for (int l = 0; l < KPP_MAX_TRIALS; ++l) {
      if (l < Lnext && fblk[l] == NONE && run >= s_tgt[l]) {  // searchsorted, side = left: first cum >= value
        fblk[l] = b;
        flo[l] = before;
      }
    }
  }
#pragma unroll
  for (int l = 0; l < KPP_MAX_TRIALS; ++l)
    if (fblk[l] != NONE) atomicMin(&s_blk[l], fblk[l]);
  __syncthreads();
#pragma unroll
  for (int l = 0; l < KPP_MAX_TRIALS; ++l)
    if (fblk[l] != NONE && fblk[l] == s_blk[l]) s_lo[l] = flo[l];
  // ---- level 2: the rows of each trial's block (wave l stages them, thread l walks them)
  if (w < Lnext && s_blk[w] != NONE) {
    const double* src = dmin + (long)s_best * n;
    const long rb = (long)s_blk[w] * KPP_ROWS;
    for (int r = lane; r < KPP_ROWS; r += 64) s_rows[w][r] = rb + r < n ? src[rb + r] : 0.0;
  }
  __syncthreads();
  if (t < Lnext) {
    const double E2 = 2.0 * stt->E, tgt = s_tgt[t];
    int cand = n - 1, amb = 1;  // beyond the last running sum: np.clip(., n - 1); only rounding gets a value there
    if (s_blk[t] != NONE) {
      const long rb = (long)s_blk[t] * KPP_ROWS;
      const int nr = (int)min((long)KPP_ROWS, (long)n - rb);
      double cum = s_lo[t];
      cand = (int)rb + nr - 1;  // the block's share said the value is reached here; its rows in sequence may fall a rounding short
      bool found = false;
      for (int q = 0; q < nr && !found; q += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s_rows[t][q + j];  // zeros behind the last row
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const double before = cum;
          cum += v[j];
          if (!found && q + j < nr && cum >= tgt) {
            found = true;
            cand = (int)rb + q + j;
            amb = (cum - tgt <= E2) || (cand > 0 && tgt - before <= E2);
          }
        }
      }
    }
    s_cand[t] = cand;
    s_amb[t] = amb;
  }
  __syncthreads();
  if (t == 0) {
    int flag = s_flag;
    for (int l = 0; l < Lnext; ++l) {
      stt->cand[l] = s_cand[l];
      flag |= s_amb[l];
    }
    stt->info[0] |= flag;
    stt->info[1] = c + 1;
    info_dev[0] = stt->info[0];
    info_dev[1] = c + 1;
  }
}

// closest_dist_sq of the finished run, out of the last step's buffer
__global__ __launch_bounds__(256) void kpp_closest_kernel(const double* __restrict__ dmin, const KppState* __restrict__ stt, int n,
                                                         double* __restrict__ closest) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) closest[i] = dmin[(long)stt->best * n + i];
}

static inline long kpp_align(long b) { return (b + 255) & ~255l; }

}  // namespace mused

using namespace mused;

extern "C" {

int mused_kmeans_moments(const double* X, long ld, int n, int d, double* mean_out, double* tol_out, void* stream) {
  MUSED_REQUIRE(X && mean_out && tol_out && n > 0 && d > 0 && ld >= d, "mused_kmeans_moments: bad arguments");
  hipLaunchKernelGGL(kpp_moments_kernel, dim3(1), dim3(KPP_MOM_THREADS), 0, (hipStream_t)stream, X, ld, n, d, mean_out, tol_out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// workspace of mused_kmeans_seed: centred rows, row norms, closest, dmin (2 buffers of 8 x n), block shares (8 x blocks), state
long mused_kmeans_seed_ws_bytes(int n, int d, int k) {
  if (n <= 0 || d <= 0 || k <= 0) return -1;
  const long nblk = (n + KPP_ROWS - 1) / KPP_ROWS;
  return kpp_align(8l * n * d) + 2 * kpp_align(8l * n) + 2 * kpp_align(8l * KPP_MAX_TRIALS * n) +
         kpp_align(8l * KPP_MAX_TRIALS * nblk) + kpp_align(sizeof(KppState));
}

int mused_kmeans_seed(const double* X, long ld, int n, int d, int k, const double* mean, int first, const double* U, int trials,
                      double* centers_out, int* indices_out, int* info_dev, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && mean && centers_out && indices_out && info_dev && ws && n > 0 && d > 0 && k > 0 && k <= n && ld >= d,
                "mused_kmeans_seed: bad arguments");
  MUSED_REQUIRE(k <= 1024 && d <= 512, "mused_kmeans_seed: k <= 1024 and d <= 512");
  MUSED_REQUIRE(first >= 0 && first < n, "mused_kmeans_seed: first centre outside [0, n)");
  MUSED_REQUIRE(k == 1 || (U && trials >= 1 && trials <= KPP_MAX_TRIALS), "mused_kmeans_seed: 1 <= trials <= 8");
  MUSED_REQUIRE(ws_bytes >= mused_kmeans_seed_ws_bytes(n, d, k), "mused_kmeans_seed: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = cdiv(n, KPP_ROWS);
  char* w = (char*)ws;
  double* Xc = (double*)w; w += kpp_align(8l * n * d);
  double* xsq = (double*)w; w += kpp_align(8l * n);
  double* closest = (double*)w; w += kpp_align(8l * n);
  double* dmin[2];
  dmin[0] = (double*)w; w += kpp_align(8l * KPP_MAX_TRIALS * n);
  dmin[1] = (double*)w; w += kpp_align(8l * KPP_MAX_TRIALS * n);
  double* ppot = (double*)w; w += kpp_align(8l * KPP_MAX_TRIALS * nblk);
  KppState* stt = (KppState*)w;
  hipLaunchKernelGGL(kpp_center_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, X, ld, mean, n, d, Xc, xsq);
  hipLaunchKernelGGL(kpp_setup_kernel, dim3(1), dim3(KPP_STEP_THREADS), 0, st, xsq, n, d, first, stt);
  for (int c = 0; c < k; ++c) {
    const int L = c == 0 ? 1 : trials, Lnext = c + 1 < k ? trials : 0;
    hipLaunchKernelGGL(kpp_dist_kernel, dim3(nblk), dim3(256), 0, st, Xc, xsq, n, d, L, c == 0 ? 1 : 0, dmin[(c + 1) & 1], stt,
                       dmin[c & 1], ppot, nblk);
    hipLaunchKernelGGL(kpp_step_kernel, dim3(1), dim3(KPP_STEP_THREADS), 0, st, Xc, n, d, c, L, Lnext,
                       Lnext ? U + (long)c * trials : (const double*)nullptr, dmin[c & 1], ppot, nblk, centers_out, indices_out,
                       stt, info_dev);
  }
  hipLaunchKernelGGL(kpp_closest_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, dmin[(k - 1) & 1], stt, n, closest);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
