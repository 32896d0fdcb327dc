// Cluster quality without ground truth, on fp64 rows and int32 labels on the device (specification: mused_amd/silhouette.py,
// pinned to scikit-learn 1.7 by the tests):
//
//   mused_silhouette        sklearn.metrics.silhouette_samples(X, labels, metric="euclidean") and the sum of the samples
//   mused_cluster_indices   sklearn.metrics.davies_bouldin_score and calinski_harabasz_score
//
// Both start from the rows ORDERED BY LABEL (sil_prepare): a stable LSD radix sort (radix_sort.h) of the sign-biased labels,
// the heads of the label runs scanned into a cluster number per sorted row (block_scan.h), the run offsets seg[0 .. C], and
// the rows gathered once into that order (even pitch: 16-byte loads for any d).  O(n + C) workspace beside the gathered rows
// (and, for the indices, the C x d centroids); no n x n and no n x C array.
//
// Silhouette.  In the sorted order the columns of any row tile arrive cluster by cluster.  A workgroup owns a 128-row tile
// and walks ALL column tiles in ascending order with the fp64 MFMA tile of gemm_f64.h (x_i . x_j in the accumulators, the
// arrangement of dbscan.hip); d(i, j) = sqrt(max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j)), exactly 0 for i == j.  A row needs three
// numbers: the running sum over the cluster whose columns are arriving, a(i) and the running minimum b(i); thread t < 128
// of the workgroup keeps them for row t of the tile.  Inside a column tile the kernel loops over the clusters the tile
// intersects (usually one or two; 128 one-row clusters are the worst case and take 128 turns): the four columns a lane holds
// of a row are added in column order, the 16 lanes that hold the row's 64 columns of the wave are combined by shuffles, the
// two column waves leave their halves in LDS and the row's thread adds them, left half first.  When a cluster's last column
// has passed, its sum becomes a(i) (own cluster, divided by size - 1) or a candidate for b(i) (divided by size).
// Every sum has ONE order that depends on nothing but (n, the sorted order): two runs give the same bits.  No atomic on a
// floating-point value anywhere in this file; the flags are integer atomicOr.
//
// Column slices.  Below 256 row tiles (n <= 32,640) n / 128 workgroups leave most of the GPU idle, so the column tiles are cut
// into S = col_slices(tiles) <= 16 runs of whole tiles and workgroup (row tile, slice) walks one run: about 512 workgroups.
// A cluster that lies inside a slice is settled there; of the clusters a slice cuts it leaves, per row, the sum of the one
// that began before the slice and ended in it (head) and of the one still open at its end (tail), with its a and b so far:
// 4 S n doubles.  sil_merge_kernel then walks a row's slices in ascending order and closes the cut clusters: carry + head.
// S depends on n alone, so the order of every sum still does.  S = 1 (n > 32,640, or MUSED_SIL_SLICES=1, read per call):
// the tile kernel settles every cluster itself and writes the samples; no merge.
//
// Not built: the symmetric half-square schedule of dbscan.hip (half the flops, but a tile then serves rows AND columns, whose
// clusters differ: n x C partial sums or floating-point atomics, i.e. either the memory or the reproducibility this entry
// promises).
//
// Indices.  One workgroup per cluster sums its rows per coordinate (8 row lanes per coordinate, combined in a fixed order),
// then the distance of every row to the centroid from the differences (sum (x - c)^2, a wave per row); a wave per cluster
// takes the centroid distances to all other clusters; one workgroup adds the per-cluster numbers in a fixed tree.
// O(n d + C^2 d) work.
#include "pair_tile.h"
#include "dbscan_common.h"
#include "radix_sort.h"

namespace mused {

constexpr int SIL_FLAG_NONFINITE = 2, SIL_FLAG_LABELS = 4;
constexpr int SIL_PART_DOUBLES = 2 /*parity*/ * 2 /*column waves*/ * GEMM_BM;
constexpr int SIL_LDS_BYTES = GEMM_LDS_BYTES + SIL_PART_DOUBLES * 8;
constexpr int SIL_REDUCE_THREADS = 1024;

struct SilWs {
  int *key[2], *val[2], *hist, *cid, *seg, *info;
  double *nrm, *Xs, *part;   // part: [slices][4][n] {head, tail, a, b} of a row in a slice (slices > 1 only)
  // indices only
  double *cen, *mean, *intra, *wk, *extra, *dbr, *mx;
};

static long sil_pitch(int d) { return ((long)d + 1) & ~1l; }

static size_t sil_layout(long n, int d, bool indices, char* base, SilWs* ws) {
  SilWs sizing;
  SilWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  for (int i = 0; i < 2; ++i) {
    w.key[i] = c.take<int>(n);
    w.val[i] = c.take<int>(n);
  }
  w.hist = c.take<int>(256 * (size_t)((n + RADIX_TILE - 1) / RADIX_TILE));
  w.cid = c.take<int>(n);
  w.seg = c.take<int>(n + 1);
  w.info = c.take<int>(4);
  w.nrm = c.take<double>(n);
  w.Xs = c.take<double>((size_t)n * sil_pitch(d));
  const int slices = col_slices(cdiv(n, GEMM_BM));
  w.part = (!indices && slices > 1) ? c.take<double>((size_t)slices * 4 * n) : nullptr;
  if (indices) {
    w.cen = c.take<double>((size_t)n * d);
    w.mean = c.take<double>(d);
    w.intra = c.take<double>(n);
    w.wk = c.take<double>(n);
    w.extra = c.take<double>(n);
    w.dbr = c.take<double>(n);
    w.mx = c.take<double>(n);
  }
  return c.off;
}

static bool sil_shape_ok(long n, int d) { return n >= 1 && n <= DB_MAX_ROWS && d >= 1 && d < (1 << 20); }

// ---- the rows ordered by label ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sil_key_kernel(const int* __restrict__ labels, int* __restrict__ key, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) key[i] = labels[i] ^ (int)0x80000000u;  // sign-biased: unsigned byte order is the labels' order
}

__global__ __launch_bounds__(256) void sil_head_kernel(const int* __restrict__ key, int* __restrict__ cid, int n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) cid[p] = (p == 0 || key[p - 1] != key[p]) ? 1 : 0;
}

// cid[] holds the exclusive scan of the heads, info[1] their number C: cid[p] <- the cluster of sorted row p, seg[c] <- its
// first row, seg[C] <- n; C outside [2, n - 1] raises flag 4
__global__ __launch_bounds__(256) void sil_seg_kernel(const int* __restrict__ key, int* __restrict__ cid, int* __restrict__ seg,
                                                     int* __restrict__ info, int n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const bool head = p == 0 || key[p - 1] != key[p];
  const int c = cid[p] + (head ? 1 : 0) - 1;
  cid[p] = c;
  if (head) seg[c] = p;
  if (p == 0) {
    const int C = info[1];
    seg[C] = n;
    if (C < 2 || C > n - 1) atomicOr(info, SIL_FLAG_LABELS);
  }
}

__global__ __launch_bounds__(256) void sil_gather_kernel(const double* __restrict__ X, long ld, const int* __restrict__ perm,
                                                        double* __restrict__ Xs, long lds, int d, long total) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long p = e / lds;
    const int j = (int)(e - p * lds);
    Xs[e] = j < d ? X[(long)perm[p] * ld + j] : 0.0;
  }
}

// ---- silhouette --------------------------------------------------------------------------------------------------------
struct SilArgs {
  const double* nrm;  // [n] squared norms of the sorted rows
  const int* cid;     // [n] cluster of a sorted row
  const int* seg;     // [C + 1] first sorted row of a cluster
  const int* perm;    // [n] caller's row of a sorted row
  const int* info;    // {flags, C, 0, 0}
  double* samples;    // [n] caller's order
  double* part;       // [slices][4][n], slices > 1
};

constexpr double SIL_A_UNSET = -1.0;  // (sums of distances are >= 0 or NaN)

// s(i) from a(i), b(i) and the size of the row's cluster
__device__ __forceinline__ double sil_sample(double av, double bv, int size) {
  const double s = (bv - av) / fmax(av, bv);
  return (size == 1 || !(s == s)) ? 0.0 : s;  // scikit-learn's nan_to_num: a row alone in its cluster, 0 / 0
}

template <bool VEC>
__global__ __launch_bounds__(GEMM_THREADS, 2) void sil_tile_kernel(GemmArgs g, SilArgs a, int tiles, int slices) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (a.info[0] != 0) return;  // flagged: nothing is written (uniform over the grid)
  double* part = smem + GEMM_LDS_BYTES / 8;  // [parity][column wave][row of the tile]
  const int n = g.M;
  // workgroup (row tile, slice), row tile fastest: the workgroups in flight walk the same column panels
  const int slice = blockIdx.x / tiles;
  const int m0 = (blockIdx.x - slice * tiles) * GEMM_BM;
  const int t_lo = (int)((long)slice * tiles / slices), t_hi = (int)((long)(slice + 1) * tiles / slices);
  const int col_lo = t_lo * GEMM_BN;
  const double* X = reinterpret_cast<const double*>(g.A);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1, kq = lane >> 4, li = lane & 15;

  // the state of row m0 + t, kept by thread t < 128
  const int orow = m0 + (int)threadIdx.x;
  const bool owner = threadIdx.x < GEMM_BM && orow < n;
  const int own = owner ? a.cid[orow] : -1;
  double run = 0.0, av = SIL_A_UNSET, bv = __longlong_as_double(0x7ff0000000000000ll), head = 0.0;
  int step = 0;  // cluster turns so far: the parity of `part`

  for (int J = t_lo; J < t_hi; ++J) {
    const int n0 = J * GEMM_BN;
    v4f64 acc[4][4];
    gemm_tile_mainloop<double, double, true, true, VEC>(g, X, X, m0, n0, 0, g.K, smem, acc);

    // Rows and columns beyond n read entry n - 1 (no branch around a load, as in dbscan_tile_kernel); such a column belongs
    // to no cluster, such a row has no owner.
    double ncol[4];
    int colv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      colv[j] = n0 + wc * 64 + j * 16 + li;
      ncol[j] = a.nrm[min(colv[j], n - 1)];
    }
    // the distances of the patch, in place
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr * 64 + i * 16 + kq + 4 * r;
        const double nrow = a.nrm[min(row, n - 1)];
        double t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double dd = nrow + ncol[j] - 2.0 * acc[i][j][r];
          t[j] = (row == colv[j]) ? 0.0 : sqrt(fmax(dd, 0.0));
        }
        // the row is complete HERE: left to itself the compiler interleaves the square roots of the whole patch and spills
        asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j][r] = t[j];
      }
    }
    const int c_lo = a.cid[n0], c_hi = a.cid[min(n0 + GEMM_BN, n) - 1];
    for (int c = c_lo; c <= c_hi; ++c, ++step) {
      const int s0 = a.seg[c], s1 = a.seg[c + 1];
      bool in[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) in[j] = colv[j] >= s0 && colv[j] < s1;  // (s1 <= n: columns beyond n are in no cluster)
      double* pw = part + (step & 1) * (2 * GEMM_BM) + wc * GEMM_BM + wr * 64;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double p = 0.0;
#pragma unroll
          for (int j = 0; j < 4; ++j) p += in[j] ? acc[i][j][r] : 0.0;
          // the 16 lanes that share kq hold the 64 columns of this row in this wave
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) p += __shfl_xor(p, o);
          asm volatile("" : "+v"(p));  // (one row's reduction at a time)
          if (li == 0) pw[i * 16 + kq + 4 * r] = p;
        }
      }
      // One barrier a turn: the halves of turn s are read behind it from part[s & 1]; a wave writes that half again in turn
      // s + 2, behind the barrier of turn s + 1, which the readers reach only after their reads.
      __syncthreads();
      if (threadIdx.x < GEMM_BM) {
        const double* pr = part + (step & 1) * (2 * GEMM_BM) + threadIdx.x;
        run += pr[0] + pr[GEMM_BM];
        if (s1 <= n0 + GEMM_BN) {  // the cluster's last column has passed
          const int size = s1 - s0;
          if (s0 < col_lo) head = run;  // it began before this slice: sil_merge_kernel closes it
          else if (c == own) av = run / (double)(size - 1);
          else bv = fmin(bv, run / (double)size);
          run = 0.0;
        }
      }
    }
  }
  if (!owner) return;
  if (slices == 1) {
    a.samples[a.perm[orow]] = sil_sample(av, bv, a.seg[own + 1] - a.seg[own]);
  } else {
    double* p = a.part + (size_t)slice * 4 * n + orow;
    p[0] = head;
    p[(size_t)n] = run;  // the cluster still open at the slice's end (0 without one)
    p[2 * (size_t)n] = av;
    p[3 * (size_t)n] = bv;
  }
}

// slices > 1: sorted row p takes its slices in ascending order; a cluster cut by slice boundaries is closed where it ends
__global__ __launch_bounds__(256) void sil_merge_kernel(SilArgs a, int n, int tiles, int slices) {
  if (a.info[0] != 0) return;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int own = a.cid[p];
  double av = SIL_A_UNSET, bv = __longlong_as_double(0x7ff0000000000000ll), carry = 0.0;
  for (int s = 0; s < slices; ++s) {
    const int col_lo = (int)((long)s * tiles / slices) * GEMM_BN;
    const int col_hi = min((int)((long)(s + 1) * tiles / slices) * GEMM_BN, n);
    const int cf = a.cid[col_lo], cl = a.cid[col_hi - 1];
    const bool before = a.seg[cf] < col_lo, open = a.seg[cl + 1] > col_hi;
    const double* q = a.part + (size_t)s * 4 * n + p;
    const double head = q[0], tail = q[(size_t)n], sa = q[2 * (size_t)n], sb = q[3 * (size_t)n];
    if (sa != SIL_A_UNSET) av = sa;  // (a NaN, the 0 / 0 of a row alone in its cluster, is taken too)
    bv = fmin(bv, sb);
    if (before) {
      if (cf == cl && open) {  // one cluster covers the whole slice and goes on
        carry += tail;
        continue;
      }
      const double tot = carry + head;
      const int size = a.seg[cf + 1] - a.seg[cf];
      if (cf == own) av = tot / (double)(size - 1);
      else bv = fmin(bv, tot / (double)size);
      carry = 0.0;
    }
    if (open) carry = tail;
  }
  a.samples[a.perm[p]] = sil_sample(av, bv, a.seg[own + 1] - a.seg[own]);
}

// v[0 .. m) added by ONE workgroup in a fixed order: thread t takes t, t + T, ..., then a tree over the threads
__device__ __forceinline__ double sil_block_sum(const double* __restrict__ v, int m, double* red /*[SIL_REDUCE_THREADS]*/) {
  double s = 0.0;
  for (int i = threadIdx.x; i < m; i += SIL_REDUCE_THREADS) s += v[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = SIL_REDUCE_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double sil_block_max(const double* __restrict__ v, int m, double* red) {
  double s = 0.0;
  for (int i = threadIdx.x; i < m; i += SIL_REDUCE_THREADS) s = fmax(s, v[i]);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = SIL_REDUCE_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

struct SilInfoOut {
  int flags, clusters;
  double sum;
};

__global__ __launch_bounds__(SIL_REDUCE_THREADS) void sil_finish_kernel(const double* __restrict__ samples, const int* __restrict__ info,
                                                                       SilInfoOut* __restrict__ out, int n) {
  __shared__ double red[SIL_REDUCE_THREADS];
  const int flags = info[0];
  const double s = flags ? 0.0 : sil_block_sum(samples, n, red);  // (uniform)
  if (threadIdx.x == 0) {
    out->flags = flags;
    out->clusters = info[1];
    out->sum = flags ? __longlong_as_double(0x7ff8000000000000ll) : s;
  }
}

// ---- Davies-Bouldin and Calinski-Harabasz ----------------------------------------------------------------------------------
struct IdxArgs {
  const double* Xs;
  long lds;
  const int* seg;
  const int* info;
  double *cen, *mean, *intra, *wk, *extra, *dbr, *mx;
  int n, d;
};

// cluster c: cen[c][.] <- the mean of its rows, intra[c] <- the mean distance to it, wk[c] <- the sum of the squared distances
__global__ __launch_bounds__(256) void idx_centroid_kernel(IdxArgs a) {
  __shared__ double red[8][32];
  __shared__ double wsum[2][4];
  if (a.info[0] != 0) return;
  const int C = a.info[1], t = threadIdx.x, tx = t & 31, ty = t >> 5, lane = t & 63, w = t >> 6;
  for (int c = blockIdx.x; c < C; c += gridDim.x) {
    const int s0 = a.seg[c], s1 = a.seg[c + 1];
    const double m = (double)(s1 - s0);
    double* cen = a.cen + (long)c * a.d;
    for (int j0 = 0; j0 < a.d; j0 += 32) {
      const int j = j0 + tx;
      double s = 0.0;
      if (j < a.d)
        for (int p = s0 + ty; p < s1; p += 8) s += a.Xs[(long)p * a.lds + j];
      red[ty][tx] = s;
      __syncthreads();
      if (ty == 0 && j < a.d) {
        double tot = red[0][tx];
#pragma unroll
        for (int q = 1; q < 8; ++q) tot += red[q][tx];
        cen[j] = tot / m;
      }
      __syncthreads();  // (also: the centroid is visible to the workgroup)
    }
    double ds = 0.0, d2s = 0.0;
    for (int p = s0 + w; p < s1; p += 4) {
      const double* x = a.Xs + (long)p * a.lds;
      double q = 0.0;
      for (int j = lane; j < a.d; j += 64) {
        const double df = x[j] - cen[j];
        q += df * df;
      }
      q = wave_sum(q);
      ds += sqrt(q);
      d2s += q;
    }
    if (lane == 0) {
      wsum[0][w] = ds;
      wsum[1][w] = d2s;
    }
    __syncthreads();
    if (t == 0) {
      a.intra[c] = (((wsum[0][0] + wsum[0][1]) + wsum[0][2]) + wsum[0][3]) / m;
      a.wk[c] = ((wsum[1][0] + wsum[1][1]) + wsum[1][2]) + wsum[1][3];
    }
    __syncthreads();
  }
}

// mean[j] <- sum_c size_c cen[c][j] / n, clusters in ascending order
__global__ __launch_bounds__(256) void idx_mean_kernel(IdxArgs a) {
  if (a.info[0] != 0) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.d) return;
  const int C = a.info[1];
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += (double)(a.seg[c + 1] - a.seg[c]) * a.cen[(long)c * a.d + j];
  a.mean[j] = s / (double)a.n;
}

// a wave per cluster k: extra[k] = size_k |c_k - mean|^2, dbr[k] = max_l (intra_k + intra_l) / M_kl with M_kl = |c_k - c_l|
// (a zero distance counts as infinite, the diagonal included: ratio 0), mx[k] = max_l M_kl
__global__ __launch_bounds__(256) void idx_pair_kernel(IdxArgs a) {
  if (a.info[0] != 0) return;
  const int C = a.info[1], lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int k = blockIdx.x * 4 + w; k < C; k += gridDim.x * 4) {
    const double* ck = a.cen + (long)k * a.d;
    double q = 0.0;
    for (int j = lane; j < a.d; j += 64) {
      const double df = ck[j] - a.mean[j];
      q += df * df;
    }
    q = wave_sum(q);
    const double sk = a.intra[k];
    double R = 0.0, M = 0.0;
    for (int l = 0; l < C; ++l) {
      if (l == k) continue;
      const double* cl = a.cen + (long)l * a.d;
      double e = 0.0;
      for (int j = lane; j < a.d; j += 64) {
        const double df = ck[j] - cl[j];
        e += df * df;
      }
      e = sqrt(wave_sum(e));
      M = fmax(M, e);
      R = fmax(R, e == 0.0 ? 0.0 : (sk + a.intra[l]) / e);
    }
    if (lane == 0) {
      a.extra[k] = (double)(a.seg[k + 1] - a.seg[k]) * q;
      a.dbr[k] = R;
      a.mx[k] = M;
    }
  }
}

__global__ __launch_bounds__(SIL_REDUCE_THREADS) void idx_finish_kernel(IdxArgs a, double* __restrict__ out, int* __restrict__ info_out) {
  __shared__ double red[SIL_REDUCE_THREADS];
  const int flags = a.info[0], C = a.info[1];
  if (threadIdx.x == 0) {
    info_out[0] = flags;
    info_out[1] = C;
    info_out[2] = info_out[3] = 0;
  }
  if (flags) return;  // (uniform) `out` is left as it is
  const double sumR = sil_block_sum(a.dbr, C, red);
  const double B = sil_block_sum(a.extra, C, red);
  const double W = sil_block_sum(a.wk, C, red);
  const double maxS = sil_block_max(a.intra, C, red);
  const double maxM = sil_block_max(a.mx, C, red);
  if (threadIdx.x == 0) {
    // scikit-learn: np.allclose(intra_dists, 0) or np.allclose(centroid_distances, 0) -> 0.0 (atol 1e-8)
    out[0] = (maxS <= 1e-8 || maxM <= 1e-8) ? 0.0 : sumR / (double)C;
    out[1] = (W == 0.0) ? 1.0 : B * (double)(a.n - C) / (W * ((double)C - 1.0));
  }
}

// Orders the rows by label on the stream: w.val[0] = the permutation, w.cid / w.seg / w.info, the gathered rows and norms.
static int sil_prepare(const double* X, long n, int d, long ld, const int* labels, const SilWs& w, hipStream_t st) {
  const dim3 rows(cdiv(n, 256)), blk(256);
  MUSED_CHECK_HIP(hipMemsetAsync(w.info, 0, 16, st));
  hipLaunchKernelGGL(sil_key_kernel, rows, blk, 0, st, labels, w.key[0], (int)n);
  int cur = 0;
  for (int shift = 0; shift < 32; shift += 8) {
    const int rc = radix_sort_pass(w.key[cur], shift ? w.val[cur] : nullptr, (int)n, RadixCount{(int)n, nullptr}, shift, w.hist,
                                   w.key[cur ^ 1], w.val[cur ^ 1], nullptr, nullptr, st);
    if (rc) return rc;
    cur ^= 1;
  }
  // (four passes: the sorted pairs are back in key[0], val[0])
  hipLaunchKernelGGL(sil_head_kernel, rows, blk, 0, st, w.key[0], w.cid, (int)n);
  hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, st, w.cid, (int)n, w.info + 1);
  hipLaunchKernelGGL(sil_seg_kernel, rows, blk, 0, st, w.key[0], w.cid, w.seg, w.info, (int)n);
  const long lds = sil_pitch(d), total = n * lds;
  const int gblocks = (int)(total / 256 + 1 < 65536 ? total / 256 + 1 : 65536);
  hipLaunchKernelGGL(sil_gather_kernel, dim3(gblocks), blk, 0, st, X, ld, w.val[0], w.Xs, lds, d, total);
  MUSED_LAUNCH_CHECK();
  const int rc = mused_row_sq_norms(w.Xs, MUSED_F64, n, d, lds, w.nrm, (void*)st);
  if (rc) return rc;
  hipLaunchKernelGGL(norms_finite_kernel, rows, blk, 0, st, w.nrm, (int)n, w.info, SIL_FLAG_NONFINITE);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// the tile kernel over (row tile, slice) and, with several slices, their merge
static int sil_launch(const GemmArgs& g, const SilArgs& a, bool vec, int tiles, int slices, hipStream_t st) {
  const int rc = pair_launch<sil_tile_kernel<true>, sil_tile_kernel<false>>(vec, tiles * slices, SIL_LDS_BYTES, st, g, a, tiles, slices);
  if (rc) return rc;
  if (slices > 1) {
    hipLaunchKernelGGL(sil_merge_kernel, dim3(cdiv(g.M, 256)), dim3(256), 0, st, a, g.M, tiles, slices);
    MUSED_LAUNCH_CHECK();
  }
  return MUSED_OK;
}

}  // namespace mused

using namespace mused;

extern "C" {

// bytes of workspace mused_silhouette needs (-1: n outside [1, 2^19] or a bad d)
long mused_silhouette_ws_bytes(long n, int d) {
  if (!sil_shape_ok(n, d)) return -1;
  return (long)sil_layout(n, d, false, nullptr, nullptr);
}

// column slices mused_silhouette cuts n rows into (csrc/silhouette.hip, head of the file); -1 outside [1, 2^19]
int mused_silhouette_slices(long n) {
  if (n < 1 || n > DB_MAX_ROWS) return -1;
  return col_slices(cdiv(n, GEMM_BM));
}

long mused_cluster_indices_ws_bytes(long n, int d) {
  if (!sil_shape_ok(n, d)) return -1;
  return (long)sil_layout(n, d, true, nullptr, nullptr);
}

int mused_silhouette(const double* X, long n, int d, long ld, const int* labels, double* samples_out, void* info_out, void* ws,
                     long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && labels && samples_out && info_out && ws, "mused_silhouette: null argument");
  MUSED_REQUIRE(sil_shape_ok(n, d) && ld >= d, "mused_silhouette: bad shape (n=%ld d=%d ld=%ld; n <= 2^19)", n, d, ld);
  MUSED_REQUIRE(ws_bytes >= (long)sil_layout(n, d, false, nullptr, nullptr), "mused_silhouette: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  SilWs w;
  sil_layout(n, d, false, (char*)ws, &w);
  int rc;
  if ((rc = sil_prepare(X, n, d, ld, labels, w, st))) return rc;
  const long lds = sil_pitch(d);
  const GemmArgs g = self_product_args(w.Xs, lds, n, d);
  SilArgs a{w.nrm, w.cid, w.seg, w.val[0], w.info, samples_out, w.part};
  const int tiles = cdiv(n, GEMM_BM);
  const char* one = getenv("MUSED_SIL_SLICES");  // "1": no column slices (diagnostic; the workspace is sized for the default)
  const int slices = (one && one[0] == '1' && one[1] == 0) ? 1 : col_slices(tiles);
  if ((rc = sil_launch(g, a, vec_ok<double>(w.Xs, lds, 0), tiles, slices, st))) return rc;
  hipLaunchKernelGGL(sil_finish_kernel, dim3(1), dim3(SIL_REDUCE_THREADS), 0, st, samples_out, w.info, (SilInfoOut*)info_out, (int)n);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

int mused_cluster_indices(const double* X, long n, int d, long ld, const int* labels, double* out, int* info_out, void* ws,
                          long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && labels && out && info_out && ws, "mused_cluster_indices: null argument");
  MUSED_REQUIRE(sil_shape_ok(n, d) && ld >= d, "mused_cluster_indices: bad shape (n=%ld d=%d ld=%ld; n <= 2^19)", n, d, ld);
  MUSED_REQUIRE(ws_bytes >= (long)sil_layout(n, d, true, nullptr, nullptr), "mused_cluster_indices: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  SilWs w;
  sil_layout(n, d, true, (char*)ws, &w);
  int rc;
  if ((rc = sil_prepare(X, n, d, ld, labels, w, st))) return rc;
  IdxArgs a{w.Xs, sil_pitch(d), w.seg, w.info, w.cen, w.mean, w.intra, w.wk, w.extra, w.dbr, w.mx, (int)n, d};
  const int cblocks = (int)(n < 4096 ? n : 4096);
  hipLaunchKernelGGL(idx_centroid_kernel, dim3(cblocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(idx_mean_kernel, dim3(cdiv(d, 256)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(idx_pair_kernel, dim3(cdiv(cblocks, 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(idx_finish_kernel, dim3(1), dim3(SIL_REDUCE_THREADS), 0, st, a, out, info_out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
