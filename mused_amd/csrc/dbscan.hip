// sklearn.cluster.DBSCAN(eps, min_samples, metric="euclidean").fit_predict on fp64 rows (perform_dbscan_clustering,
// matrix_operations.py:235-238) WITHOUT an n x n array, neighbour lists or an n x n bitmask: O(n) workspace.
//
// scikit-learn's index-order depth-first search has a closed form (mused_amd/dbscan.py, pinned to scikit-learn by the tests).
// With N(i) = { j : d2(i, j) <= eps^2 }, i included:
//   core rows      |N(i)| >= min_samples
//   clusters       connected components of the core rows under d2 <= eps^2, numbered by ascending smallest core index
//   non-core rows  the smallest label among the core neighbours, -1 without one
//
// All pair work runs on the fp64 MFMA tile of gemm_f64.h (a 128 x 128 tile of x_i . x_j left in the accumulators, the
// arrangement of knn_fused.hip); the distances are RECOMPUTED by each of the three tile passes (2 n^2 d flop per pass over the
// full square; the passes visit every unordered pair of row tiles once, by cyclic tile distance like knn_fused.hip, and
// serve both orientations of a tile from one evaluation, so the three passes decide every pair from the same bits):
//
//   dbscan_init       parent[i] = i, count[i] = 0, non-finite norm -> flag 2          (after mused_row_sq_norms)
//   tile pass COUNT   count[i] += |N(i) in the tile| (one atomic per row and wave); a pair i != j with
//                     |d2 - eps^2| <= tau(i, j) raises flag 1 (tau: below)
//   dbscan_core       tile flags (has core rows / has non-core rows), the number of core rows
//   tile pass UNION   union-find over the core-core edges: read-only find of both ends (roots cached per row and column
//                     of the thread's patch), compare-and-swap on parent[] only where the roots differ, the LARGER root
//                     hooked under the smaller -- parent[x] <= x always, so a component's final root is its smallest core
//                     index, which is what the numbering needs.  Tiles without core rows on either side exit at once.
//   dbscan_flatten    root[i] = find(i) for core rows, INT_MAX for the others
//   dbscan_rank       one workgroup: rank[i] = number of roots below i (exclusive prefix sum), the number of clusters
//   tile pass BORDER  non-core rows only: root[i] = min over the core neighbours of their final root (atomicMin; the rank is
//                     monotone in the root index, so the smallest root carries the smallest label).  Tiles that pair no
//                     non-core row with a core row exit at once.
//   dbscan_labels     labels[i] = rank[root[i]], -1 for INT_MAX
//
// Kernel boundaries are the only synchronisation between workgroups: no workgroup waits for another.  The union pass is
// lock-free: a failed compare-and-swap means the root was hooked by someone else in the meantime, and the loop goes on from
// its new parent.  Every atomic is a device-scope vector atomic on global memory.
//
// Rounding.  d2 = |x|^2 + |y|^2 - 2 x.y here and in scikit-learn's brute path (d > 15), sum (x - y)^2 in its k-d tree
// (d <= 15, its node bounds included); each is within (d + 8) 2^-52 (|x|^2 + |y|^2) of the exact value whatever the order of its sums (derivation:
// mused_amd/dbscan.py tau_coefficient), and eps * eps, pow(eps, 2) and the exact square lie within 1 ulp
// of one another.  tau(i, j) = 2 (d + 8) 2^-52 (|x_i|^2 + |x_j|^2) + 4 ulp(eps^2): where no pair is within tau of eps^2
// every comparison, and with it every label, equals scikit-learn's.  Otherwise flag 1 is raised and the caller runs
// scikit-learn itself: exact labels or a flag, never labels that hang on the last bits.
#include "pair_tile.h"
#include "dbscan_common.h"
#include "union_find.h"

namespace mused {

constexpr int DB_COUNT = 0, DB_UNION = 1, DB_BORDER = 2;

struct DbArgs {
  const double* nrm;  // [n] squared norms
  int* count;         // [n] |N(i)|
  int* parent;        // [n] union-find forest over the core rows, parent[x] <= x
  int* root;          // [n] final root of a core row / smallest final root among the core neighbours of another (DB_NONE: none)
  int* tflag;         // [tiles] DB_HAS_CORE | DB_HAS_NONCORE
  int* info;          // {flags, clusters, core rows, 0}
  double eps2, ctau, etau;  // tau(i, j) = ctau * (nrm[i] + nrm[j]) + etau
  int min_samples;
};

// tile (I, (I + delta) mod tiles), delta in [0, tiles / 2]: every unordered pair of row tiles once (pair_tile.h)
template <int PASS, bool VEC>
__global__ __launch_bounds__(GEMM_THREADS, 2) void dbscan_tile_kernel(GemmArgs g, DbArgs a, int tiles) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  int I, delta, J;
  pair_slot(tiles / 2 + 1, I, delta);
  if (!pair_tile(I, delta, tiles, J)) return;
  const bool both = (delta != 0);  // a diagonal tile holds both orientations of its pairs itself
  if (PASS == DB_UNION) {
    if (!(a.tflag[I] & DB_HAS_CORE) || !(a.tflag[J] & DB_HAS_CORE)) return;
  }
  if (PASS == DB_BORDER) {
    const int fi = a.tflag[I], fj = a.tflag[J];
    if (!(((fi & DB_HAS_NONCORE) && (fj & DB_HAS_CORE)) || ((fj & DB_HAS_NONCORE) && (fi & DB_HAS_CORE)))) return;
  }
  const int m0 = I * GEMM_BM, n0 = J * GEMM_BN;
  const double* X = reinterpret_cast<const double*>(g.A);
  v4f64 acc[4][4];
  gemm_tile_mainloop<double, double, true, true, VEC>(g, X, X, m0, n0, 0, g.K, smem, acc);

  int lane, wr, wc, kq, li;
  patch_lanes(lane, wr, wc, kq, li);
  const int n = g.M;

  // Rows and columns beyond n read entry n - 1 (no branch around a load: with branches inside the row loop the compiler sinks
  // the column side and the margin behind them and keeps the distances of the whole patch alive) and are masked by `ok`.
  double ncol[4];
  int ccol[4];  // COUNT: neighbours seen in the column; UNION: cached root; BORDER: core column: its root, else the running min
  bool cok[4], corec[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = patch_col(n0, wc, li) + j * 16;
    const int cc = min(col, n - 1);
    cok[j] = col < n;
    ncol[j] = a.nrm[cc];
    corec[j] = (PASS != DB_COUNT) && cok[j] && a.count[cc] >= a.min_samples;
    if (PASS == DB_COUNT) ccol[j] = 0;
    if (PASS == DB_UNION) ccol[j] = corec[j] ? db_find(a.parent, col) : -1;
    if (PASS == DB_BORDER) ccol[j] = corec[j] ? a.root[cc] : DB_NONE;
  }
  int rsum[16];  // COUNT / BORDER: the row's count / minimum over this wave's 64 columns
  // COUNT: smallest |d2 - eps^2| - tau of the patch (a running minimum instead of 64 comparison masks)
  double slack = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = patch_row(m0, wr, kq) + i * 16 + 4 * r;
      const int rc = min(row, n - 1);
      const bool rok = row < n;
      const double nrow = a.nrm[rc];
      const bool corer = (PASS != DB_COUNT) && rok && a.count[rc] >= a.min_samples;
      int racc = (PASS == DB_COUNT) ? 0 : (PASS == DB_UNION ? -1 : DB_NONE);  // count / cached root (lazy) / running min
      const int rroot = (PASS == DB_BORDER && corer) ? a.root[rc] : DB_NONE;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = patch_col(n0, wc, li) + j * 16;
        const bool ok = rok && cok[j];
        const double s = nrow + ncol[j];
        const double dd = s - 2.0 * acc[i][j][r];
        const bool same = (row == col);
        const bool in = ok && (same || dd <= a.eps2);
        if (PASS == DB_COUNT) {
          slack = fmin(slack, (ok && !same) ? fabs(dd - a.eps2) - (a.ctau * s + a.etau) : slack);
          racc += in ? 1 : 0;
          ccol[j] += in ? 1 : 0;
        }
        if (PASS == DB_UNION) {
          if (in && !same && corer && corec[j]) {
            if (racc < 0) racc = db_find(a.parent, row);
            if (racc != ccol[j]) racc = ccol[j] = db_unite(a.parent, racc, ccol[j]);
          }
        }
        if (PASS == DB_BORDER) {
          racc = (in && !corer && corec[j]) ? min(racc, ccol[j]) : racc;        // row side: the core column's root
          ccol[j] = (in && corer && !corec[j]) ? min(ccol[j], rroot) : ccol[j];  // column side: the core row's root
        }
      }
      if (PASS == DB_COUNT || PASS == DB_BORDER) {
        // the 16 lanes that share kq hold the 64 columns of this row in this wave
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const int x = __shfl_xor(racc, o);
          racc = (PASS == DB_COUNT) ? racc + x : min(racc, x);
        }
        rsum[i * 4 + r] = racc;
        // the row's results are complete HERE: left to itself the compiler postpones the margin and the column side of all
        // 16 rows behind the loop and spills the distances of the whole patch for it
        if (PASS == DB_BORDER) asm volatile("" : "+v"(ccol[0]), "+v"(ccol[1]), "+v"(ccol[2]), "+v"(ccol[3]), "+v"(rsum[i * 4 + r]));
        if (PASS == DB_COUNT) asm volatile("" : "+v"(slack), "+v"(ccol[0]), "+v"(ccol[1]), "+v"(ccol[2]), "+v"(ccol[3]), "+v"(rsum[i * 4 + r]));
      }
    }
  }
  if (PASS == DB_COUNT || PASS == DB_BORDER) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = patch_row(m0, wr, kq) + (q >> 2) * 16 + 4 * (q & 3);
      if (li == 0 && row < n) {
        if (PASS == DB_COUNT && rsum[q]) atomicAdd(a.count + row, rsum[q]);
        if (PASS == DB_BORDER && rsum[q] != DB_NONE) atomicMin(a.root + row, rsum[q]);
      }
    }
    // the 4 lanes that share li hold the 64 rows of this column in this wave; a diagonal tile has served both orientations of
    // its pairs from the row side
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int v = ccol[j];
      if (PASS == DB_BORDER && corec[j]) v = DB_NONE;  // (held the column's own root)
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const int x = __shfl_xor(v, o);
        v = (PASS == DB_COUNT) ? v + x : min(v, x);
      }
      const int col = patch_col(n0, wc, li) + j * 16;
      if (both && kq == 0 && col < n) {
        if (PASS == DB_COUNT && v) atomicAdd(a.count + col, v);
        if (PASS == DB_BORDER && v != DB_NONE) atomicMin(a.root + col, v);
      }
    }
  }
  if (PASS == DB_COUNT) {
    if (__ballot(slack <= 0.0) && lane == 0) atomicOr(a.info, 1);
  }
}

__global__ void dbscan_init_kernel(DbArgs a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4) a.info[i] = 0;
  if (i >= n) return;
  a.parent[i] = i;
  a.count[i] = 0;
  a.root[i] = DB_NONE;
}

__global__ void dbscan_core_kernel(DbArgs a, int n, int tiles) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < tiles) {
    int f = 0;
    const int hi = min(n, (i + 1) * GEMM_BM);
    for (int r = i * GEMM_BM; r < hi; ++r) f |= (a.count[r] >= a.min_samples) ? DB_HAS_CORE : DB_HAS_NONCORE;
    a.tflag[i] = f;
  }
  const bool core = i < n && a.count[i] >= a.min_samples;
  const int c = __popcll(__ballot(core));
  if (c && (threadIdx.x & 63) == 0) atomicAdd(a.info + 2, c);
}

__global__ void dbscan_flatten_kernel(DbArgs a, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || a.count[i] < a.min_samples) return;
  int x = i, p = a.parent[x];  // the forest is final: plain reads
  while (p != x) {
    x = p;
    p = a.parent[x];
  }
  a.root[i] = x;
}

__global__ void dbscan_labels_kernel(DbArgs a, const int* __restrict__ rank, int* __restrict__ labels, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = a.root[i];
  labels[i] = (r == DB_NONE) ? -1 : rank[r];
}

struct DbWs {
  double* nrm;
  int *count, *parent, *root, *rank, *tflag, *info;
};

static size_t db_layout(long n, char* base, DbWs* ws) {
  DbWs sizing;
  DbWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  w.nrm = c.take<double>(n);
  w.count = c.take<int>(n);
  w.parent = c.take<int>(n);
  w.root = c.take<int>(n);
  w.rank = c.take<int>(n);
  w.tflag = c.take<int>((n + GEMM_BM - 1) / GEMM_BM);
  w.info = c.take<int>(4);
  return c.off;
}

template <int PASS>
static int db_pass(const GemmArgs& g, const DbArgs& a, bool vec, int tiles, hipStream_t st) {
  return pair_launch<dbscan_tile_kernel<PASS, true>, dbscan_tile_kernel<PASS, false>>(vec, pair_grid(tiles), GEMM_LDS_BYTES, st, g,
                                                                                          a, tiles);
}

}  // namespace mused

using namespace mused;

extern "C" {

// bytes of workspace mused_dbscan needs for n rows (n <= 2^19): 24 n + 4 ceil(n / 128) and some alignment
long mused_dbscan_ws_bytes(long n) {
  if (n <= 0 || n > DB_MAX_ROWS) return -1;
  return (long)db_layout(n, nullptr, nullptr);
}

// Replaces DBSCAN(eps=eps, min_samples=min_samples, metric="euclidean").fit_predict(X) (matrix_operations.py:235-238) for
// fp64 rows on the device.  labels_out: n int32 (device), -1 = noise.  info_out: 4 int32 (device) = {flags, clusters, core
// rows, 0}; flags: 1 some pair lies within tau of eps^2 (head of this file), 2 a row is not finite -- with either one the
// labels are NOT scikit-learn's: run it on the host (it raises on non-finite input).  Enqueue-only.
int mused_dbscan(const double* X, long n, int d, long ld, double eps, int min_samples, int* labels_out, int* info_out,
                 void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && labels_out && info_out && ws, "mused_dbscan: null argument");
  MUSED_REQUIRE(n > 0 && n <= DB_MAX_ROWS && d > 0 && ld >= d, "mused_dbscan: bad shape (n=%ld d=%d ld=%ld)", n, d, ld);
  MUSED_REQUIRE(eps > 0.0 && eps * eps < 1.7976931348623157e308 && min_samples >= 1, "mused_dbscan: need eps > 0 (finite square), min_samples >= 1");
  MUSED_REQUIRE(ws_bytes >= (long)db_layout(n, nullptr, nullptr), "mused_dbscan: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  DbWs w;
  db_layout(n, (char*)ws, &w);
  const int tiles = cdiv(n, GEMM_BM);
  const double eps2 = eps * eps;
  DbArgs a{w.nrm, w.count, w.parent, w.root, w.tflag, w.info, eps2, pair_tau_coeff(d), ulp4(eps2), min_samples};
  const GemmArgs g = self_product_args(X, ld, n, d);
  const bool vec = vec_ok<double>(X, ld, 0);
  const dim3 rows(cdiv(n, 256)), blk(256);
  int rc;
  if ((rc = mused_row_sq_norms(X, MUSED_F64, n, d, ld, w.nrm, stream))) return rc;
  hipLaunchKernelGGL(dbscan_init_kernel, rows, blk, 0, st, a, (int)n);
  hipLaunchKernelGGL(norms_finite_kernel, rows, blk, 0, st, w.nrm, (int)n, w.info, 2);  // (behind init, which clears the flag)
  if ((rc = db_pass<DB_COUNT>(g, a, vec, tiles, st))) return rc;
  hipLaunchKernelGGL(dbscan_core_kernel, rows, blk, 0, st, a, (int)n, tiles);
  if ((rc = db_pass<DB_UNION>(g, a, vec, tiles, st))) return rc;
  hipLaunchKernelGGL(dbscan_flatten_kernel, rows, blk, 0, st, a, (int)n);
  hipLaunchKernelGGL(dbscan_rank_kernel, dim3(1), dim3(DB_RANK_THREADS), 0, st, w.root, w.rank, w.info, (int)n);
  if ((rc = db_pass<DB_BORDER>(g, a, vec, tiles, st))) return rc;
  hipLaunchKernelGGL(dbscan_labels_kernel, rows, blk, 0, st, a, w.rank, labels_out, (int)n);
  MUSED_LAUNCH_CHECK();
  MUSED_CHECK_HIP(hipMemcpyAsync(info_out, w.info, 16, hipMemcpyDeviceToDevice, st));
  return MUSED_OK;
}

}  // extern "C"
