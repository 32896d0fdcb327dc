// Exact Euclidean minimum spanning tree of n fp64 rows by Boruvka rounds on the fp64 MFMA distance tiles of gemm_f64.h, with
// O(n) workspace beside the n - 1 output edges: no n x n array, neighbour list or bitmask.  It is the O(n^2 d) part of
// sklearn.cluster.HDBSCAN(min_samples <= 2, metric="euclidean"): there the mutual-reachability distance IS the distance
// (mused_amd/hdbscan.py), so scikit-learn's Prim loop builds this tree.
//
// A round (specification: mused_amd/hdbscan.py emst_boruvka; comp[] = every row's root at the start of the round):
//
//   tile pass BEST    best[i] = smallest d2(i, j) over the columns j with comp[j] != comp[i]               (64-bit atomicMin on
//                     the bits of d2 >= 0, which order like the numbers)
//   tile pass SECOND  over the same columns: bcol[i] / bcol2[i] = smallest / largest column with d2 == best[i] (atomicMin /
//                     atomicMax), second[i] = smallest d2 > best[i].  For a fixed row the edge order (d2, min(i, j), max(i, j))
//                     grows with j, so bcol[i] is the row's smallest outgoing edge under it; the row's next smallest
//                     outgoing d2 to a different column is best[i] itself where bcol2[i] != bcol[i], second[i] otherwise.
//   emst_comp_best    cbest[comp[i]] = min over the component's rows of best[i]
//   emst_comp_key     ckey[comp[i]] = min of (min(i, bcol[i]) << 32 | max(i, bcol[i])) over its rows with best[i] == cbest:
//                     the component's smallest outgoing edge under the total order, its PICK.  Exactly one row of the
//                     component holds it (the end of the edge that lies inside).
//   emst_pick         every row with an outgoing edge tests its own candidate for the component's runner-up -- its second
//                     if it holds the pick, its best otherwise -- against the pick (flag 1, below); the row that holds the
//                     pick unites the two ends (union_find.h) and, exactly when ITS compare-and-swap joined two trees,
//                     appends the edge through an atomic counter.  Under one total order the picks of a round form a
//                     forest, so every distinct pick is appended once (a pick shared by two components: by whichever got
//                     there first) and the n - 1 edges are the tree.
//   emst_flatten      comp[i] = root of i, the per-row state reset for the next round, and per row tile the component all
//                     its rows share (-1: several): a tile pair inside one component is skipped by both passes.
//   emst_round_end    one thread: rounds run + 1; `done` when n - 1 edges are written (or when a round wrote none, which only
//                     distances that are not finite can cause: flag 2).
//
// Every kernel of a round first reads the device word `done` and returns if it is set; only emst_round_end, which runs
// alone, writes it.  The call enqueues ceil(log2 n) rounds (every round at least halves the number of components) and reads
// nothing back.  Kernel boundaries are the only synchronisation between workgroups, no workgroup waits for another, every
// atomic is a device-scope vector atomic on global memory, and since min and max commute the state after each kernel, and
// with it the picked edge set, does not depend on scheduling (the ORDER of the output edges does).
//
// Symmetry.  The tile passes visit every unordered pair of row tiles once, by cyclic tile distance like dbscan.hip, and ONE
// evaluation of d2 = max(0, (|x_i|^2 + |x_j|^2) - 2 x_i.x_j) serves row i (candidate column j) and row j (candidate column
// i); a diagonal tile uses its entries with row < col only, for both sides.  Both passes of a round, and every later round,
// run the same main loop on the same tile, so a pair has ONE d2 throughout: the equality test of pass SECOND and the
// tie rule of the total order rely on that.
//
// Rounding (flag 1).  With e(d) = (d + 8) 2^-52 (|x|^2 + |y|^2) bounding the error of any evaluation of d2 (dot form here,
// direct sums in scikit-learn's k-d tree and Prim loop; mused_amd/dbscan.py tau_coefficient) and 4 ulp(d2) covering two
// squared sums that round to the same root, tau(i, j) = 2 (d + 8) 2^-52 (|x_i|^2 + |x_j|^2) + 4 ulp(d2(i, j)).  A row i
// whose candidate is the edge (i, j) with d2 = v bounds tau from its own side: |x_j| <= |x_i| + sqrt(v), so
// |x_i|^2 + |x_j|^2 <= 3 |x_i|^2 + 2 v, and v - 2 (d + 8) 2^-52 (3 |x_i|^2 + 2 v) - 4 ulp(v) grows with v: when the row's
// smallest candidate clears the pick by tau(pick) + that bound, so does every other outgoing edge of the row.  Flag 1 is
// raised when some row's candidate does not.  Without it in any round every pick is the strict minimum of its component's
// cut under scikit-learn's evaluation too, hence an MST edge there (cut property), and the components of every round and the
// final edge set coincide.  Exact or a flag; never a tree that hangs on the last bits.
#include "pair_tile.h"
#include "union_find.h"

namespace mused {

typedef unsigned long long em_u64;

constexpr int EM_BEST = 0, EM_SECOND = 1;
constexpr long EM_MAX_ROWS = 1l << 19;  // the tile grid of one launch, as in dbscan.hip
constexpr em_u64 EM_INF = 0x7ff0000000000000ull;  // bits of +inf: no outgoing edge seen
constexpr int EM_NOCOL = 0x7fffffff;
constexpr int EM_FLAT_THREADS = GEMM_BM;  // emst_flatten: one workgroup per row tile

struct EmArgs {
  const double* nrm;  // [n] squared norms
  em_u64* best;       // [n] bits of the row's smallest outgoing d2 of this round
  em_u64* second;     // [n] bits of its smallest outgoing d2 above best
  int* bcol;          // [n] smallest column with d2 == best
  int* bcol2;         // [n] largest column with d2 == best
  int* comp;          // [n] root of the row at the start of the round
  int* parent;        // [n] union-find forest, parent[x] <= x
  em_u64* cbest;      // [n] by root: smallest best of the component
  em_u64* ckey;       // [n] by root: min(i, j) << 32 | max(i, j) of the component's pick
  int* tcomp;         // [tiles] the one component of the row tile, -1 with several
  int* info;          // {flags, edges written, rounds run, 0}
  int* ctl;           // {done, edges written before this round}
  int *edge_a, *edge_b;
  double* edge_d2;
  double ctau;        // 2 (d + 8) 2^-52
};

__device__ __forceinline__ em_u64 em_load64(const em_u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// (the stored value only ever falls: a stale read lets an atomic through that changes nothing, never holds one back)
__device__ __forceinline__ void em_min64(em_u64* p, em_u64 v) {
  if (v < em_load64(p)) atomicMin(p, v);
}
__device__ __forceinline__ double em_dmin(double a, double b) { return b < a ? b : a; }  // keeps a when b is NaN
__device__ __forceinline__ em_u64 em_key(int i, int j) { return ((em_u64)(unsigned)min(i, j) << 32) | (em_u64)(unsigned)max(i, j); }

// tile (I, (I + delta) mod tiles), delta in [0, tiles / 2]: the grid of dbscan_tile_kernel
template <int PASS, bool VEC>
__global__ __launch_bounds__(GEMM_THREADS, 2) void emst_tile_kernel(GemmArgs g, EmArgs a, int tiles) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (db_load(a.ctl)) return;  // done
  int I, delta, J;
  pair_slot(tiles / 2 + 1, I, delta);
  if (!pair_tile(I, delta, tiles, J)) return;
  const bool both = (delta != 0);  // a diagonal tile: the entries with row < col, for both sides
  {
    const int ti = a.tcomp[I], tj = a.tcomp[J];
    if (ti >= 0 && ti == tj) return;  // every pair of the tile lies inside one component
  }
  const int m0 = I * GEMM_BM, n0 = J * GEMM_BN;
  const double* X = reinterpret_cast<const double*>(g.A);
  v4f64 acc[4][4];
  gemm_tile_mainloop<double, double, true, true, VEC>(g, X, X, m0, n0, 0, g.K, smem, acc);

  int lane, wr, wc, kq, li;
  patch_lanes(lane, wr, wc, kq, li);
  const int n = g.M;
  const double inf = __longlong_as_double((long long)EM_INF);

  // rows and columns beyond n read entry n - 1 and are masked (no branch around a load: dbscan_tile_kernel)
  double ncol[4], cval[4];  // BEST: the column's running minimum; SECOND: its best of pass BEST
  double csec[4];
  int ccomp[4], cmin[4], cmax[4];
  bool cok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = patch_col(n0, wc, li) + j * 16;
    const int cc = min(col, n - 1);
    cok[j] = col < n;
    ncol[j] = a.nrm[cc];
    ccomp[j] = a.comp[cc];
    cval[j] = (PASS == EM_BEST) ? inf : __longlong_as_double((long long)a.best[cc]);
    csec[j] = inf;
    cmin[j] = EM_NOCOL;
    cmax[j] = -1;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = patch_row(m0, wr, kq) + i * 16 + 4 * r;
      const int rc = min(row, n - 1);
      const bool rok = row < n;
      const double nrow = a.nrm[rc];
      const int rcomp = a.comp[rc];
      double rval = (PASS == EM_BEST) ? inf : __longlong_as_double((long long)a.best[rc]);
      double rsec = inf;
      int rmin = EM_NOCOL, rmax = -1;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = patch_col(n0, wc, li) + j * 16;
        const double s = nrow + ncol[j];
        double dd = s - 2.0 * acc[i][j][r];
        dd = dd < 0.0 ? 0.0 : dd;  // (NaN stays NaN and passes no comparison below)
        const bool use = rok && cok[j] && (both || row < col) && rcomp != ccomp[j];
        if (PASS == EM_BEST) {
          rval = (use && dd < rval) ? dd : rval;
          cval[j] = (use && dd < cval[j]) ? dd : cval[j];
        } else {
          const bool req = use && dd == rval, ceq = use && dd == cval[j];
          rmin = req ? min(rmin, col) : rmin;
          rmax = req ? max(rmax, col) : rmax;
          rsec = (use && dd > rval && dd < rsec) ? dd : rsec;
          cmin[j] = ceq ? min(cmin[j], row) : cmin[j];
          cmax[j] = ceq ? max(cmax[j], row) : cmax[j];
          csec[j] = (use && dd > cval[j] && dd < csec[j]) ? dd : csec[j];
        }
      }
      // the 16 lanes that share kq hold the 64 columns of this row in this wave
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        if (PASS == EM_BEST) {
          rval = em_dmin(rval, __shfl_xor(rval, o));
        } else {
          rsec = em_dmin(rsec, __shfl_xor(rsec, o));
          rmin = min(rmin, __shfl_xor(rmin, o));
          rmax = max(rmax, __shfl_xor(rmax, o));
        }
      }
      if (li == 0 && rok) {
        if (PASS == EM_BEST) {
          em_min64(a.best + row, (em_u64)__double_as_longlong(rval));
        } else {
          em_min64(a.second + row, (em_u64)__double_as_longlong(rsec));
          if (rmin != EM_NOCOL) {
            atomicMin(a.bcol + row, rmin);
            atomicMax(a.bcol2 + row, rmax);
          }
        }
      }
      // the row is complete HERE: keeps the compiler from postponing the column side of all 16 rows behind the loop and
      // holding the distances of the whole patch for it (dbscan_tile_kernel)
      if (PASS == EM_BEST) asm volatile("" : "+v"(cval[0]), "+v"(cval[1]), "+v"(cval[2]), "+v"(cval[3]));
      else asm volatile("" : "+v"(csec[0]), "+v"(csec[1]), "+v"(csec[2]), "+v"(csec[3]), "+v"(cmin[0]), "+v"(cmin[1]), "+v"(cmin[2]), "+v"(cmin[3]),
                             "+v"(cmax[0]), "+v"(cmax[1]), "+v"(cmax[2]), "+v"(cmax[3]));
    }
  }
  // the 4 lanes that share li hold the 64 rows of this column in this wave
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double v = (PASS == EM_BEST) ? cval[j] : csec[j];
    int lo = cmin[j], hi = cmax[j];
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      v = em_dmin(v, __shfl_xor(v, o));
      if (PASS == EM_SECOND) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
      }
    }
    const int col = patch_col(n0, wc, li) + j * 16;
    if (kq == 0 && col < n) {
      em_min64((PASS == EM_BEST ? a.best : a.second) + col, (em_u64)__double_as_longlong(v));
      if (PASS == EM_SECOND && lo != EM_NOCOL) {
        atomicMin(a.bcol + col, lo);
        atomicMax(a.bcol2 + col, hi);
      }
    }
  }
}

__global__ void emst_init_kernel(EmArgs a, int n, int tiles) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4) a.info[i] = 0;
  if (i < 2) a.ctl[i] = 0;
  if (i < tiles) a.tcomp[i] = -1;
  if (i < n) a.parent[i] = i;
}

// one thread, alone on the stream: the only writer of `done`.  first: before round 0 (nothing to do for one row or rows
// that are not finite); otherwise the end of a round.
__global__ void emst_round_end_kernel(EmArgs a, int n, int first) {
  if (blockIdx.x || threadIdx.x) return;
  if (first) {
    a.ctl[0] = (n == 1 || (a.info[0] & 2)) ? 1 : 0;
    return;
  }
  if (a.ctl[0]) return;
  a.info[2] += 1;
  const int edges = a.info[1];
  if (edges >= n - 1) {
    a.ctl[0] = 1;
  } else if (edges == a.ctl[1]) {  // a round that joined nothing: some component has no finite distance to the rest
    a.info[0] |= 2;
    a.ctl[0] = 1;
  }
  a.ctl[1] = edges;
}

// one workgroup per row tile: the rows' roots (the forest is final between rounds: plain reads), the state of the next
// round, and the tile's summary
__global__ __launch_bounds__(EM_FLAT_THREADS) void emst_flatten_kernel(EmArgs a, int n) {
  __shared__ int first, mixed;
  if (a.ctl[0]) return;  // (uniform over the grid)
  const int i = blockIdx.x * EM_FLAT_THREADS + threadIdx.x;
  int x = -1;
  if (i < n) {
    x = i;
    int p = a.parent[x];
    while (p != x) {
      x = p;
      p = a.parent[x];
    }
    a.comp[i] = x;
    a.best[i] = EM_INF;
    a.second[i] = EM_INF;
    a.bcol[i] = EM_NOCOL;
    a.bcol2[i] = -1;
    a.cbest[i] = EM_INF;
    a.ckey[i] = ~0ull;
  }
  if (threadIdx.x == 0) {
    first = x;  // (row blockIdx.x * 128 exists: the grid has ceil(n / 128) workgroups)
    mixed = 0;
  }
  __syncthreads();
  if (i < n && x != first) atomicOr(&mixed, 1);
  __syncthreads();
  if (threadIdx.x == 0) a.tcomp[blockIdx.x] = mixed ? -1 : first;
}

__global__ void emst_comp_best_kernel(EmArgs a, int n) {
  if (a.ctl[0]) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const em_u64 b = a.best[i];
  if (b != EM_INF) em_min64(a.cbest + a.comp[i], b);
}

__global__ void emst_comp_key_kernel(EmArgs a, int n) {
  if (a.ctl[0]) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const em_u64 b = a.best[i];
  if (b == EM_INF) return;
  const int c = a.comp[i], j = a.bcol[i];
  if ((unsigned)j >= (unsigned)n) {  // pass SECOND did not find the column pass BEST saw (flag 4, never expected)
    atomicOr(a.info, 4);
    return;
  }
  if (b == a.cbest[c]) em_min64(a.ckey + c, em_key(i, j));
}

__global__ void emst_pick_kernel(EmArgs a, int n) {
  if (a.ctl[0]) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const em_u64 b = a.best[i];
  if (b == EM_INF) return;  // no outgoing edge (only distances that are not finite do that)
  const int c = a.comp[i], j = a.bcol[i];
  const em_u64 p = a.cbest[c], k = a.ckey[c];
  if ((unsigned)j >= (unsigned)n || k == ~0ull) return;  // (flag 4 was raised by emst_comp_key)
  const bool mine = (b == p && em_key(i, j) == k);
  // the row's candidate for the component's runner-up: its next outgoing edge if it holds the pick, its best otherwise
  const em_u64 v = mine ? (a.bcol2[i] != j ? b : a.second[i]) : b;
  const double pd = __longlong_as_double((long long)p);
  if (v != EM_INF) {
    const double vd = __longlong_as_double((long long)v);
    const int pa = (int)(k >> 32), pb = (int)(k & 0xffffffffull);
    const double tau_pick = a.ctau * (a.nrm[pa] + a.nrm[pb]) + ulp4(pd);
    const double tau_cand = a.ctau * (3.0 * a.nrm[i] + 2.0 * vd) + ulp4(vd);  // bound of tau(i, its column): head of this file
    if (!(vd - pd > tau_pick + tau_cand)) atomicOr(a.info, 1);
  }
  if (mine) {
    bool joined;
    db_unite(a.parent, i, j, &joined);
    if (joined) {
      const int at = atomicAdd(a.info + 1, 1);
      if (at < n - 1) {  // (a forest of n rows has no more edges; the test keeps a broken invariant inside the arrays)
        a.edge_a[at] = i;
        a.edge_b[at] = j;
        a.edge_d2[at] = pd;
      }
    }
  }
}

struct EmWs {
  double* nrm;
  em_u64 *best, *second, *cbest, *ckey;
  int *bcol, *bcol2, *comp, *parent, *tcomp, *info, *ctl;
};

static size_t em_layout(long n, char* base, EmWs* ws) {
  EmWs sizing;
  EmWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  w.nrm = c.take<double>(n);
  w.best = c.take<em_u64>(n);
  w.second = c.take<em_u64>(n);
  w.cbest = c.take<em_u64>(n);
  w.ckey = c.take<em_u64>(n);
  w.bcol = c.take<int>(n);
  w.bcol2 = c.take<int>(n);
  w.comp = c.take<int>(n);
  w.parent = c.take<int>(n);
  w.tcomp = c.take<int>((n + GEMM_BM - 1) / GEMM_BM);
  w.info = c.take<int>(4);
  w.ctl = c.take<int>(2);
  return c.off;
}

template <int PASS>
static int em_pass(const GemmArgs& g, const EmArgs& a, bool vec, int tiles, hipStream_t st) {
  return pair_launch<emst_tile_kernel<PASS, true>, emst_tile_kernel<PASS, false>>(vec, pair_grid(tiles), GEMM_LDS_BYTES, st, g, a,
                                                                                      tiles);
}

}  // namespace mused

using namespace mused;

extern "C" {

// bytes of workspace mused_emst needs for n rows (n <= 2^19): 56 n + 4 ceil(n / 128) and some alignment
long mused_emst_ws_bytes(long n) {
  if (n <= 0 || n > EM_MAX_ROWS) return -1;
  return (long)em_layout(n, nullptr, nullptr);
}

// The exact Euclidean minimum spanning tree of n fp64 rows (head of this file).  edge_a, edge_b (n - 1 int32, device) and
// edge_d2 (n - 1 fp64, device: the kernel's own d2) receive the edges in arbitrary order and orientation.  info_out: 4 int32
// (device) = {flags, edges written, rounds run, 0}; flags: 1 some component's runner-up lies within rounding of its pick,
// 2 a row (or a squared distance) is not finite, 4 the two tile passes of a round disagreed about a distance (never expected:
// an internal error) -- with any of them the edges are NOT to be used.  Enqueue-only.
int mused_emst(const double* X, long n, int d, long ld, int* edge_a, int* edge_b, double* edge_d2, int* info_out, void* ws,
               long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && info_out && ws, "mused_emst: null argument");
  MUSED_REQUIRE(n > 0 && n <= EM_MAX_ROWS && d > 0 && ld >= d, "mused_emst: bad shape (n=%ld d=%d ld=%ld)", n, d, ld);
  MUSED_REQUIRE(n == 1 || (edge_a && edge_b && edge_d2), "mused_emst: null edge array");
  MUSED_REQUIRE(ws_bytes >= (long)em_layout(n, nullptr, nullptr), "mused_emst: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  EmWs w;
  em_layout(n, (char*)ws, &w);
  const int tiles = cdiv(n, GEMM_BM);
  EmArgs a{w.nrm, w.best, w.second, w.bcol, w.bcol2, w.comp, w.parent, w.cbest, w.ckey, w.tcomp, w.info, w.ctl,
           edge_a, edge_b, edge_d2, pair_tau_coeff(d)};
  const GemmArgs g = self_product_args(X, ld, n, d);
  const bool vec = vec_ok<double>(X, ld, 0);
  const dim3 rows(cdiv(n, 256)), blk(256), one(1);
  int rounds = 0;  // ceil(log2 n): every round at least halves the number of components
  while ((1l << rounds) < n) ++rounds;
  int rc;
  if ((rc = mused_row_sq_norms(X, MUSED_F64, n, d, ld, w.nrm, stream))) return rc;
  hipLaunchKernelGGL(emst_init_kernel, rows, blk, 0, st, a, (int)n, tiles);
  hipLaunchKernelGGL(norms_finite_kernel, rows, blk, 0, st, w.nrm, (int)n, w.info, 2);  // (behind init, which clears the flag)
  hipLaunchKernelGGL(emst_round_end_kernel, one, dim3(64), 0, st, a, (int)n, 1);
  hipLaunchKernelGGL(emst_flatten_kernel, dim3(tiles), dim3(EM_FLAT_THREADS), 0, st, a, (int)n);
  for (int r = 0; r < rounds; ++r) {
    if ((rc = em_pass<EM_BEST>(g, a, vec, tiles, st))) return rc;
    if ((rc = em_pass<EM_SECOND>(g, a, vec, tiles, st))) return rc;
    hipLaunchKernelGGL(emst_comp_best_kernel, rows, blk, 0, st, a, (int)n);
    hipLaunchKernelGGL(emst_comp_key_kernel, rows, blk, 0, st, a, (int)n);
    hipLaunchKernelGGL(emst_pick_kernel, rows, blk, 0, st, a, (int)n);
    hipLaunchKernelGGL(emst_flatten_kernel, dim3(tiles), dim3(EM_FLAT_THREADS), 0, st, a, (int)n);
    hipLaunchKernelGGL(emst_round_end_kernel, one, dim3(64), 0, st, a, (int)n, 0);
  }
  MUSED_LAUNCH_CHECK();
  MUSED_CHECK_HIP(hipMemcpyAsync(info_out, w.info, 16, hipMemcpyDeviceToDevice, st));
  return MUSED_OK;
}

}  // extern "C"
