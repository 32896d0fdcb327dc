// Incremental DBSCAN under insertions (the reference's DBSCAN_incr approach, main.py:87-91) on fp64 rows: after every insert
// the labels of ALL rows inserted so far equal sklearn.cluster.DBSCAN(eps, min_samples).fit_predict(those rows), numbering
// included -- the rule of mused_amd/dbscan_incr.py (pinned to scikit-learn's refit by the tests; NOT pinned to the `incdbscan`
// package, which is not available).  An insert costs (rows it touches) x (all rows) distances, never all x all.
//
// State, owned by the caller, over the n rows so far: nrm[i], count[i] = |N(i)|, parent[] (union-find over the core rows,
// parent[x] <= x: a component's root is its smallest core index), best[i] (a non-core row's smallest root among its core
// neighbours as of the last insert, DB_NONE without one).  Inserting rows n0 .. n0 + w - 1:
//
//   norms, dbi_begin  nrm of the new rows; parent / count / best of the new slice; rootb[i] = find(i) for the rows that are
//                     core BEFORE the insert, -1 for the others; a non-finite norm raises flag 2
//   tile pass COUNT   new rows x all rows: count[new] += |N(new)| (both orientations of a new-new pair lie in the rectangle,
//                     so the row side counts them, once each), count[old] += the new rows within eps (column side, old
//                     columns only); a pair i != j with |d2 - eps^2| <= tau(i, j) raises flag 1 (tau: csrc/dbscan.hip)
//   dbi_core          tile flags, the number of core rows, dirtyA = rows that are core now and were not (old rows among
//                     them), compacted into a list                                        [the host reads flags, |dirtyA|]
//   tile pass UNION   dirtyA x all rows: every core-core edge within eps^2 is united (db_unite, the larger root under the
//                     smaller).  Two old clusters merge here through an old row that has only now turned core.
//   dbi_resolve       core rows: root[i] = find(i); dirtyB = those whose root differs from rootb (every newly core row
//                     included), compacted.  Non-core rows: best = find(best): roots only ever decrease, so a stale
//                     minimum resolves to a root that is still <= the root of every neighbour that did not move
//                                                                                                 [the host reads |dirtyB|]
//   tile pass BCOL    dirtyB x all rows: best[b] = min(best[b], root[c]) for the non-core b within eps^2 of c (atomicMin)
//   tile pass BROW    new rows x all rows: a new non-core row gets the smallest root among its core neighbours
//                     (both border passes are skipped for min_samples <= 2: a non-core row then has no neighbour)
//   dbscan_rank, dbi_labels   rank[r] = number of roots below r; core rows rank[root], the others rank[best] or -1
//
// The A side of a tile pass is a contiguous slice of the rows (COUNT, BROW) or a staging panel into which the dirty rows
// are gathered, with their row ids beside it (UNION, BCOL); either is walked in chunks of `chunk` rows.  The B side is all
// rows.  The tile is the fp64 MFMA tile of gemm_f64.h and the epilogues are those of csrc/dbscan.hip, one-sided.  The
// distance of a pair has the same bits in every pass and in either orientation (the same products summed in the same
// order), so the passes agree with one another.  No n x n array, no neighbour list, no pass over all x all.
// Every write to global memory is a vector store or a device-scope vector atomic; kernel boundaries are the only
// synchronisation between workgroups.
//
// DELETING a set D of m of the n rows held; S = the rest (the rule: mused_amd/dbscan_incr.py).  The O(n) kernels below take
// "is row i deleted, and where does a survivor go" as a policy passed by value; the two entries differ in nothing else but how
// D reaches UNCOUNT and in what the list needs:
//
//   prefix (DelPrefix; mused_dbscan_incr_delete)     D = [0, m): dead(i) = i < m, pos(i) = i - m; no array
//   mask (DelMask; mused_dbscan_incr_delete_rows)    D = the positions dele[] (strictly ascending): dead(i) = dead[i],
//                                                    pos(i) = pos[i] = the survivors below i
//
//   dbr_check         (mask) dele[] strictly ascending in [0, n), or flag 4: the host reads it and returns before anything is written
//   dbd_begin         rootb[i] = find(i) for the core rows, -1 for the others; best = find(best) for the non-core rows that
//                     have one (the remembered root, kept in place); the list of affected roots is cleared (mask: dead[] too)
//   dbr_dead          (mask) dead[i] = 1 for the rows of D
//   tile pass UNCOUNT count[j] -= the rows of D within eps (column side, per-wave reduction before the atomic).  No rounding
//                     test: every pair was tested when the later of its two rows was inserted.  prefix: the slice D on the A
//                     side with a.n0 = m: columns below m take no part, column tiles that lie wholly in D return at once.
//                     mask: D gathered into the staging panel, a.n0 = 0: a dead column is subtracted from as well, and dropped
//   dbd_mark          aff[rootb[i]] = 1 for the core rows of D and for the rows of S that were core and are not any more
//                     (these are counted, and become their own parent again).  mask: then count[D] = 0, so that a dead row is
//                     a non-core column to REBUILD and BPANEL, which read core columns only
//   dbd_select        R = the rows of S that are still core under an affected root: parent[x] = x, compacted into a list; B
//                     (min_samples >= 3) = the rows that lost core status and the non-core rows whose best is an affected
//                     root: best = DB_NONE, compacted into a second list; tile flags over the rows of S (DB_HAS_CORE,
//                     DB_HAS_NONCORE, DB_HAS_REBUILD: the tile holds a row of R), the number of core rows
//                                                                                             [the host reads |R|, |B|]
//   tile pass REBUILD R x S through the staging panel: the UNION epilogue over the core columns of S (all of them that lie
//                     within eps of a row of R are in R); column tiles without a row of R return before their main loop
//   dbd_resolve       root[i] = find(i) for the core rows of S, DB_NONE for every other row
//   tile pass BPANEL  B x S through the staging panel: the BROW epilogue, best[b] = the smallest root among the core columns
//   dbr_scan, blockscan   (mask) pos[]: block totals, their scan in one workgroup, the positions
//   dbd_compact       survivor i becomes pos(i).  The four state arrays are written, renumbered, INTO THE WORKSPACE and copied
//                     back behind the kernel (no workgroup reads an entry that another has overwritten); the roots go,
//                     renumbered, into the array rootb held.  pos keeps the order: parent[x] <= x still holds.  mask:
//                     surv[pos[i]] = i
//   dbi_gather        (mask) the surviving rows, packed, into X_out (the rows do have to move here; the prefix leaves them)
//   dbscan_rank, dbi_labels   over the n - m survivors
#include "pair_tile.h"
#include "dbscan_common.h"
#include "union_find.h"
#include "block_scan.h"

namespace mused {

constexpr int DBI_COUNT = 0, DBI_UNION = 1, DBI_BCOL = 2, DBI_BROW = 3;   // an insert's passes
constexpr int DBI_UNCOUNT = 4, DBI_REBUILD = 5, DBI_BPANEL = 6;           // a delete's: columns below a.n0 (= m) take no part
constexpr long DBI_MAX_CHUNK = 1l << 16;  // 512 x 4096 tiles of 256 threads: far below the 2^32 threads of one launch

struct DbiArgs {
  const double* nrm;
  int *count, *parent, *best;
  const int* root;    // [n] BCOL / BROW: final root of a core row, DB_NONE for the others
  const int* ids;     // row ids of the A rows (staging panel); nullptr: a_base + local row (slice)
  const int* tflag;   // [tiles of all rows] DB_HAS_CORE | DB_HAS_NONCORE (| DB_HAS_REBUILD)
  const int* aflag;   // BROW: the same per 128-row tile of the new slice, from this chunk's first tile on
  int* info;          // {flags, clusters, core rows, -, |dirtyA|, |dirtyB|, -, -}
  double eps2, ctau, etau;
  int min_samples, a_base, n0;   // n0: rows before the insert; for a delete m, the first surviving row
};

// A rows [I * 128, ...) of the chunk against rows [J * 128, ...) of all rows; consecutive workgroups (one XCD's share) walk
// the A tiles of one B tile, so the chunk stays in L2 while the rows stream by once.  Grid: tiles_a * tiles_b.
template <int PASS, bool VEC>
__global__ __launch_bounds__(GEMM_THREADS, 2) void dbscan_incr_tile_kernel(GemmArgs g, DbiArgs a) {
  // the delete's passes share the epilogues: UNCOUNT the column side of COUNT (subtracting), REBUILD all of UNION, BPANEL all of
  // BROW with the A rows in a staging panel
  constexpr bool DEL = PASS >= DBI_UNCOUNT;
  constexpr bool UNI = PASS == DBI_UNION || PASS == DBI_REBUILD, BRW = PASS == DBI_BROW || PASS == DBI_BPANEL;
  constexpr bool CNT = PASS == DBI_COUNT || PASS == DBI_UNCOUNT;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tiles_a = (g.M + GEMM_BM - 1) / GEMM_BM;
  const int e = xcd_remap(blockIdx.x, gridDim.x);
  const int J = e / tiles_a, I = e - J * tiles_a;
  if (PASS == DBI_UNION && !(a.tflag[J] & DB_HAS_CORE)) return;
  if (PASS == DBI_BCOL && !(a.tflag[J] & DB_HAS_NONCORE)) return;
  if (PASS == DBI_BROW && (!(a.tflag[J] & DB_HAS_CORE) || !(a.aflag[I] & DB_HAS_NONCORE))) return;
  if (PASS == DBI_UNCOUNT && (J + 1) * GEMM_BN <= a.n0) return;
  if (PASS == DBI_REBUILD && !(a.tflag[J] & DB_HAS_REBUILD)) return;
  if (PASS == DBI_BPANEL && !(a.tflag[J] & DB_HAS_CORE)) return;
  const int m0 = I * GEMM_BM, n0 = J * GEMM_BN;
  v4f64 acc[4][4];
  gemm_tile_mainloop<double, double, true, true, VEC>(g, reinterpret_cast<const double*>(g.A), reinterpret_cast<const double*>(g.B),
                                                      m0, n0, 0, g.K, smem, acc);

  int lane, wr, wc, kq, li;
  patch_lanes(lane, wr, wc, kq, li);
  const int ma = g.M, n = g.N;

  // Rows and columns beyond the end read the last entry and are masked (no branch around a load: csrc/dbscan.hip)
  double ncol[4];
  int ccol[4];  // COUNT: new rows seen in the column; UNION: cached root; BCOL: running min; BROW: the core column's root
  bool cok[4], corec[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = patch_col(n0, wc, li) + j * 16;
    const int cc = min(col, n - 1);
    cok[j] = col < n && (!DEL || col >= a.n0);
    ncol[j] = a.nrm[cc];
    corec[j] = !CNT && cok[j] && a.count[cc] >= a.min_samples;
    if (CNT) ccol[j] = 0;
    if (UNI) ccol[j] = corec[j] ? db_find(a.parent, col) : -1;
    if (PASS == DBI_BCOL) ccol[j] = DB_NONE;
    if (BRW) ccol[j] = corec[j] ? a.root[cc] : DB_NONE;
  }
  int rsum[16];  // COUNT / BROW: the row's count / minimum over this wave's 64 columns
  int rids[16];
  double slack = __longlong_as_double(0x7ff0000000000000ll);  // COUNT: smallest |d2 - eps^2| - tau of the patch
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = patch_row(m0, wr, kq) + i * 16 + 4 * r;
      const bool rok = lrow < ma;
      const int lr = min(lrow, ma - 1);
      const int rid = a.ids ? a.ids[lr] : a.a_base + lr;  // (a valid row also where rok is false)
      rids[i * 4 + r] = rid;
      const double nrow = a.nrm[rid];
      // UNION, BCOL: every A row is core.  BROW: only the non-core rows of the slice take part
      const bool rtake = rok && (PASS != DBI_BROW || a.count[rid] < a.min_samples);
      const int rroot = (PASS == DBI_BCOL) ? a.root[rid] : DB_NONE;
      int racc = CNT ? 0 : (UNI ? -1 : DB_NONE);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = patch_col(n0, wc, li) + j * 16;
        const bool ok = rtake && cok[j];
        const double s = nrow + ncol[j];
        const double dd = s - 2.0 * acc[i][j][r];
        const bool same = (rid == col);
        const bool in = ok && (same || dd <= a.eps2);
        if (PASS == DBI_COUNT) {
          slack = fmin(slack, (ok && !same) ? fabs(dd - a.eps2) - (a.ctau * s + a.etau) : slack);
          racc += in ? 1 : 0;
          ccol[j] += in ? 1 : 0;
        }
        if (PASS == DBI_UNCOUNT) ccol[j] += in ? 1 : 0;
        if (UNI) {
          if (in && !same && corec[j]) {
            if (racc < 0) racc = db_find(a.parent, rid);
            if (racc != ccol[j]) racc = ccol[j] = db_unite(a.parent, racc, ccol[j]);
          }
        }
        if (PASS == DBI_BCOL) ccol[j] = (in && !corec[j]) ? min(ccol[j], rroot) : ccol[j];
        if (BRW) racc = (in && corec[j]) ? min(racc, ccol[j]) : racc;
      }
      if (PASS == DBI_COUNT || BRW) {
        // the 16 lanes that share kq hold the 64 columns of this row in this wave
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const int x = __shfl_xor(racc, o);
          racc = (PASS == DBI_COUNT) ? racc + x : min(racc, x);
        }
        rsum[i * 4 + r] = racc;
        // the row's results are complete HERE (csrc/dbscan.hip: otherwise the distances of the whole patch stay alive)
        if (BRW) asm volatile("" : "+v"(rsum[i * 4 + r]));
        if (PASS == DBI_COUNT) asm volatile("" : "+v"(slack), "+v"(ccol[0]), "+v"(ccol[1]), "+v"(ccol[2]), "+v"(ccol[3]), "+v"(rsum[i * 4 + r]));
      }
      if (PASS == DBI_BCOL || PASS == DBI_UNCOUNT) asm volatile("" : "+v"(ccol[0]), "+v"(ccol[1]), "+v"(ccol[2]), "+v"(ccol[3]));
    }
  }
  if (PASS == DBI_COUNT || BRW) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int lrow = patch_row(m0, wr, kq) + (q >> 2) * 16 + 4 * (q & 3);
      if (li == 0 && lrow < ma) {
        if (PASS == DBI_COUNT && rsum[q]) atomicAdd(a.count + rids[q], rsum[q]);
        if (BRW && rsum[q] != DB_NONE) atomicMin(a.best + rids[q], rsum[q]);
      }
    }
  }
  if (CNT || PASS == DBI_BCOL) {
    // the 4 lanes that share li hold the 64 rows of this column in this wave
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int v = ccol[j];
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const int x = __shfl_xor(v, o);
        v = CNT ? v + x : min(v, x);
      }
      const int col = patch_col(n0, wc, li) + j * 16;
      if (kq == 0 && col < n) {
        if (PASS == DBI_COUNT && v && col < a.n0) atomicAdd(a.count + col, v);  // (new columns: counted from their row side)
        if (PASS == DBI_UNCOUNT && v) atomicSub(a.count + col, v);  // (v counts columns of S only)
        if (PASS == DBI_BCOL && v != DB_NONE) atomicMin(a.best + col, v);
      }
    }
  }
  if (PASS == DBI_COUNT) {
    if (__ballot(slack <= 0.0) && lane == 0) atomicOr(a.info, 1);
  }
}

// (behind the memset of info)
__global__ void dbi_begin_kernel(DbiArgs a, int* __restrict__ rootb, int n0, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i < n0) {
    rootb[i] = a.count[i] >= a.min_samples ? db_find(a.parent, i) : -1;
  } else if (i < n) {
    a.parent[i] = i;
    a.count[i] = 0;
    a.best[i] = DB_NONE;
    rootb[i] = -1;
    bad = norm_not_finite(a.nrm[i]);
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(a.info, 2);
}

// appends i to list[] (counter: *cnt) for the lanes with `take`: one atomic per wave
__device__ __forceinline__ void dbi_append(bool take, int i, int* list, int* cnt) {
  const unsigned long long bal = __ballot(take);
  if (!bal) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(cnt, __popcll(bal));
  base = __shfl(base, 0);
  if (take) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = i;
}

__global__ void dbi_core_kernel(DbiArgs a, const int* __restrict__ rootb, int* __restrict__ list, int* __restrict__ tflag,
                                int* __restrict__ aflag, int n0, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int tiles = (n + GEMM_BM - 1) / GEMM_BM, tiles_new = (n - n0 + GEMM_BM - 1) / GEMM_BM;
  if (i < tiles) {
    int f = 0;
    const int hi = min(n, (i + 1) * GEMM_BM);
    for (int r = i * GEMM_BM; r < hi; ++r) f |= (a.count[r] >= a.min_samples) ? DB_HAS_CORE : DB_HAS_NONCORE;
    tflag[i] = f;
  }
  if (i < tiles_new) {
    int f = 0;
    const int hi = min(n, n0 + (i + 1) * GEMM_BM);
    for (int r = n0 + i * GEMM_BM; r < hi; ++r) f |= (a.count[r] >= a.min_samples) ? DB_HAS_CORE : DB_HAS_NONCORE;
    aflag[i] = f;
  }
  const bool core = i < n && a.count[i] >= a.min_samples;
  const int c = __popcll(__ballot(core));
  if (c && (threadIdx.x & 63) == 0) atomicAdd(a.info + 2, c);
  dbi_append(core && rootb[i] < 0, i, list, a.info + 4);
}

__global__ void dbi_gather_kernel(const double* __restrict__ X, long ld, int d, const int* __restrict__ ids, int m,
                                  double* __restrict__ panel, int ldp) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)m * d) return;
  const int r = (int)(t / d), k = (int)(t - (long)r * d);
  panel[(long)r * ldp + k] = X[(long)ids[r] * ld + k];
}

__global__ void dbi_resolve_kernel(DbiArgs a, const int* __restrict__ rootb, int* __restrict__ root, int* __restrict__ list, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool moved = false;
  if (i < n) {
    if (a.count[i] >= a.min_samples) {
      const int r = db_find(a.parent, i);
      root[i] = r;
      moved = r != rootb[i];
    } else {
      root[i] = DB_NONE;
      const int b = a.best[i];
      if (b != DB_NONE) a.best[i] = db_find(a.parent, b);
    }
  }
  dbi_append(moved, i, list, a.info + 5);
}

__global__ void dbi_labels_kernel(const int* __restrict__ root, const int* __restrict__ best, const int* __restrict__ rank,
                                  int* __restrict__ labels, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = root[i] != DB_NONE ? root[i] : best[i];
  labels[i] = (r == DB_NONE) ? -1 : rank[r];
}

// ---- the O(n) kernels of a delete -------------------------------------------------------------------------------------
// Which rows are deleted and where a survivor goes: a policy, passed by value.  DelPrefix: D = [0, m).  DelMask: D = dele[0 .. m),
// marked in mark[]; map[i] = the survivors below i; surv[map[i]] = i feeds the row gather.  The tile passes are the same
// instances for both: with a.n0 = 0 every column takes part, UNCOUNT also subtracts from the dead columns, which are dropped,
// and dbd_mark then stores count[D] = 0, so that a dead row is a non-core column to REBUILD and BPANEL, which read core columns only.
struct DelPrefix {
  static constexpr bool MASK = false;
  int m;
  __device__ __forceinline__ bool dead(int i) const { return i < m; }
  __device__ __forceinline__ int pos(int i) const { return i - m; }
};

struct DelMask {
  static constexpr bool MASK = true;
  int* mark;
  const int* map;
  int* surv;
  __device__ __forceinline__ bool dead(int i) const { return mark[i] != 0; }
  __device__ __forceinline__ int pos(int i) const { return map[i]; }
};

// (behind the memset of info)
template <class P>
__global__ void dbd_begin_kernel(DbiArgs a, P del, int* __restrict__ rootb, int* __restrict__ aff, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  aff[i] = 0;
  if constexpr (P::MASK) del.mark[i] = 0;
  if (a.count[i] >= a.min_samples) {
    rootb[i] = db_find(a.parent, i);
  } else {
    rootb[i] = -1;
    const int b = a.best[i];
    if (b != DB_NONE) a.best[i] = db_find(a.parent, b);
  }
}

// behind UNCOUNT: the components that lose a core row; under a mask a dead row has count 0 from here on
template <class P>
__global__ void dbd_mark_kernel(DbiArgs a, P del, const int* __restrict__ rootb, int* __restrict__ aff, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool gone = i < n && del.dead(i);
  const bool was = i < n && rootb[i] >= 0;
  const bool lost = was && !gone && a.count[i] < a.min_samples;
  if (was && (gone || lost)) aff[rootb[i]] = 1;   // (every writer stores the same value)
  if (lost) a.parent[i] = i;                       // a non-core row is its own parent
  if constexpr (P::MASK) {
    if (gone) a.count[i] = 0;
  }
  const int c = __popcll(__ballot(lost));
  if (c && (threadIdx.x & 63) == 0) atomicAdd(a.info + 3, c);
}

template <class P>
__global__ void dbd_select_kernel(DbiArgs a, P del, const int* __restrict__ rootb, const int* __restrict__ aff,
                                  int* __restrict__ list_r, int* __restrict__ list_b, int* __restrict__ tflag, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int tiles = (n + GEMM_BM - 1) / GEMM_BM;
  if (i < tiles) {
    int f = 0;
    const int hi = min(n, (i + 1) * GEMM_BM);
    for (int r = i * GEMM_BM; r < hi; ++r) {
      if (del.dead(r)) continue;
      const bool core = a.count[r] >= a.min_samples;
      f |= core ? (aff[rootb[r]] ? DB_HAS_CORE | DB_HAS_REBUILD : DB_HAS_CORE) : DB_HAS_NONCORE;
    }
    tflag[i] = f;
  }
  const bool in = i < n && !del.dead(i);
  const bool core = in && a.count[i] >= a.min_samples;   // (core now: core before too, counts only fell)
  const bool reb = core && aff[rootb[i]];
  bool bord = false;
  if (in && !core && a.min_samples > 2) {
    const int b = a.best[i];
    bord = rootb[i] >= 0 || (b != DB_NONE && aff[b]);     // lost core status, or its minimum came from an affected root
    if (bord) a.best[i] = DB_NONE;
  }
  if (reb) a.parent[i] = i;
  const int c = __popcll(__ballot(core));
  if (c && (threadIdx.x & 63) == 0) atomicAdd(a.info + 2, c);
  dbi_append(reb, i, list_r, a.info + 4);
  dbi_append(bord, i, list_b, a.info + 5);
}

// (m: the first column that takes part, a.n0 of the tile passes)
__global__ void dbd_resolve_kernel(DbiArgs a, int* __restrict__ root, int m, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  root[i] = (i >= m && a.count[i] >= a.min_samples) ? db_find(a.parent, i) : DB_NONE;
}

// survivor i -> pos(i), into the second set of arrays (nothing of the state is overwritten here); parent, best and the roots
// are renumbered through the same map, which keeps the order: parent[x] <= x still holds
template <class P>
__global__ void dbd_compact_kernel(DbiArgs a, P del, const int* __restrict__ root, double* __restrict__ nrm2, int* __restrict__ count2,
                                   int* __restrict__ parent2, int* __restrict__ best2, int* __restrict__ root2, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || del.dead(i)) return;
  const int p = del.pos(i);
  const int r = root[i], b = a.best[i];
  nrm2[p] = a.nrm[i];
  count2[p] = a.count[i];
  parent2[p] = del.pos(a.parent[i]);
  best2[p] = (r != DB_NONE || b == DB_NONE) ? DB_NONE : del.pos(b);   // (a core row's best is read nowhere)
  root2[p] = r == DB_NONE ? DB_NONE : del.pos(r);
  if constexpr (P::MASK) del.surv[p] = i;
}

// ---- a delete of any rows alone: the list's check, the mask, the positions ----------------------------------------------------------
constexpr int DBR_FLAG_LIST = 4;   // dele[] is not strictly ascending in [0, n)

// (behind the memset of info; writes nothing else)
__global__ void dbr_check_kernel(const int* __restrict__ dele, int m, int n, int* __restrict__ info) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (t < m) {
    const int v = dele[t];
    bad = v < 0 || v >= n || (t > 0 && dele[t - 1] >= v);
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(info, DBR_FLAG_LIST);
}

__global__ void dbr_dead_kernel(const int* __restrict__ dele, int m, int* __restrict__ dead) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < m) dead[dele[t]] = 1;
}

// pos[i] = number of survivors below i: the exclusive scan of the keep mask in three launches (the pattern of csrc/tokenise.hip):
// the totals of blocks of 1024 rows, their scan in one workgroup, the positions
constexpr int DBR_SCAN_THREADS = 1024;
template <bool WRITE>
__global__ __launch_bounds__(DBR_SCAN_THREADS) void dbr_scan_kernel(const int* __restrict__ dead, int* __restrict__ blk,
                                                                   int* __restrict__ pos, int n) {
  __shared__ int wtot[DBR_SCAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = blockIdx.x * DBR_SCAN_THREADS + t;
  const unsigned long long bal = __ballot(i < n && !dead[i]);
  if (lane == 0) wtot[wave] = __popcll(bal);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < DBR_SCAN_THREADS / 64; ++w) {
    const int c = wtot[w];
    total += c;
    before += w < wave ? c : 0;
  }
  if (!WRITE) {
    if (t == 0) blk[blockIdx.x] = total;
  } else if (i < n) {
    pos[i] = blk[blockIdx.x] + before + __popcll(bal & ((1ull << lane) - 1ull));
  }
}

struct DbiWs {
  int *rootb, *root, *rank, *list, *tflag, *aflag, *info;
  double* panel;
};

static inline int dbi_ldp(int d) { return (d + 1) & ~1; }  // even: the panel's rows stay 16-byte aligned

static size_t dbi_layout(long n, int d, long chunk, char* base, DbiWs* ws) {
  DbiWs sizing;
  DbiWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  const size_t tiles = (n + GEMM_BM - 1) / GEMM_BM;
  w.rootb = c.take<int>(n);
  w.root = c.take<int>(n);
  w.rank = c.take<int>(n);
  w.list = c.take<int>(n);
  w.tflag = c.take<int>(tiles);
  w.aflag = c.take<int>(tiles);
  w.info = c.take<int>(8);
  w.panel = c.take<double>((size_t)chunk * dbi_ldp(d));
  return c.off;
}

struct DbdWs {
  int *rootb, *root, *rank, *list_r, *list_b, *aff, *tflag, *info, *count2, *parent2, *best2;
  double *nrm2, *panel;
};

static size_t dbd_layout(long n, int d, long chunk, char* base, DbdWs* ws) {
  DbdWs sizing;
  DbdWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  for (int** p : {&w.rootb, &w.root, &w.rank, &w.list_r, &w.list_b, &w.aff, &w.count2, &w.parent2, &w.best2}) *p = c.take<int>(n);
  w.tflag = c.take<int>((n + GEMM_BM - 1) / GEMM_BM);
  w.info = c.take<int>(8);
  w.nrm2 = c.take<double>(n);
  w.panel = c.take<double>((size_t)chunk * dbi_ldp(d));
  return c.off;
}

// a delete of any rows: the prefix delete's workspace and, behind it, dead[], pos[], surv[] and the scan's block totals
struct DbrWs {
  DbdWs k;
  int *dead, *pos, *surv, *blk;
};

static size_t dbr_layout(long n, int d, long chunk, char* base, DbrWs* ws) {
  DbrWs sizing;
  DbrWs& w = ws ? *ws : sizing;
  WsCarver c{base, dbd_layout(n, d, chunk, base, &w.k)};
  w.dead = c.take<int>(n);
  w.pos = c.take<int>(n);
  w.surv = c.take<int>(n);
  w.blk = c.take<int>((n + DBR_SCAN_THREADS - 1) / DBR_SCAN_THREADS);
  return c.off;
}

static bool dbi_shape_ok(long n, int d, long chunk) {
  return n >= 1 && n <= DB_MAX_ROWS && d >= 1 && d < (1 << 20) && chunk >= GEMM_BM && chunk <= DBI_MAX_CHUNK && chunk % GEMM_BM == 0;
}

// one pass over the new slice (list == nullptr) or over list[0 .. count) through the staging panel, in chunks
template <int PASS>
static int dbi_pass(const double* X, long ld, int d, long n, long n0, long count, const int* list, long chunk, const DbiWs& w,
                    DbiArgs a, bool vec, hipStream_t st) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.B = X; g.ldb = ld; g.N = (int)n; g.K = d;
  for (long c0 = 0; c0 < count; c0 += chunk) {
    const long m = count - c0 < chunk ? count - c0 : chunk;
    g.M = (int)m;
    if (list) {
      const long total = m * d;
      hipLaunchKernelGGL(dbi_gather_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, X, ld, d, list + c0, (int)m, w.panel, dbi_ldp(d));
      g.A = w.panel; g.lda = dbi_ldp(d);
      a.ids = list + c0;
    } else {
      g.A = X + (n0 + c0) * ld; g.lda = ld;
      a.ids = nullptr;
      a.a_base = (int)(n0 + c0);
      a.aflag = w.aflag + c0 / GEMM_BM;
    }
    const int rc = pair_launch<dbscan_incr_tile_kernel<PASS, true>, dbscan_incr_tile_kernel<PASS, false>>(
        vec, cdiv(g.M, GEMM_BM) * cdiv(g.N, GEMM_BN), GEMM_LDS_BYTES, st, g, a);
    if (rc) return rc;
  }
  return MUSED_OK;
}

// A delete from begin to BPANEL (behind the memset of info).  UNCOUNT takes D as the slice [0, m) (ids == nullptr; a.n0 = m) or
// through the staging panel with ids[0 .. m) as the row ids (a.n0 = 0).  Synchronises the stream once, to read |R| and |B|
template <class P>
static int dbd_front(P del, const DbdWs& k, const DbiArgs& a, const double* X, long ld, int d, long n, const int* ids, long m,
                     long chunk, hipStream_t st) {
  DbiWs w;
  memset(&w, 0, sizeof(w));
  w.panel = k.panel;
  w.aflag = k.tflag;  // (the slice walk offsets it; UNCOUNT does not read it)
  const bool vec = vec_ok<double>(X, ld, 0);
  const dim3 rows(cdiv(n, 256)), blk(256);
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc;
  hipLaunchKernelGGL(dbd_begin_kernel<P>, rows, blk, 0, st, a, del, k.rootb, k.aff, (int)n);
  if constexpr (P::MASK) hipLaunchKernelGGL(dbr_dead_kernel, dim3(cdiv(m, 256)), blk, 0, st, ids, (int)m, del.mark);
  if ((rc = dbi_pass<DBI_UNCOUNT>(X, ld, d, n, 0, m, ids, chunk, w, a, vec, st))) return rc;
  hipLaunchKernelGGL(dbd_mark_kernel<P>, rows, blk, 0, st, a, del, k.rootb, k.aff, (int)n);
  hipLaunchKernelGGL(dbd_select_kernel<P>, rows, blk, 0, st, a, del, k.rootb, k.aff, k.list_r, k.list_b, k.tflag, (int)n);
  MUSED_LAUNCH_CHECK();
  MUSED_CHECK_HIP(hipMemcpyAsync(info, k.info, 32, hipMemcpyDeviceToHost, st));
  MUSED_CHECK_HIP(hipStreamSynchronize(st));
  const long n_r = info[4], n_b = info[5];
  if ((rc = dbi_pass<DBI_REBUILD>(X, ld, d, n, 0, n_r, k.list_r, chunk, w, a, vec, st))) return rc;
  hipLaunchKernelGGL(dbd_resolve_kernel, rows, blk, 0, st, a, k.root, a.n0, (int)n);  // (a dead row under a mask has count 0: DB_NONE)
  return dbi_pass<DBI_BPANEL>(X, ld, d, n, 0, n_b, k.list_b, chunk, w, a, vec, st);
}

// Behind the compact kernel: the ns survivors' state back from the workspace, their labels, the info word.  Synchronises the stream
static int dbd_finish(const DbdWs& k, const DbiArgs& a, double* nrm, long ns, int* labels_out, int* info_out, hipStream_t st) {
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  MUSED_LAUNCH_CHECK();
  MUSED_CHECK_HIP(hipMemcpyAsync(nrm, k.nrm2, 8 * (size_t)ns, hipMemcpyDeviceToDevice, st));
  MUSED_CHECK_HIP(hipMemcpyAsync(a.count, k.count2, 4 * (size_t)ns, hipMemcpyDeviceToDevice, st));
  MUSED_CHECK_HIP(hipMemcpyAsync(a.parent, k.parent2, 4 * (size_t)ns, hipMemcpyDeviceToDevice, st));
  MUSED_CHECK_HIP(hipMemcpyAsync(a.best, k.best2, 4 * (size_t)ns, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(dbscan_rank_kernel, dim3(1), dim3(DB_RANK_THREADS), 0, st, k.rootb, k.rank, k.info, (int)ns);
  hipLaunchKernelGGL(dbi_labels_kernel, dim3(cdiv(ns, 256)), dim3(256), 0, st, k.rootb, k.best2, k.rank, labels_out, (int)ns);
  MUSED_LAUNCH_CHECK();
  MUSED_CHECK_HIP(hipMemcpyAsync(info, k.info, 32, hipMemcpyDeviceToHost, st));
  MUSED_CHECK_HIP(hipStreamSynchronize(st));
  memcpy(info_out, info, 24);
  return MUSED_OK;
}

}  // namespace mused

using namespace mused;

extern "C" {

// bytes of workspace mused_dbscan_incr_insert needs while the rows number at most `capacity`
long mused_dbscan_incr_ws_bytes(long capacity, int d, long chunk) {
  if (!dbi_shape_ok(capacity, d, chunk)) return -1;
  return (long)dbi_layout(capacity, d, chunk, nullptr, nullptr);
}

// One insert (head of this file).  X: ALL n0 + w rows (pitch ld), the new ones already in place behind the n0 old ones.
// Synchronises the stream (it reads the dirty counts between the phases): not enqueue-only, not for stream capture.
int mused_dbscan_incr_insert(const double* X, long ld, int d, double* nrm, int* count, int* parent, int* best, long n0, long w,
                             double eps, int min_samples, long chunk, int* labels_out, int* info_out, void* ws, long ws_bytes,
                             void* stream) {
  MUSED_REQUIRE(X && nrm && count && parent && best && labels_out && info_out && ws, "mused_dbscan_incr_insert: null argument");
  MUSED_REQUIRE(n0 >= 0 && w >= 1 && n0 <= DB_MAX_ROWS && w <= DB_MAX_ROWS && dbi_shape_ok(n0 + w, d, chunk) && ld >= d,
                "mused_dbscan_incr_insert: bad shape (n0=%ld w=%ld d=%d ld=%ld chunk=%ld; at most 2^19 rows in all, chunk a "
                "multiple of 128 in [128, 65536])", n0, w, d, ld, chunk);
  MUSED_REQUIRE(eps > 0.0 && eps * eps < 1.7976931348623157e308 && min_samples >= 1,
                "mused_dbscan_incr_insert: need eps > 0 (finite square), min_samples >= 1");
  const long n = n0 + w;
  MUSED_REQUIRE(ws_bytes >= (long)dbi_layout(n, d, chunk, nullptr, nullptr), "mused_dbscan_incr_insert: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  DbiWs k;
  dbi_layout(n, d, chunk, (char*)ws, &k);
  const double eps2 = eps * eps;
  DbiArgs a{nrm, count, parent, best, k.root, nullptr, k.tflag, k.aflag, k.info, eps2, pair_tau_coeff(d), ulp4(eps2),
            min_samples, (int)n0, (int)n0};
  const bool vec = vec_ok<double>(X, ld, 0);
  const dim3 rows(cdiv(n, 256)), blk(256);
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc;
  MUSED_CHECK_HIP(hipMemsetAsync(k.info, 0, 32, st));
  if ((rc = mused_row_sq_norms(X + n0 * ld, MUSED_F64, w, d, ld, nrm + n0, stream))) return rc;
  hipLaunchKernelGGL(dbi_begin_kernel, rows, blk, 0, st, a, k.rootb, (int)n0, (int)n);
  if ((rc = dbi_pass<DBI_COUNT>(X, ld, d, n, n0, w, nullptr, chunk, k, a, vec, st))) return rc;
  hipLaunchKernelGGL(dbi_core_kernel, rows, blk, 0, st, a, k.rootb, k.list, k.tflag, k.aflag, (int)n0, (int)n);
  MUSED_LAUNCH_CHECK();
  MUSED_CHECK_HIP(hipMemcpyAsync(info, k.info, 32, hipMemcpyDeviceToHost, st));
  MUSED_CHECK_HIP(hipStreamSynchronize(st));
  if (info[0]) {  // a flag: the counts no longer decide the labels (or a row is not finite); nothing further is computed
    memcpy(info_out, info, 12);
    info_out[3] = info_out[4] = info_out[5] = 0;
    return MUSED_OK;
  }
  const long n_a = info[4];
  if ((rc = dbi_pass<DBI_UNION>(X, ld, d, n, n0, n_a, k.list, chunk, k, a, vec, st))) return rc;
  hipLaunchKernelGGL(dbi_resolve_kernel, rows, blk, 0, st, a, k.rootb, k.root, k.list, (int)n);
  MUSED_LAUNCH_CHECK();
  if (min_samples > 2) {
    MUSED_CHECK_HIP(hipMemcpyAsync(info, k.info, 32, hipMemcpyDeviceToHost, st));
    MUSED_CHECK_HIP(hipStreamSynchronize(st));
    if ((rc = dbi_pass<DBI_BCOL>(X, ld, d, n, n0, (long)info[5], k.list, chunk, k, a, vec, st))) return rc;
    if ((rc = dbi_pass<DBI_BROW>(X, ld, d, n, n0, w, nullptr, chunk, k, a, vec, st))) return rc;
  }
  hipLaunchKernelGGL(dbscan_rank_kernel, dim3(1), dim3(DB_RANK_THREADS), 0, st, k.root, k.rank, k.info, (int)n);
  hipLaunchKernelGGL(dbi_labels_kernel, rows, blk, 0, st, k.root, best, k.rank, labels_out, (int)n);
  MUSED_LAUNCH_CHECK();
  MUSED_CHECK_HIP(hipMemcpyAsync(info, k.info, 32, hipMemcpyDeviceToHost, st));
  MUSED_CHECK_HIP(hipStreamSynchronize(st));
  memcpy(info_out, info, 12);
  info_out[3] = info[4] + info[5];
  info_out[4] = info[4];
  info_out[5] = info[5];
  return MUSED_OK;
}

// bytes of workspace mused_dbscan_incr_delete needs while the rows number at most `capacity`
long mused_dbscan_incr_delete_ws_bytes(long capacity, int d, long chunk) {
  if (!dbi_shape_ok(capacity, d, chunk)) return -1;
  return (long)dbd_layout(capacity, d, chunk, nullptr, nullptr);
}

// One delete of the m oldest rows (head of this file).  X: the n rows held (pitch ld); they are not modified, the caller's rows
// start at X + m * ld afterwards.  Synchronises the stream (it reads |R| and |B| between the phases): not enqueue-only.
int mused_dbscan_incr_delete(const double* X, long ld, int d, double* nrm, int* count, int* parent, int* best, long n, long m,
                             double eps, int min_samples, long chunk, int* labels_out, int* info_out, void* ws, long ws_bytes,
                             void* stream) {
  MUSED_REQUIRE(X && nrm && count && parent && best && labels_out && info_out && ws, "mused_dbscan_incr_delete: null argument");
  MUSED_REQUIRE(dbi_shape_ok(n, d, chunk) && ld >= d && m >= 1 && m <= n,
                "mused_dbscan_incr_delete: bad shape (n=%ld m=%ld d=%d ld=%ld chunk=%ld; 1 <= m <= n <= 2^19, chunk a multiple of "
                "128 in [128, 65536])", n, m, d, ld, chunk);
  MUSED_REQUIRE(eps > 0.0 && eps * eps < 1.7976931348623157e308 && min_samples >= 1,
                "mused_dbscan_incr_delete: need eps > 0 (finite square), min_samples >= 1");
  MUSED_REQUIRE(ws_bytes >= (long)dbd_layout(n, d, chunk, nullptr, nullptr), "mused_dbscan_incr_delete: workspace too small");
  memset(info_out, 0, 24);
  if (m == n) return MUSED_OK;  // the empty state: nothing of the arrays describes a row any more
  hipStream_t st = (hipStream_t)stream;
  DbdWs k;
  dbd_layout(n, d, chunk, (char*)ws, &k);
  const DbiArgs a{nrm, count, parent, best, k.root, nullptr, k.tflag, nullptr, k.info, eps * eps, 0.0, 0.0, min_samples, 0, (int)m};
  const DelPrefix del{(int)m};
  int rc;
  MUSED_CHECK_HIP(hipMemsetAsync(k.info, 0, 32, st));
  if ((rc = dbd_front(del, k, a, X, ld, d, n, nullptr, m, chunk, st))) return rc;
  hipLaunchKernelGGL(dbd_compact_kernel<DelPrefix>, dim3(cdiv(n, 256)), dim3(256), 0, st, a, del, k.root, k.nrm2, k.count2, k.parent2,
                     k.best2, k.rootb, (int)n);
  return dbd_finish(k, a, nrm, n - m, labels_out, info_out, st);
}

// bytes of workspace mused_dbscan_incr_delete_rows needs while the rows number at most `capacity`
long mused_dbscan_incr_delete_rows_ws_bytes(long capacity, int d, long chunk) {
  if (!dbi_shape_ok(capacity, d, chunk)) return -1;
  return (long)dbr_layout(capacity, d, chunk, nullptr, nullptr);
}

// One delete of the rows at positions dele[0 .. m) (DEVICE, strictly ascending, in [0, n)) of the n rows held.  X: the rows held
// (pitch ld), not modified; X_out (pitch ld_out, no overlap with the rows held) receives the n - m survivors, packed in order.
// A list that is not strictly ascending in [0, n) sets DBR_FLAG_LIST in info_out[0] and nothing else is written.  Synchronises
// the stream (it reads the list's flag, then |R| and |B|, between the phases): not enqueue-only.
int mused_dbscan_incr_delete_rows(const double* X, long ld, int d, double* X_out, long ld_out, double* nrm, int* count, int* parent,
                                  int* best, long n, const int* dele, long m, double eps, int min_samples, long chunk,
                                  int* labels_out, int* info_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(X && X_out && nrm && count && parent && best && dele && labels_out && info_out && ws,
                "mused_dbscan_incr_delete_rows: null argument");
  MUSED_REQUIRE(dbi_shape_ok(n, d, chunk) && ld >= d && ld_out >= d && ld_out < (1l << 31) && m >= 1 && m <= n,
                "mused_dbscan_incr_delete_rows: bad shape (n=%ld m=%ld d=%d ld=%ld ld_out=%ld chunk=%ld; 1 <= m <= n <= 2^19, chunk a "
                "multiple of 128 in [128, 65536])", n, m, d, ld, ld_out, chunk);
  MUSED_REQUIRE(eps > 0.0 && eps * eps < 1.7976931348623157e308 && min_samples >= 1,
                "mused_dbscan_incr_delete_rows: need eps > 0 (finite square), min_samples >= 1");
  MUSED_REQUIRE(ws_bytes >= (long)dbr_layout(n, d, chunk, nullptr, nullptr), "mused_dbscan_incr_delete_rows: workspace too small");
  const long ns = n - m;
  MUSED_REQUIRE(ns == 0 || X_out + ((ns - 1) * ld_out + d) <= X || X + ((n - 1) * ld + d) <= X_out,
                "mused_dbscan_incr_delete_rows: X_out overlaps the rows held");
  hipStream_t st = (hipStream_t)stream;
  DbrWs r;
  dbr_layout(n, d, chunk, (char*)ws, &r);
  const DbdWs& k = r.k;
  const DbiArgs a{nrm, count, parent, best, k.root, nullptr, k.tflag, nullptr, k.info, eps * eps, 0.0, 0.0, min_samples, 0, 0};
  const DelMask del{r.dead, r.pos, r.surv};
  const dim3 rows(cdiv(n, 256)), blk(256), scan(cdiv(n, DBR_SCAN_THREADS));
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int rc;
  memset(info_out, 0, 24);
  MUSED_CHECK_HIP(hipMemsetAsync(k.info, 0, 32, st));
  hipLaunchKernelGGL(dbr_check_kernel, dim3(cdiv(m, 256)), blk, 0, st, dele, (int)m, (int)n, k.info);
  MUSED_LAUNCH_CHECK();
  MUSED_CHECK_HIP(hipMemcpyAsync(info, k.info, 32, hipMemcpyDeviceToHost, st));
  MUSED_CHECK_HIP(hipStreamSynchronize(st));
  if (info[0]) {  // a bad list: no array has been written
    info_out[0] = info[0];
    return MUSED_OK;
  }
  if (m == n) return MUSED_OK;  // the empty state: nothing of the arrays describes a row any more
  if ((rc = dbd_front(del, k, a, X, ld, d, n, dele, m, chunk, st))) return rc;
  hipLaunchKernelGGL(dbr_scan_kernel<false>, scan, dim3(DBR_SCAN_THREADS), 0, st, r.dead, r.blk, r.pos, (int)n);
  hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, st, r.blk, (int)scan.x, (int*)nullptr);
  hipLaunchKernelGGL(dbr_scan_kernel<true>, scan, dim3(DBR_SCAN_THREADS), 0, st, r.dead, r.blk, r.pos, (int)n);
  hipLaunchKernelGGL(dbd_compact_kernel<DelMask>, rows, blk, 0, st, a, del, k.root, k.nrm2, k.count2, k.parent2, k.best2, k.rootb, (int)n);
  hipLaunchKernelGGL(dbi_gather_kernel, dim3(cdiv(ns * d, 256)), blk, 0, st, X, ld, d, r.surv, (int)ns, X_out, (int)ld_out);
  return dbd_finish(k, a, nrm, ns, labels_out, info_out, st);
}

}  // extern "C"
