// DBSCAN's eps from the data (specification: mused_amd/kdist.py): the squared distance of every row to its k-th nearest row,
// the row itself counted (scikit-learn's convention for min_samples and for NearestNeighbors.kneighbors(X)), and the knee of
// the sorted curve of their roots.
//
//   mused_kth_distance   kd2[i] = the k-th smallest of d2(i, j) over all j, d2 = max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j), exactly 0
//                        for j == i
//   mused_eps_knee       v = sort(sqrt(kd2)); the knee rule of kdist.knee and the midpoint eps of kdist.eps_from_curve
//
// k-th distances.  The full-square schedule of silhouette.hip: a workgroup owns a 128-row tile and walks column tiles with the
// fp64 MFMA tile of gemm_f64.h (x_i . x_j in the accumulators, the arrangement of pair_tile.h).  Every row of the tile keeps
// the k smallest d2 it has seen as an ascending list in LDS, best[j][row], all +inf at first; best[k - 1][row] is the row's
// threshold.  Of a column tile only the entries BELOW the threshold leave the accumulators (an entry equal to the k-th value
// does not change it): each is appended to the row's staging slots (an LDS integer counter per row; 64 slots a row, laid
// over the operand buffers of the GEMM stage, which are idle between two main loops), and the row's thread inserts the staged
// values into the list.  A row with more than 64 passing entries (the first tiles of a slice; a ramp, whose last row tile
// sees every distance descend) keeps the rest in the accumulators: a bit per entry marks what has been staged, and the
// round is repeated against the lowered thresholds until no row is left over.  Nothing is dropped, and a tile none of whose
// entries pass costs one barrier.
// The k-th smallest of a multiset does not depend on the order its members arrive in, so the order the counters hand the slots
// out in does not reach the result: two calls give the same bits.  No floating-point atomic, no global candidate list.
//
// Two instances by the list length: 8 (k <= 8: 8 KB of lists beside the 72 KB of the stage = 80 KB, two workgroups a CU) and
// 64 (k <= 64: 136 KB, one workgroup a CU), each VEC and plain.  MUSED_KDIST_WIDE=1 (read per call) runs the second for every
// k; what the split buys was measured that way.
//
// Column slices.  Below 256 row tiles the column tiles are cut into S = col_slices(tiles) <= 16 runs of whole tiles (pair_tile.h,
// the rule of silhouette.hip); workgroup (row tile, slice) leaves its k smallest in
// part[slice][j][row], and kd_merge_kernel walks the S ascending lists of a row to their k-th smallest.  S n k doubles.
//
// Knee.  The roots are sorted by their bit patterns (a non-negative double's is monotone in its value): two rounds of four
// radix_sort.h passes, the low word first, then the high word gathered into the low word's order; the stable passes make it
// one sort of the 64-bit pattern.  One workgroup then evaluates g_i = i / (n - 1) - (v_i - v_0) / (v_{n-1} - v_0) (divisions
// and subtractions only: the bits of the NumPy rule), takes its FIRST maximum i* by a reduction whose ties go to the smaller
// index, the first nxt > i* with v[nxt] > v[i*] the same way, and writes eps = 0.5 (v[i*] + v[nxt]).
#include "pair_tile.h"
#include "dbscan_common.h"
#include "radix_sort.h"

namespace mused {

constexpr int KD_FLAG_NONFINITE = 2;  // (mused_amd.dbscan.FLAG_NONFINITE)
constexpr int KD_FLAG_FLAT = 4;       // the sorted curve is flat: v[n - 1] == v[0]
constexpr int KD_MAX_K = 64;
constexpr int KD_NARROW_K = 8;
constexpr int KD_STAGE = 64;          // staging slots a row
constexpr int KD_CNT_OFF = KD_STAGE * GEMM_BM;  // (doubles) the 128 counters sit behind the slots, inside the GEMM stage
// The counters and the four wave flags of kd_block_any lie in the SECOND buffer of the B operand: a main loop writes it only
// behind its first barrier, which a wave reaches after it has read the flags of the round before.
static_assert(KD_CNT_OFF >= 3 * GEMM_BK * GEMM_LD && (KD_CNT_OFF + GEMM_BM / 2 + 2) * 8 <= GEMM_LDS_BYTES,
              "staging slots, counters and wave flags lie over the GEMM stage");
constexpr int KD_KNEE_THREADS = 1024;

static size_t kd_lds_bytes(int kcap) { return (size_t)GEMM_LDS_BYTES + (size_t)kcap * GEMM_BM * 8; }

struct KdWs {
  int* info;     // {flags, 0, 0, 0}
  double* nrm;   // [n]
  double* part;  // [slices][k][n], slices > 1
};

static size_t kd_layout(long n, int k, char* base, KdWs* ws) {
  KdWs sizing;
  KdWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  w.info = c.take<int>(4);
  w.nrm = c.take<double>(n);
  const int slices = col_slices(cdiv(n, GEMM_BM));
  w.part = slices > 1 ? c.take<double>((size_t)slices * k * n) : nullptr;
  return c.off;
}

static bool kd_shape_ok(long n, int k) { return n >= 1 && n <= DB_MAX_ROWS && k >= 1 && k <= KD_MAX_K && k <= n; }

struct KdArgs {
  const double* nrm;
  const int* info;
  double* kd2;   // [n], slices == 1
  double* part;  // [slices][k][n], slices > 1
};

// p of any thread of the workgroup, with ONE barrier and no static LDS: a flag per wave.  Between two calls the workgroup
// passes another barrier (the appends', or a main loop's), so a flag is not rewritten while a wave still reads it.
__device__ __forceinline__ bool kd_block_any(bool p, int* wany) {
  const bool w = __ballot(p) != 0ull;
  if ((threadIdx.x & 63) == 0) wany[threadIdx.x >> 6] = w ? 1 : 0;
  __syncthreads();
  return (wany[0] | wany[1] | wany[2] | wany[3]) != 0;
}

template <bool VEC, int KCAP>
__global__ __launch_bounds__(GEMM_THREADS, KCAP <= KD_NARROW_K ? 2 : 1) void kd_tile_kernel(GemmArgs g, KdArgs a, int k, int tiles,
                                                                                           int slices) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  if (a.info[0] != 0) return;  // flagged: nothing is written (uniform over the grid)
  double* best = smem + GEMM_LDS_BYTES / 8;  // [KCAP][row of the tile], ascending in the first index
  double* stage = smem;                      // [KD_STAGE][row of the tile], valid between two main loops
  int* cnt = reinterpret_cast<int*>(smem + KD_CNT_OFF);  // [row of the tile], as the slots
  int* wany = cnt + GEMM_BM;                             // [wave]
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  const int n = g.M;
  // workgroup (row tile, slice), row tile fastest: the workgroups in flight walk the same column panels
  const int slice = blockIdx.x / tiles;
  const int m0 = (blockIdx.x - slice * tiles) * GEMM_BM;
  const int t_lo = (int)((long)slice * tiles / slices), t_hi = (int)((long)(slice + 1) * tiles / slices);
  const double* X = reinterpret_cast<const double*>(g.A);
  int lane, wr, wc, kq, li;
  patch_lanes(lane, wr, wc, kq, li);
  const int t = threadIdx.x;
  const double* thr = best + (k - 1) * GEMM_BM;  // the thresholds of the tile's rows

  for (int e = t; e < k * GEMM_BM; e += GEMM_THREADS) best[e] = inf;
  // (the first main loop's barriers order this before the first read of a threshold)

  for (int J = t_lo; J < t_hi; ++J) {
    const int n0 = J * GEMM_BN;
    v4f64 acc[4][4];
    gemm_tile_mainloop<double, double, true, true, VEC>(g, X, X, m0, n0, 0, g.K, smem, acc);
    // (its last barrier: every wave is done with the operand buffers, the slots and counters may be written)

    // Rows and columns beyond n read entry n - 1 (no branch around a load, as in dbscan_tile_kernel); their entries become
    // +inf, which passes no threshold.
    // (what follows is derived from lbase BEHIND the main loop: hoisted out of the tile loop, the row norms and the LDS
    // addresses of 16 rows would stay in registers through the main loop, which has none to spare)
    int lbase = wr * 64 + kq;
    asm volatile("" : "+v"(lbase));
    double ncol[4];
    int colv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      colv[j] = patch_col(n0, wc, li) + 16 * j;
      ncol[j] = a.nrm[min(colv[j], n - 1)];
    }
    // the squared distances of the patch, in place
    int any = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lrow = lbase + 16 * i + 4 * r;
        const int row = m0 + lrow;
        const double nrow = a.nrm[min(row, n - 1)];
        const double th = thr[lrow];
        double v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double dd = fmax(nrow + ncol[j] - 2.0 * acc[i][j][r], 0.0);
          v[j] = (row >= n || colv[j] >= n) ? inf : (row == colv[j] ? 0.0 : dd);
          any |= v[j] < th ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j][r] = v[j];
      }
    }
    if (t < GEMM_BM) cnt[t] = 0;
    if (!kd_block_any(any != 0, wany)) continue;  // nothing below any threshold: the next column tile

    unsigned long long staged = 0ull;  // bit 16 i + 4 r + j: the entry has been staged and does not come again
    for (;;) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lrow = lbase + 16 * i + 4 * r;
          const double th = thr[lrow];
          // one counter update a row and lane: the lane's passing entries take consecutive slots
          bool p[4];
          int c = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            p[j] = acc[i][j][r] < th && !((staged >> (16 * i + 4 * r + j)) & 1ull);
            c += p[j] ? 1 : 0;
          }
          if (c) {
            int slot = atomicAdd(&cnt[lrow], c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (p[j]) {
                if (slot < KD_STAGE) {
                  stage[slot * GEMM_BM + lrow] = acc[i][j][r];
                  staged |= 1ull << (16 * i + 4 * r + j);
                }
                ++slot;
              }
            }
          }
        }
      }
      __syncthreads();
      bool over = false;
      if (t < GEMM_BM) {
        const int c = cnt[t];
        over = c > KD_STAGE;
        const int m = over ? KD_STAGE : c;
        for (int s = 0; s < m; ++s) {
          const double v = stage[s * GEMM_BM + t];
          if (v < thr[t]) {  // (the threshold falls while the row's values go in)
            int j = k - 1;
            while (j > 0 && best[(j - 1) * GEMM_BM + t] > v) {
              best[j * GEMM_BM + t] = best[(j - 1) * GEMM_BM + t];
              --j;
            }
            best[j * GEMM_BM + t] = v;
          }
        }
        cnt[t] = 0;
      }
      // behind this barrier: the lists and thresholds are complete, the counters are zero, the slots are free again (for
      // another round or for the next main loop)
      if (!kd_block_any(over, wany)) break;
    }
  }
  __syncthreads();  // (every list is complete: its thread's last insertion, or the +inf of the start, lies behind a barrier)
  const int orow = m0 + t;
  if (t >= GEMM_BM || orow >= n) return;
  if (slices == 1) {
    a.kd2[orow] = thr[t];
  } else {
    double* p = a.part + (size_t)slice * k * n + orow;
    for (int j = 0; j < k; ++j) p[(size_t)j * n] = best[j * GEMM_BM + t];
  }
}

// slices > 1: the k-th smallest of the union of a row's S ascending lists (a list of a slice with fewer than k columns ends
// in +inf); ties between lists do not matter, the value is the same
__global__ __launch_bounds__(256) void kd_merge_kernel(KdArgs a, int n, int k, int slices) {
  if (a.info[0] != 0) return;
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  // the head of every list and its position, in registers (the loops over s are unrolled: no indexed register array)
  double cur[MAX_COL_SLICES];
  int head[MAX_COL_SLICES];
#pragma unroll
  for (int s = 0; s < MAX_COL_SLICES; ++s) {
    head[s] = 0;
    cur[s] = s < slices ? a.part[(size_t)s * k * n + row] : inf;
  }
  double v = 0.0;
  for (int taken = 0; taken < k; ++taken) {
    double lo = cur[0];
    int arg = 0;
#pragma unroll
    for (int s = 1; s < MAX_COL_SLICES; ++s)
      if (cur[s] < lo) lo = cur[s], arg = s;
    v = lo;
    int h = 0;
#pragma unroll
    for (int s = 0; s < MAX_COL_SLICES; ++s) h = (s == arg) ? head[s] + 1 : h;
    const double next = h < k ? a.part[((size_t)arg * k + h) * n + row] : inf;
#pragma unroll
    for (int s = 0; s < MAX_COL_SLICES; ++s) {
      head[s] = (s == arg) ? h : head[s];
      cur[s] = (s == arg) ? next : cur[s];
    }
  }
  a.kd2[row] = v;
}

__global__ void kd_info_kernel(const int* __restrict__ info, int* __restrict__ out, int slices, int kcap) {
  out[0] = info[0];
  out[1] = slices;
  out[2] = kcap;
  out[3] = 0;
}

template <int KCAP>
static int kd_launch(const GemmArgs& g, const KdArgs& a, bool vec, int k, int tiles, int slices, hipStream_t st) {
  return pair_launch<kd_tile_kernel<true, KCAP>, kd_tile_kernel<false, KCAP>>(vec, tiles * slices, kd_lds_bytes(KCAP), st, g, a, k,
                                                                            tiles, slices);
}

// ---- the knee ---------------------------------------------------------------------------------------------------------------
struct KneeWs {
  double *sorted, *root;  // sorted FIRST: the curve stays at the start of the workspace for the caller
  int *key[2], *val[2], *hi, *hi2, *hist, *info;
};

static size_t knee_layout(long n, char* base, KneeWs* ws) {
  KneeWs sizing;
  KneeWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  w.sorted = c.take<double>(n);
  w.root = c.take<double>(n);
  for (int i = 0; i < 2; ++i) {
    w.key[i] = c.take<int>(n);
    w.val[i] = c.take<int>(n);
  }
  w.hi = c.take<int>(n);
  w.hi2 = c.take<int>(n);
  w.hist = c.take<int>(256 * (size_t)((n + RADIX_TILE - 1) / RADIX_TILE));
  w.info = c.take<int>(4);
  return c.off;
}

// root[i] = sqrt(kd2[i]) (+0 for a zero of either sign), its low and high words; a value that is negative or not finite
// raises the flag
__global__ __launch_bounds__(256) void knee_root_kernel(const double* __restrict__ kd2, double* __restrict__ root, int* __restrict__ lo,
                                                       int* __restrict__ hi, int* __restrict__ info, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const double q = i < n ? kd2[i] : 0.0;
  const bool bad = !(q >= 0.0) || norm_not_finite(q);
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(info, KD_FLAG_NONFINITE);
  if (i >= n) return;
  const double v = bad ? 0.0 : sqrt(q) + 0.0;
  const long long b = __double_as_longlong(v);
  root[i] = v;
  lo[i] = (int)(b & 0xffffffffll);
  hi[i] = (int)(b >> 32);
}

__global__ __launch_bounds__(256) void knee_gather_kernel(const double* __restrict__ root, const int* __restrict__ perm,
                                                         double* __restrict__ sorted, int n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) sorted[p] = root[perm[p]];
}

struct KneeOut {
  long long knee, nxt;
  double v_knee, v_nxt, eps;
  long long flags;
};

// one workgroup: the first maximum of g, then the first larger value behind it
__global__ __launch_bounds__(KD_KNEE_THREADS) void knee_rule_kernel(const double* __restrict__ v, const int* __restrict__ info,
                                                                   KneeOut* __restrict__ out, int n) {
  __shared__ double rg[KD_KNEE_THREADS];
  __shared__ int ri[KD_KNEE_THREADS];
  const int t = threadIdx.x;
  int flags = info[0];
  const double v0 = v[0], span = v[n - 1] - v[0];
  if (!flags && !(span > 0.0)) flags = KD_FLAG_FLAT;
  if (flags) {  // (uniform)
    if (t == 0) {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      *out = KneeOut{-1, -1, nan, nan, nan, flags};
    }
    return;
  }
  const double nm1 = (double)(n - 1);
  double bg = -__longlong_as_double(0x7ff0000000000000ll);
  int bi = n;
  for (int i = t; i < n; i += KD_KNEE_THREADS) {
    const double x = (double)i / nm1, y = (v[i] - v0) / span;
    const double gi = x - y;
    if (gi > bg) bg = gi, bi = i;  // (ascending i: the first of equal values stays)
  }
  rg[t] = bg;
  ri[t] = bi;
  __syncthreads();
  for (int o = KD_KNEE_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) {
      const double og = rg[t + o];
      const int oi = ri[t + o];
      if (og > rg[t] || (og == rg[t] && oi < ri[t])) rg[t] = og, ri[t] = oi;
    }
    __syncthreads();
  }
  const int knee = ri[0];
  __syncthreads();
  const double vk = v[knee];
  int first = n;
  for (int i = knee + 1 + t; i < n; i += KD_KNEE_THREADS)
    if (v[i] > vk) {
      first = i;
      break;
    }
  ri[t] = first;
  __syncthreads();
  for (int o = KD_KNEE_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) ri[t] = min(ri[t], ri[t + o]);
    __syncthreads();
  }
  if (t == 0) {
    const int nxt = ri[0];  // (exists: g <= 0 where v equals its maximum, g_0 = 0, so v[knee] < v[n - 1])
    const double vn = v[min(nxt, n - 1)];
    *out = KneeOut{knee, nxt, vk, vn, 0.5 * (vk + vn), 0};
  }
}

}  // namespace mused

using namespace mused;

extern "C" {

// bytes of workspace mused_kth_distance needs (-1: n outside [1, 2^19] or k outside [1, min(n, 64)])
long mused_kth_distance_ws_bytes(long n, int k) {
  if (!kd_shape_ok(n, k)) return -1;
  return (long)kd_layout(n, k, nullptr, nullptr);
}

int mused_kth_distance(const double* X, long n, int d, long ld, int k, double* kd2_out, int* info_out, void* ws, long ws_bytes,
                       void* stream) {
  MUSED_REQUIRE(X && kd2_out && info_out && ws, "mused_kth_distance: null argument");
  MUSED_REQUIRE(kd_shape_ok(n, k) && d >= 1 && d < (1 << 20) && ld >= d,
                "mused_kth_distance: bad shape (n=%ld d=%d ld=%ld k=%d; n <= 2^19, 1 <= k <= min(n, 64))", n, d, ld, k);
  MUSED_REQUIRE(ws_bytes >= (long)kd_layout(n, k, nullptr, nullptr), "mused_kth_distance: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  KdWs w;
  kd_layout(n, k, (char*)ws, &w);
  MUSED_CHECK_HIP(hipMemsetAsync(w.info, 0, 16, st));
  int rc;
  if ((rc = mused_row_sq_norms(X, MUSED_F64, n, d, ld, w.nrm, stream))) return rc;
  hipLaunchKernelGGL(norms_finite_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, w.nrm, (int)n, w.info, KD_FLAG_NONFINITE);
  MUSED_LAUNCH_CHECK();
  const GemmArgs g = self_product_args(X, ld, n, d);
  const int tiles = cdiv(n, GEMM_BM), slices = col_slices(tiles);
  const KdArgs a{w.nrm, w.info, kd2_out, w.part};
  const bool vec = vec_ok<double>(X, ld, 0);
  const char* wide = getenv("MUSED_KDIST_WIDE");  // "1": the 64-long lists for every k (diagnostic: what the split at 8 buys)
  const bool narrow = k <= KD_NARROW_K && !(wide && wide[0] == '1' && wide[1] == 0);
  rc = narrow ? kd_launch<KD_NARROW_K>(g, a, vec, k, tiles, slices, st) : kd_launch<KD_MAX_K>(g, a, vec, k, tiles, slices, st);
  if (rc) return rc;
  if (slices > 1) hipLaunchKernelGGL(kd_merge_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, a, (int)n, k, slices);
  hipLaunchKernelGGL(kd_info_kernel, dim3(1), dim3(1), 0, st, w.info, info_out, slices, narrow ? KD_NARROW_K : KD_MAX_K);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// bytes of workspace mused_eps_knee needs (-1: n outside [1, 2^19])
long mused_eps_knee_ws_bytes(long n) {
  if (n < 1 || n > DB_MAX_ROWS) return -1;
  return (long)knee_layout(n, nullptr, nullptr);
}

int mused_eps_knee(const double* kd2, long n, void* out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(kd2 && out && ws, "mused_eps_knee: null argument");
  MUSED_REQUIRE(n >= 1 && n <= DB_MAX_ROWS, "mused_eps_knee: bad shape (n=%ld; 1 <= n <= 2^19)", n);
  MUSED_REQUIRE(ws_bytes >= (long)knee_layout(n, nullptr, nullptr), "mused_eps_knee: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  KneeWs w;
  knee_layout(n, (char*)ws, &w);
  const dim3 rows(cdiv(n, 256)), blk(256);
  MUSED_CHECK_HIP(hipMemsetAsync(w.info, 0, 16, st));
  hipLaunchKernelGGL(knee_root_kernel, rows, blk, 0, st, kd2, w.root, w.key[0], w.hi, w.info, (int)n);
  MUSED_LAUNCH_CHECK();
  // the low words (the index travels as the value; the last pass gathers the high words into the order reached), then the
  // high words: eight stable passes, the pairs back in key[0], val[0]
  int cur = 0;
  for (int pass = 0; pass < 8; ++pass) {
    const bool first = pass == 0, turn = pass == 3;
    const int* key_in = pass == 4 ? w.hi2 : w.key[cur];
    const int rc = radix_sort_pass(key_in, first ? nullptr : w.val[cur], (int)n, RadixCount{(int)n, nullptr}, (pass & 3) * 8, w.hist,
                                   w.key[cur ^ 1], w.val[cur ^ 1], turn ? w.hi : nullptr, turn ? w.hi2 : nullptr, st);
    if (rc) return rc;
    cur ^= 1;
  }
  hipLaunchKernelGGL(knee_gather_kernel, rows, blk, 0, st, w.root, w.val[0], w.sorted, (int)n);
  hipLaunchKernelGGL(knee_rule_kernel, dim3(1), dim3(KD_KNEE_THREADS), 0, st, w.sorted, w.info, (KneeOut*)out, (int)n);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
