// Scoring a partition against the truth without regard to label numbering: what ARI, AMI, homogeneity / completeness /
// V-measure, Fowlkes-Mallows, purity and the matched accuracy need, from the true-class x predicted-cluster contingency
// table.  The rule is mused_amd/partition_scores.py (scikit-learn 1.7.2's arithmetic); the host finishes the values.
//
// (a) partition_table_kernel, one workgroup of SC_THREADS threads per segment: steps 1-3 of score_table.h, then from the
//     finished table the row and column sums, six exact 64-bit integers (integer atomics: order cannot matter) and MI and
//     the two entropies in fp64 with the arithmetic of score.hip's sc_finalise (fixed share per thread, fixed tree).  The
//     table, a and b always go to the segment's slice of the workspace.
// (b) partition_lgamma_kernel: L[m] = lgamma(m + 1), m = 0 .. seg_len, once per call (every segment has the same N).
// (c) partition_emi_kernel, grid (segment, row slot): the expected mutual information of scikit-learn's
//     _expected_mutual_info_fast.pyx, every term evaluated as written there.  A row's terms are dealt to SP_EMI_SLICES
//     workgroups by nij; each sums its share per lane in a fixed order and by a fixed tree into one partial per (segment,
//     row, slice); partition_emi_merge_kernel adds a segment's partials in a fixed order.  No floating-point atomic: the result is a function of the segment's labels alone.
#include "score_table.h"

#include <stdlib.h>

#pragma clang fp contract(off)   // term1 * term2 * term3 and p * x + p * y as scikit-learn writes them

namespace mused {

constexpr int SP_FLAG_NO_EMI = 64;            // the EMI slot is NaN: not asked for, seg_len > 2^24 or more than 2^34 terms
constexpr long SP_EMI_MAX_N = 1l << 24;
constexpr unsigned long long SP_EMI_MAX_TERMS = 1ull << 34;
constexpr long SP_LG_TABLE_MAX = 1l << 22;    // the log-gamma table holds up to 2^22 + 1 values (32 MiB); beyond: direct
constexpr int SP_INTS = 8;
constexpr int SP_NACC = 6;                    // sum n^2, sum a^2, sum b^2, sum of column maxima, of row maxima, EMI terms
constexpr int SP_EMI_THREADS = 256;
constexpr int SP_EMI_WAVES = SP_EMI_THREADS / 64;
constexpr int SP_EMI_SLICES = 8;                // workgroups a row's terms are dealt to, by nij: two classes still fill 16

struct PartLds {
  ScoreLds s;
  unsigned long long acc[SP_NACC];
};
static_assert(sizeof(PartLds) <= 160 * 1024, "one workgroup's LDS");

// one copy of each library function instead of one per call site; the table and the direct path share sp_lgamma1
__device__ __attribute__((noinline)) double sp_log(double x) { return log(x); }
__device__ __attribute__((noinline)) double sp_lgamma1(int m) { return lgamma((double)m + 1.0); }

__device__ __forceinline__ double sp_snap(double term) { return fabs(term) < 0x1p-52 ? 0.0 : term; }

__device__ __forceinline__ unsigned long long sp_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Sums of the finished table.  Thread 0 returns with the segment's results written.
template <bool LDS>
__device__ __forceinline__ void sp_finalise(PartLds& p, int* __restrict__ gtab, int* __restrict__ ab, int* __restrict__ tout, int T,
                                            int P, long n, bool emi_ok, double* __restrict__ out, long* __restrict__ ints,
                                            int* __restrict__ inf) {
  ScoreLds& s = p.s;
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  unsigned long long acc[SP_NACC];
#pragma unroll
  for (int k = 0; k < SP_NACC; ++k) acc[k] = 0;
  // rows by wave: sum and maximum
  for (int i = w; i < T; i += SC_WAVES) {
    int sum = 0, mx = 0;
    for (int j = l; j < P; j += 64) {
      const int v = sc_cell<LDS>(s, gtab, i * P + j);
      sum += v;
      mx = v > mx ? v : mx;
      acc[0] += (unsigned long long)v * (unsigned long long)v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o);
      const int other = __shfl_xor(mx, o);
      mx = other > mx ? other : mx;
    }
    if (l == 0) {
      s.rs[i] = sum;
      acc[1] += (unsigned long long)sum * (unsigned long long)sum;
      acc[4] += (unsigned long long)mx;
    }
  }
  // columns by thread
  for (int j = t; j < P; j += SC_THREADS) {
    int sum = 0, mx = 0;
    for (int i = 0; i < T; ++i) {
      const int v = sc_cell<LDS>(s, gtab, i * P + j);
      sum += v;
      mx = v > mx ? v : mx;
    }
    s.cs[j] = sum;
    acc[2] += (unsigned long long)sum * (unsigned long long)sum;
    acc[3] += (unsigned long long)mx;
  }
  __syncthreads();
  // the number of EMI terms: nij from max(1, a + b - N) to min(a, b) for every cell
  for (int e = t; e < T * P; e += SC_THREADS) {
    const int i = e / P, j = e - i * P;
    const long a = s.rs[i], b = s.cs[j];
    const long lo = a + b - n > 1 ? a + b - n : 1, hi = a < b ? a : b;
    if (hi >= lo) acc[5] += (unsigned long long)(hi - lo + 1);
  }
#pragma unroll
  for (int k = 0; k < SP_NACC; ++k) {
    const unsigned long long v = sp_wave_sum(acc[k]);
    if (l == 0 && v) atomicAdd(&p.acc[k], v);   // integers: exact in any order
  }

  // [0] MI: non-zero cells in index order, [1] [2] the entropies of the two sides (negated at the end)
  double sum[3] = {0.0, 0.0, 0.0};
  const double dn = (double)n, logn = sp_log(dn);
  for (int e = t; e < T * P; e += SC_THREADS) {
    const int c = sc_cell<LDS>(s, gtab, e);
    if (!c) continue;
    const int i = e / P, j = e - i * P;
    const double dc = (double)c, logc = sp_log(dc);
    const double pr = dc / dn;
    const double lo = -sp_log((double)((long long)s.rs[i] * (long long)s.cs[j])) + logn + logn;
    sum[0] += sp_snap(pr * (logc - logn) + pr * lo);
  }
  for (int i = t; i < T; i += SC_THREADS) {
    const double c = (double)s.rs[i];
    sum[1] += (c / dn) * (sp_log(c) - logn);
  }
  for (int j = t; j < P; j += SC_THREADS) {
    const double c = (double)s.cs[j];
    sum[2] += (c / dn) * (sp_log(c) - logn);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double v = wave_sum(sum[k]);
    if (l == 0) s.red[k][w] = v;
  }
  // the table, a and b for the EMI kernel and the caller
  if (LDS)
    for (int e = t; e < T * P; e += SC_THREADS) gtab[e] = s.tab[e];
  if (tout)
    for (int e = t; e < T * P; e += SC_THREADS) tout[e] = sc_cell<LDS>(s, gtab, e);
  for (int i = t; i < T; i += SC_THREADS) ab[i] = s.rs[i];
  for (int j = t; j < P; j += SC_THREADS) ab[SC_MAXC + j] = s.cs[j];
  __syncthreads();
  if (t < 3) {   // the waves' partial sums in wave order
    double v = 0.0;
    for (int h = 0; h < SC_WAVES; ++h) v += s.red[t][h];
    s.red[t][0] = v;
  }
  __syncthreads();
  if (t != 0) return;
  const unsigned long long terms = p.acc[5];
  const bool emi = emi_ok && terms <= SP_EMI_MAX_TERMS;
  out[0] = s.red[0][0] > 0.0 ? s.red[0][0] : 0.0;
  out[1] = T == 1 ? 0.0 : -s.red[1][0];
  out[2] = P == 1 ? 0.0 : -s.red[2][0];
  out[3] = emi ? 0.0 : __longlong_as_double(0x7ff8000000000000ll);   // the merge kernel writes the value
  out[4] = out[5] = out[6] = out[7] = 0.0;
#pragma unroll
  for (int k = 0; k < SP_NACC; ++k) ints[k] = (long)p.acc[k];
  ints[6] = n;
  ints[7] = 0;
  inf[0] = T;
  inf[1] = P;
  inf[2] = emi ? 0 : SP_FLAG_NO_EMI;
  inf[3] = inf[4] = inf[5] = inf[6] = inf[7] = 0;
}

__global__ __launch_bounds__(SC_THREADS) void partition_table_kernel(const int* __restrict__ truth, const int* __restrict__ pred,
                                                                      long seg_len, long cells_cap, int vec, int emi_ok,
                                                                      double* __restrict__ out_all, long* __restrict__ ints_all,
                                                                      int* __restrict__ info_all, int* __restrict__ table_out,
                                                                      int* __restrict__ tabs, int* __restrict__ ab_all) {
  extern __shared__ __align__(16) unsigned char sp_raw[];
  PartLds& p = *reinterpret_cast<PartLds*>(sp_raw);
  ScoreLds& s = p.s;
  const int t = threadIdx.x;
  const long seg = blockIdx.x;
  const int* tr = truth + seg * seg_len;
  const int* pr = pred + seg * seg_len;
  int* gtab = tabs + seg * cells_cap;
  int* tout = table_out ? table_out + seg * cells_cap : nullptr;
  double* out = out_all + seg * SC_OUT;
  long* ints = ints_all + seg * SP_INTS;
  int* inf = info_all + seg * SC_INFO;

  if (t < SP_NACC) p.acc[t] = 0;   // ordered before its use by the barriers of the steps below
  int T, P;
  sc_presence_ranks(s, tr, pr, seg_len, vec, T, P);
  int flags = s.bad ? SC_FLAG_RANGE : 0;
  if (T > SC_MAXC || P > SC_MAXC || (long)T * (long)P > cells_cap) flags |= SC_FLAG_SIZE;
  if (flags) {   // uniform
    if (t < SC_OUT) out[t] = 0.0;
    if (t < SP_INTS) ints[t] = t == 6 ? seg_len : 0;
    if (t < SC_INFO) inf[t] = t == 0 ? T : t == 1 ? P : t == 2 ? flags : 0;
    return;
  }
  const bool in_lds = sc_build_table(s, tr, pr, seg_len, vec, T, P, gtab);
  if (in_lds) sp_finalise<true>(p, gtab, ab_all + seg * 2 * SC_MAXC, tout, T, P, seg_len, emi_ok != 0, out, ints, inf);
  else sp_finalise<false>(p, gtab, ab_all + seg * 2 * SC_MAXC, tout, T, P, seg_len, emi_ok != 0, out, ints, inf);
}

__global__ __launch_bounds__(256) void partition_lgamma_kernel(double* __restrict__ L, long count) {
  for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < count; m += (long)gridDim.x * blockDim.x) L[m] = sp_lgamma1((int)m);
}

template <bool TAB>
__device__ __forceinline__ double sp_lg(const double* __restrict__ L, int m) {
  return TAB ? L[m] : sp_lgamma1(m);
}

// Slice blockIdx.z of rows i = blockIdx.y, blockIdx.y + gridDim.y, ... of segment blockIdx.x.  The threads form 256 / g groups
// of g lanes, g the smallest power of two >= a_i (at most 64): group q takes the columns q, q + 256 / g, ..., and of a column's
// values of nij, g apart per lane, the slice takes every SP_EMI_SLICES-th.  Every index of L lies in [0, N]: nij <= min(a, b) and N - a - b + nij >= 0 from the start of the range.
template <bool TAB>
__global__ __launch_bounds__(SP_EMI_THREADS) void partition_emi_kernel(long seg_len, const int* __restrict__ info_all,
                                                                        const int* __restrict__ ab_all, const double* __restrict__ L,
                                                                        double* __restrict__ part_all, int part_rows) {
  __shared__ double red[SP_EMI_WAVES];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const long seg = blockIdx.x;
  const int* inf = info_all + seg * SC_INFO;
  const int T = inf[0], P = inf[1];
  if (inf[2] || T < 2 || P < 2) return;   // uniform: flagged, or a side with one value (EMI = 0)
  const int* a = ab_all + seg * 2 * SC_MAXC;
  const int* b = a + SC_MAXC;
  double* part = part_all + seg * part_rows * SP_EMI_SLICES;
  const int N = (int)seg_len, slice = blockIdx.z;
  const double dN = (double)N, log_N = sp_log(dN), gln_N = sp_lg<TAB>(L, N);
  for (int i = blockIdx.y; i < T; i += gridDim.y) {
    const int ai = a[i];
    int g = 1;
    while (g < ai && g < 64) g <<= 1;
    const int q = t / g, nq = SP_EMI_THREADS / g, lg = t - q * g;
    const double log_a = sp_log((double)ai), gln_a = sp_lg<TAB>(L, ai), gln_Na = sp_lg<TAB>(L, N - ai);
    double emi = 0.0;
    for (int j = q; j < P; j += nq) {
      const int bj = b[j];
      const double log_b = sp_log((double)bj), gln_b = sp_lg<TAB>(L, bj), gln_Nb = sp_lg<TAB>(L, N - bj);
      const int start = ai + bj - N > 1 ? ai + bj - N : 1, end = ai < bj ? ai : bj;
      for (int nij = start + lg + g * slice; nij <= end; nij += g * SP_EMI_SLICES) {
        const double term1 = (double)nij / dN;
        const double log_Nnij = log_N + sp_log((double)nij);
        const double term2 = log_Nnij - log_a - log_b;
        const double gln_Nnij = sp_lg<TAB>(L, nij) + gln_N;
        const double gln = gln_a + gln_b + gln_Na + gln_Nb - gln_Nnij - sp_lg<TAB>(L, ai - nij) - sp_lg<TAB>(L, bj - nij) -
                           sp_lg<TAB>(L, N - ai - bj + nij);
        const double term3 = exp(gln);
        emi += term1 * term2 * term3;
      }
    }
    const double v = wave_sum(emi);
    if (l == 0) red[w] = v;
    __syncthreads();
    if (t == 0) {
      double r = red[0];
      for (int h = 1; h < SP_EMI_WAVES; ++h) r += red[h];
      part[i * SP_EMI_SLICES + slice] = r;
    }
    __syncthreads();
  }
}

// A segment's T x SP_EMI_SLICES partials in a fixed order: thread t takes entries t, t + 256, ..., then the fixed tree.
__global__ __launch_bounds__(SP_EMI_THREADS) void partition_emi_merge_kernel(const int* __restrict__ info_all,
                                                                              const double* __restrict__ part_all,
                                                                              double* __restrict__ out_all, int part_rows) {
  __shared__ double red[SP_EMI_WAVES];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const long seg = blockIdx.x;
  const int* inf = info_all + seg * SC_INFO;
  const int T = inf[0], P = inf[1];
  if (inf[2] || T < 2 || P < 2) return;   // the table kernel wrote 0.0 (a side with one value) or NaN (flag 64)
  const double* part = part_all + seg * part_rows * SP_EMI_SLICES;
  double acc = 0.0;
  for (int i = t; i < T * SP_EMI_SLICES; i += SP_EMI_THREADS) acc += part[i];
  const double v = wave_sum(acc);
  if (l == 0) red[w] = v;
  __syncthreads();
  if (t == 0) {
    double r = red[0];
    for (int h = 1; h < SP_EMI_WAVES; ++h) r += red[h];
    out_all[seg * SC_OUT + 3] = r;
  }
}

struct PartWs {
  double *L, *part;
  int *ab, *tabs;
  int part_rows;
  size_t bytes;
};

static PartWs part_carve(void* ws, long n_seg, long seg_len, long cells_cap) {
  WsCarver c{static_cast<char*>(ws)};
  PartWs r;
  r.L = c.take<double>(seg_len <= SP_LG_TABLE_MAX ? (size_t)seg_len + 1 : 1);
  r.part_rows = (int)(seg_len < SC_MAXC ? seg_len : SC_MAXC);   // T <= seg_len
  r.part = c.take<double>((size_t)n_seg * r.part_rows * SP_EMI_SLICES);
  r.ab = c.take<int>((size_t)n_seg * 2 * SC_MAXC);
  r.tabs = c.take<int>((size_t)n_seg * (size_t)cells_cap);
  r.bytes = c.off;
  return r;
}

}  // namespace mused

using namespace mused;

extern "C" {

long mused_score_partitions_ws_bytes(long n_seg, long seg_len, long cells_cap) {
  if (n_seg < 1 || seg_len < 1 || cells_cap < 1) return 256;
  return (long)part_carve(nullptr, n_seg, seg_len, cells_cap).bytes;
}

int mused_score_partitions(const int* truth, const int* pred, long n_seg, long seg_len, long cells_cap, int want_emi, double* out,
                           long* ints, int* info, int* table_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(truth && pred && out && ints && info && ws && n_seg > 0 && seg_len > 0 && cells_cap > 0,
                "mused_score_partitions: bad arguments");
  MUSED_REQUIRE(seg_len < (1l << 31) && n_seg < (1l << 31) && cells_cap <= (long)SC_MAXC * SC_MAXC,
                "mused_score_partitions: seg_len and n_seg must stay below 2^31, cells_cap at or below 4096^2");
  MUSED_REQUIRE((uintptr_t)ws % 8 == 0 && ws_bytes >= mused_score_partitions_ws_bytes(n_seg, seg_len, cells_cap),
                "mused_score_partitions: workspace too small or not 8-byte aligned");
  static LdsOptIn opt;
  const hipError_t aerr = allow_dynamic_lds(opt, reinterpret_cast<const void*>(partition_table_kernel), sizeof(PartLds));
  MUSED_CHECK_HIP(aerr);
  const hipStream_t st = (hipStream_t)stream;
  const PartWs w = part_carve(ws, n_seg, seg_len, cells_cap);
  // 16-byte loads need every segment to start on a 16-byte boundary
  const bool vec = ((uintptr_t)truth % 16 == 0) && ((uintptr_t)pred % 16 == 0) && (n_seg == 1 || seg_len % 4 == 0);
  const bool emi_ok = want_emi && seg_len <= SP_EMI_MAX_N;
  hipLaunchKernelGGL(partition_table_kernel, dim3((unsigned)n_seg), dim3(SC_THREADS), sizeof(PartLds), st, truth, pred, seg_len,
                     cells_cap, vec ? 1 : 0, emi_ok ? 1 : 0, out, ints, info, table_out, w.tabs, w.ab);
  MUSED_LAUNCH_CHECK();
  if (!emi_ok) return MUSED_OK;
  // MUSED_PARTITION_LGAMMA=direct (read per call): no table, every log-gamma evaluated where it is used -- the same values
  const char* mode = getenv("MUSED_PARTITION_LGAMMA");
  const bool tab = seg_len <= SP_LG_TABLE_MAX && !(mode && strcmp(mode, "direct") == 0);
  const long rows = 4096 / n_seg;
  const dim3 grid((unsigned)n_seg, (unsigned)(rows < 1 ? 1 : rows > w.part_rows ? w.part_rows : rows), SP_EMI_SLICES);
  if (tab) {
    const long blocks = (seg_len + 1 + 255) / 256;
    hipLaunchKernelGGL(partition_lgamma_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, st, w.L, seg_len + 1);
    MUSED_LAUNCH_CHECK();
    hipLaunchKernelGGL(partition_emi_kernel<true>, grid, dim3(SP_EMI_THREADS), 0, st, seg_len, info, w.ab, w.L, w.part, w.part_rows);
  } else {
    hipLaunchKernelGGL(partition_emi_kernel<false>, grid, dim3(SP_EMI_THREADS), 0, st, seg_len, info, w.ab, w.L, w.part, w.part_rows);
  }
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(partition_emi_merge_kernel, dim3((unsigned)n_seg), dim3(SP_EMI_THREADS), 0, st, info, w.part, out, w.part_rows);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
