// Scoring a run: the seven numbers of the reference's compute_all_metrics (metrics_evaluation.py:47-92) from the
// true-class x predicted-cluster contingency table, one workgroup of SC_THREADS threads per segment of labels, one launch.
// The arithmetic is the one mused_amd/scores.py states (scikit-learn's); what differs is the device `log` and the order
// of the fp64 sums, so five values agree within rounding while accuracy and MAE (one division of exact integers each)
// are equal.
//
// Per segment: (1) presence bits of both sides in LDS, label values -1 .. 65534 at offset 1; (2) ranks = per-word prefix
// counts plus a popcount below the bit, computed where needed; (3) the T x P counts, in LDS while T * P <= SC_LDS_CELLS,
// else in the segment's slice of the workspace (cleared here), with integer atomics: equal cells of the 256 rows a wave
// holds are combined first; (4) row / column sums, then the sums of the seven values: every thread takes its share in a
// fixed order, a fixed tree follows, no floating-point atomics -- the result is a function of the segment's labels alone.
#include "internal.h"

#pragma clang fp contract(off)   // p * x + p * y as scikit-learn writes it: two products and a sum

namespace mused {

constexpr int SC_THREADS = 1024;
constexpr int SC_WAVES = 16;
constexpr int SC_WORDS = 1024;         // 64-bit presence words per side: 65,536 label values
constexpr int SC_MAXC = 4096;          // largest T, P
constexpr int SC_LDS_CELLS = 24576;    // largest table kept in LDS (96 KiB)
constexpr int SC_OUT = 8, SC_INFO = 8; // doubles of out, ints of info per segment
constexpr int SC_FLAG_RANGE = 4, SC_FLAG_SIZE = 8;   // the label chains' flag values (match_labels.h)
constexpr int SC_SUMS = 9;

static_assert(SC_THREADS == SC_WORDS, "one thread per presence word in the rank pass");

struct ScoreLds {
  unsigned long long bm[2][SC_WORDS];   // presence of value v at bit v + 1: [0] true, [1] predicted
  int pre[2][SC_WORDS];                 // set bits in the words before this one
  int rs[SC_MAXC], cs[SC_MAXC];         // row and column sums
  int wtot[2][SC_WAVES];
  double red[SC_SUMS][SC_WAVES];
  unsigned long long iacc[2];           // sum |t - c|, agreeing rows
  int inter, pe, bad;
  int tab[SC_LDS_CELLS];
};
static_assert(sizeof(ScoreLds) <= 160 * 1024, "one workgroup's LDS");

// Four consecutive labels of both sides (rows 4 q .. 4 q + 3 of the segment); returns how many exist.
__device__ __forceinline__ int sc_load4(const int* __restrict__ tr, const int* __restrict__ pr, long q, long n, bool vec, int* a,
                                        int* b) {
  const long i = q << 2;
  if (i >= n) return 0;
  if (vec && i + 3 < n) {
    const int4 x = *reinterpret_cast<const int4*>(tr + i), y = *reinterpret_cast<const int4*>(pr + i);
    a[0] = x.x, a[1] = x.y, a[2] = x.z, a[3] = x.w;
    b[0] = y.x, b[1] = y.y, b[2] = y.z, b[3] = y.w;
    return 4;
  }
  const int c = (int)(n - i < 4 ? n - i : 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = j < c ? tr[i + j] : 0;
    b[j] = j < c ? pr[i + j] : 0;
  }
  return c;
}

__device__ __forceinline__ int sc_rank(const ScoreLds& s, int side, int v) {
  const unsigned x = (unsigned)v + 1u;
  return s.pre[side][x >> 6] + __popcll(s.bm[side][x >> 6] & ((1ull << (x & 63)) - 1ull));
}

template <bool LDS>
__device__ __forceinline__ void sc_add(ScoreLds& s, int* __restrict__ gtab, int cell, int v) {
  if (LDS) atomicAdd(&s.tab[cell], v);
  else atomicAdd(&gtab[cell], v);
}

template <bool LDS>
__device__ __forceinline__ int sc_cell(const ScoreLds& s, const int* gtab, int e) {
  return LDS ? s.tab[e] : __hip_atomic_load(&gtab[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Step 3.  A wave holds up to 256 rows per pass.  Twice, the cell of its first row still uncounted is taken, every row
// of the wave in that cell is counted by ballot and ONE add is issued; what is left after that adds itself.  (Binary
// labels at noise rate 0.95: 19 of 20 rows share a cell, and two rounds leave 1 row in 400.)
template <bool LDS>
__device__ __forceinline__ void sc_counts(ScoreLds& s, const int* __restrict__ tr, const int* __restrict__ pr, long n, bool vec,
                                          int P, int* __restrict__ gtab) {
  const int t = threadIdx.x, l = t & 63;
  const long nq = (n + 3) >> 2;
  unsigned long long dsum = 0, agree = 0;
  for (long base = 0; base < nq; base += SC_THREADS) {   // uniform trip count: the ballots below need every lane
    int a[4], b[4], c[4];
    bool act[4];
    const int cnt = sc_load4(tr, pr, base + t, n, vec, a, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      act[j] = j < cnt;
      c[j] = 0;
      if (act[j]) {
        c[j] = sc_rank(s, 0, a[j]) * P + sc_rank(s, 1, b[j]);
        const long d = (long)a[j] - (long)b[j];
        dsum += (unsigned long long)(d < 0 ? -d : d);
        agree += a[j] == b[j];
      }
    }
    for (int r = 0; r < 2; ++r) {
      const unsigned long long b0 = __ballot(act[0]), b1 = __ballot(act[1]), b2 = __ballot(act[2]), b3 = __ballot(act[3]);
      if (!(b0 | b1 | b2 | b3)) break;
      const int js = b0 ? 0 : b1 ? 1 : b2 ? 2 : 3;
      const unsigned long long bj = js == 0 ? b0 : js == 1 ? b1 : js == 2 ? b2 : b3;
      const int leader = __ffsll((long long)bj) - 1;
      const int lc = __shfl(js == 0 ? c[0] : js == 1 ? c[1] : js == 2 ? c[2] : c[3], leader);
      int total = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool hit = act[j] && c[j] == lc;
        total += __popcll(__ballot(hit));
        act[j] = act[j] && !hit;
      }
      if (l == leader) sc_add<LDS>(s, gtab, lc, total);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (act[j]) sc_add<LDS>(s, gtab, c[j], 1);
  }
  atomicAdd(&s.iacc[0], dsum);   // integers: exact in any order
  atomicAdd(&s.iacc[1], agree);
}

// one copy of the library's fp64 log instead of one per call site
__device__ __attribute__((noinline)) double sc_log(double x) { return log(x); }

__device__ __forceinline__ double sc_snap(double term) { return fabs(term) < 0x1p-52 ? 0.0 : term; }

// Step 4, from the finished table.  Thread 0 returns with the results written.
template <bool LDS>
__device__ __forceinline__ void sc_finalise(ScoreLds& s, const int* gtab, int T, int P, long n, double* __restrict__ out,
                                            int* __restrict__ inf) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  // row sums by wave, column sums by integer atomics on the way
  for (int i = w; i < T; i += SC_WAVES) {
    int acc = 0;
    for (int j = l; j < P; j += 64) {
      const int v = sc_cell<LDS>(s, gtab, i * P + j);
      acc += v;
      if (v) atomicAdd(&s.cs[j], v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (l == 0) s.rs[i] = acc;
  }
  __syncthreads();
  // event rows: true value > 0, that is rank >= e0 = how many of the values -1 and 0 are present
  const int e0 = __popcll(s.bm[0][0] & 3ull);
  const long ne = n - (e0 >= 1 ? s.rs[0] : 0) - (e0 >= 2 ? s.rs[1] : 0);
  const int Te = T - e0;
  int pe_local = 0;
  for (int j = t; j < P; j += SC_THREADS) {
    const int ce = s.cs[j] - (e0 >= 1 ? sc_cell<LDS>(s, gtab, j) : 0) - (e0 >= 2 ? sc_cell<LDS>(s, gtab, P + j) : 0);
    pe_local += ce > 0;
  }
  if (pe_local) atomicAdd(&s.pe, pe_local);
  __syncthreads();
  const int Pe = s.pe;
  const bool ev = Te > 1 && Pe > 1;   // metrics_evaluation.py:61

  double sum[SC_SUMS];
#pragma unroll
  for (int k = 0; k < SC_SUMS; ++k) sum[k] = 0.0;
  const double dn = (double)n, logn = sc_log(dn), dne = (double)ne, logne = ev ? sc_log(dne) : 0.0;
  // [0] MI of the whole table, [1] MI of the event rows: non-zero cells in index order
  for (int e = t; e < T * P; e += SC_THREADS) {
    const int c = sc_cell<LDS>(s, gtab, e);
    if (!c) continue;
    const int i = e / P, j = e - i * P;
    const double dc = (double)c, logc = sc_log(dc);
    {
      const double p = dc / dn;
      const double lo = -sc_log((double)((long long)s.rs[i] * (long long)s.cs[j])) + logn + logn;
      sum[0] += sc_snap(p * (logc - logn) + p * lo);
    }
    if (ev && i >= e0) {
      const int ce = s.cs[j] - (e0 >= 1 ? sc_cell<LDS>(s, gtab, j) : 0) - (e0 >= 2 ? sc_cell<LDS>(s, gtab, P + j) : 0);
      const double p = dc / dne;
      const double lo = -sc_log((double)((long long)s.rs[i] * (long long)ce)) + logne + logne;
      sum[1] += sc_snap(p * (logc - logne) + p * lo);
    }
  }
  // [2] [3] entropies of the two sides, [4] [5] of the event rows (negated at the end)
  for (int i = t; i < T; i += SC_THREADS) {
    const double c = (double)s.rs[i], lc = sc_log(c);
    sum[2] += (c / dn) * (lc - logn);
    if (ev && i >= e0) sum[4] += (c / dne) * (lc - logne);
  }
  for (int j = t; j < P; j += SC_THREADS) {
    const double c = (double)s.cs[j];
    sum[3] += (c / dn) * (sc_log(c) - logn);
    if (ev) {
      const int ce = s.cs[j] - (e0 >= 1 ? sc_cell<LDS>(s, gtab, j) : 0) - (e0 >= 2 ? sc_cell<LDS>(s, gtab, P + j) : 0);
      if (ce > 0) sum[5] += ((double)ce / dne) * (sc_log((double)ce) - logne);
    }
  }
  // [6] [7] [8] f1, precision, recall times the class weight (true_sum).  A class only the predictions hold has weight
  // 0 and adds 0.  A value sits at the same bit of both bitmaps, so the owner of a word sees both ranks.
  {
    unsigned long long wt = s.bm[0][t];
    const unsigned long long wp = s.bm[1][t];
    int i = s.pre[0][t];
    while (wt) {
      const unsigned long long bit = wt & (~wt + 1ull);
      wt ^= bit;
      const double a = (double)s.rs[i];
      double tp = 0.0, ps = 0.0;
      if (wp & bit) {
        const int j = s.pre[1][t] + __popcll(wp & (bit - 1ull));
        tp = (double)sc_cell<LDS>(s, gtab, i * P + j);
        ps = (double)s.cs[j];
      }
      sum[6] += ((2.0 * tp) / (a + ps)) * a;
      sum[7] += (ps != 0.0 ? tp / ps : 0.0) * a;
      sum[8] += (tp / a) * a;
      ++i;
    }
  }
#pragma unroll
  for (int k = 0; k < SC_SUMS; ++k) {
    const double v = wave_sum(sum[k]);
    if (l == 0) s.red[k][w] = v;
  }
  __syncthreads();
  if (t < SC_SUMS) {   // the waves' partial sums in wave order
    double v = 0.0;
    for (int h = 0; h < SC_WAVES; ++h) v += s.red[t][h];
    s.red[t][0] = v;
  }
  __syncthreads();
  if (t != 0) return;
#pragma unroll
  for (int k = 0; k < SC_SUMS; ++k) sum[k] = s.red[k][0];
  double nmi, nmi_e = 0.0;
  if (T == 1 && P == 1) nmi = 1.0;
  else {
    const double mi = sum[0] > 0.0 ? sum[0] : 0.0;
    const double ht = T == 1 ? 0.0 : -sum[2], hp = P == 1 ? 0.0 : -sum[3];
    nmi = mi == 0.0 ? 0.0 : mi / ((ht + hp) / 2.0);
  }
  if (ev) {
    const double mi = sum[1] > 0.0 ? sum[1] : 0.0;
    nmi_e = mi == 0.0 ? 0.0 : mi / ((-sum[4] + -sum[5]) / 2.0);
  }
  const unsigned long long dsum = s.iacc[0], agree = s.iacc[1];
  out[0] = sum[6] / dn;
  out[1] = nmi;
  out[2] = nmi_e;
  out[3] = sum[7] / dn;
  out[4] = sum[8] / dn;
  out[5] = (double)agree / dn;
  out[6] = (double)dsum / dn;
  out[7] = (double)dsum;
  inf[0] = T;
  inf[1] = P;
  inf[2] = T + P - s.inter;
  inf[3] = (int)ne;
  inf[4] = (int)agree;
  inf[5] = inf[6] = inf[7] = 0;
}

__global__ __launch_bounds__(SC_THREADS) void score_labels_kernel(const int* __restrict__ truth, const int* __restrict__ pred,
                                                                   long seg_len, long cells_cap, int vec,
                                                                   double* __restrict__ out_all, int* __restrict__ info_all,
                                                                   int* __restrict__ ws) {
  extern __shared__ __align__(16) unsigned char sc_raw[];
  ScoreLds& s = *reinterpret_cast<ScoreLds*>(sc_raw);
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const long seg = blockIdx.x;
  const int* tr = truth + seg * seg_len;
  const int* pr = pred + seg * seg_len;
  int* gtab = ws + seg * cells_cap;
  double* out = out_all + seg * SC_OUT;
  int* inf = info_all + seg * SC_INFO;

  s.bm[0][t] = 0;
  s.bm[1][t] = 0;
  for (int i = t; i < SC_MAXC; i += SC_THREADS) s.rs[i] = s.cs[i] = 0;
  if (t == 0) {
    s.iacc[0] = s.iacc[1] = 0;
    s.inter = s.pe = s.bad = 0;
  }
  __syncthreads();
  // step 1: presence
  const long nq = (seg_len + 3) >> 2;
  for (long q = t; q < nq; q += SC_THREADS) {
    int a[4], b[4];
    const int cnt = sc_load4(tr, pr, q, seg_len, vec != 0, a, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // constant indices: a and b stay in registers
      if (j >= cnt) continue;
      const unsigned x = (unsigned)a[j] + 1u, y = (unsigned)b[j] + 1u;
      if (x >= 65536u || y >= 65536u) {
        s.bad = 1;
        continue;
      }
      const unsigned long long mx = 1ull << (x & 63), my = 1ull << (y & 63);
      if (!(s.bm[0][x >> 6] & mx)) atomicOr(&s.bm[0][x >> 6], mx);   // the plain read only spares repeated atomics
      if (!(s.bm[1][y >> 6] & my)) atomicOr(&s.bm[1][y >> 6], my);
    }
  }
  __syncthreads();
  // step 2: exclusive prefix counts of the words
  const unsigned long long wt = s.bm[0][t], wp = s.bm[1][t];
  const int ct = __popcll(wt), cp = __popcll(wp), cu = __popcll(wt & wp);
  int it = ct, ip = cp;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int vt = __shfl_up(it, o), vp = __shfl_up(ip, o);
    if (l >= o) {
      it += vt;
      ip += vp;
    }
  }
  if (l == 63) {
    s.wtot[0][w] = it;
    s.wtot[1][w] = ip;
  }
  if (cu) atomicAdd(&s.inter, cu);
  __syncthreads();
  int T = 0, P = 0, offt = 0, offp = 0;
  for (int h = 0; h < SC_WAVES; ++h) {
    if (h == w) {
      offt = T;
      offp = P;
    }
    T += s.wtot[0][h];
    P += s.wtot[1][h];
  }
  s.pre[0][t] = offt + it - ct;
  s.pre[1][t] = offp + ip - cp;
  int flags = s.bad ? SC_FLAG_RANGE : 0;
  if (T > SC_MAXC || P > SC_MAXC || (long)T * (long)P > cells_cap) flags |= SC_FLAG_SIZE;
  if (flags) {   // uniform
    if (t < SC_OUT) out[t] = 0.0;
    if (t < SC_INFO) inf[t] = t == 0 ? T : t == 1 ? P : t == 5 ? flags : 0;
    return;
  }
  // step 3: counts
  const int cells = T * P;
  const bool in_lds = cells <= SC_LDS_CELLS;
  if (in_lds) {
    for (int e = t; e < cells; e += SC_THREADS) s.tab[e] = 0;
  } else {
    for (int e = t; e < cells; e += SC_THREADS) gtab[e] = 0;
    __threadfence();
  }
  __syncthreads();   // also completes `pre`
  if (in_lds) sc_counts<true>(s, tr, pr, seg_len, vec != 0, P, gtab);
  else sc_counts<false>(s, tr, pr, seg_len, vec != 0, P, gtab);
  __threadfence();
  __syncthreads();
  if (in_lds) sc_finalise<true>(s, gtab, T, P, seg_len, out, inf);
  else sc_finalise<false>(s, gtab, T, P, seg_len, out, inf);
}

}  // namespace mused

using namespace mused;

extern "C" {

long mused_score_ws_bytes(long n_seg, long cells_cap) {
  if (n_seg < 1 || cells_cap < 1) return 4;
  return 4l * n_seg * cells_cap;
}

int mused_score_labels(const int* truth, const int* pred, long n_seg, long seg_len, long cells_cap, double* out, int* info,
                       void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(truth && pred && out && info && ws && n_seg > 0 && seg_len > 0 && cells_cap > 0, "mused_score_labels: bad arguments");
  MUSED_REQUIRE(seg_len < (1l << 31) && n_seg < (1l << 31) && cells_cap <= (long)SC_MAXC * SC_MAXC,
                "mused_score_labels: seg_len and n_seg must stay below 2^31, cells_cap at or below 4096^2");
  MUSED_REQUIRE(ws_bytes >= mused_score_ws_bytes(n_seg, cells_cap), "mused_score_labels: workspace too small");
  static std::once_flag once;
  static hipError_t aerr = hipSuccess;
  std::call_once(once, [] {
    CaptureLock lk(capture_mutex());
    aerr = hipFuncSetAttribute(reinterpret_cast<const void*>(score_labels_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)sizeof(ScoreLds));
  });
  MUSED_CHECK_HIP(aerr);
  // 16-byte loads need every segment to start on a 16-byte boundary
  const bool vec = ((uintptr_t)truth % 16 == 0) && ((uintptr_t)pred % 16 == 0) && (n_seg == 1 || seg_len % 4 == 0);
  hipLaunchKernelGGL(score_labels_kernel, dim3((unsigned)n_seg), dim3(SC_THREADS), sizeof(ScoreLds), (hipStream_t)stream, truth, pred,
                     seg_len, cells_cap, vec ? 1 : 0, out, info, (int*)ws);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
