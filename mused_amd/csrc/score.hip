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
// Steps 1-3 live in score_table.h, which score_partitions.hip shares.
#include "score_table.h"

#pragma clang fp contract(off)   // p * x + p * y as scikit-learn writes it: two products and a sum

namespace mused {

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
  const int t = threadIdx.x;
  const long seg = blockIdx.x;
  const int* tr = truth + seg * seg_len;
  const int* pr = pred + seg * seg_len;
  int* gtab = ws + seg * cells_cap;
  double* out = out_all + seg * SC_OUT;
  int* inf = info_all + seg * SC_INFO;

  int T, P;
  sc_presence_ranks(s, tr, pr, seg_len, vec, T, P);
  int flags = s.bad ? SC_FLAG_RANGE : 0;
  if (T > SC_MAXC || P > SC_MAXC || (long)T * (long)P > cells_cap) flags |= SC_FLAG_SIZE;
  if (flags) {   // uniform
    if (t < SC_OUT) out[t] = 0.0;
    if (t < SC_INFO) inf[t] = t == 0 ? T : t == 1 ? P : t == 5 ? flags : 0;
    return;
  }
  const bool in_lds = sc_build_table(s, tr, pr, seg_len, vec, T, P, gtab);
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
  static LdsOptIn opt;
  const hipError_t aerr = allow_dynamic_lds(opt, reinterpret_cast<const void*>(score_labels_kernel), sizeof(ScoreLds));
  MUSED_CHECK_HIP(aerr);
  // 16-byte loads need every segment to start on a 16-byte boundary
  const bool vec = ((uintptr_t)truth % 16 == 0) && ((uintptr_t)pred % 16 == 0) && (n_seg == 1 || seg_len % 4 == 0);
  hipLaunchKernelGGL(score_labels_kernel, dim3((unsigned)n_seg), dim3(SC_THREADS), sizeof(ScoreLds), (hipStream_t)stream, truth, pred,
                     seg_len, cells_cap, vec ? 1 : 0, out, info, (int*)ws);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
