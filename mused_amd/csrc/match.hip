// The label chain of approach "sSVDMC_pot" on the device: matched_t = match_clusters(matched_{t-1}, raw_t, "pot", min_overlap)
// (matrix_operations.py:155-210 with ot.sinkhorn written out -- the specification is mused_amd/sinkhorn.py) for a whole run
// of windows in ONE launch.  The windows are sequential by definition, so one workgroup of 16 waves owns the chain.
//
// Per window:
//   1. presence flags of the label values of prev / new in LDS (labels are k-means indices, 0 <= label < 1024), their
//      ranks by a ballot prefix scan: the sorted distinct values np.unique returns, P and N of them
//   2. the P x N positional overlap counts: integer atomics on a workspace (order independent)
//   3. the min_overlap rule and the feasibility test (every row and every column keeps a finite entry)
//   4. cost = |-overlap| or 1e9, / max, K = exp(cost / -0.1); then the Sinkhorn-Knopp iteration
//   5. plan > 0.5 max(plan), the largest selected row of a column wins (np.where's row-major order), relabel
//
// Layout of K (and of every sum): wave w owns rows w, w + 16, ...; lane l owns columns l, l + 64, ...  One lane holds its
// (rows / 16) x (columns / 64) entries in a private array.  The register file of a CU holds 512 KiB -- exactly 256 x 256
// doubles -- and 150 x 150 doubles already exceed LDS, so the largest size class keeps the rows of a wave beyond its first
// MT_RREG in the workspace (read twice per iteration, coalesced, L2 resident); K never goes through LDS.
// What the compiler makes of the private array (ROCm 7, 128 VGPRs per lane at 16 waves): P <= 32, N <= 64 all of it in
// registers, no scratch; the <10, 3> class 104 bytes of scratch per lane, a handful of reloads per iteration; the <16, 4>
// class 488 bytes, about four doubles of K reloaded from scratch for most rows in every iteration -- per-lane scratch
// (L1 / L2 resident), not registers.  DESIGN section 8 has the measured cost of that class.
//   row sums     (K v)_i     lane: fma chain over its columns in ascending order, then the wave butterfly (wave_ops.h)
//   column sums  (K^T u)_j   lane: fma chain over its rows in ascending order -> part[wave][j] in LDS -> every wave adds
//                            the 16 partials in wave order
// The order of every sum is a function of (i, j) alone, not of the size class.  u_i is needed by the wave that owns row
// i only, and the error check of iteration ii, |v (K^T u) - b|, IS the column sum iteration ii + 1 starts with: with the
// partials double-buffered one iteration costs ONE workgroup barrier.  u is never stored: it follows from v (u = 1 / (Kp v)),
// also at the exit.
//
// The host's sums run in BLAS's order, so the plan agrees within rounding, not bit for bit.  A decision rounding could turn
// raises a flag and ends the chain at that window (DESIGN section 8 derives the two margins):
//   MT_FLAG_SELECT  a plan entry within delta of the selection threshold 0.5 max(plan)
//   MT_FLAG_STOP    an error check within delta' of stopThr
//   MT_FLAG_RANGE   a label outside [0, 1024);  MT_FLAG_SIZE  P or N beyond 256
// The caller finishes a flagged window with the host specification and relaunches behind it.
#include "internal.h"
#include "match_labels.h"
#include "wave_ops.h"

namespace mused {

constexpr int MT_RREG = 10;       // rows per wave the largest size class keeps in its private array (of 16)
constexpr int MT_FLAG_SELECT = 1, MT_FLAG_STOP = 2;
constexpr int MT_ITERMAX = 1000;
constexpr double MT_STOPTHR = 1e-9;
constexpr double MT_REG = 0.1;
constexpr double MT_UNIT = 1.1102230246251565e-16;   // 2^-53
// 1 / (1 - tanh^2(D / 4)) for D = 2 / reg = 20, the largest Hilbert diameter of K for costs in [0, 1]: cosh^2(5)
constexpr double MT_HILBERT_AMP = 5507.0;

constexpr long MT_WS_OV_BYTES = 4l * MT_MAXC * MT_MAXC;
constexpr long MT_WS_KX_BYTES = 8l * (16 - MT_RREG) * 4 * MT_THREADS;

struct MatchLds {
  double part[2][MT_WAVES][MT_MAXC];  // column-sum partials, double-buffered over the iterations
  double red[2][MT_WAVES];
  ChainLds ch;      // steps 1, 2 and 5, the marks of step 3 and the selection (match_labels.h)
};
// the two words mt_chain zeroes before every window: an entry below min_overlap was seen; the largest count that reaches it
constexpr int MT_ANY_INF = 0, MT_MAX_OV = 1;

__device__ __forceinline__ double wave_allmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wave_allmin(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}

// Steps 3 - 5 of one window for the size class (RPW rows per wave, CPL columns per lane; rows r >= RREG live in kx).
// Returns the flag word; s.ch.map_row holds the selection when it is 0.  Not inlined: each size class gets its own register
// allocation (with 16 waves a lane has 128 VGPRs; what hipcc cannot keep of k[][] beside the working set it spills).
template <int RPW, int CPL, int RREG>
__device__ __noinline__ int match_solve(MatchLds& s, int P, int N, int min_overlap, const int* __restrict__ ov,
                                        double* __restrict__ kx_, double* __restrict__ plan_out, int* iters_out,
                                        int* feasible_out, float* margin_out) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  // a function that is not inlined sees generic pointers; with the address space named the workspace rows are loaded
  // from a uniform base plus the lane's offset instead of one 64-bit address register pair per entry
  typedef __attribute__((address_space(1))) double gdouble;
  gdouble* kx = (gdouble*)kx_;
  double k[RREG > 0 ? RREG : 1][CPL];
  // entry (r, c) of a row beyond the registers: kx[((r - RREG) * CPL + c) * MT_THREADS + t] (uniform base, lane offset t)
// BODY sees row r (i = r * 16 + w) of this lane's entries as kr[0 .. CPL): registers for r < RREG, a copy from kx beyond
#define MT_FOR_ROWS(BODY)                                                                      \
  _Pragma("unroll") for (int r = 0; r < RREG; ++r) {                                            \
    double* kr = k[r];                                                                         \
    BODY                                                                                       \
  }                                                                                            \
  _Pragma("unroll") for (int r = RREG; r < RPW; ++r) {                                          \
    double kr[CPL];                                                                            \
    _Pragma("unroll") for (int c = 0; c < CPL; ++c) kr[c] = (kx + ((r - RREG) * CPL + c) * MT_THREADS)[t]; \
    BODY                                                                                       \
  }

  // the row / column / any-inf marks of this lane's entries and the largest count
  int mx = 0;
#pragma unroll
  for (int r = 0; r < RPW; ++r)
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int i = r * MT_WAVES + w, j = c * 64 + l;
      if (i < P && j < N) {
        const int cnt = __hip_atomic_load(&ov[i * N + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cnt >= min_overlap) {
          s.ch.row_ok[i] = 1;
          s.ch.col_ok[j] = 1;
          mx = max(mx, cnt);
        } else {
          s.ch.word[MT_ANY_INF] = 1;
        }
      }
    }
  if (mx > 0) atomicMax(&s.ch.word[MT_MAX_OV], mx);
  if (!mt_feasible(s.ch, P, N)) {
    *feasible_out = 0;
    *iters_out = 0;
    *margin_out = 0.f;
    return 0;
  }
  *feasible_out = 1;

  // cost -> K, the operations of the specification: inf -> 1e9, abs, / max, exp(M / -reg); 0 outside the matrix
  const double max_ov = (double)s.ch.word[MT_MAX_OV];
  const double cmax = s.ch.word[MT_ANY_INF] ? fmax(1e9, max_ov) : max_ov;
  auto k_entry = [&](int r, int c) -> double {
    const int i = r * MT_WAVES + w, j = c * 64 + l;
    if (i >= P || j >= N) return 0.0;
    const int cnt = __hip_atomic_load(&ov[i * N + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return exp(((cnt >= min_overlap ? (double)cnt : 1e9) / cmax) / (-MT_REG));
  };
#pragma unroll
  for (int r = 0; r < RREG; ++r)
#pragma unroll
    for (int c = 0; c < CPL; ++c) k[r][c] = k_entry(r, c);
#pragma unroll
  for (int r = RREG; r < RPW; ++r)
#pragma unroll
    for (int c = 0; c < CPL; ++c) (kx + ((r - RREG) * CPL + c) * MT_THREADS)[t] = k_entry(r, c);

  const double bN = 1.0 / (double)N, aP = 1.0 / (double)P, ainv = 1.0 / aP;
  const double bnorm = sqrt((double)N) * bN;
  const int nmax = max(P, N);
  const double e_side = 4.0 * (nmax + 4) * MT_UNIT;   // rounding of one iteration in Hilbert's metric, one side
  double v[CPL], cp[CPL];
  bool cv[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    cv[c] = c * 64 + l < N;
    v[c] = cv[c] ? bN : 0.0;
    cp[c] = 0.0;
  }
  // K^T u for u = ones(P) / P
  MT_FOR_ROWS(if (r * MT_WAVES + w < P) {
    _Pragma("unroll") for (int c = 0; c < CPL; ++c) cp[c] = fma(kr[c], aP, cp[c]);
  })
#pragma unroll
  for (int c = 0; c < CPL; ++c) s.part[0][w][c * 64 + l] = cp[c];

  int it = MT_ITERMAX, flags = 0;
  double err_prev = -1.0;
  for (int ii = 0; ii < MT_ITERMAX; ++ii) {
    __syncthreads();   // the one barrier of an iteration: the partials of K^T u are complete
    const int buf = ii & 1;
    double ktu[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      double a = s.part[buf][0][c * 64 + l];
#pragma unroll
      for (int h = 1; h < MT_WAVES; ++h) a += s.part[buf][h][c * 64 + l];
      ktu[c] = a;
      __builtin_amdgcn_sched_barrier(0);   // 16 reads in flight, not 16 * CPL: the registers hold K
    }
    if (ii > 0 && (ii - 1) % 10 == 0) {
      // the check of iteration ii - 1: err = |v * (K^T u) - b| with the u, v that iteration produced.  Every wave
      // computes it from the same numbers in the same order, so the branch is uniform over the workgroup.
      double q = 0.0;
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const double d = cv[c] ? v[c] * ktu[c] - bN : 0.0;
        q = fma(d, d, q);
      }
      const double err = sqrt(wave_allsum(q));
      // delta': what the scalings of the two implementations can differ by after ii iterations, as a change of err
      double amp = fmin((double)ii, MT_HILBERT_AMP);
      if (err_prev > 0.0 && err < err_prev) amp = fmin(amp, sqrt((double)nmax) * 10.0 / (1.0 - err / err_prev));
      const double dstop = (4.0 * e_side * amp + 2.0 * (nmax + 4) * MT_UNIT) * (bnorm + err);
      if (fabs(err - MT_STOPTHR) <= dstop) flags |= MT_FLAG_STOP;
      err_prev = err;
      if (flags || err < MT_STOPTHR) {
        it = ii;
        break;
      }
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      v[c] = cv[c] ? bN / ktu[c] : 0.0;
      cp[c] = 0.0;
    }
    MT_FOR_ROWS(if (r * MT_WAVES + w < P) {
      double a = 0.0;
      _Pragma("unroll") for (int c = 0; c < CPL; ++c) a = fma(kr[c], v[c], a);
      const double u = 1.0 / (ainv * wave_allsum(a));
      _Pragma("unroll") for (int c = 0; c < CPL; ++c) cp[c] = fma(kr[c], u, cp[c]);
      __builtin_amdgcn_sched_barrier(0);   // one row at a time: interleaving the rows' reductions spills K
    })
#pragma unroll
    for (int c = 0; c < CPL; ++c) s.part[buf ^ 1][w][c * 64 + l] = cp[c];
  }
  *iters_out = it;
  if (flags) {
    *margin_out = 0.f;
    return flags;
  }

  // plan = u[:, None] * K * v[None, :] with u = 1 / (Kp v); its maximum, then the selection
  auto row_u = [&](const double* kr) -> double {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) a = fma(kr[c], v[c], a);
    return 1.0 / (ainv * wave_allsum(a));
  };
  double pmax = 0.0;
  MT_FOR_ROWS(if (r * MT_WAVES + w < P) {
    const double u = row_u(kr);
    _Pragma("unroll") for (int c = 0; c < CPL; ++c) pmax = fmax(pmax, (u * kr[c]) * v[c]);
    __builtin_amdgcn_sched_barrier(0);
  })
  pmax = wave_allmax(pmax);
  if (l == 0) s.red[0][w] = pmax;
  __syncthreads();
  pmax = s.red[0][0];
#pragma unroll
  for (int h = 1; h < MT_WAVES; ++h) pmax = fmax(pmax, s.red[0][h]);
  const double thr = pmax * 0.5;
  double mrg = 1.0e300;
  MT_FOR_ROWS(if (r * MT_WAVES + w < P) {
    const int i = r * MT_WAVES + w;
    const double u = row_u(kr);
    _Pragma("unroll") for (int c = 0; c < CPL; ++c) {
      const int j = c * 64 + l;
      if (j < N) {
        const double p = (u * kr[c]) * v[c];
        if (p > thr) atomicMax(&s.ch.map_row[j], i);
        mrg = fmin(mrg, fabs(p - thr) / thr);
        if (plan_out) plan_out[i * N + j] = p;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  })
#undef MT_FOR_ROWS
  mrg = wave_allmin(mrg);
  if (l == 0) s.red[1][w] = mrg;
  __syncthreads();
  mrg = s.red[1][0];
#pragma unroll
  for (int h = 1; h < MT_WAVES; ++h) mrg = fmin(mrg, s.red[1][h]);
  *margin_out = (float)mrg;
  // delta: the plans of the two implementations differ by 2 D relative, D = 2 e_side min(it, amp); entry and threshold both move
  const double dsel = 4.0 * (2.0 * e_side * fmin((double)it, MT_HILBERT_AMP));
  return mrg <= dsel ? MT_FLAG_SELECT : 0;
}

__global__ __launch_bounds__(MT_THREADS) void match_pot_chain_kernel(const int* __restrict__ raw, int K_windows, int W,
                                                                     const int* __restrict__ prev0, int min_overlap,
                                                                     int* __restrict__ matched, int* __restrict__ info,
                                                                     double* __restrict__ plan_out, int* __restrict__ ov,
                                                                     double* __restrict__ kx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mt_lds[];
  MatchLds& s = *reinterpret_cast<MatchLds*>(mt_lds);
  mt_chain(s.ch, raw, K_windows, W, prev0, matched, info, ov, [&](int tw, int P, int N) {
    // match_solve is not inlined, and it addresses LDS with ds instructions only if the compiler's constant propagation
    // across functions, which runs before this lambda is inlined, sees every call site pass the LDS base itself.  A `s`
    // captured by reference is a load from the closure at that point: match_solve then takes a generic pointer, uses flat
    // loads and stores for LDS, and the <16, 4> class grows from 16,908 to 18,712 instructions and from 488 to 516 bytes
    // of scratch.  So the lambda names mt_lds again.
    MatchLds& s = *reinterpret_cast<MatchLds*>(mt_lds);
    int iters = 0, feasible = 0, flags;
    float margin = 0.f;
    double* po = plan_out ? plan_out + (long)tw * MT_MAXC * MT_MAXC : nullptr;
    if (P <= 2 * MT_WAVES && N <= 64) flags = match_solve<2, 1, 2>(s, P, N, min_overlap, ov, kx, po, &iters, &feasible, &margin);
    else if (P <= 10 * MT_WAVES && N <= 192) flags = match_solve<10, 3, 10>(s, P, N, min_overlap, ov, kx, po, &iters, &feasible, &margin);
    else flags = match_solve<16, 4, MT_RREG>(s, P, N, min_overlap, ov, kx, po, &iters, &feasible, &margin);
    if (!flags) __syncthreads();   // map_row is complete
    return ChainSolved{iters, feasible, flags, __float_as_int(margin)};
  });
}

}  // namespace mused

using namespace mused;

extern "C" {

long mused_match_pot_ws_bytes(void) { return MT_WS_OV_BYTES + MT_WS_KX_BYTES; }

int mused_match_pot_chain(const int* raw, int K_windows, int W, const int* prev0, int min_overlap, int* matched_out,
                          int* info_out, double* plan_out, void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(raw && matched_out && info_out && ws && K_windows > 0 && W > 0, "mused_match_pot_chain: bad arguments");
  MUSED_REQUIRE((long)K_windows * W < (1l << 31) && K_windows < (1 << 24), "mused_match_pot_chain: K_windows * W must stay below 2^31");
  MUSED_REQUIRE(ws_bytes >= mused_match_pot_ws_bytes(), "mused_match_pot_chain: workspace too small");
  static LdsOptIn opt;
  const hipError_t aerr = allow_dynamic_lds(opt, reinterpret_cast<const void*>(match_pot_chain_kernel), sizeof(MatchLds));
  MUSED_CHECK_HIP(aerr);
  int* ov = (int*)ws;
  double* kx = (double*)((char*)ws + MT_WS_OV_BYTES);
  hipLaunchKernelGGL(match_pot_chain_kernel, dim3(1), dim3(MT_THREADS), sizeof(MatchLds), (hipStream_t)stream, raw, K_windows, W,
                     prev0, min_overlap, matched_out, info_out, plan_out, ov, kx);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
