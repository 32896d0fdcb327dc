// Fusion of M <= 8 modality bitmasks by a truth table, in ONE pass: every input word read once, every output word written once.
//   subset s in [0, 2^M): bit m set when modality m has the edge;  out bit (i, j) = T[s(i, j)],  T = 256 bits (4 uint64).
// OR, AND, "at least t of M" and every weighted vote  sum_m w_m [A_m has (i, j)] >= tau  are tables; the table of
// (weights, tau) is built on the HOST (fuse_threshold_table below: the fp64 sum from 0.0, IN MODALITY ORDER, of w_m over the set
// bits -- plain additions, nothing reassociated -- compared with >= tau; T[0] = 0 always), so the device does no floating point.
// Kernel: a thread loads its word (its 16-byte pair of words where the buffers allow it) from each of the M masks and evaluates
// the table on all 64 bits at once, as a multiplexer tree over the modalities: f_L(base) = x[L-1] ? f_{L-1}(base + 2^(L-1)) :
// f_{L-1}(base), f_0(base) = T[base] spread over the word -- 2^M - 1 bitwise selects, the leaves wave-uniform (the table comes
// by value in the launch arguments and lives in scalar registers).  M is a template parameter: the tree unrolls fully.
// The masks share one pitch and T[0] = 0, so the kernel runs over the n * words words as one flat array: padding words and the
// columns >= n of inputs that keep them clear stay clear.  A thread reads all of its inputs before it writes: out may be any input.
#include "internal.h"

namespace mused {

constexpr int FUSE_TABLE_MAX_M = 8;
constexpr int FUSE_TABLE_MAX_PAIR_M = 6;   // the 16-byte kernel up to here (below)

struct FuseTableArgs {
  const unsigned long long* p[FUSE_TABLE_MAX_M];
  unsigned long long t[4];
};

// L modalities still to decide (x[0 .. L-1]); BASE = the subset bits of the modalities above them
template <int L, int BASE>
struct FuseMux {
  static __device__ __forceinline__ unsigned long long eval(const unsigned long long* x, const FuseTableArgs& a) {
    const unsigned long long lo = FuseMux<L - 1, BASE>::eval(x, a);
    const unsigned long long hi = FuseMux<L - 1, BASE + (1 << (L - 1))>::eval(x, a);
    return (x[L - 1] & hi) | (~x[L - 1] & lo);
  }
};

template <int BASE>
struct FuseMux<0, BASE> {
  static __device__ __forceinline__ unsigned long long eval(const unsigned long long*, const FuseTableArgs& a) {
    return 0ull - ((a.t[BASE >> 6] >> (BASE & 63)) & 1ull);
  }
};

// The last select has two wave-uniform inputs: c0 ^ (x & (c0 ^ c1)) keeps both in scalar registers (a select of two uniform
// words would first copy them into vector registers, 2^M of them)
template <int BASE>
struct FuseMux<1, BASE> {
  static __device__ __forceinline__ unsigned long long eval(const unsigned long long* x, const FuseTableArgs& a) {
    const unsigned long long c0 = FuseMux<0, BASE>::eval(x, a);
    const unsigned long long d = c0 ^ FuseMux<0, BASE + 1>::eval(x, a);
    return c0 ^ (x[0] & d);
  }
};

// PAIR: `total` counts 16-byte pairs of words (every pointer 16-byte aligned, n * words even).  Two trees share the 2^M leaf
// constants: up to M = 6 they fit the scalar registers of 8 waves per SIMD (75 at M = 6); at M = 7 and 8 the pair kernel would
// take 106 (7 waves), so those run one word per thread (42 at M = 8) and the pair kernel is not instantiated for them
// (measured at M = 8, n = 10^4: 41.0 us with pairs, 35.5 us without; there the 2^M selects, not the bytes, set the time)
template <int M, bool PAIR>
__global__ void __launch_bounds__(256) adj_fuse_table_kernel(FuseTableArgs a, long total, unsigned long long* out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if constexpr (PAIR) {
    unsigned long long x0[M], x1[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const ulonglong2 v = reinterpret_cast<const ulonglong2*>(a.p[m])[i];
      x0[m] = v.x;
      x1[m] = v.y;
    }
    ulonglong2 r;
    r.x = FuseMux<M, 0>::eval(x0, a);
    r.y = FuseMux<M, 0>::eval(x1, a);
    reinterpret_cast<ulonglong2*>(out)[i] = r;
  } else {
    unsigned long long x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = a.p[m][i];
    out[i] = FuseMux<M, 0>::eval(x, a);
  }
}

template <int M>
static int adj_fuse_table_launch(const FuseTableArgs& a, long words_total, bool pair, unsigned long long* out, hipStream_t st) {
  if constexpr (M <= FUSE_TABLE_MAX_PAIR_M) {
    if (pair) {
      const long total = words_total / 2;
      hipLaunchKernelGGL((adj_fuse_table_kernel<M, true>), dim3(cdiv(total, 256)), dim3(256), 0, st, a, total, out);
      MUSED_LAUNCH_CHECK();
      return MUSED_OK;
    }
  }
  hipLaunchKernelGGL((adj_fuse_table_kernel<M, false>), dim3(cdiv(words_total, 256)), dim3(256), 0, st, a, words_total, out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// The table of (weights, tau): T[s] = 1 iff s != 0 and score(s) >= tau.  weights NULL: every weight 1.0.  MUSED_ERR_ARG on a
// weight that is not finite and > 0 and on a tau that is not finite, not > 0 or above the score of the full subset
static int fuse_threshold_table(const double* weights, int M, double tau, unsigned long long* table, const char* who) {
  MUSED_REQUIRE(M >= 1 && M <= FUSE_TABLE_MAX_M, "%s: M = %d modalities outside 1 .. %d", who, M, FUSE_TABLE_MAX_M);
  double w[FUSE_TABLE_MAX_M];
  for (int m = 0; m < M; ++m) {
    w[m] = weights ? weights[m] : 1.0;
    MUSED_REQUIRE(w[m] > 0.0 && w[m] <= 1.7976931348623157e308, "%s: weight %d = %g is not finite and > 0", who, m, w[m]);
  }
  table[0] = table[1] = table[2] = table[3] = 0ull;
  double full = 0.0;
  for (int s = 1; s < (1 << M); ++s) {
    double score = 0.0;            // plain fp64 additions in modality order
    for (int m = 0; m < M; ++m)
      if ((s >> m) & 1) score = score + w[m];
    full = score;                  // the last subset is the full one
    if (score >= tau) table[s >> 6] |= 1ull << (s & 63);
  }
  MUSED_REQUIRE(tau > 0.0 && tau <= 1.7976931348623157e308, "%s: tau = %g is not finite and > 0", who, tau);
  MUSED_REQUIRE(tau <= full, "%s: tau = %.17g is above the score of all %d modalities, %.17g", who, tau, M, full);
  return MUSED_OK;
}

}  // namespace mused

using namespace mused;

extern "C" {

int mused_adj_fuse_table(const unsigned long long* const* masks, int M, const unsigned long long* table, int n, int words,
                         unsigned long long* out, void* stream) {
  MUSED_REQUIRE(masks && table && out, "mused_adj_fuse_table: null pointer");
  MUSED_REQUIRE(M >= 1 && M <= FUSE_TABLE_MAX_M, "mused_adj_fuse_table: M = %d modalities outside 1 .. %d", M, FUSE_TABLE_MAX_M);
  MUSED_REQUIRE(n > 0 && words >= (n + 63) / 64, "mused_adj_fuse_table: bad sizes n=%d words=%d (words >= ceil(n/64))", n, words);
  MUSED_REQUIRE(!(table[0] & 1ull), "mused_adj_fuse_table: table bit 0 is set (no modality, no edge)");
  for (int s = 1 << M; s < 256; ++s)
    MUSED_REQUIRE(!((table[s >> 6] >> (s & 63)) & 1ull), "mused_adj_fuse_table: table bit %d is set, at or above 2^M = %d", s, 1 << M);
  FuseTableArgs a;
  memset(&a, 0, sizeof(a));
  const long words_total = (long)n * words;
  bool pair = (words_total % 2 == 0) && ((uintptr_t)out % 16 == 0);
  for (int m = 0; m < M; ++m) {
    MUSED_REQUIRE(masks[m], "mused_adj_fuse_table: mask %d is null", m);
    a.p[m] = masks[m];
    pair = pair && ((uintptr_t)masks[m] % 16 == 0);
  }
  for (int q = 0; q < 4; ++q) a.t[q] = table[q];
  hipStream_t st = (hipStream_t)stream;
  switch (M) {
    case 1: return adj_fuse_table_launch<1>(a, words_total, pair, out, st);
    case 2: return adj_fuse_table_launch<2>(a, words_total, pair, out, st);
    case 3: return adj_fuse_table_launch<3>(a, words_total, pair, out, st);
    case 4: return adj_fuse_table_launch<4>(a, words_total, pair, out, st);
    case 5: return adj_fuse_table_launch<5>(a, words_total, pair, out, st);
    case 6: return adj_fuse_table_launch<6>(a, words_total, pair, out, st);
    case 7: return adj_fuse_table_launch<7>(a, words_total, pair, out, st);
    default: return adj_fuse_table_launch<8>(a, words_total, pair, out, st);
  }
}

int mused_adj_fuse_threshold(const unsigned long long* const* masks, const double* weights, int M, double tau, int n,
                             int words, unsigned long long* out, void* stream) {
  unsigned long long table[4];
  int rc;
  if ((rc = fuse_threshold_table(weights, M, tau, table, "mused_adj_fuse_threshold"))) return rc;
  return mused_adj_fuse_table(masks, M, table, n, words, out, stream);
}

}  // extern "C"
