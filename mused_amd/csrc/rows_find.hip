// Rows looked up by value: the position of each of q query rows among n held rows of d fp64 each, or -1 -- the rule of
// mused_amd/rows_find.py.  Two rows are equal when all d doubles have the same bits (-0.0 is not +0.0; a NaN row finds a row
// with the same NaN bits).  A value held at positions h1 < h2 < ... and asked for at query positions q1 < q2 < ...: query q_k
// gets h_k, and -1 beyond the last held occurrence.  The output depends on nothing but the values: two runs agree.
//
//   rf_insert   the n + q rows (element e < n: held row e; e >= n: query e - n) go into one open-addressing table of
//               2 (n + q) + 1 slots keyed by their bytes.  The hash only places a row, the d words identify it: the slot
//               that holds an equal row (or the free slot the row claims with a compare-and-swap) is the row's GROUP.  Which
//               slot a value ends in depends on the order of the claims; the groups do not
//   sort        a stable LSD radix sort of the elements by group, 8 bits a pass (radix_sort.h).  The elements start in the
//               order (held by position, queries by position) and the sort is stable: inside a group the held positions
//               ascend, then the query positions ascend
//   rf_heads    per group the sorted index of its first element and of its first query
//   rf_assign   the k-th query of a group takes the k-th held element of it
//
// O(n + q) workspace, no pass over the values on the host, enqueue-only.  Every write to global memory is a vector store or
// a device-scope vector atomic.
#include "internal.h"
#include "radix_sort.h"

namespace mused {

constexpr long RF_MAX_ELEMS = 1l << 24;

struct RfRows {
  const unsigned long long *X, *Q;  // the rows as their bits
  long ld, ldq;
  int n, total, d;                  // total = n + q
};

__device__ __forceinline__ const unsigned long long* rf_row(const RfRows& a, int e) {
  return e < a.n ? a.X + (long)e * a.ld : a.Q + (long)(e - a.n) * a.ldq;
}

__global__ __launch_bounds__(256) void rf_insert_kernel(RfRows a, int* __restrict__ table, int slots, int* __restrict__ grp) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const unsigned long long* row = rf_row(a, e);
  unsigned h = 2166136261u;  // FNV-1a over the 32-bit halves, then a finaliser
  for (int k = 0; k < a.d; ++k) {
    const unsigned long long v = row[k];
    h = (h ^ (unsigned)v) * 16777619u;
    h = (h ^ (unsigned)(v >> 32)) * 16777619u;
  }
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  int slot = (int)(h % (unsigned)slots);
  for (int probe = 0; probe < slots; ++probe) {   // (slots > total: a free slot is always met)
    const int old = atomicCAS(&table[slot], -1, e);
    bool same = old == -1;
    if (!same) {
      const unsigned long long* other = rf_row(a, old);
      same = true;
      for (int k = 0; k < a.d && same; ++k) same = other[k] == row[k];
    }
    if (same) {
      grp[e] = slot;
      return;
    }
    slot = slot + 1 == slots ? 0 : slot + 1;
  }
}

// sorted by group: first[g] = the sorted index of the group's first element, firstq[g] = of its first query
__global__ __launch_bounds__(256) void rf_heads_kernel(const int* __restrict__ key, const int* __restrict__ val, int n, int total,
                                                      int* __restrict__ first, int* __restrict__ firstq) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int g = key[t];
  const bool head = t == 0 || key[t - 1] != g;
  if (head) first[g] = t;
  if (val[t] >= n && (head || val[t - 1] < n)) firstq[g] = t;
}

__global__ __launch_bounds__(256) void rf_assign_kernel(const int* __restrict__ key, const int* __restrict__ val, int n, int total,
                                                       const int* __restrict__ first, const int* __restrict__ firstq,
                                                       int* __restrict__ idx_out, int* __restrict__ info) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  bool query = false, found = false;
  if (t < total) {
    const int e = val[t];
    query = e >= n;
    if (query) {
      const int g = key[t];
      const int s = first[g], fq = firstq[g];
      const int k = t - fq;            // this query's rank among the group's queries
      found = k < fq - s;              // fq - s held rows in the group
      idx_out[e - n] = found ? val[s + k] : -1;
    }
  }
  const int nf = __popcll(__ballot(found)), nq = __popcll(__ballot(query));
  if ((threadIdx.x & 63) == 0) {
    if (nf) atomicAdd(info, nf);
    if (nq - nf) atomicAdd(info + 1, nq - nf);
  }
}

struct RfWs {
  int *table, *key[2], *val[2], *hist, *first, *firstq;
};

static long rf_slots(long total) { return 2 * total + 1; }

static size_t rf_layout(long total, char* base, RfWs* ws) {
  RfWs sizing;
  RfWs& w = ws ? *ws : sizing;
  WsCarver c{base};
  const long slots = rf_slots(total), nb = (total + RADIX_TILE - 1) / RADIX_TILE;
  w.table = c.take<int>(slots);
  w.first = c.take<int>(slots);
  w.firstq = c.take<int>(slots);
  for (int i = 0; i < 2; ++i) {
    w.key[i] = c.take<int>(total);
    w.val[i] = c.take<int>(total);
  }
  w.hist = c.take<int>(256 * (size_t)nb);
  return c.off;
}

static bool rf_shape_ok(long n, long q, int d) { return n >= 0 && q >= 0 && n + q <= RF_MAX_ELEMS && d >= 1 && d < (1 << 20); }

}  // namespace mused

using namespace mused;

extern "C" {

// bytes of workspace mused_rows_find needs (-1: n or q negative, n + q beyond 2^24, a bad d)
long mused_rows_find_ws_bytes(long n, long q, int d) {
  if (!rf_shape_ok(n, q, d)) return -1;
  return (long)rf_layout(n + q > 0 ? n + q : 1, nullptr, nullptr);
}

// idx_out[k] (DEVICE, q int32) = the position of query row k among the n held rows, or -1 (head of this file); info_out
// (DEVICE, 4 int32) = {found, not found, 0, 0}.  X: n x d fp64 (pitch ld), Q: q x d fp64 (pitch ldq).  Enqueue-only.
int mused_rows_find(const double* X, long ld, long n, const double* Q, long ldq, long q, int d, int* idx_out, int* info_out,
                    void* ws, long ws_bytes, void* stream) {
  MUSED_REQUIRE(info_out && ws && (X || n == 0) && ((Q && idx_out) || q == 0), "mused_rows_find: null argument");
  MUSED_REQUIRE(rf_shape_ok(n, q, d) && ld >= d && ldq >= d,
                "mused_rows_find: bad shape (n=%ld q=%ld d=%d ld=%ld ldq=%ld; n + q <= 2^24)", n, q, d, ld, ldq);
  const long total = n + q;
  MUSED_REQUIRE(ws_bytes >= (long)rf_layout(total > 0 ? total : 1, nullptr, nullptr), "mused_rows_find: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  MUSED_CHECK_HIP(hipMemsetAsync(info_out, 0, 16, st));
  if (q == 0) return MUSED_OK;
  RfWs k;
  rf_layout(total, (char*)ws, &k);
  const long slots = rf_slots(total);
  RfRows a{reinterpret_cast<const unsigned long long*>(X), reinterpret_cast<const unsigned long long*>(Q), ld, ldq, (int)n, (int)total, d};
  const dim3 elems(cdiv(total, 256)), blk(256);
  MUSED_CHECK_HIP(hipMemsetAsync(k.table, 0xff, 4 * (size_t)slots, st));   // -1: a free slot
  hipLaunchKernelGGL(rf_insert_kernel, elems, blk, 0, st, a, k.table, (int)slots, k.key[0]);
  int cur = 0;
  for (int shift = 0; shift < 32 && ((slots - 1) >> shift) != 0; shift += 8) {
    const int rc = radix_sort_pass(k.key[cur], shift ? k.val[cur] : nullptr, (int)total, RadixCount{(int)total, nullptr}, shift,
                                   k.hist, k.key[cur ^ 1], k.val[cur ^ 1], nullptr, nullptr, st);
    if (rc) return rc;
    cur ^= 1;
  }
  hipLaunchKernelGGL(rf_heads_kernel, elems, blk, 0, st, k.key[cur], k.val[cur], (int)n, (int)total, k.first, k.firstq);
  hipLaunchKernelGGL(rf_assign_kernel, elems, blk, 0, st, k.key[cur], k.val[cur], (int)n, (int)total, k.first, k.firstq, idx_out,
                     info_out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
