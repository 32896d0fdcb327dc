// Rows looked up by value: the position of each of q query rows among n held rows of d fp64 each, or -1 -- the rule of
// mused_amd/rows_find.py.  Two rows are equal when all d doubles have the same bits (-0.0 is not +0.0; a NaN row finds a row
// with the same NaN bits).  A value held at positions h1 < h2 < ... and asked for at query positions q1 < q2 < ...: query q_k
// gets h_k, and -1 beyond the last held occurrence.  The output depends on nothing but the values: two runs agree.
//
//   rf_insert   the n + q rows (element e < n: held row e; e >= n: query e - n) go into one open-addressing table of
//               2 (n + q) + 1 slots keyed by their bytes.  The hash only places a row, the d words identify it: the slot
//               that holds an equal row (or the free slot the row claims with a compare-and-swap) is the row's GROUP.  Which
//               slot a value ends in depends on the order of the claims; the groups do not
//   rf_hist, rf_scatter   a stable LSD radix sort of the elements by group, 8 bits a pass (the sort of csrc/tokenise.hip: a
//               histogram per tile of 1024 elements, one scan (block_scan.h), ranks by wave ballots).  The elements start
//               in the order (held by position, queries by position) and the sort is stable: inside a group the held
//               positions ascend, then the query positions ascend
//   rf_heads    per group the sorted index of its first element and of its first query
//   rf_assign   the k-th query of a group takes the k-th held element of it
//
// O(n + q) workspace, no pass over the values on the host, enqueue-only.  Every write to global memory is a vector store or
// a device-scope vector atomic.
#include "internal.h"
#include "block_scan.h"

namespace mused {

constexpr int RF_TILE = 1024;          // elements per wave of the radix passes
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

__device__ __forceinline__ int rf_digit(int key, int shift) { return (key >> shift) & 255; }

// hist[digit * nb + tile] <- elements of the tile with that digit
__global__ __launch_bounds__(64) void rf_hist_kernel(const int* __restrict__ key, int total, int shift, int* __restrict__ hist, int nb) {
  __shared__ int c[256];
  const int lane = threadIdx.x;
  for (int j = lane; j < 256; j += 64) c[j] = 0;
  __syncthreads();
  const long t0 = (long)blockIdx.x * RF_TILE;
  for (int q = 0; q < RF_TILE; q += 64) {
    const long i = t0 + q + lane;
    if (i < total) atomicAdd(&c[rf_digit(key[i], shift)], 1);
  }
  __syncthreads();
  for (int j = lane; j < 256; j += 64) hist[(long)j * nb + blockIdx.x] = c[j];
}

// hist scanned (digit-major): element i of tile b goes to hist[digit][b] + its rank among the tile's earlier elements of the
// digit.  val == nullptr: the element is its own index (the first pass)
__global__ __launch_bounds__(64) void rf_scatter_kernel(const int* __restrict__ key, const int* __restrict__ val, int total, int shift,
                                                       const int* __restrict__ hist, int nb, int* __restrict__ key_out,
                                                       int* __restrict__ val_out) {
  __shared__ int run[256];
  const int lane = threadIdx.x;
  for (int j = lane; j < 256; j += 64) run[j] = hist[(long)j * nb + blockIdx.x];
  __syncthreads();
  const long t0 = (long)blockIdx.x * RF_TILE;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int q = 0; q < RF_TILE; q += 64) {
    const long i = t0 + q + lane;
    const bool live = i < total;
    const int k = live ? key[i] : 0;
    const int dg = rf_digit(k, shift);
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (dg >> bit) & 1;
      const unsigned long long m = __ballot(live && on);
      peers &= on ? m : ~m;
    }
    const int ahead = __popcll(peers & below);
    const int p = live ? run[dg] + ahead : 0;
    __syncthreads();
    if (live && ahead == 0) run[dg] += __popcll(peers);  // one lane per digit present in the chunk
    __syncthreads();
    if (live && (unsigned)p < (unsigned)total) {
      key_out[p] = k;
      val_out[p] = val ? val[i] : (int)i;
    }
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
  const long slots = rf_slots(total), nb = (total + RF_TILE - 1) / RF_TILE;
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
  const int nb = (int)cdiv(total, RF_TILE);
  RfRows a{reinterpret_cast<const unsigned long long*>(X), reinterpret_cast<const unsigned long long*>(Q), ld, ldq, (int)n, (int)total, d};
  const dim3 elems(cdiv(total, 256)), blk(256);
  MUSED_CHECK_HIP(hipMemsetAsync(k.table, 0xff, 4 * (size_t)slots, st));   // -1: a free slot
  hipLaunchKernelGGL(rf_insert_kernel, elems, blk, 0, st, a, k.table, (int)slots, k.key[0]);
  int cur = 0;
  for (int shift = 0; shift < 32 && ((slots - 1) >> shift) != 0; shift += 8) {
    hipLaunchKernelGGL(rf_hist_kernel, dim3(nb), dim3(64), 0, st, k.key[cur], (int)total, shift, k.hist, nb);
    hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, st, k.hist, 256 * nb);
    hipLaunchKernelGGL(rf_scatter_kernel, dim3(nb), dim3(64), 0, st, k.key[cur], shift ? k.val[cur] : (const int*)nullptr, (int)total,
                       shift, k.hist, nb, k.key[cur ^ 1], k.val[cur ^ 1]);
    cur ^= 1;
  }
  hipLaunchKernelGGL(rf_heads_kernel, elems, blk, 0, st, k.key[cur], k.val[cur], (int)n, (int)total, k.first, k.firstq);
  hipLaunchKernelGGL(rf_assign_kernel, elems, blk, 0, st, k.key[cur], k.val[cur], (int)n, (int)total, k.first, k.firstq, idx_out,
                     info_out);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // extern "C"
