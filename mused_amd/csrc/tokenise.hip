// The one tokenised pass of the "text" modality (mused_amd/text.py: TextCorpus) from the bytes of the corpus: scikit-learn's
// default analyser on ASCII text is a rule on bytes -- lower-case 'A'..'Z', every maximal run of [0-9A-Za-z_] of length >= 2
// is a token -- and Python's str order on such tokens is byte order.  The rule, statement by statement: mused_amd/tokens.py.
//
// The corpus is one buffer: the strings of the D valid rows, each followed by one separator byte that is no word byte;
// document d is buf[docptr[d], docptr[d + 1]), so no run crosses a document.  Two calls, because the alphabetical order
// of the V distinct tokens is made on the host between them (sorted() over V strings, the order of `_sort_features`):
//
//   mused_tokenise_scan
//     scan     (count, block scan, write) classify and lower-case 16 bytes per thread, mark the start of every run of
//              length >= 2, count per block of 4096 bytes, exclusive scan of the block counts, then write tok_start / tok_len
//              in TEXT ORDER (the order comes from the scan, not from atomics; a run may cross a block's byte range: the
//              thread that owns its start walks to its end).  The document of a token is never stored: tok_start
//              ascends, so the tokens of document d are the slice between two binary searches of docptr[d], docptr[d + 1].
//     docs     one thread per document: its token count -> the longest document (info[3]) and the flag for one beyond the cap
//     insert   one thread per token into an open-addressing table of token indices keyed by the token's bytes: atomicCAS
//              on the slot, linear probing; identity is decided by comparing ALL bytes of the two tokens.  A slot is read only
//              through the return value of the atomic (a plain load of a slot is not seen across XCDs within a launch).
//              Once filled a slot keeps a token of the same bytes; WHICH equal token represents the group, and which
//              slot a group ends up in, is arbitrary and nothing downstream depends on it.
//     compact  (count, block scan, write) occupied slots -> provisional ids 0 .. V - 1 (slot order), voc_start / voc_len,
//              and the slot now holds the id
//   host: reads info, then the V spans; sorts; uploads rank[V] (provisional id -> rank in the sorted vocabulary)
//   mused_tokenise_build
//     rows     one workgroup per document, twice (count, then write, with the exclusive scan of the counts = rowptr in
//              between): (term << 32 | position) of its tokens to LDS, bitonic sort; equal terms collapse to one entry: cnt =
//              run length, first position = the run's smallest; pos = rank of the first position among the entries
//              (a second sort, of first position << 16 | entry)
//     postings stable LSD radix sort of the entries by term, 8 bits a pass (radix_sort.h; the last pass also gathers the
//              entries' rows): entries are row-major, so rows ascend inside a term.  gpostptr[t] = first sorted entry >= t.
// No float anywhere and no result that depends on arrival order: two calls on the same input give identical bytes.
//
// Text that is not pure ASCII takes the same steps on CODE POINTS (mused_tokenise_cp_scan / _cp_build; the rule:
// mused_amd/tokens.py, "code points").  The corpus is one uint32 per code point, and the caller hands in a class table
// of one uint32 per code point -- lowered code point in the low 21 bits, TK_CP_WORD, TK_CP_END -- so no Unicode version
// is compiled in.  Two kernels are siblings of the byte ones, everything from `docs` onward is shared:
//     scan     8 code points per thread (two 16-byte loads), 2048 per workgroup; the count pass writes the table entry of
//              every element to `low` (below 128 the ALU rule of the byte path, which the table's first 128 entries
//              equal), so the write pass, the run walk and the insert kernel read flags and lowered code points from
//              `low` and never the table.  A token starts at a word element whose predecessor is no word element or
//              ends the run (U+0130: a word code point that lower-cases to 'i' and a combining dot, which is no word
//              code point), that does not end the run itself and has a word element behind it; its owner walks on
//              while the current element does not end the run and the next one is a word element.
//     insert   hashes and compares the 21-bit lowered code points of the two tokens, flags masked off
// Two tokens may touch ("aİbİ" holds "ai" and "bi"), so a buffer of n code points holds up to n / 2 tokens.
#include "common.h"
#include "internal.h"
#include "radix_sort.h"

namespace mused {

constexpr int TK_MAX_DOC_TOKENS = 8192;  // keys (8 B), second keys (4 B), run heads (4 B) of one document in LDS: 128 KiB + 80 B
constexpr int TK_SCAN_THREADS = 256;
constexpr int TK_SCAN_TILE = TK_SCAN_THREADS * 16;  // bytes per workgroup of the scan
constexpr int TK_FLAG_DOC = 1;       // a document holds more tokens than the caller's cap
constexpr int TK_FLAG_TABLE = 2;     // more tokens than table slots: nothing was inserted
constexpr int TK_FLAG_STATE = 4;     // the workspace is not what mused_tokenise_scan left (ids or slices out of range)
constexpr unsigned char TK_BLANK = ' ';

__device__ __forceinline__ bool tk_is_word(unsigned c) {
  return (c - '0' < 10u) | ((c | 32u) - 'a' < 26u) | (c == '_');
}
__device__ __forceinline__ unsigned char tk_lower(unsigned c) { return (unsigned char)(c - 'A' < 26u ? c + 32u : c); }

// WRITE = false: lower-cased bytes -> low, token starts per block -> blk[block]
// WRITE = true:  blk holds the exclusive scan of those counts; tok_start / tok_len in text order (reads `low`)
template <bool WRITE>
__global__ __launch_bounds__(TK_SCAN_THREADS) void tk_scan_kernel(const unsigned char* __restrict__ src, long n,
                                                                 unsigned char* __restrict__ low, int* __restrict__ blk,
                                                                 int* __restrict__ tok_start, int* __restrict__ tok_len,
                                                                 int tok_cap) {
  __shared__ int ws[16];
  const long base = (long)blockIdx.x * TK_SCAN_TILE + threadIdx.x * 16;
  unsigned char b[18];  // the byte before, 16 bytes, the byte behind
  if (base + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(src + base);
    const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j + 1] = (unsigned char)(q[j >> 2] >> (8 * (j & 3)));
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j + 1] = base + j < n ? src[base + j] : TK_BLANK;
  }
  b[0] = (base > 0 && base - 1 < n) ? src[base - 1] : TK_BLANK;
  b[17] = base + 16 < n ? src[base + 16] : TK_BLANK;
  unsigned wbits = 0;
#pragma unroll
  for (int j = 0; j < 18; ++j) wbits |= tk_is_word(b[j]) ? (1u << j) : 0u;
  // bit j of starts: byte base + j is a word byte behind a non-word byte and in front of a word byte
  const unsigned starts = ((wbits >> 1) & ~wbits & (wbits >> 2)) & 0xffffu;
  const int mine = __popc(starts);
  if (!WRITE) {
    if (base + 16 <= n) {
      unsigned q[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 16; ++j) q[j >> 2] |= (unsigned)tk_lower(b[j + 1]) << (8 * (j & 3));
      *reinterpret_cast<uint4*>(low + base) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (base + j < n) low[base + j] = tk_lower(b[j + 1]);
    }
  }
  int total;
  const int before = block_excl_scan(mine, ws, total);
  if (!WRITE) {
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
    return;
  }
  int o = blk[blockIdx.x] + before;
  unsigned s = starts;
  while (s) {
    const int j = __ffs(s) - 1;
    s &= s - 1;
    long e = base + j + 2;  // the run holds bytes base + j and base + j + 1
    while (e < n && tk_is_word(low[e])) ++e;
    if (o < tok_cap) {
      tok_start[o] = (int)(base + j);
      tok_len[o] = (int)(e - (base + j));
    }
    ++o;
  }
}

__global__ __launch_bounds__(256) void tk_docs_kernel(const int* __restrict__ docptr, int n_docs, const int* __restrict__ tok_start,
                                                     int max_doc_tokens, int* __restrict__ info) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  const int T = info[0];
  int nt = 0;
  if (d < n_docs) nt = lower_bound(tok_start, 0, T, docptr[d + 1]) - lower_bound(tok_start, 0, T, docptr[d]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nt = max(nt, __shfl_xor(nt, o));
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&info[3], nt);
    if (nt > max_doc_tokens) atomicOr(&info[2], TK_FLAG_DOC);
  }
}

__device__ __forceinline__ bool tk_same_bytes(const unsigned char* __restrict__ low, int s0, int s1, int len) {
  for (int i = 0; i < len; ++i)
    if (low[s0 + i] != low[s1 + i]) return false;
  return true;
}

__global__ __launch_bounds__(256) void tk_insert_kernel(const unsigned char* __restrict__ low, const int* __restrict__ tok_start,
                                                       const int* __restrict__ tok_len, int* __restrict__ table, int slots,
                                                       int* __restrict__ tok_slot, int* __restrict__ info) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int T = info[0];
  if (T > slots) {  // a table that cannot hold every token distinct: the probe loop would not end
    if (t == 0) atomicOr(&info[2], TK_FLAG_TABLE);
    return;
  }
  if (t >= T) return;
  const int s = tok_start[t], len = tok_len[t];
  unsigned h = 2166136261u;  // FNV-1a, then a finaliser: the hash only places the token, the bytes identify it
  for (int i = 0; i < len; ++i) h = (h ^ low[s + i]) * 16777619u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  int slot = (int)(h % (unsigned)slots);
  for (int probe = 0; probe < slots; ++probe) {
    const int old = atomicCAS(&table[slot], -1, t);
    if (old == -1 || (tok_len[old] == len && tk_same_bytes(low, tok_start[old], s, len))) {
      tok_slot[t] = slot;
      return;
    }
    slot = slot + 1 == slots ? 0 : slot + 1;
  }
}

// ---- code points: one uint32 an element; an element of `low` is its class-table entry ----
constexpr int TK_CP_PER_THREAD = 8;
constexpr int TK_CP_TILE = TK_SCAN_THREADS * TK_CP_PER_THREAD;  // code points per workgroup of the scan
constexpr unsigned TK_CP_MASK = 0x1fffffu;  // the lowered code point
constexpr unsigned TK_CP_WORD = 1u << 21;
constexpr unsigned TK_CP_END = 1u << 22;    // a word code point behind which the run ends
constexpr long TK_CP_TABLE_MAX = 0x110000;

__device__ __forceinline__ unsigned tk_cp_entry(unsigned c, const unsigned* __restrict__ cls, unsigned n_cls) {
  if (c < 128u) return (unsigned)tk_lower(c) | (tk_is_word(c) ? TK_CP_WORD : 0u);
  return c < n_cls ? cls[c] : (unsigned)TK_BLANK;  // beyond the table: no word code point
}

// WRITE = false: src = code points; table entries -> low, token starts per block -> blk[block]
// WRITE = true:  src = low; blk holds the exclusive scan of those counts; tok_start / tok_len in text order
template <bool WRITE>
__global__ __launch_bounds__(TK_SCAN_THREADS) void tk_cp_scan_kernel(const unsigned* __restrict__ src, long n,
                                                                    const unsigned* __restrict__ cls, unsigned n_cls,
                                                                    unsigned* __restrict__ low, int* __restrict__ blk,
                                                                    int* __restrict__ tok_start, int* __restrict__ tok_len,
                                                                    int tok_cap) {
  __shared__ int ws[16];
  constexpr int P = TK_CP_PER_THREAD;
  const long base = (long)blockIdx.x * TK_CP_TILE + threadIdx.x * P;
  const unsigned blank = TK_BLANK;  // as a code point and as a table entry: no word element
  unsigned e[P + 2];                // the element before, P elements, the element behind
  if (base + P <= n) {
#pragma unroll
    for (int q = 0; q < P / 4; ++q) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + base + 4 * q);
      e[4 * q + 1] = v.x;
      e[4 * q + 2] = v.y;
      e[4 * q + 3] = v.z;
      e[4 * q + 4] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < P; ++j) e[j + 1] = base + j < n ? src[base + j] : blank;
  }
  e[0] = (base > 0 && base - 1 < n) ? src[base - 1] : blank;
  e[P + 1] = base + P < n ? src[base + P] : blank;
  if (!WRITE) {
#pragma unroll
    for (int j = 0; j < P + 2; ++j) e[j] = tk_cp_entry(e[j], cls, n_cls);
    if (base + P <= n) {
#pragma unroll
      for (int q = 0; q < P / 4; ++q)
        *reinterpret_cast<uint4*>(low + base + 4 * q) = make_uint4(e[4 * q + 1], e[4 * q + 2], e[4 * q + 3], e[4 * q + 4]);
    } else {
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (base + j < n) low[base + j] = e[j + 1];
    }
  }
  unsigned wbits = 0, cbits = 0;  // bit j: e[j] is a word element / is one and the run goes on behind it
#pragma unroll
  for (int j = 0; j < P + 2; ++j) {
    wbits |= (e[j] & TK_CP_WORD) ? (1u << j) : 0u;
    cbits |= (e[j] & (TK_CP_WORD | TK_CP_END)) == TK_CP_WORD ? (1u << j) : 0u;
  }
  // bit j of starts: element base + j goes on, the one before it does not, the one behind it is a word element
  const unsigned starts = ((cbits >> 1) & ~cbits & (wbits >> 2)) & ((1u << P) - 1u);
  const int mine = __popc(starts);
  int total;
  const int before = block_excl_scan(mine, ws, total);
  if (!WRITE) {
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
    return;
  }
  int o = blk[blockIdx.x] + before;
  unsigned s = starts;
  while (s) {
    const int j = __ffs(s) - 1;
    s &= s - 1;
    long last = base + j + 1;  // the run holds elements base + j and base + j + 1
    while (!(src[last] & TK_CP_END) && last + 1 < n && (src[last + 1] & TK_CP_WORD)) ++last;
    if (o < tok_cap) {
      tok_start[o] = (int)(base + j);
      tok_len[o] = (int)(last + 1 - (base + j));
    }
    ++o;
  }
}

__device__ __forceinline__ bool tk_cp_same(const unsigned* __restrict__ low, int s0, int s1, int len) {
  for (int i = 0; i < len; ++i)
    if ((low[s0 + i] ^ low[s1 + i]) & TK_CP_MASK) return false;
  return true;
}

// tk_insert_kernel on code points: identity is the sequence of ALL 21 bits of the lowered code points
__global__ __launch_bounds__(256) void tk_cp_insert_kernel(const unsigned* __restrict__ low, const int* __restrict__ tok_start,
                                                          const int* __restrict__ tok_len, int* __restrict__ table, int slots,
                                                          int* __restrict__ tok_slot, int* __restrict__ info) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int T = info[0];
  if (T > slots) {  // a table that cannot hold every token distinct: the probe loop would not end
    if (t == 0) atomicOr(&info[2], TK_FLAG_TABLE);
    return;
  }
  if (t >= T) return;
  const int s = tok_start[t], len = tok_len[t];
  unsigned h = 2166136261u;  // FNV-1a over whole code points, then a finaliser
  for (int i = 0; i < len; ++i) h = (h ^ (low[s + i] & TK_CP_MASK)) * 16777619u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  int slot = (int)(h % (unsigned)slots);
  for (int probe = 0; probe < slots; ++probe) {
    const int old = atomicCAS(&table[slot], -1, t);
    if (old == -1 || (tok_len[old] == len && tk_cp_same(low, tok_start[old], s, len))) {
      tok_slot[t] = slot;
      return;
    }
    slot = slot + 1 == slots ? 0 : slot + 1;
  }
}

// WRITE = false: occupied slots per block -> blk[block];  WRITE = true: blk scanned; slot -> provisional id, spans written
template <bool WRITE>
__global__ __launch_bounds__(256) void tk_compact_kernel(int* __restrict__ table, int slots, int* __restrict__ blk,
                                                        const int* __restrict__ tok_start, const int* __restrict__ tok_len,
                                                        int* __restrict__ voc_start, int* __restrict__ voc_len, int voc_cap) {
  __shared__ int ws[16];
  const long slot = (long)blockIdx.x * 256 + threadIdx.x;
  const int t = slot < slots ? table[slot] : -1;
  int total;
  const int before = block_excl_scan(t >= 0 ? 1 : 0, ws, total);
  if (!WRITE) {
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
    return;
  }
  if (t >= 0) {
    const int id = blk[blockIdx.x] + before;
    if (id < voc_cap) {
      voc_start[id] = tok_start[t];
      voc_len[id] = tok_len[t];
    }
    table[slot] = id;
  }
}

template <class K>
__device__ __forceinline__ void tk_bitonic(K* a, int n) {
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = threadIdx.x; p < (n >> 1); p += blockDim.x) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const K x = a[i], y = a[i | j];
        if ((x > y) == ((i & k) == 0)) {
          a[i] = y;
          a[i | j] = x;
        }
      }
      __syncthreads();
    }
}

struct TkRows {
  const int *docptr, *tok_start, *tok_slot, *table, *rank, *vrow;
  int n_docs, T, V, slots, n;  // n: power of two >= the longest document's token count
};

// WRITE = false: rowcnt[d] <- distinct terms of document d.  WRITE = true: rowptr scanned; term / cnt / pos / ent_row written
template <bool WRITE>
__global__ __launch_bounds__(256) void tk_rows_kernel(TkRows a, int* __restrict__ rowcnt, const int* __restrict__ rowptr,
                                                     int* __restrict__ term, int* __restrict__ cnt, int* __restrict__ pos,
                                                     int* __restrict__ ent_row, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long tk_smem[];
  const int n = a.n, d = blockIdx.x, tid = threadIdx.x, bd = blockDim.x;
  unsigned long long* keys = tk_smem;                      // [n]
  unsigned* k2 = reinterpret_cast<unsigned*>(keys + n);    // [n]
  int* ws = reinterpret_cast<int*>(k2 + n);                // [16]
  int* hidx = ws + 16;                                     // [n + 1]
  const int t0 = lower_bound(a.tok_start, 0, a.T, a.docptr[d]);
  const int nt = lower_bound(a.tok_start, 0, a.T, a.docptr[d + 1]) - t0;
  if (nt < 0 || nt > n) {  // uniform over the workgroup
    if (tid == 0) {
      atomicOr(&info[2], TK_FLAG_STATE);
      if (!WRITE) rowcnt[d] = 0;
    }
    return;
  }
  bool bad = false;
  for (int i = tid; i < n; i += bd) {
    unsigned long long k = ~0ull;
    if (i < nt) {
      const int slot = a.tok_slot[t0 + i];
      int id = (unsigned)slot < (unsigned)a.slots ? a.table[slot] : -1;
      int r = (unsigned)id < (unsigned)a.V ? a.rank[id] : -1;
      if ((unsigned)r >= (unsigned)a.V) {
        bad = true;
        r = 0;
      }
      k = ((unsigned long long)(unsigned)r << 32) | (unsigned)i;
    }
    keys[i] = k;
  }
  if (bad) atomicOr(&info[2], TK_FLAG_STATE);
  tk_bitonic(keys, n);
  int L = 0;
  for (int base = 0; base < n; base += bd) {
    const int i = base + tid;
    const bool head = i < nt && (i == 0 || (unsigned)(keys[i] >> 32) != (unsigned)(keys[i - 1] >> 32));
    int tot;
    const int e = L + block_excl_scan(head ? 1 : 0, ws, tot);
    if (head) hidx[e] = i;
    L += tot;
  }
  if (!WRITE) {
    if (tid == 0) rowcnt[d] = L;
    return;
  }
  if (tid == 0) hidx[L] = nt;
  __syncthreads();
  const int o0 = rowptr[d];
  const int row = a.vrow[d];
  for (int e = tid; e < n; e += bd) {
    unsigned q = ~0u;
    if (e < L) {
      const int i = hidx[e];
      const unsigned long long k = keys[i];
      term[o0 + e] = (int)(k >> 32);
      cnt[o0 + e] = hidx[e + 1] - i;
      ent_row[o0 + e] = row;
      q = ((unsigned)k << 16) | (unsigned)e;  // first position and entry, both < 2^13
    }
    k2[e] = q;
  }
  tk_bitonic(k2, n);
  for (int r = tid; r < L; r += bd) pos[o0 + (k2[r] & 0xffffu)] = r;
}

__global__ __launch_bounds__(256) void tk_postptr_kernel(const int* __restrict__ sorted_key, const int* __restrict__ nnz_p, int V,
                                                        int* __restrict__ gpostptr) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t <= V) gpostptr[t] = lower_bound(sorted_key, 0, *nnz_p, t);
}

// the workspace both calls carve alike: the build reads what the scan left
struct TkWs {
  long tok_cap, nb_scan, nb_tab, bytes;
  unsigned char* low;  // bytes: the lower-cased text ...
  unsigned* low_cp;    // ... code points: the class-table entries
  int *docptr, *blk, *tok_start, *tok_len, *tok_slot, *table, *blk2, *ent_row, *key[2], *val[2], *hist;
};

static long tk_default_slots(long n_bytes) { return 2 * (n_bytes / 3 + 1); }

// n elements (code points if `cp`, else bytes), at most tok_cap tokens, `tile` elements per workgroup of the scan.  A null
// base only sizes
static TkWs tk_layout_of(long n, long n_docs, long slots, bool cp, long tok_cap, long tile, void* base) {
  TkWs l{};
  WsCarver c{static_cast<char*>(base)};
  l.tok_cap = tok_cap;
  l.nb_scan = (n + tile - 1) / tile;
  l.nb_tab = (slots + 255) / 256;
  if (cp) l.low_cp = c.take<unsigned>(n);
  else l.low = c.take<unsigned char>(n);
  l.docptr = c.take<int>(n_docs + 1);
  l.blk = c.take<int>(l.nb_scan);
  l.tok_start = c.take<int>(tok_cap);
  l.tok_len = c.take<int>(tok_cap);
  l.tok_slot = c.take<int>(tok_cap);
  l.table = c.take<int>(slots);
  l.blk2 = c.take<int>(l.nb_tab);
  l.ent_row = c.take<int>(tok_cap);
  for (int i = 0; i < 2; ++i) {
    l.key[i] = c.take<int>(tok_cap);
    l.val[i] = c.take<int>(tok_cap);
  }
  l.hist = c.take<int>(256 * (size_t)cdiv(tok_cap, RADIX_TILE));
  l.bytes = (long)c.off;
  return l;
}

// a token is two word bytes or more and a non-word byte (or the end of the buffer) behind them
static TkWs tk_layout(long n_bytes, long n_docs, long slots, void* base) {
  return tk_layout_of(n_bytes, n_docs, slots, false, n_bytes / 3 + 1, TK_SCAN_TILE, base);
}

// code points: two tokens may touch, so a token is two elements or more and nothing else
static long tk_cp_default_slots(long n_cp) { return 2 * (n_cp / 2 + 1); }
static TkWs tk_cp_layout(long n_cp, long n_docs, long slots, void* base) {
  return tk_layout_of(n_cp, n_docs, slots, true, n_cp / 2 + 1, TK_CP_TILE, base);
}
// below 2^30 code points every element offset, token count and block count is an int and the workspace stays below 2^36 bytes
static bool tk_cp_sizes_ok(long n_cp, long n_docs, long slots) {
  return n_cp >= 1 && n_cp < (1l << 30) && n_docs >= 1 && n_docs <= n_cp && slots >= 1 && slots < (1l << 31);
}

static bool tk_sizes_ok(long n_bytes, long n_docs, long slots) {
  return n_bytes >= 1 && n_bytes < (1l << 31) && n_docs >= 1 && n_docs <= n_bytes && slots >= 1 && slots < (1l << 31);
}

static size_t tk_rows_lds(int n) { return (size_t)(8l * n + 4l * n + 4 * 16 + 4l * (n + 1) + 15) / 16 * 16; }

// what follows the scan on either kind of element: docs, insert, compact (the vocabulary's spans and provisional ids)
static int tk_vocab_launch(const TkWs& l, long n_docs, long slots, int max_doc_tokens, int* voc_start, int* voc_len,
                           long voc_cap, int* info, hipStream_t st) {
  hipLaunchKernelGGL(tk_docs_kernel, dim3(cdiv(n_docs, 256)), dim3(256), 0, st, l.docptr, (int)n_docs, l.tok_start,
                     max_doc_tokens, info);
  MUSED_LAUNCH_CHECK();
  if (l.low_cp)
    hipLaunchKernelGGL(tk_cp_insert_kernel, dim3(cdiv(l.tok_cap, 256)), dim3(256), 0, st, l.low_cp, l.tok_start, l.tok_len,
                       l.table, (int)slots, l.tok_slot, info);
  else
    hipLaunchKernelGGL(tk_insert_kernel, dim3(cdiv(l.tok_cap, 256)), dim3(256), 0, st, l.low, l.tok_start, l.tok_len, l.table,
                       (int)slots, l.tok_slot, info);
  MUSED_LAUNCH_CHECK();
  const int cap = (int)(voc_cap < (1l << 31) ? voc_cap : (1l << 31) - 1);
  hipLaunchKernelGGL(tk_compact_kernel<false>, dim3((unsigned)l.nb_tab), dim3(256), 0, st, l.table, (int)slots, l.blk2,
                     l.tok_start, l.tok_len, voc_start, voc_len, cap);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, st, l.blk2, (int)l.nb_tab, info + 1);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tk_compact_kernel<true>, dim3((unsigned)l.nb_tab), dim3(256), 0, st, l.table, (int)slots, l.blk2,
                     l.tok_start, l.tok_len, voc_start, voc_len, cap);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// rows and postings: nothing here reads text, so bytes and code points share it
static int tk_build_launch(const TkWs& l, long n_docs, long slots, int n_tokens, int n_terms, int doc_tokens, const int* rank,
                           const int* vrow, int* doc_rowptr, int* term, int* cnt, int* pos, int* gpostptr, int* gpostrow,
                           int* gpostent, int* info, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  int n = 1;
  while (n < doc_tokens) n <<= 1;
  const size_t lds = tk_rows_lds(n);
  static LdsOptIn opt[2];
  const size_t most = tk_rows_lds(TK_MAX_DOC_TOKENS);
  hipError_t aerr = allow_dynamic_lds(opt[0], reinterpret_cast<const void*>(tk_rows_kernel<false>), most);
  aerr = allow_dynamic_lds(aerr, opt[1], reinterpret_cast<const void*>(tk_rows_kernel<true>), most);
  MUSED_CHECK_HIP(aerr);
  TkRows a{l.docptr, l.tok_start, l.tok_slot, l.table, rank, vrow, (int)n_docs, n_tokens, n_terms, (int)slots, n};
  const int threads = n / 2 < 64 ? 64 : (n / 2 > 256 ? 256 : n / 2);
  hipLaunchKernelGGL(tk_rows_kernel<false>, dim3((unsigned)n_docs), dim3(threads), lds, st, a, doc_rowptr, doc_rowptr, term, cnt,
                     pos, l.ent_row, info);
  MUSED_LAUNCH_CHECK();
  // doc_rowptr[n_docs] <- the sum: the scan's total lands where the exclusive scan of n_docs + 1 counts would put it
  hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, st, doc_rowptr, (int)n_docs, doc_rowptr + n_docs);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tk_rows_kernel<true>, dim3((unsigned)n_docs), dim3(threads), lds, st, a, doc_rowptr, doc_rowptr, term, cnt,
                     pos, l.ent_row, info);
  MUSED_LAUNCH_CHECK();
  const RadixCount nnz{0, doc_rowptr + n_docs};  // at most n_tokens: the grids cover that many
  int bits = 0;
  while (bits < 24 && (1 << bits) < n_terms) ++bits;
  const int passes = bits <= 8 ? 1 : (bits <= 16 ? 2 : 3);
  const int* kin = term;
  const int* vin = nullptr;
  for (int p = 0; p < passes; ++p) {
    const bool last = p == passes - 1;  // the last pass also gathers the entries' rows
    int* vout = last ? gpostent : l.val[p & 1];
    const int rc = radix_sort_pass(kin, vin, n_tokens, nnz, 8 * p, l.hist, l.key[p & 1], vout, last ? l.ent_row : nullptr,
                                   last ? gpostrow : nullptr, st);
    if (rc) return rc;
    kin = l.key[p & 1];
    vin = vout;
  }
  hipLaunchKernelGGL(tk_postptr_kernel, dim3(cdiv((long)n_terms + 1, 256)), dim3(256), 0, st, kin, nnz.ptr, n_terms, gpostptr);
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

}  // namespace mused

using namespace mused;

extern "C" {

long mused_tokenise_ws_bytes(long n_bytes, long n_docs, long table_slots) {
  const long slots = table_slots == 0 && n_bytes >= 1 ? tk_default_slots(n_bytes) : table_slots;
  return tk_sizes_ok(n_bytes, n_docs, slots) ? tk_layout(n_bytes, n_docs, slots, nullptr).bytes : -1;
}

int mused_tokenise_scan(const unsigned char* buf, long n_bytes, const int* docptr_host, long n_docs, long table_slots,
                        int max_doc_tokens, int* voc_start, int* voc_len, long voc_cap, int* info, void* ws, long ws_bytes,
                        void* stream) {
  const long slots = table_slots == 0 && n_bytes >= 1 ? tk_default_slots(n_bytes) : table_slots;
  MUSED_REQUIRE(tk_sizes_ok(n_bytes, n_docs, slots),
                "mused_tokenise_scan: bad sizes (bytes=%ld in [1, 2^31), docs=%ld in [1, bytes], table slots=%ld in [1, 2^31))",
                n_bytes, n_docs, table_slots);
  MUSED_REQUIRE(buf && docptr_host && voc_start && voc_len && info, "mused_tokenise_scan: an array is missing");
  MUSED_REQUIRE(((uintptr_t)buf & 15) == 0, "mused_tokenise_scan: the buffer must start on a 16-byte boundary");
  MUSED_REQUIRE(docptr_host[0] == 0 && docptr_host[n_docs] == n_bytes,
                "mused_tokenise_scan: docptr runs from %d to %d, not from 0 to the %ld bytes of the buffer", docptr_host[0],
                docptr_host[n_docs], n_bytes);
  for (long d = 0; d < n_docs; ++d)
    MUSED_REQUIRE(docptr_host[d + 1] > docptr_host[d], "mused_tokenise_scan: document %ld is empty or docptr descends (a document "
                  "holds at least its separator)", d);
  MUSED_REQUIRE(max_doc_tokens >= 1 && max_doc_tokens <= TK_MAX_DOC_TOKENS,
                "mused_tokenise_scan: max_doc_tokens=%d outside [1, %d] (one document is sorted in LDS)", max_doc_tokens,
                TK_MAX_DOC_TOKENS);
  const TkWs l = tk_layout(n_bytes, n_docs, slots, ws);
  MUSED_REQUIRE(voc_cap >= 1, "mused_tokenise_scan: voc_cap=%ld", voc_cap);
  MUSED_REQUIRE(ws && ws_bytes >= l.bytes && ((uintptr_t)ws & 15) == 0,
                "mused_tokenise_scan: workspace of %ld bytes, need %ld (16-byte aligned)", ws_bytes, l.bytes);
  hipStream_t st = (hipStream_t)stream;
  MUSED_CHECK_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int), st));
  MUSED_CHECK_HIP(hipMemsetAsync(l.table, 0xff, (size_t)slots * sizeof(int), st));
  MUSED_CHECK_HIP(hipMemcpyAsync(l.docptr, docptr_host, (size_t)(n_docs + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  const int cap = (int)l.tok_cap;
  hipLaunchKernelGGL(tk_scan_kernel<false>, dim3((unsigned)l.nb_scan), dim3(TK_SCAN_THREADS), 0, st, buf, n_bytes, l.low, l.blk,
                     l.tok_start, l.tok_len, cap);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, st, l.blk, (int)l.nb_scan, info + 0);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tk_scan_kernel<true>, dim3((unsigned)l.nb_scan), dim3(TK_SCAN_THREADS), 0, st, l.low, n_bytes, l.low, l.blk,
                     l.tok_start, l.tok_len, cap);
  MUSED_LAUNCH_CHECK();
  return tk_vocab_launch(l, n_docs, slots, max_doc_tokens, voc_start, voc_len, voc_cap, info, st);
}

int mused_tokenise_build(long n_bytes, long n_docs, long table_slots, int n_tokens, int n_terms, int doc_tokens,
                         const int* rank, const int* vrow, int* doc_rowptr, int* term, int* cnt, int* pos, int* gpostptr,
                         int* gpostrow, int* gpostent, int* info, void* ws, long ws_bytes, void* stream) {
  const long slots = table_slots == 0 && n_bytes >= 1 ? tk_default_slots(n_bytes) : table_slots;
  MUSED_REQUIRE(tk_sizes_ok(n_bytes, n_docs, slots),
                "mused_tokenise_build: bad sizes (bytes=%ld in [1, 2^31), docs=%ld in [1, bytes], table slots=%ld in [1, 2^31))",
                n_bytes, n_docs, table_slots);
  const TkWs l = tk_layout(n_bytes, n_docs, slots, ws);
  MUSED_REQUIRE(n_tokens >= 1 && n_tokens <= l.tok_cap && n_tokens <= slots && n_terms >= 1 && n_terms <= n_tokens &&
                    n_terms < (1 << 24),
                "mused_tokenise_build: %d tokens (at most %ld and the table's %ld slots), %d terms (at most 2^24 - 1: three "
                "radix passes)", n_tokens, l.tok_cap, slots, n_terms);
  MUSED_REQUIRE(doc_tokens >= 1 && doc_tokens <= TK_MAX_DOC_TOKENS && doc_tokens <= n_tokens,
                "mused_tokenise_build: the longest document has %d tokens, outside [1, %d]", doc_tokens, TK_MAX_DOC_TOKENS);
  MUSED_REQUIRE(rank && vrow && doc_rowptr && term && cnt && pos && gpostptr && gpostrow && gpostent && info,
                "mused_tokenise_build: an array is missing");
  MUSED_REQUIRE(ws && ws_bytes >= l.bytes && ((uintptr_t)ws & 15) == 0,
                "mused_tokenise_build: workspace of %ld bytes, need %ld (16-byte aligned)", ws_bytes, l.bytes);
  return tk_build_launch(l, n_docs, slots, n_tokens, n_terms, doc_tokens, rank, vrow, doc_rowptr, term, cnt, pos, gpostptr, gpostrow,
                         gpostent, info, stream);
}

long mused_tokenise_cp_ws_bytes(long n_cp, long n_docs, long table_slots) {
  const long slots = table_slots == 0 && n_cp >= 1 ? tk_cp_default_slots(n_cp) : table_slots;
  return tk_cp_sizes_ok(n_cp, n_docs, slots) ? tk_cp_layout(n_cp, n_docs, slots, nullptr).bytes : -1;
}

int mused_tokenise_cp_scan(const unsigned* buf, long n_cp, const unsigned* cls, long n_cls, const int* docptr_host, long n_docs,
                           long table_slots, int max_doc_tokens, int* voc_start, int* voc_len, long voc_cap, int* info, void* ws,
                           long ws_bytes, void* stream) {
  const long slots = table_slots == 0 && n_cp >= 1 ? tk_cp_default_slots(n_cp) : table_slots;
  MUSED_REQUIRE(tk_cp_sizes_ok(n_cp, n_docs, slots),
                "mused_tokenise_cp_scan: bad sizes (code points=%ld in [1, 2^30), docs=%ld in [1, code points], table slots=%ld "
                "in [1, 2^31))", n_cp, n_docs, table_slots);
  MUSED_REQUIRE(buf && cls && docptr_host && voc_start && voc_len && info, "mused_tokenise_cp_scan: an array is missing");
  MUSED_REQUIRE(n_cls >= 128 && n_cls <= TK_CP_TABLE_MAX,
                "mused_tokenise_cp_scan: a class table of %ld entries, outside [128, %ld]", n_cls, TK_CP_TABLE_MAX);
  MUSED_REQUIRE(((uintptr_t)buf & 15) == 0, "mused_tokenise_cp_scan: the buffer must start on a 16-byte boundary");
  MUSED_REQUIRE(docptr_host[0] == 0 && docptr_host[n_docs] == n_cp,
                "mused_tokenise_cp_scan: docptr runs from %d to %d, not from 0 to the %ld code points of the buffer",
                docptr_host[0], docptr_host[n_docs], n_cp);
  for (long d = 0; d < n_docs; ++d)
    MUSED_REQUIRE(docptr_host[d + 1] > docptr_host[d], "mused_tokenise_cp_scan: document %ld is empty or docptr descends (a "
                  "document holds at least its separator)", d);
  MUSED_REQUIRE(max_doc_tokens >= 1 && max_doc_tokens <= TK_MAX_DOC_TOKENS,
                "mused_tokenise_cp_scan: max_doc_tokens=%d outside [1, %d] (one document is sorted in LDS)", max_doc_tokens,
                TK_MAX_DOC_TOKENS);
  const TkWs l = tk_cp_layout(n_cp, n_docs, slots, ws);
  MUSED_REQUIRE(voc_cap >= 1, "mused_tokenise_cp_scan: voc_cap=%ld", voc_cap);
  MUSED_REQUIRE(ws && ws_bytes >= l.bytes && ((uintptr_t)ws & 15) == 0,
                "mused_tokenise_cp_scan: workspace of %ld bytes, need %ld (16-byte aligned)", ws_bytes, l.bytes);
  hipStream_t st = (hipStream_t)stream;
  MUSED_CHECK_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int), st));
  MUSED_CHECK_HIP(hipMemsetAsync(l.table, 0xff, (size_t)slots * sizeof(int), st));
  MUSED_CHECK_HIP(hipMemcpyAsync(l.docptr, docptr_host, (size_t)(n_docs + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  const int cap = (int)l.tok_cap;
  hipLaunchKernelGGL(tk_cp_scan_kernel<false>, dim3((unsigned)l.nb_scan), dim3(TK_SCAN_THREADS), 0, st, buf, n_cp, cls,
                     (unsigned)n_cls, l.low_cp, l.blk, l.tok_start, l.tok_len, cap);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(blockscan_kernel, dim3(1), dim3(BLOCKSCAN_THREADS), 0, st, l.blk, (int)l.nb_scan, info + 0);
  MUSED_LAUNCH_CHECK();
  hipLaunchKernelGGL(tk_cp_scan_kernel<true>, dim3((unsigned)l.nb_scan), dim3(TK_SCAN_THREADS), 0, st, l.low_cp, n_cp, cls,
                     (unsigned)n_cls, l.low_cp, l.blk, l.tok_start, l.tok_len, cap);
  MUSED_LAUNCH_CHECK();
  return tk_vocab_launch(l, n_docs, slots, max_doc_tokens, voc_start, voc_len, voc_cap, info, st);
}

int mused_tokenise_cp_build(long n_cp, long n_docs, long table_slots, int n_tokens, int n_terms, int doc_tokens, const int* rank,
                            const int* vrow, int* doc_rowptr, int* term, int* cnt, int* pos, int* gpostptr, int* gpostrow,
                            int* gpostent, int* info, void* ws, long ws_bytes, void* stream) {
  const long slots = table_slots == 0 && n_cp >= 1 ? tk_cp_default_slots(n_cp) : table_slots;
  MUSED_REQUIRE(tk_cp_sizes_ok(n_cp, n_docs, slots),
                "mused_tokenise_cp_build: bad sizes (code points=%ld in [1, 2^30), docs=%ld in [1, code points], table slots=%ld "
                "in [1, 2^31))", n_cp, n_docs, table_slots);
  const TkWs l = tk_cp_layout(n_cp, n_docs, slots, ws);
  MUSED_REQUIRE(n_tokens >= 1 && n_tokens <= l.tok_cap && n_tokens <= slots && n_terms >= 1 && n_terms <= n_tokens &&
                    n_terms < (1 << 24),
                "mused_tokenise_cp_build: %d tokens (at most %ld and the table's %ld slots), %d terms (at most 2^24 - 1: three "
                "radix passes)", n_tokens, l.tok_cap, slots, n_terms);
  MUSED_REQUIRE(doc_tokens >= 1 && doc_tokens <= TK_MAX_DOC_TOKENS && doc_tokens <= n_tokens,
                "mused_tokenise_cp_build: the longest document has %d tokens, outside [1, %d]", doc_tokens, TK_MAX_DOC_TOKENS);
  MUSED_REQUIRE(rank && vrow && doc_rowptr && term && cnt && pos && gpostptr && gpostrow && gpostent && info,
                "mused_tokenise_cp_build: an array is missing");
  MUSED_REQUIRE(ws && ws_bytes >= l.bytes && ((uintptr_t)ws & 15) == 0,
                "mused_tokenise_cp_build: workspace of %ld bytes, need %ld (16-byte aligned)", ws_bytes, l.bytes);
  return tk_build_launch(l, n_docs, slots, n_tokens, n_terms, doc_tokens, rank, vrow, doc_rowptr, term, cnt, pos, gpostptr, gpostrow,
                         gpostent, info, stream);
}

}  // extern "C"
