// fp64 MFMA GEMM core for gfx950 (v_mfma_f64_16x16x4_f64), templated on the
// storage layout of both operands, the input dtype and an epilogue functor.
//
//   C[m][n] = sum_k opA(m, k) * opB(k, n)          m < M, n < N, k in [k_lo, k_hi)
//
// Operand layouts ("K-contiguous" = the reduction index is the fast axis):
//   A_KC = true  : A stored [M][K]  (row-major, lda)      -> "N" operand
//   A_KC = false : A stored [K][M]  (lda)                  -> "T" operand
//   B_KC = true  : B stored [N][K]  (ldb)   (C = A * B^T)
//   B_KC = false : B stored [K][N]  (ldb)   (C = A * B)
//
// Tiling: 128 x 128 output tile per 256-thread workgroup (4 waves as 2 x 2, each
// wave 64 x 64 = 4 x 4 MFMA tiles, 16 accumulators of 4 f64), K-step 16 staged
// through LDS as [k][m] with a 144-double row pitch (the two k-rows a 32-lane
// ds_read_b64 group touches fall on opposite halves of the 256-B bank row), two
// LDS buffers, next tile prefetched into registers under the MFMAs.
// One f64 MFMA is 64 cycles per SIMD, 16 of them per 8 ds_read_b64: the loop is
// matrix-pipe bound by construction.
// Symmetric launches (GemmArgs::sym): tiles on or above the diagonal only.  An off-diagonal tile runs the loop above and
// stores its result twice (the second time transposed through LDS); a diagonal tile stages ONE operand and computes the
// 36 blocks with block-row <= block-column, 9 MFMAs per wave and K sub-step on 4 / 6 / 7 / 8 ds_read_b64 ("diagonal
// tile" below; measured alone at order 256: 0.82 - 0.84 of the time of three ordinary tiles).
// v_mfma_f64_16x16x4_f64 is an FMA chain over k whose products do not depend on which operand is A
// and which is B (measured: the symmetric and the full product of one matrix agree in every bit), so the mirrored
// entries carry the bits a direct computation gives.
#pragma once
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include "internal.h"

namespace mused {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int GEMM_BM = 128;
constexpr int GEMM_BN = 128;
constexpr int GEMM_BK = 16;
constexpr int GEMM_LD = 144;  // LDS row pitch in doubles
constexpr int GEMM_THREADS = 256;
constexpr int GEMM_LDS_BYTES = 2 /*operands*/ * 2 /*buffers*/ * GEMM_BK * GEMM_LD * 8;

struct GemmArgs {
  const void* A;
  const void* B;
  long lda, ldb;
  long strideA, strideB;  // per batch (blockIdx.z), in elements
  int M, N, K;
  int kchunk;  // split-K: batch index z covers k in [z*kchunk, min(K,(z+1)*kchunk)) when splitk != 0
  int splitk;
  int bsplit;  // batched split-K: blockIdx.z = batch entry * bsplit + split; the split covers k in [split * kchunk, ...), the epilogue
               // sees z = blockIdx.z (partial results, summed in split order by gemm_batched_splitk_reduce)
  int tiles_m, tiles_n;
  const int* rep;  // optional (batched launches): batch entry z is computed only if rep[z] == z
  const int* list;  // optional, instead of rep: list[0] entries are computed, workgroup z of the batch takes entry list[1 + z]
                    // (the workgroups that only exit lie behind the working ones in dispatch order)
  const int* kact;  // optional (plain batched launches): entry z multiplies over k < kact[z] only -- for operands that are
                    // exact zeros from there on: the skipped terms are fma(0, 0, acc), the result is bit-identical
  int sym;  // C = A A^T (A == B, M == N) with a symmetric epilogue: only tiles on or above the diagonal are computed,
            // each off-diagonal tile is also written mirrored (epi.put(z, col, row, epi.value(col, row, v))), and a
            // diagonal tile computes its 36 blocks of 16 x 16 on or above the diagonal from the one staged operand and
            // mirrors the 28 above it: 36 + 64 + 36 of 4 x 64 block products for a 2 x 2 grid of tiles.  Callers set 0 / 1;
            // the launcher turns 1 into 2 (diagonal tiles as described) unless MUSED_GEMM_SYM_DIAG=0 (1: diagonal tiles
            // run the ordinary main loop).  Bit for bit the full product either way.
  // Optional second row segment of an operand built from sketch buffers (TAIL instantiations of the kernel only: launches
  // with tail == null run the kernels they always ran).  Row r of entry z of such an operand, nk = tail_split[z * tail_split_stride]:
  //   r < nk                    the operand's own row r, as ever
  //   nk <= r < nk + tail_pend  row r - nk of the lane's tail: tail + (z / tail_per) * tail_stride, the operand's row pitch
  //   r >= nk + tail_pend       +0.0, whatever the operand holds there: read from tail_zero, a row of the operand's length that
  //                             holds +0.0 (a select behind the loads would make every K step wait for them)
  // Which operands: both of a launch with two K-contiguous operands (the Gram: their M / N rows split), the K-rows operand B
  // ([K][N]: its k rows split) of a launch with A K-contiguous.  The launchers refuse a tail on anything else.
  // Tile order, K order and MFMA sequence are the plain kernel's: the staged doubles are those of the materialised operand.
  const double* tail;
  long tail_stride;
  int tail_per;
  const int* tail_split;
  int tail_split_stride;
  int tail_pend;
  const double* tail_zero;
  // Optional fill source of a symmetric launch with a tail (the Gram of sketch buffers): P P^T of the tail rows of every lane,
  // formed beforehand -- lane (z / tail_per) at fill + (z / tail_per) * fill_stride, leading dimension fill_ld >= tail_pend,
  // only its tail_pend x tail_pend corner is read.  A tile (tm, tn), tm <= tn, with 128 tm >= nk holds nothing but entries of
  // it and +0.0: C[i][j] = PP[i - nk][j - nk] for i, j < nk + tail_pend, +0.0 elsewhere.  Such a tile runs no K loop: the
  // workgroup copies it (and its mirror) through epi.put.  The copied doubles are the ones the K loop gives -- an entry of
  // the MFMA's K chain does not depend on where in a tile it is computed (tests/test_gpu_swfd_ppt.py) -- for finite
  // operands: a zero row times a row with an infinity is NaN when computed and +0.0 when copied.
  const double* fill;
  long fill_stride;
  int fill_ld;
  // Second batch level (GRP instantiations of the kernel only): entry z reads its operands at
  // (z % grp_per) * strideA + (z / grp_per) * grp_stride -- row blocks of several lanes read in place.
  int grp_per;
  long grp_stride;
};

// the split of one batch entry (TAIL kernels): rows [nk, nend) come from `tail`, rows from nend on are zero
struct GemmSplit {
  const double* tail;
  const double* zero;
  int nk, nend;
};
// Row r of a split operand: where it starts, and whether it is a zero row (r >= nend or r >= nrows: the address is then
// that of the row of zeros).
__device__ __forceinline__ const double* split_row(const double* __restrict__ base, long ld, const GemmSplit& sp, int r, int nrows,
                                                   bool& zero) {
  zero = r >= sp.nend || r >= nrows;
  return zero ? sp.zero : (r < sp.nk ? base + (long)r * ld : sp.tail + (long)(r - sp.nk) * ld);
}

// ---- staging -------------------------------------------------------------
// K-contiguous operand: tile rows [r0, r0+128), k in [k0, k0+16).  Thread t owns
// row (t & 127) and the 8 consecutive k's of half (t >> 7).
template <typename TIn, bool VEC>
__device__ __forceinline__ void stage_load_kc(const TIn* __restrict__ src, long ld, int r0, int nrows, int k0,
                                              int kend, TIn (&r)[8]) {
  const int m = threadIdx.x & 127;
  const int kh = threadIdx.x >> 7;
  const int row = r0 + m;
  const int k = k0 + kh * 8;
  if (row < nrows) {
    const TIn* p = src + (long)row * ld + k;
    if (VEC && k + 8 <= kend) {
      if (sizeof(TIn) == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        const float4 b = *reinterpret_cast<const float4*>(p + 4);
        r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
        r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
      } else {
        const double2* q = reinterpret_cast<const double2*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double2 v = q[j];
          r[2 * j] = v.x;
          r[2 * j + 1] = v.y;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = (k + j < kend) ? p[j] : (TIn)0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (TIn)0;
  }
}

// (The staging registers hold the operand in its INPUT type and are converted to fp64 here, on the way into LDS: a conversion
// at load time makes every load wait for its data at once -- the fp32 similarity GEMM then exposed two global-load
// latencies per K step.)
template <typename TIn>
__device__ __forceinline__ void stage_store_kc(double* __restrict__ lds, const TIn (&r)[8]) {
  const int m = threadIdx.x & 127;
  const int kh = threadIdx.x >> 7;
#pragma unroll
  for (int j = 0; j < 8; ++j) lds[(kh * 8 + j) * GEMM_LD + m] = (double)r[j];
}

// MN-contiguous operand stored [K][MN]: thread t owns k-row (t >> 4) and the 8
// consecutive columns starting at (t & 15) * 8.
template <typename TIn, bool VEC>
__device__ __forceinline__ void stage_load_mc(const TIn* __restrict__ src, long ld, int c0, int ncols, int k0,
                                              int kend, TIn (&r)[8]) {
  const int kk = threadIdx.x >> 4;
  const int c = c0 + (threadIdx.x & 15) * 8;
  const int k = k0 + kk;
  if (k < kend) {
    const TIn* p = src + (long)k * ld + c;
    if (VEC && c + 8 <= ncols) {
      if (sizeof(TIn) == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        const float4 b = *reinterpret_cast<const float4*>(p + 4);
        r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
        r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
      } else {
        const double2* q = reinterpret_cast<const double2*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double2 v = q[j];
          r[2 * j] = v.x;
          r[2 * j + 1] = v.y;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = (c + j < ncols) ? p[j] : (TIn)0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (TIn)0;
  }
}

template <typename TIn>
__device__ __forceinline__ void stage_store_mc(double* __restrict__ lds, const TIn (&r)[8]) {
  const int kk = threadIdx.x >> 4;
  const int c = (threadIdx.x & 15) * 8;
  double* p = lds + kk * GEMM_LD + c;
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = (double)r[j];
}

// Full-tile variants (all 128 rows / columns and all 16 k's inside the operand, vectorisable): no per-thread branch, so the
// loads stay in flight across the MFMAs of the current K step (with the bounds checks of the general variants the compiler
// waits for the data at the end of each conditional region).
template <typename TIn>
__device__ __forceinline__ void stage_load8(const TIn* __restrict__ p, TIn (&r)[8]) {
  if (sizeof(TIn) == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
    r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
  } else {
    const double2* q = reinterpret_cast<const double2*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double2 v = q[j];
      r[2 * j] = v.x;
      r[2 * j + 1] = v.y;
    }
  }
}
template <typename TIn>
__device__ __forceinline__ void stage_load_kc_full(const TIn* __restrict__ src, long ld, int r0, int k0, TIn (&r)[8]) {
  stage_load8(src + (long)(r0 + (threadIdx.x & 127)) * ld + k0 + (threadIdx.x >> 7) * 8, r);
}
template <typename TIn>
__device__ __forceinline__ void stage_load_mc_full(const TIn* __restrict__ src, long ld, int c0, int k0, TIn (&r)[8]) {
  stage_load8(src + (long)(k0 + (threadIdx.x >> 4)) * ld + c0 + (threadIdx.x & 15) * 8, r);
}

// Split operands (GemmSplit): the row a thread stages is given by its address (null: a zero row).
template <bool VEC>
__device__ __forceinline__ void stage_load_kc_row(const double* __restrict__ prow, int k0, int kend, double (&r)[8]) {
  const int k = k0 + (threadIdx.x >> 7) * 8;
  if (prow) {
    const double* p = prow + k;
    if (VEC && k + 8 <= kend) {
      stage_load8(p, r);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = (k + j < kend) ? p[j] : 0.0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = 0.0;
  }
}
template <bool VEC>
__device__ __forceinline__ void stage_load_mc_row(const double* __restrict__ prow, int c0, int ncols, double (&r)[8]) {
  const int c = c0 + (threadIdx.x & 15) * 8;
  if (prow) {
    const double* p = prow + c;
    if (VEC && c + 8 <= ncols) {
      stage_load8(p, r);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = (c + j < ncols) ? p[j] : 0.0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = 0.0;
  }
}

// XCD-aware workgroup id: blocks b and b+8 share an XCD (observed round-robin
// dispatch; speed only).  Give every XCD a contiguous run of tiles so that
// neighbouring tiles (same A rows) hit the same L2.  Bijective for any nwg.
__device__ __forceinline__ int xcd_remap(int pid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = pid & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (pid >> 3);
}

// One 128 x 128 output tile: K loop of the workgroup (staging through LDS, MFMA), result left in the accumulators.
// C/D map of v_mfma_f64_16x16x4_f64 inside the wave's 64 x 64 block: acc[i][j][r] is the element
//   row = wr * 64 + i * 16 + (lane >> 4) + 4 * r,   col = wc * 64 + j * 16 + (lane & 15)      (wr = wave >> 1, wc = wave & 1).
// TAIL: operands with a second row segment (GemmArgs::tail, doubles only); `sp` is the entry's split.
template <typename TA, typename TB, bool A_KC, bool B_KC, bool VEC, bool TAIL = false>
__device__ __forceinline__ void gemm_tile_mainloop(const GemmArgs& g, const TA* __restrict__ A, const TB* __restrict__ B,
                                                   int m0, int n0, int k_lo, int k_hi, double* smem,
                                                   v4f64 (&acc)[4][4], const GemmSplit& sp = GemmSplit{}) {
  double* As = smem;                                 // [2][BK][LD]
  double* Bs = smem + 2 * GEMM_BK * GEMM_LD;         // [2][BK][LD]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int kq = lane >> 4, li = lane & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};

  TA ra[8];
  TB rb[8];
  const int nkt = (k_hi - k_lo + GEMM_BK - 1) / GEMM_BK;

  const bool full_mn = VEC && m0 + GEMM_BM <= g.M && n0 + GEMM_BN <= g.N;  // (uniform over the workgroup)
  // TAIL: a K-contiguous split operand gives every thread one row for the whole K loop (pa / pb; za / zb: it is a zero row,
  // which the steps that are not full stage without loading); a K-rows split operand gives it another row every K step
  const double *pa = nullptr, *pb = nullptr;
  bool za = false, zb = false;
  constexpr bool split_a = TAIL && A_KC && B_KC;  // (B always splits; which operands split is fixed by the layouts: GemmArgs::tail)
  if constexpr (TAIL) {
    static_assert(!TAIL || (std::is_same<TA, double>::value && std::is_same<TB, double>::value), "split operands are doubles");
    if (split_a) pa = split_row((const double*)A, g.lda, sp, m0 + (threadIdx.x & 127), g.M, za);
    if (B_KC) pb = split_row((const double*)B, g.ldb, sp, n0 + (threadIdx.x & 127), g.N, zb);
  }
  auto load_tile = [&](int kt) {
    const int k0 = k_lo + kt * GEMM_BK;
    if constexpr (TAIL) {
      double(&da)[8] = (double(&)[8])ra;
      double(&db)[8] = (double(&)[8])rb;
      // one uniform branch, as below: no conditional region between the loads of a full step
      if (VEC && k0 + GEMM_BK <= k_hi && (split_a || m0 + GEMM_BM <= g.M) && (B_KC || n0 + GEMM_BN <= g.N)) {
        if constexpr (split_a) stage_load8(pa + k0 + (threadIdx.x >> 7) * 8, da);
        else if constexpr (A_KC) stage_load_kc_full<TA>(A, g.lda, m0, k0, ra);
        else stage_load_mc_full<TA>(A, g.lda, m0, k0, ra);
        if constexpr (B_KC) {
          stage_load8(pb + k0 + (threadIdx.x >> 7) * 8, db);
        } else {
          const double* p = split_row((const double*)B, g.ldb, sp, k0 + (threadIdx.x >> 4), k_hi, zb);
          stage_load8(p + n0 + (threadIdx.x & 15) * 8, db);
        }
        return;
      }
      if constexpr (split_a) stage_load_kc_row<VEC>(za ? nullptr : pa, k0, k_hi, da);
      else if constexpr (A_KC) stage_load_kc<TA, VEC>(A, g.lda, m0, g.M, k0, k_hi, ra);
      else stage_load_mc<TA, VEC>(A, g.lda, m0, g.M, k0, k_hi, ra);
      if constexpr (B_KC) {
        stage_load_kc_row<VEC>(zb ? nullptr : pb, k0, k_hi, db);
      } else {
        const double* p = split_row((const double*)B, g.ldb, sp, k0 + (threadIdx.x >> 4), k_hi, zb);
        stage_load_mc_row<VEC>(zb ? nullptr : p, n0, g.N, db);
      }
      return;
    }
    if (full_mn && k0 + GEMM_BK <= k_hi) {
      if (A_KC) stage_load_kc_full<TA>(A, g.lda, m0, k0, ra); else stage_load_mc_full<TA>(A, g.lda, m0, k0, ra);
      if (B_KC) stage_load_kc_full<TB>(B, g.ldb, n0, k0, rb); else stage_load_mc_full<TB>(B, g.ldb, n0, k0, rb);
      return;
    }
    if (A_KC) stage_load_kc<TA, VEC>(A, g.lda, m0, g.M, k0, k_hi, ra);
    else      stage_load_mc<TA, VEC>(A, g.lda, m0, g.M, k0, k_hi, ra);
    if (B_KC) stage_load_kc<TB, VEC>(B, g.ldb, n0, g.N, k0, k_hi, rb);
    else      stage_load_mc<TB, VEC>(B, g.ldb, n0, g.N, k0, k_hi, rb);
  };
  auto store_tile = [&](int buf) {
    double* a = As + buf * GEMM_BK * GEMM_LD;
    double* b = Bs + buf * GEMM_BK * GEMM_LD;
    if (A_KC) stage_store_kc(a, ra); else stage_store_mc(a, ra);
    if (B_KC) stage_store_kc(b, rb); else stage_store_mc(b, rb);
  };

  if (nkt > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();

  int cur = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const bool more = (kt + 1 < nkt);
    if (more) load_tile(kt + 1);
    const double* a = As + cur * GEMM_BK * GEMM_LD + wr * 64 + li;
    const double* b = Bs + cur * GEMM_BK * GEMM_LD + wc * 64 + li;
#pragma unroll
    for (int kk = 0; kk < GEMM_BK / 4; ++kk) {
      double fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = a[(kk * 4 + kq) * GEMM_LD + i * 16];
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = b[(kk * 4 + kq) * GEMM_LD + j * 16];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (more) store_tile(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
}

// ---- diagonal tile of a symmetric launch -----------------------------------
// A 128 x 128 tile on the diagonal of C = A A^T is symmetric itself: of its 8 x 8 blocks of 16 x 16 only the 36 with
// block-row i <= block-column j are computed, 9 per wave, and the 28 below the diagonal are the mirrors of those above.
// Both MFMA operands are fragments of the ONE staged panel: fragment b = As[k][b * 16 + (lane & 15)] is the row fragment
// of block-row b and the column fragment of block-column b alike, so nothing is loaded or stored for B.
// Block n of wave w is (DIAG_I[w][n], DIAG_J[w][n]); wave w reads fragments 0 .. DIAG_NF[w] - 1 (4 / 6 / 7 / 8 ds_read_b64
// per 9 MFMAs).  A block of column j with i < j is mirrored in the group of its column: DIAG_GRP[w][.] = {j, first i, count}.
constexpr int DIAG_I[4][9] = {{0, 0, 1, 0, 1, 2, 0, 1, 2}, {3, 0, 1, 2, 3, 4, 0, 1, 2}, {3, 4, 5, 0, 1, 2, 3, 4, 5}, {6, 0, 1, 2, 3, 4, 5, 6, 7}};
constexpr int DIAG_J[4][9] = {{0, 1, 1, 2, 2, 2, 3, 3, 3}, {3, 4, 4, 4, 4, 4, 5, 5, 5}, {5, 5, 5, 6, 6, 6, 6, 6, 6}, {6, 7, 7, 7, 7, 7, 7, 7, 7}};
constexpr int DIAG_NF[4] = {4, 6, 7, 8};
constexpr int DIAG_NGRP[4] = {3, 2, 2, 1};
constexpr int DIAG_GRP[4][3][3] = {{{1, 0, 1}, {2, 0, 2}, {3, 0, 3}}, {{4, 0, 4}, {5, 0, 3}, {0, 0, 0}}, {{5, 3, 2}, {6, 0, 6}, {0, 0, 0}}, {{7, 0, 7}, {0, 0, 0}, {0, 0, 0}}};
constexpr int DIAG_PATCH_LD = 130;  // pitch of the wave's 16-row transposition patch: 2 (mod 32), writes (li, kq) -> li * 130 + kq hit 32 banks

constexpr int diag_acc_index(int w, int i, int j) {
  for (int n = 0; n < 9; ++n)
    if (DIAG_I[w][n] == i && DIAG_J[w][n] == j) return n;
  return -1;
}

// the 4 K sub-steps of one staged panel for wave W: 9 accumulators, every index a compile-time constant
template <int W, int N = 0>
__device__ __forceinline__ void diag_mfma9(const double (&f)[8], v4f64 (&acc)[9]) {
  if constexpr (N < 9) {
    constexpr int i = DIAG_I[W][N], j = DIAG_J[W][N];
    acc[N] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[i], f[j], acc[N], 0, 0, 0);
    diag_mfma9<W, N + 1>(f, acc);
  }
}
template <int W>
__device__ __forceinline__ void diag_kstep(const double* __restrict__ a, v4f64 (&acc)[9]) {
#pragma unroll
  for (int kk = 0; kk < GEMM_BK / 4; ++kk) {
    double f[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) f[b] = (b < DIAG_NF[W]) ? a[kk * 4 * GEMM_LD + b * 16] : 0.0;
    diag_mfma9<W>(f, acc);
  }
}

// K loop of a diagonal tile: as gemm_tile_mainloop with one operand.  Every computed element is the same chain as there
// (K steps of 16 ascending, four MFMAs per step in kk order, from +0.0).
template <typename TA, bool A_KC, bool VEC, bool TAIL = false>
__device__ __forceinline__ void gemm_tile_mainloop_diag(const GemmArgs& g, const TA* __restrict__ A, int m0, int k_lo, int k_hi,
                                                        double* As, int wave, v4f64 (&acc)[9], const GemmSplit& sp = GemmSplit{}) {
  const int lane = threadIdx.x & 63;
  const int kq = lane >> 4, li = lane & 15;
#pragma unroll
  for (int n = 0; n < 9; ++n) acc[n] = (v4f64){0.0, 0.0, 0.0, 0.0};

  TA ra[8];
  const int nkt = (k_hi - k_lo + GEMM_BK - 1) / GEMM_BK;
  const bool full_m = VEC && m0 + GEMM_BM <= g.M;  // (uniform over the workgroup)
  // TAIL: the thread's row of the split operand, as in gemm_tile_mainloop
  const double* pa = nullptr;
  bool za = false;
  constexpr bool split_a = TAIL && A_KC;
  if constexpr (TAIL) {
    if (split_a) pa = split_row((const double*)A, g.lda, sp, m0 + (threadIdx.x & 127), g.M, za);
  }
  auto load_tile = [&](int kt) {
    const int k0 = k_lo + kt * GEMM_BK;
    if constexpr (TAIL) {
      if constexpr (split_a) {
        double(&da)[8] = (double(&)[8])ra;
        if (VEC && k0 + GEMM_BK <= k_hi) stage_load8(pa + k0 + (threadIdx.x >> 7) * 8, da);
        else stage_load_kc_row<VEC>(za ? nullptr : pa, k0, k_hi, da);
        return;
      }
    }
    if (full_m && k0 + GEMM_BK <= k_hi) {
      if (A_KC) stage_load_kc_full<TA>(A, g.lda, m0, k0, ra); else stage_load_mc_full<TA>(A, g.lda, m0, k0, ra);
      return;
    }
    if (A_KC) stage_load_kc<TA, VEC>(A, g.lda, m0, g.M, k0, k_hi, ra);
    else      stage_load_mc<TA, VEC>(A, g.lda, m0, g.M, k0, k_hi, ra);
  };
  auto store_tile = [&](int buf) {
    double* a = As + buf * GEMM_BK * GEMM_LD;
    if (A_KC) stage_store_kc(a, ra); else stage_store_mc(a, ra);
  };

  if (nkt > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();

  int cur = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const bool more = (kt + 1 < nkt);
    if (more) load_tile(kt + 1);
    const double* a = As + cur * GEMM_BK * GEMM_LD + kq * GEMM_LD + li;
    switch (wave) {  // wave-uniform
      case 0: diag_kstep<0>(a, acc); break;
      case 1: diag_kstep<1>(a, acc); break;
      case 2: diag_kstep<2>(a, acc); break;
      default: diag_kstep<3>(a, acc); break;
    }
    if (more) store_tile(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
}

// Stores of wave W's 9 blocks, and of the mirrors of those above the diagonal.  The mirrors of the blocks of one column j
// (block-rows i0 .. i0 + cnt - 1) are rows j * 16 .. + 15, columns i0 * 16 .. of the tile: transposed through a wave-private
// LDS patch of 16 rows, so that a store instruction writes runs of at least 128 contiguous bytes (512 from cnt = 4 on).
template <int W, int GI, int II, typename Epi>
__device__ __forceinline__ void diag_mirror_fill(const GemmArgs& g, const Epi& epi, int m0, double* patch, const v4f64 (&acc)[9]) {
  constexpr int j = DIAG_GRP[W][GI][0], i0 = DIAG_GRP[W][GI][1], cnt = DIAG_GRP[W][GI][2];
  if constexpr (II < cnt) {
    constexpr int n = diag_acc_index(W, i0 + II, j);
    static_assert(n >= 0, "block not held by this wave");
    const int lane = threadIdx.x & 63;
    const int kq = lane >> 4, li = lane & 15;
    const int col = m0 + j * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rl = II * 16 + kq + 4 * r;
      const int rg = m0 + i0 * 16 + rl;
      // entry (col, row) of the result: evaluated in ITS orientation (the epilogue need not be commutative)
      patch[li * DIAG_PATCH_LD + rl] = (rg < g.M && col < g.N) ? epi.value(col, rg, acc[n][r]) : 0.0;
    }
    diag_mirror_fill<W, GI, II + 1>(g, epi, m0, patch, acc);
  }
}

template <int W, int GI, typename Epi>
__device__ __forceinline__ void diag_mirror_groups(const GemmArgs& g, const Epi& epi, int z, int m0, double* patch,
                                                   const v4f64 (&acc)[9]) {
  if constexpr (GI < DIAG_NGRP[W]) {
    constexpr int j = DIAG_GRP[W][GI][0], i0 = DIAG_GRP[W][GI][1], cnt = DIAG_GRP[W][GI][2];
    constexpr int width = cnt * 16;
    const int lane = threadIdx.x & 63;
    diag_mirror_fill<W, GI, 0>(g, epi, m0, patch, acc);
    // wave-private patch: LDS operations of one wave complete in order, no barrier
#pragma unroll
    for (int t = 0; t < width / 4; ++t) {
      const int idx = t * 64 + lane;
      const int c = idx / width, off = idx % width;
      const int rowm = m0 + j * 16 + c, colm = m0 + i0 * 16 + off;
      if (rowm < g.N && colm < g.M) epi.put(z, rowm, colm, patch[c * DIAG_PATCH_LD + off]);
    }
    diag_mirror_groups<W, GI + 1>(g, epi, z, m0, patch, acc);
  }
}

template <int W, int N, typename Epi>
__device__ __forceinline__ void diag_store_blocks(const GemmArgs& g, const Epi& epi, int z, int m0, const v4f64 (&acc)[9]) {
  if constexpr (N < 9) {
    const int lane = threadIdx.x & 63;
    const int col = m0 + DIAG_J[W][N] * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + DIAG_I[W][N] * 16 + (lane >> 4) + 4 * r;
      if (row < g.M && col < g.N) epi(z, row, col, acc[N][r]);
    }
    diag_store_blocks<W, N + 1>(g, epi, z, m0, acc);
  }
}

template <int W, typename Epi>
__device__ __forceinline__ void diag_epilogue(const GemmArgs& g, const Epi& epi, int z, int m0, double* smem,
                                              const v4f64 (&acc)[9]) {
  diag_store_blocks<W, 0>(g, epi, z, m0, acc);
  diag_mirror_groups<W, 0>(g, epi, z, m0, smem + W * (16 * DIAG_PATCH_LD), acc);
}

// MUSED_GEMM_SYM_DIAG=0: the diagonal tiles of symmetric launches run the ordinary main loop (all 64 blocks, two operands).
inline int gemm_sym_diag_enabled() {
  static const int on = [] {
    const char* s = getenv("MUSED_GEMM_SYM_DIAG");
    return (s && s[0] == '0') ? 0 : 1;
  }();
  return on;
}

// A tile that is copied (GemmArgs::fill): rows [r0, r0 + 128) x columns [c0, c0 + 128) of entry z, r0 and c0 >= nk.  A thread
// owns one column and every second row: a wave's load and its store each cover 512 contiguous bytes of one row.
template <typename Epi>
__device__ __forceinline__ void gemm_fill_tile(const GemmArgs& g, const Epi& epi, int z, const double* __restrict__ pp, int nk,
                                               int nend, int r0, int c0) {
  const int c = c0 + (threadIdx.x & 127);
  if (c >= g.N) return;
  const bool cin = c < nend;
  const int rlim = min(g.M, r0 + GEMM_BM);
#pragma unroll 8
  for (int r = r0 + (threadIdx.x >> 7); r < rlim; r += 2) {
    const double v = (cin && r < nend) ? pp[(long)(r - nk) * g.fill_ld + (c - nk)] : 0.0;
    epi.put(z, r, c, epi.value(r, c, v));
  }
}

// Epilogue concept:  void operator()(int batch, int row, int col, double v) const
template <typename TA, typename TB, bool A_KC, bool B_KC, bool VEC, typename Epi, bool TAIL = false, bool GRP = false>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_f64_kernel(GemmArgs g, Epi epi) {
  extern __shared__ __attribute__((aligned(16))) double smem[];

  int z = blockIdx.z;
  int zb = g.bsplit ? z / g.bsplit : z;  // batch entry
  if (g.list) {
    if (zb >= g.list[0]) return;
    const int e = g.list[1 + zb];
    z += (e - zb) * (g.bsplit ? g.bsplit : 1);
    zb = e;
  } else if (g.rep && g.rep[zb] != zb) return;  // a duplicate of entry rep[zb]: its consumer reads that one
  int tm, tn;
  if (g.sym) {
    // C = A A^T with a symmetric epilogue: the grid holds the tiles on or above the diagonal only, row-major over
    // the triangle (consecutive workgroups of an XCD share the A row-panel); row tm starts at
    // e0(tm) = tm * tiles - tm (tm - 1) / 2.  Equal tile counts per XCD (a full grid with early exits gives the
    // XCD that owns the first tile-rows twice the average work).
    const int t = g.tiles_n, nwg = t * (t + 1) / 2;
    const int e = xcd_remap(blockIdx.x, nwg);
    int r = (int)((2.0 * t + 1.0 - sqrt((2.0 * t + 1.0) * (2.0 * t + 1.0) - 8.0 * e)) * 0.5);
    r = r < 0 ? 0 : (r > t - 1 ? t - 1 : r);
    while (r > 0 && r * t - r * (r - 1) / 2 > e) --r;
    while (r + 1 < t && (r + 1) * t - (r + 1) * r / 2 <= e) ++r;
    tm = r;
    tn = r + (e - (r * t - r * (r - 1) / 2));
  } else {
    const int nwg = g.tiles_m * g.tiles_n;
    const int wg = xcd_remap(blockIdx.x, nwg);
    // grouped tile order: consecutive workgroup ids (one XCD, dispatched together) cover 8 tile-rows x 8
    // tile-columns, so that the ~64 tiles in flight on an XCD re-use 8 A row-panels and 8 B column-panels
    // out of its L2 instead of streaming 64 different B panels from the Infinity Cache
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * g.tiles_n;
    const int group_id = wg / per_group;
    const int first_m = group_id * GROUP_M;
    const int group_size = min(g.tiles_m - first_m, GROUP_M);
    tm = first_m + (wg % group_size);
    tn = (wg % per_group) / group_size;
  }
  const int m0 = tm * GEMM_BM, n0 = tn * GEMM_BN;
  const bool mirror = g.sym && tm != tn;

  int k_lo = 0, k_hi = g.K;
  const TA* A = reinterpret_cast<const TA*>(g.A);
  const TB* B = reinterpret_cast<const TB*>(g.B);
  if (g.splitk) {
    k_lo = z * g.kchunk;
    k_hi = min(g.K, k_lo + g.kchunk);
  } else {
    if constexpr (GRP) {
      const int grp = zb / g.grp_per;
      A += (long)(zb - grp * g.grp_per) * g.strideA + (long)grp * g.grp_stride;
      B += (long)(zb - grp * g.grp_per) * g.strideB + (long)grp * g.grp_stride;
    } else {
      A += (long)zb * g.strideA;
      B += (long)zb * g.strideB;
    }
    if (g.bsplit) {
      k_lo = (z - zb * g.bsplit) * g.kchunk;
      k_hi = min(g.K, k_lo + g.kchunk);
    } else if (g.kact) {
      k_hi = min(g.K, g.kact[zb]);
    }
  }

  GemmSplit sp{};
  if constexpr (TAIL) {
    sp.nk = g.tail_split[(long)zb * g.tail_split_stride];
    sp.nend = sp.nk + g.tail_pend;
    sp.tail = g.tail + (long)(zb / g.tail_per) * g.tail_stride;
    sp.zero = g.tail_zero;
    if constexpr (A_KC && B_KC) {
      // a tile of pending rows and zero rows only: copied from the lane's P P^T (uniform over the workgroup; tm <= tn)
      if (g.fill && g.sym && m0 >= sp.nk) {
        const double* pp = g.fill + (long)(zb / g.tail_per) * g.fill_stride;
        gemm_fill_tile(g, epi, z, pp, sp.nk, sp.nend, m0, n0);
        if (mirror) gemm_fill_tile(g, epi, z, pp, sp.nk, sp.nend, n0, m0);
        return;
      }
    }
  }

  if constexpr (std::is_same<TA, TB>::value && A_KC == B_KC) {
    if (g.sym == 2 && tm == tn) {  // (uniform over the workgroup)
      const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
      v4f64 acc9[9];
      gemm_tile_mainloop_diag<TA, A_KC, VEC, TAIL>(g, A, m0, k_lo, k_hi, smem, w, acc9, sp);
      // behind the main loop's last barrier every wave is done with the operand buffers: the patches may overwrite them
      switch (w) {
        case 0: diag_epilogue<0>(g, epi, z, m0, smem, acc9); break;
        case 1: diag_epilogue<1>(g, epi, z, m0, smem, acc9); break;
        case 2: diag_epilogue<2>(g, epi, z, m0, smem, acc9); break;
        default: diag_epilogue<3>(g, epi, z, m0, smem, acc9); break;
      }
      return;
    }
  }

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int kq = lane >> 4, li = lane & 15;

  v4f64 acc[4][4];
  gemm_tile_mainloop<TA, TB, A_KC, B_KC, VEC, TAIL>(g, A, B, m0, n0, k_lo, k_hi, smem, acc, sp);

  // C/D map of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + wc * 64 + j * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr * 64 + i * 16 + kq + 4 * r;
        if (row < g.M && col < g.N) epi(z, row, col, acc[i][j][r]);
      }
    }
  }
  if (mirror) {
    // the same 64 x 64 block of the wave, written to (col, row): transposed through a wave-private LDS patch
    // (32 columns at a time, pitch 65) so that every store instruction writes 512 contiguous bytes of one row
    __syncthreads();  // all waves are done with the operand buffers
    double* patch = smem + wave * (32 * 65);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int j = half * 2 + jj;
          const int col = n0 + wc * 64 + j * 16 + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rl = i * 16 + kq + 4 * r;
            // entry (col, row) of the result: evaluated in ITS orientation (the epilogue need not be commutative)
            const int rg = m0 + wr * 64 + rl;
            patch[(jj * 16 + li) * 65 + rl] = (rg < g.M && col < g.N) ? epi.value(col, rg, acc[i][j][r]) : 0.0;
          }
        }
      // wave-private patch: LDS operations of one wave complete in order, no barrier
      const int rowm = m0 + wr * 64 + lane;
#pragma unroll 8
      for (int c = 0; c < 32; ++c) {
        const int colm = n0 + wc * 64 + half * 32 + c;
        if (colm < g.N && rowm < g.M) epi.put(z, colm, rowm, patch[c * 65 + lane]);
      }
    }
  }
}

// ---- plain epilogue --------------------------------------------------------
struct EpiStore {
  double* C;
  long ldc;
  long strideC;
  double alpha;
  __device__ __forceinline__ void operator()(int z, int row, int col, double v) const {
    C[(long)z * strideC + (long)row * ldc + col] = alpha * v;
  }
  // symmetric launches: value(row, col, v) is what operator() would store, put() stores it somewhere else
  __device__ __forceinline__ double value(int, int, double v) const { return alpha * v; }
  __device__ __forceinline__ void put(int z, int row, int col, double val) const {
    C[(long)z * strideC + (long)row * ldc + col] = val;
  }
};

template <typename TA, typename TB, bool A_KC, bool B_KC, bool VEC, typename Epi, bool TAIL = false, bool GRP = false>
int gemm_f64_prepare_t() {
  // > 64 KiB of dynamic LDS needs the attribute once per kernel; done outside stream capture.  Several host
  // threads drive the library (sketch groups + the main path): one-time, thread-safe.
  static LdsOptIn opt;
  auto k = gemm_f64_kernel<TA, TB, A_KC, B_KC, VEC, Epi, TAIL, GRP>;
  const hipError_t err = allow_dynamic_lds(opt, reinterpret_cast<const void*>(k), GEMM_LDS_BYTES);
  MUSED_CHECK_HIP(err);
  return MUSED_OK;
}

template <typename TA, typename TB, bool A_KC, bool B_KC, typename Epi, bool TAIL = false, bool GRP = false>
int gemm_f64_launch_t(GemmArgs g, int batch, Epi epi, bool vec, hipStream_t stream) {
  g.tiles_m = cdiv(g.M, GEMM_BM);
  g.tiles_n = cdiv(g.N, GEMM_BN);
  if (g.sym) g.sym = (g.sym != 3 && gemm_sym_diag_enabled()) ? 2 : 1;  // (3: the caller asks for ordinary diagonal tiles)
  if (g.M <= 0 || g.N <= 0 || batch <= 0) return MUSED_OK;
  dim3 grid(g.sym ? g.tiles_n * (g.tiles_n + 1) / 2 : g.tiles_m * g.tiles_n, 1, batch);
  int rc;
  if (vec) {
    if ((rc = gemm_f64_prepare_t<TA, TB, A_KC, B_KC, true, Epi, TAIL, GRP>())) return rc;
    hipLaunchKernelGGL((gemm_f64_kernel<TA, TB, A_KC, B_KC, true, Epi, TAIL, GRP>), grid, dim3(GEMM_THREADS), GEMM_LDS_BYTES,
                       stream, g, epi);
  } else {
    if ((rc = gemm_f64_prepare_t<TA, TB, A_KC, B_KC, false, Epi, TAIL, GRP>())) return rc;
    hipLaunchKernelGGL((gemm_f64_kernel<TA, TB, A_KC, B_KC, false, Epi, TAIL, GRP>), grid, dim3(GEMM_THREADS), GEMM_LDS_BYTES,
                       stream, g, epi);
  }
  MUSED_LAUNCH_CHECK();
  return MUSED_OK;
}

// 16-byte vector loads are legal when base pointers, leading dimensions and
// batch strides keep every 8-element group 16-B aligned.
template <typename T>
static inline bool vec_ok(const void* p, long ld, long stride) {
  const long e = 16 / (long)sizeof(T);
  return ((uintptr_t)p % 16 == 0) && (ld % e == 0) && (stride % e == 0);
}

}  // namespace mused
