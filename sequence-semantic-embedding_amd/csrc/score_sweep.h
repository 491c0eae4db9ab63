// The fp32 index sweep shared by sse_score_rank, sse_score_above, sse_score_topk_filtered, sse_score_topk_grouped and
// sse_score_topk_after (score_rank.hip, score_above.hip and -- the last three calls -- score_eligible.h; DESIGN K6i):
// [N,S] x [S,P] on v_mfma_f32_32x32x2_f32 from the fragment-order index, the sweep of score_topk_kernel's COLLECT variant with
// the queries taken row-major.  score_rank_kernel, score_above_kernel and eligible_sweep_kernel each keep their own prologue
// (what a lane holds per column) and epilogue (what it does with a tile's 16 scores per column) and call the pieces below in
// this order:
//   sweep_decode         workgroup = (block of NQ x 32 columns, index split)
//   sweep_stage_queries  the block's query rows into LDS as MFMA B fragments [k-group][column tile][1 KiB]
//   sweep_tile_range     a wave walks its split's tiles w, w + 8, ...
//   SWEEP_TILE_MFMA      one index tile (32 rows, M) x NQ column tiles (N): index fragments from global memory PF k-groups
//                        ahead (a ring in registers), query fragments from LDS
//   sweep_row ...        a lane owns column (lane & 31) of every column tile and 16 rows of the index tile
// A column is a (query, label) or (query, threshold) pair for rank and above, a query for filtered, grouped and after.
#pragma once
#include "sse_kernels.h"

#define SWEEP_THREADS 512           // 8 waves = 2 per SIMD, as score_topk_kernel
#define SWEEP_LDS_MAX (160 * 1024)  // dynamic LDS of a workgroup; a kernel with static LDS of its own passes less

// XCD-aware decode, as score_topk_kernel: the workgroups of one XCD (blockIdx % 8) sweep the same index range
__device__ __forceinline__ void sweep_decode(int NSPLIT, int &split, int &qb) {
  const int b = blockIdx.x, xcd = b & 7, j = b >> 3;
  if (NSPLIT <= 8) {
    const int per = 8 / NSPLIT;
    split = xcd / per;
    qb = j * per + xcd % per;
  } else {
    const int m = NSPLIT >> 3;
    split = xcd + 8 * (j % m);
    qb = j / m;
  }
}

// smem [KG][NQ][256] <- the query rows of columns qb * NQ * 32 ... straight from the row-major queries (the values
// launch_pack_rows produces); columns past P and dimensions past S are zero.  VIA_PAIR_Q: a column's row of q is
// pair_q[column] (rank, above); otherwise the column itself (filtered, grouped: pair_q unused).
template <int NQ, bool VIA_PAIR_Q>
__device__ __forceinline__ void sweep_stage_queries(float *smem, const float *q, const int32_t *pair_q, int qb, int P, int S, int KG,
                                                    int tid) {
  f32x4 *dst = reinterpret_cast<f32x4 *>(smem);
  for (int i = tid; i < NQ * KG * 64; i += SWEEP_THREADS) {
    const int kg = (i >> 6) / NQ, l = i & 63, pair = (qb * NQ + (i >> 6) % NQ) * 32 + (l & 31);
    f32x4 v = {0, 0, 0, 0};
    if (pair < P) {
      const int k0 = kg * 8 + (l >> 5) * 4;
      const float *src = q + (size_t)(VIA_PAIR_Q ? pair_q[pair] : pair) * S + k0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k0 + e < S) v[e] = src[e];
    }
    dst[i] = v;
  }
}

// the n-tiles [t0, t1) of a split
__device__ __forceinline__ void sweep_tile_range(int NT, int NSPLIT, int split, int &t0, int &t1) {
  const int tps = (NT + NSPLIT - 1) / NSPLIT;  // n-tiles per split
  t0 = split * tps;
  t1 = min(NT, t0 + tps);
}

// only the index's last tile has rows >= N (zero padding); -1: N is a whole number of tiles
__device__ __forceinline__ int sweep_tail_tile(int64_t N) { return (N & 31) ? (int)(N >> 5) : -1; }

// f32x16 acc[NQ]; acc[q] = index tile `tile` x column tile q over all KG k-groups; qs = smem + lane * 4.
//   1. The first KG % PF k-groups one by one, then a ring of PF = 4 index fragments in flight over the rest (no branch in the
//      unrolled body: a refill past the tile's end re-reads its last k-group and is never used).
//   2. The column fragments of the next k-group are read from LDS in front of this k-group's MFMAs; the order is pinned
//      between the two sched_barrier(0), as in score_small_index_kernel: the compiler otherwise sinks the refills behind the
//      block and waits for them at once.
//   3. The wave runs at raised priority from the first MFMA to the last.
// A macro, not a function: hipcc simplifies an inlined function on its own before it inlines it, and the four kernels then
// come out with other register counts and occupancies than with this text in their bodies (profiles/score_sweep_refactor.txt).
#define SWEEP_TILE_MFMA(NQ, idxp, tile, KG, qs, lane, acc)                                                                          \
  f32x16 acc[NQ];                                                                                                                   \
  {                                                                                                                                 \
    constexpr int PF = 4;                                                                                                           \
    const f32x4 *ap = reinterpret_cast<const f32x4 *>(idxp) + (size_t)(tile) * (KG) * 64 + (lane);                                  \
    _Pragma("unroll") for (int q = 0; q < NQ; ++q) acc[q] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                 \
    const int rem = (KG) & (PF - 1);                                                                                                \
    f32x4 ar[PF];                                                                                                                   \
    _Pragma("unroll") for (int d = 0; d < PF; ++d) ar[d] = ap[(size_t)min(rem + d, (KG) - 1) * 64];                                 \
    __builtin_amdgcn_s_setprio(1);                                                                                                  \
    for (int kg = 0; kg < rem; ++kg) {                                                                                              \
      const f32x4 av = ap[(size_t)kg * 64];                                                                                         \
      f32x4 bq[NQ];                                                                                                                 \
      _Pragma("unroll") for (int q = 0; q < NQ; ++q) bq[q] = *reinterpret_cast<const f32x4 *>((qs) + ((size_t)kg * NQ + q) * 256);  \
      _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                                                 \
        _Pragma("unroll") for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bq[q][e], acc[q], 0, 0, 0); \
    }                                                                                                                               \
    f32x4 bq[NQ], bqn[NQ];                                                                                                          \
    _Pragma("unroll") for (int q = 0; q < NQ; ++q)                                                                                  \
      bq[q] = *reinterpret_cast<const f32x4 *>((qs) + ((size_t)min(rem, (KG) - 1) * NQ + q) * 256);                                 \
    for (int kg0 = rem; kg0 < (KG); kg0 += PF) {                                                                                    \
      _Pragma("unroll") for (int d = 0; d < PF; ++d) {                                                                              \
        const int kg = kg0 + d;                                                                                                     \
        _Pragma("unroll") for (int q = 0; q < NQ; ++q)                                                                              \
          bqn[q] = *reinterpret_cast<const f32x4 *>((qs) + ((size_t)min(kg + 1, (KG) - 1) * NQ + q) * 256);                         \
        __builtin_amdgcn_sched_barrier(0);                                                                                          \
        _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                                               \
          _Pragma("unroll") for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[d][e], bq[q][e], acc[q], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                                                          \
        ar[d] = ap[(size_t)min(kg + PF, (KG) - 1) * 64];                                                                            \
        _Pragma("unroll") for (int q = 0; q < NQ; ++q) bq[q] = bqn[q];                                                              \
      }                                                                                                                             \
    }                                                                                                                               \
    __builtin_amdgcn_s_setprio(0);                                                                                                  \
  }

// index row of accumulator register r: sweep_row(sweep_rbase(tile, lane), r)
__device__ __forceinline__ int sweep_rbase(int tile, int lane) { return tile * 32 + 4 * (lane >> 5); }
__device__ __forceinline__ int sweep_row(int rbase, int r) { return rbase + (r & 3) + 8 * (r >> 2); }

// bit r: accumulator register r holds a row that exists (the tail tile)
__device__ __forceinline__ unsigned sweep_tail_rowmask(int rbase, int nlim) {
  unsigned m = 0u;
#pragma unroll
  for (int r = 0; r < 16; ++r) m |= (sweep_row(rbase, r) < nlim) ? (1u << r) : 0u;
  return m;
}

// row appended to column pr's buffer; the count runs on past cap (the caller's overflow mark).  !keep: counted, not stored
__device__ __forceinline__ void sweep_append(int32_t *cnt, int32_t *buf, int cap, int pr, int row, bool keep = true) {
  const int pos = atomicAdd(cnt + pr, 1);
  if (pos < cap && keep) buf[(size_t)pr * cap + pos] = row;
}

// 1, 2, 4, 8 or a multiple of 8: what sweep_decode and sweep_grid take
inline bool sweep_nsplit_ok(int NSPLIT) { return NSPLIT > 8 ? (NSPLIT & 7) == 0 : (NSPLIT >= 1 && 8 % NSPLIT == 0); }

inline int sweep_grid(int P, int NQ, int NSPLIT) {
  const int QB = (P + NQ * 32 - 1) / (NQ * 32);
  if (NSPLIT > 8) return QB * NSPLIT;
  const int per = 8 / NSPLIT;
  return (QB + per - 1) / per * 8;
}

inline size_t sweep_lds_bytes(int NQ, int KG) { return (size_t)NQ * KG * 256 * sizeof(float); }

// one sweep kernel over P columns in blocks of NQ x 32; args = the kernel's arguments
template <class Kernel, class... Args>
static hipError_t launch_sweep(Kernel kernel, int P, int NQ, int KG, int NSPLIT, size_t lds_max, hipStream_t st, const Args &...args) {
  const size_t lds = sweep_lds_bytes(NQ, KG);
  if (lds > lds_max) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(sweep_grid(P, NQ, NSPLIT)), dim3(SWEEP_THREADS), lds, st, args...);
  return hipGetLastError();
}
