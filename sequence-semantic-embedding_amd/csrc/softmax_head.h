// The pieces the two softmax loss heads are made of (inbatch_loss.hip: B x B, class_loss.hip: B x N), device side, each once.
// A head adds its own metadata, its admission rule (which walk entries are negatives of an own row), where the positive sits,
// and how it cuts its walk; everything numeric below is common, so that one fix reaches both objectives.
//
// No logit matrix exists.  The normalised operands are staged once, zero padded to 32 rows and 32 columns (smx_stage_rows), then
// every pass recomputes the 32 x 32 logit tiles on v_mfma_f32_32x32x2_f32 where it needs them (smx_logit_tile).  A tile is
// always formed with the OWN index on the lane and the WALK index in the 16 accumulator registers (A operand = walk rows,
// B operand = own rows): register r of lane l holds walk row mfma_row(r, l) against own row l & 31.  So
//   - a lane of a rows pass carries one row's running (max, sum) instead of sixteen (smx_update, smx_merge, smx_rows_reduce), and
//   - the gradient tile G, written over the accumulator, is already the A operand of the product that sums over the walk
//     index (SMX_GRAD_ACCUMULATE): register r of lane l holds walk row mfma_row(r, l), which is k = 0 for the lower lane half
//     and k = 1 (4 rows further) for the upper one; the B operand is row mfma_row(r, l) of the walked encodings, one float per
//     lane.  16 MFMAs, one per register, cover the 32 walk rows of the tile.
// The waves of a workgroup take walk tiles w, w + SMX_NW, ..; their partial results are added in wave order through LDS.  No
// order depends on anything but the shapes and there are no atomics: the same inputs give the same bits.  The expressions
// below reach the compiler as they are written (every function is inlined); reordering one changes those bits.
#pragma once
#include <cmath>

#include "sse_kernels.h"

constexpr int SMX_NW = 8;         // waves per workgroup
constexpr int SMX_ST = 4;         // 32-column tiles of S per gradient workgroup: 4 up to 128 staged columns, 8 above (half the
constexpr int SMX_ST_WIDE = 8;    // logit recomputation per column of S, for 64 more accumulator registers)
constexpr float SMX_NEG_INF = -INFINITY;

inline size_t smx_round32(int x) { return (size_t)round_up(x, 32); }                 // staged rows / columns
inline bool smx_wide(size_t Sp) { return Sp > 32 * SMX_ST; }                         // which gradient kernel
inline unsigned smx_s_tiles(size_t Sp) {                                             // gradient workgroups along S
  return smx_wide(Sp) ? (unsigned)((Sp + 32 * SMX_ST_WIDE - 1) / (32 * SMX_ST_WIDE)) : 1u;
}

// Staging and its backward take K rows of one wave together (the in-batch head its source and target row, the class head one
// row): the K rows' loads are in flight at once, where one row after the other waits for memory K times -- 0.4 us per kernel
// at the launch-bound batch sizes (profiles/loss_head_refactor.txt).
struct SmxStage {
  const float *x;  // in: the raw row [S]
  float *n;        // in: where the normalised row goes [Sp], zero padded
  float rn, clamped;  // out: 1 / norm; 1 when the sum of squares lies below the clamp of loss_kernel (train.hip), else 0
};

template <int K>
__device__ __forceinline__ void smx_stage_rows(SmxStage (&r)[K], int S, int Sp, int lane) {
  float ss[K];
#pragma unroll
  for (int k = 0; k < K; ++k) ss[k] = 0.0f;
  for (int d = lane; d < S; d += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) ss[k] += r[k].x[d] * r[k].x[d];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) ss[k] += __shfl_xor(ss[k], o);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    r[k].rn = 1.0f / sqrtf(fmaxf(ss[k], 1e-12f));
    r[k].clamped = ss[k] < 1e-12f ? 1.0f : 0.0f;
  }
  for (int d = lane; d < Sp; d += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) r[k].n[d] = d < S ? r[k].x[d] * r[k].rn : 0.0f;
  }
}

// l2_normalize backward: out = rn * (dn - n * (n . dn)), no n . dn term below the clamp (as loss_kernel)
struct SmxUnstage {
  const float *n, *dn;  // the normalised row and its gradient
  float rn, clamped;    // as smx_stage_rows left them
  float *out;           // the raw row's gradient [S]
};

template <int K>
__device__ __forceinline__ void smx_normalize_backward(const SmxUnstage (&r)[K], int S, int lane) {
  float p[K];
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] = 0.0f;
  for (int d = lane; d < S; d += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] += r[k].n[d] * r[k].dn[d];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] += __shfl_xor(p[k], o);
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
    if (r[k].clamped != 0.0f) p[k] = 0.0f;
  for (int d = lane; d < S; d += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) r[k].out[d] = r[k].rn * (r[k].dn[d] - r[k].n[d] * p[k]);
  }
}

// acc[r] = sum_k walk[wbase + mfma_row(r, lane)][k] * own[obase + (lane & 31)][k] over the Sp staged columns.  Lane (row, k half)
// reads one float4 of its row per 8 columns; component e of the two halves is the k pair of one MFMA (both operands permute k
// alike).  Every row read must exist (the staged row counts are multiples of 32) and is 16-byte aligned (Sp % 32 == 0).
__device__ __forceinline__ f32x16 smx_logit_tile(const float *__restrict__ walk, int wbase, const float *__restrict__ own, int obase, int Sp,
                                                 int lane) {
  const float *pa = walk + (size_t)(wbase + (lane & 31)) * Sp + 4 * (lane >> 5);
  const float *pb = own + (size_t)(obase + (lane & 31)) * Sp + 4 * (lane >> 5);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int s0 = 0; s0 < Sp; s0 += 32) {
    f32x4 av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = *reinterpret_cast<const f32x4 *>(pa + s0 + 8 * u);
      bv[u] = *reinterpret_cast<const f32x4 *>(pb + s0 + 8 * u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][e], bv[u][e], acc, 0, 0, 0);
  }
  return acc;
}

// (m, s), the running (max, sum of exp(. - max)) of a set of logits, takes in one more logit x
__device__ __forceinline__ void smx_update(float &m, float &s, float x) {
  if (x > m) {
    s = s * expf(m - x) + 1.0f;
    m = x;
  } else {
    s += expf(x - m);
  }
}

// (m, s) <- the pair of the union with a disjoint set (m2, s2); an empty set is (-inf, 0)
__device__ __forceinline__ void smx_merge(float &m, float &s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  if (M == SMX_NEG_INF) {
    s = 0.0f;
  } else {
    s = s * expf(m - M) + s2 * expf(m2 - M);
  }
  m = M;
}

// End of a rows pass (every thread of the workgroup calls it): each lane brings the (m, s) of the walk entries it admitted for
// own row lane & 31 and lpos, the positive's logit (-inf unless this lane met it).  The two lane halves of a row are merged,
// then the waves in wave order; true on lanes 0 .. 31 of wave 0, which then hold their row's result.
__device__ __forceinline__ bool smx_rows_reduce(float &m, float &s, float &lpos, int lane, int w) {
  __shared__ float sh_m[SMX_NW][32], sh_s[SMX_NW][32], sh_d[SMX_NW][32];
  smx_merge(m, s, __shfl_xor(m, 32), __shfl_xor(s, 32));
  lpos = fmaxf(lpos, __shfl_xor(lpos, 32));
  if (lane < 32) {
    sh_m[w][lane] = m;
    sh_s[w][lane] = s;
    sh_d[w][lane] = lpos;
  }
  __syncthreads();
  if (w != 0 || lane >= 32) return false;
  m = sh_m[0][lane];
  s = sh_s[0][lane];
  lpos = sh_d[0][lane];
  for (int ww = 1; ww < SMX_NW; ++ww) {
    smx_merge(m, s, sh_m[ww][lane], sh_s[ww][lane]);
    lpos = fmaxf(lpos, sh_d[ww][lane]);
  }
  return true;
}

// A row with label z, (m, s) over its admitted negatives and positive logit lpos: log-sum-exp, loss, accuracy
__device__ __forceinline__ void smx_row_close(float m, float s, float lpos, float z, float &lse, float &row_loss, float &row_acc) {
  const float M = fmaxf(m, lpos);
  const float tot = (m == SMX_NEG_INF ? 0.0f : s * expf(m - M)) + expf(lpos - M);
  const float l = M + logf(tot);
  lse = l;
  row_loss = z * (l - lpos);
  row_acc = (z != 0.0f && !(m > lpos)) ? 1.0f : 0.0f;
}

// G entry of an admitted (row, walk entry) with raw tile value g: coef (z * scale * inv_rows) * (softmax probability - 1 at the positive)
__device__ __forceinline__ float smx_grad_entry(float coef, float scale, float g, float lse, bool positive) {
  return coef * (expf(scale * g - lse) - (positive ? 1.0f : 0.0f));
}

template <int ST>
__device__ __forceinline__ void smx_grad_zero(f32x16 (&out)[ST]) {
#pragma unroll
  for (int t = 0; t < ST; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[t][r] = 0.0f;
}

// out[t] += G . (walk rows of one walk tile, columns 32 t .. 32 t + 31 of walk_tile), t < nst.  walk_tile: row 0 of the walk
// tile at the workgroup's first column of S; out: f32x16 [ST], g: f32x16.
// A macro, not a function: hipcc simplifies an inlined function on its own before it inlines it, and inbatch_grad_kernel<false, 4>
// then comes out with 170 registers instead of 168, which is one wave per SIMD less (profiles/loss_head_refactor.txt).
#define SMX_GRAD_ACCUMULATE(ST, out, g, walk_tile, Sp, nst, lane)                                                       \
  _Pragma("unroll") for (int t = 0; t < ST; ++t) {                                                                      \
    if (t < (nst)) {                                                                                                    \
      const float *pb = (walk_tile) + 32 * t + ((lane) & 31);                                                           \
      _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                                    \
        out[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], pb[(size_t)mfma_row(r, lane) * (Sp)], out[t], 0, 0, 0);     \
    }                                                                                                                   \
  }

// End of a gradient pass (every thread of the workgroup calls it): the waves' partial tiles are added in wave order, the sum
// goes to dst_tile[own row][32 t + column], t < nst.  dst_tile: own row 0 of the workgroup at its first column of S.
template <int ST>
__device__ __forceinline__ void smx_grad_reduce_store(const f32x16 (&out)[ST], float *__restrict__ dst_tile, int Sp, int nst, int lane, int w) {
  __shared__ float red[ST][16][64];
  for (int ww = 0; ww < SMX_NW; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int t = 0; t < ST; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[t][r][lane] = ww == 0 ? out[t][r] : red[t][r][lane] + out[t][r];
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < nst * 16 * 64; e += SMX_NW * 64) {
    const int t = e >> 10, r = (e >> 6) & 15, l = e & 63;
    dst_tile[(size_t)mfma_row(r, l) * Sp + 32 * t + (l & 31)] = red[t][r][l];
  }
}
