// x-projection table of lstm_fwd_kernel's table path (DESIGN.md "K2", x table).
//
// Each step's gate GEMM of the inference encoder is [x_t | 1 | h_{t-1}] . Wp, accumulated x k-groups first, then h
// k-groups, from 0.  The x part (embedding row + the constant-1 bias column) depends only on the token id and the weights,
// not on the row or the step, so the accumulators after the KGx x k-groups are computed once per token here and the
// recurrence starts its k loop at the h part from them.
//
// Bit-identical by construction: the same instruction (v_mfma_f32_32x32x2_f32 in the inference orientation: weight tile
// = A operand, sequences = B operand), the same packed weight fragments and the same embedding values in the same k
// order and operand slots as lstm_fwd.hip's gemm_pass; an output column of the MFMA depends only on its own B column, so
// putting 32 TOKENS in the columns instead of 32 sequences gives every sequence's x part bit for bit.
//
// Layout: table[v][ub][gate][lane >> 5][16] fp32 -- the 16 accumulator registers a lane of the recurrence that owns a
// sequence holding token v reads for one gate tile of unit block ub (64 contiguous bytes).
#include "sse_kernels.h"

size_t lstm_xtable_floats(int64_t V, int UBt) { return (size_t)V * UBt * 4 * 32; }

// one workgroup per (32 tokens, unit block), wave q = gate q
__global__ __launch_bounds__(256) void lstm_xtable_kernel(const float *__restrict__ emb, const float *Wp, int64_t V, int Ep,
                                                          int KGx, int KGh, int UBt, float *__restrict__ table) {
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, ub = blockIdx.y;
  const int64_t v = (int64_t)blockIdx.x * 32 + (lane & 31);
  const int half = lane >> 5;
  const float *xrow = emb + (size_t)(v < V ? v : V - 1) * Ep + half * 4;  // this lane's k half of the token's row
  const int KG = KGx + KGh;
  const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Wp), 0, (KGh / 4) * KG * 4096, 0x00020000);
  const int soff = __builtin_amdgcn_readfirstlane(ub * KG * 4096 + q * 1024);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int kg = 0; kg < KGx; ++kg) {
    const f32x4 w = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wr, lane * 16, soff + kg * 4096, 0));
    const f32x4 x = *reinterpret_cast<const f32x4 *>(xrow + kg * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], x[e], acc, 0, 0, 0);
  }
  if (v >= V) return;
  float *dst = table + (((size_t)v * UBt + ub) * 4 + q) * 32 + half * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<f32x4 *>(dst + 4 * i) = f32x4{acc[4 * i], acc[4 * i + 1], acc[4 * i + 2], acc[4 * i + 3]};
}

hipError_t launch_lstm_xtable(const float *emb, const float *Wp, int64_t V, int Ep, int KGx, int KGh, int UBt, float *table,
                              hipStream_t stream) {
  if (V <= 0 || KGx <= 0 || Ep < KGx * 8 || UBt <= 0 || UBt > KGh / 4 || (V + 31) / 32 > 0x7fffffff) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lstm_xtable_kernel, dim3((unsigned)((V + 31) / 32), UBt), dim3(256), 0, stream, emb, Wp, V, Ep, KGx, KGh,
                     UBt, table);
  return hipGetLastError();
}
