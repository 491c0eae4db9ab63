// The exchange block of an open train step (sse_train_pack_exchange / sse_train_backward_inbatch_global; layout: include/sse_hip.h):
// what one rank contributes to the global batch of a data-parallel in-batch softmax step, as ONE fixed-size run of 32-bit
// words, so that one all-gather moves it.  Token ids and row numbers travel as their bit patterns; nothing here does
// arithmetic on a word.
//   [ rows (int32), S, T, Tt | src raw (cap x S) | tgt raw (cap x S) | labels (cap) | src ids (cap x T) | tgt ids (cap x Tt) ]
#include "sse_kernels.h"

namespace {

struct ExchangeLayout {
  int cap, S, T, Tt;
  __host__ __device__ size_t src() const { return 4; }
  __host__ __device__ size_t tgt() const { return src() + (size_t)cap * S; }
  __host__ __device__ size_t labels() const { return tgt() + (size_t)cap * S; }
  __host__ __device__ size_t ids0() const { return labels() + (size_t)cap; }
  __host__ __device__ size_t ids1() const { return ids0() + (size_t)cap * T; }
  __host__ __device__ size_t floats() const { return ids1() + (size_t)cap * Tt; }
};

// one workgroup per row slot; slots B .. cap-1 are zeroed
__global__ __launch_bounds__(256) void exchange_pack_kernel(const float *__restrict__ src_raw, const float *__restrict__ tgt_raw,
                                                            const float *__restrict__ labels, const int32_t *__restrict__ ids0,
                                                            const int32_t *__restrict__ ids1, int B, ExchangeLayout L,
                                                            float *__restrict__ block) {
  const int r = blockIdx.x, t = threadIdx.x;
  const bool live = r < B;
  if (r == 0 && t < 4) block[t] = __int_as_float(t == 0 ? B : t == 1 ? L.S : t == 2 ? L.T : L.Tt);
  for (int d = t; d < L.S; d += 256) {
    block[L.src() + (size_t)r * L.S + d] = live ? src_raw[(size_t)r * L.S + d] : 0.0f;
    block[L.tgt() + (size_t)r * L.S + d] = live ? tgt_raw[(size_t)r * L.S + d] : 0.0f;
  }
  if (t == 0) block[L.labels() + r] = live ? labels[r] : 0.0f;
  for (int d = t; d < L.T; d += 256) block[L.ids0() + (size_t)r * L.T + d] = live ? __int_as_float(ids0[(size_t)r * L.T + d]) : 0.0f;
  for (int d = t; d < L.Tt; d += 256) block[L.ids1() + (size_t)r * L.Tt + d] = live ? __int_as_float(ids1[(size_t)r * L.Tt + d]) : 0.0f;
}

// one workgroup per global row g = row_off[rank] + local row: the `world` gathered blocks into contiguous arrays, rank order
__global__ __launch_bounds__(256) void exchange_compact_kernel(const float *__restrict__ gathered, const int32_t *__restrict__ row_off,
                                                               int world, ExchangeLayout L, float *__restrict__ src_raw,
                                                               float *__restrict__ tgt_raw, float *__restrict__ labels,
                                                               int32_t *__restrict__ ids0, int32_t *__restrict__ ids1) {
  const int g = blockIdx.x, t = threadIdx.x;
  int rank = 0;
  while (rank + 1 < world && row_off[rank + 1] <= g) ++rank;
  const int r = g - row_off[rank];
  if (r >= L.cap) return;  // (refused on the host: a rank never holds more than cap rows)
  const float *block = gathered + (size_t)rank * L.floats();
  for (int d = t; d < L.S; d += 256) {
    src_raw[(size_t)g * L.S + d] = block[L.src() + (size_t)r * L.S + d];
    tgt_raw[(size_t)g * L.S + d] = block[L.tgt() + (size_t)r * L.S + d];
  }
  if (t == 0) labels[g] = block[L.labels() + r];
  for (int d = t; d < L.T; d += 256) ids0[(size_t)g * L.T + d] = __float_as_int(block[L.ids0() + (size_t)r * L.T + d]);
  for (int d = t; d < L.Tt; d += 256) ids1[(size_t)g * L.Tt + d] = __float_as_int(block[L.ids1() + (size_t)r * L.Tt + d]);
}

__global__ void set_pair_kernel(float *dst, float a, float b) {
  dst[0] = a;
  dst[1] = b;
}

}  // namespace

size_t train_exchange_floats(int cap, int S, int T, int Tt) { return ExchangeLayout{cap, S, T, Tt}.floats(); }

hipError_t launch_train_exchange_pack(const float *src_raw, const float *tgt_raw, const float *labels, const int32_t *ids0,
                                      const int32_t *ids1, int B, int cap, int S, int T, int Tt, float *block, hipStream_t st) {
  hipLaunchKernelGGL(exchange_pack_kernel, dim3(cap), dim3(256), 0, st, src_raw, tgt_raw, labels, ids0, ids1, B,
                     ExchangeLayout{cap, S, T, Tt}, block);
  return hipGetLastError();
}

hipError_t launch_train_exchange_compact(const float *gathered, const int32_t *row_off, int world, int rows_global, int cap, int S, int T,
                                         int Tt, float *src_raw, float *tgt_raw, float *labels, int32_t *ids0, int32_t *ids1,
                                         hipStream_t st) {
  hipLaunchKernelGGL(exchange_compact_kernel, dim3(rows_global), dim3(256), 0, st, gathered, row_off, world, ExchangeLayout{cap, S, T, Tt},
                     src_raw, tgt_raw, labels, ids0, ids1);
  return hipGetLastError();
}

hipError_t launch_set_pair(float *dst, float a, float b, hipStream_t st) {
  hipLaunchKernelGGL(set_pair_kernel, dim3(1), dim3(1), 0, st, dst, a, b);
  return hipGetLastError();
}
