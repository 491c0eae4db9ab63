// Float64 scoring shared by the re-scoring passes (score_topk.hip) and the rank count (score_rank.hip): the dot product
// every float64 score of the library is formed with, and the order results are ranked by.  One definition, so that every
// pass returns the same bits for the same (query, row).
#pragma once
#include "sse_kernels.h"

// exact float64 scores of query row q against NB index rows n[0..NB) (frag32-packed f32 rows or row-major f64 rows),
// computed by one wave; results valid in every lane.  The rows' loads are independent and in flight together (a window of
// ~12 candidates re-scored one row at a time was a chain of 12 HBM round trips); every row's sum is formed in exactly the
// order of the single-row form below, which is this template with NB = 1: all passes produce bit-identical scores.
template <int NB>
__device__ __forceinline__ void wave_exact_dot_n(const float *qrow, const float *idxp, const double *idx64, const int64_t (&n)[NB],
                                                 int S, int KG, int lane, double (&out)[NB]) {
  double acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = 0.0;
  if (idx64) {
    for (int d = lane; d < S; d += 64) {
      double rv[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) rv[b] = idx64[(size_t)n[b] * S + d];
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[b] += (double)qrow[d] * rv[b];
    }
  } else {
    for (int j = lane; j < KG * 2; j += 64) {  // j = kg*2 + half -> 4 consecutive dims
      const int kg = j >> 1, half = j & 1;
      f32x4 v[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b)
        v[b] = *reinterpret_cast<const f32x4 *>(idxp + (size_t)(n[b] >> 5) * KG * 256 + kg * 256 + (half * 32 + (int)(n[b] & 31)) * 4);
      const int d0 = kg * 8 + half * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (d0 + e < S) {
#pragma unroll
          for (int b = 0; b < NB; ++b) acc[b] += (double)qrow[d0 + e] * (double)v[b][e];
        }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] += __shfl_xor(acc[b], o);
#pragma unroll
  for (int b = 0; b < NB; ++b) out[b] = acc[b];
}
__device__ __forceinline__ double wave_exact_dot(const float *qrow, const float *idxp, const double *idx64,
                                                 int64_t n, int S, int KG, int lane) {
  const int64_t nn[1] = {n};
  double out[1];
  wave_exact_dot_n<1>(qrow, idxp, idx64, nn, S, KG, lane, out);
  return out[0];
}

__device__ __forceinline__ bool before(double sa, int64_t ia, double sb, int64_t ib) {
  return (sa > sb) || (sa == sb && ia < ib);  // score descending, then lower row id
}
