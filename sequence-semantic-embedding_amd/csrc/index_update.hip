// In-place updates and appends of the resident scoring index (sse_index_update* / sse_index_append*, DESIGN K6n): memory-bound
// scatters over a row list (IndexRowList, sse_kernels.h) of M rows.  Cost O(M S) plus one pass over N floats for the norm
// maximum; nothing here walks the N x S index.  The tile-list forms of the bf16 converters stand beside the whole-index ones
// in score_topk.hip; the tag tile sums and max |bias| are re-formed by the setters' own kernels.
#include "sse_kernels.h"

static inline int upd_grid(int64_t items, int cap) {
  const int64_t b = (items + 255) / 256;
  return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

// one thread per id: inside [lo, hi) and above its predecessor
__global__ __launch_bounds__(256) void index_ids_check_kernel(const int64_t *__restrict__ ids, int64_t M, int64_t lo, int64_t hi,
                                                              int32_t *err) {
  bool bad = false;
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t id = ids[m];
    bad |= id < lo || id >= hi || (m > 0 && ids[m - 1] >= id);
  }
  if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(err, SSE_ERR_INDEX_IDS);
}

hipError_t launch_index_ids_check(const int64_t *ids, int64_t M, int64_t lo, int64_t hi, int32_t *err, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(index_ids_check_kernel, dim3(upd_grid(M, 1024)), dim3(256), 0, st, ids, M, lo, hi, err);
  return hipGetLastError();
}

// One thread per 16-byte piece (list entry m, piece q of KG * 2): 4 consecutive k of the row, zero past S, stored where
// pack_rows_vec_kernel stores it.  T = double: the row-major float64 image takes the values as they came and every fp32
// image (float) of them, as sse_index_upload_f64 forms them.  VEC: S % 4 == 0 and 16-byte aligned fp32 input.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void index_scatter_rows_kernel(IndexRowList rl, const T *__restrict__ rows, int S, int KG,
                                                                 int64_t total, f32x4 *__restrict__ idxp, float *__restrict__ idx_rm,
                                                                 double *__restrict__ idx64) {
  if (index_list_refused(rl)) return;
  const int Q4 = KG * 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / Q4;
    const int q = (int)(i % Q4), k0 = q * 4;
    const int64_t r = index_list_row(rl, m);
    const T *src = rows + (size_t)m * S + k0;
    f32x4 v = {0, 0, 0, 0};
    if constexpr (VEC) {
      if (k0 < S) v = *reinterpret_cast<const f32x4 *>(src);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k0 + e < S) {
          v[e] = (float)src[e];
          if constexpr (sizeof(T) == 8)
            if (idx64) idx64[(size_t)r * S + k0 + e] = src[e];
        }
    }
    idxp[((size_t)(r >> 5) * KG + (q >> 1)) * 64 + (q & 1) * 32 + (int)(r & 31)] = v;
    if (idx_rm && k0 < S) *reinterpret_cast<f32x4 *>(idx_rm + (size_t)r * S + k0) = v;  // (kept for S % 4 == 0 only)
  }
}

hipError_t launch_index_scatter_rows(const IndexRowList &l, const float *rows32, const double *rows64, int S, float *idxp,
                                     float *idx_rm, double *idx64, hipStream_t st) {
  const int KG = (S + 7) / 8;
  const int64_t total = l.M * KG * 2;
  if (total == 0) return hipSuccess;
  if (idx_rm && (S & 3)) return hipErrorInvalidValue;
  const dim3 grid(upd_grid(total, 16384)), block(256);
  f32x4 *out = reinterpret_cast<f32x4 *>(idxp);
  if (rows64)
    hipLaunchKernelGGL((index_scatter_rows_kernel<double, false>), grid, block, 0, st, l, rows64, S, KG, total, out, idx_rm, idx64);
  else if ((S & 3) == 0 && (reinterpret_cast<uintptr_t>(rows32) & 15) == 0)
    hipLaunchKernelGGL((index_scatter_rows_kernel<float, true>), grid, block, 0, st, l, rows32, S, KG, total, out, idx_rm, idx64);
  else
    hipLaunchKernelGGL((index_scatter_rows_kernel<float, false>), grid, block, 0, st, l, rows32, S, KG, total, out, idx_rm, idx64);
  return hipGetLastError();
}

// norm2[row] as pack_rows_vec_kernel forms it: 8 lanes per row, lane qq sums the pieces q = qq, qq + 8, ... of the KG * 2
// (the zero padding included), then the three-step butterfly
__global__ __launch_bounds__(256) void index_row_norms_vec_kernel(IndexRowList rl, const f32x4 *__restrict__ idxp, int KG,
                                                                  int64_t groups, float *__restrict__ norm2) {
  if (index_list_refused(rl)) return;
  const int lane = threadIdx.x & 63, rs = lane >> 3, qq = lane & 7;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int Q4 = KG * 2;
  for (int64_t g = wave0; g < groups; g += nwaves) {
    const int64_t m = g * 8 + rs;
    const bool live = m < rl.M;
    const int64_t r = live ? index_list_row(rl, m) : 0;
    float ss = 0.0f;
    for (int q = qq; q < Q4; q += 8) {
      f32x4 v = {0, 0, 0, 0};
      if (live) v = idxp[((size_t)(r >> 5) * KG + (q >> 1)) * 64 + (q & 1) * 32 + (int)(r & 31)];
      ss = row_sumsq_add4(ss, v);
    }
    ss = row_sumsq_reduce8(ss);
    if (live && qq == 0) norm2[r] = ss;
  }
}

// norm2[row] as row_norm2_max_kernel_k forms it: one wave per row, lane c sums the elements c, c + 64, ...
__global__ __launch_bounds__(256) void index_row_norms_elem_kernel(IndexRowList rl, const float *__restrict__ idxp, int S, int KG,
                                                                   float *__restrict__ norm2) {
  if (index_list_refused(rl)) return;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t m = wave0; m < rl.M; m += nwaves) {
    const int64_t r = index_list_row(rl, m);
    const float *tile = idxp + (size_t)(r >> 5) * KG * 256 + (int)(r & 31) * 4;
    float ss = 0.0f;
    for (int c = lane; c < S; c += 64) ss = row_sumsq_add1(ss, tile[(c >> 3) * 256 + ((c >> 2) & 1) * 128 + (c & 3)]);
    ss = row_sumsq_reduce64(ss);
    if (lane == 0) norm2[r] = ss;
  }
}

hipError_t launch_index_row_norms(const IndexRowList &l, const float *idxp, int S, bool vec, float *norm2, hipStream_t st) {
  if (l.M <= 0) return hipSuccess;
  const int KG = (S + 7) / 8;
  if (vec) {
    const int64_t groups = (l.M + 7) / 8, blocks = (groups + 3) / 4;
    hipLaunchKernelGGL(index_row_norms_vec_kernel, dim3((int)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, l,
                       reinterpret_cast<const f32x4 *>(idxp), KG, groups, norm2);
  } else {
    const int64_t blocks = (l.M + 3) / 4;
    hipLaunchKernelGGL(index_row_norms_elem_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, l, idxp, S, KG,
                       norm2);
  }
  return hipGetLastError();
}

// max over the rows' sums (non-negative floats order as their bits; the maximum is order-free, as the pack's atomicMax is)
__global__ __launch_bounds__(256) void index_norm_max_kernel(const float *__restrict__ norm2, int64_t N, const int32_t *err,
                                                             unsigned *out) {
  if (err && (*err & SSE_ERR_INDEX_IDS)) return;
  float best = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) best = fmaxf(best, norm2[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(best));
}

hipError_t launch_index_norm_max(const float *norm2, int64_t N, const int32_t *err, float *out_bits, hipStream_t st) {
  if (N <= 0) return hipSuccess;
  hipLaunchKernelGGL(index_norm_max_kernel, dim3(upd_grid(N, 1024)), dim3(256), 0, st, norm2, N, err,
                     reinterpret_cast<unsigned *>(out_bits));
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void index_scatter_cols_kernel(IndexRowList rl, const uint64_t *__restrict__ tags_in,
                                                                 uint64_t *__restrict__ tags, const int64_t *__restrict__ groups_in,
                                                                 int64_t *__restrict__ groups, const float *__restrict__ bias_in,
                                                                 float *__restrict__ bias) {
  if (index_list_refused(rl)) return;
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < rl.M; m += (int64_t)gridDim.x * 256) {
    const int64_t r = index_list_row(rl, m);
    if (tags_in) tags[r] = tags_in[m];
    if (groups_in) groups[r] = groups_in[m];
    if (bias_in) bias[r] = bias_in[m];
  }
}

hipError_t launch_index_scatter_cols(const IndexRowList &l, const uint64_t *tags_in, uint64_t *tags, const int64_t *groups_in,
                                     int64_t *groups, const float *bias_in, float *bias, hipStream_t st) {
  if (l.M <= 0 || (!tags_in && !groups_in && !bias_in)) return hipSuccess;
  hipLaunchKernelGGL(index_scatter_cols_kernel, dim3(upd_grid(l.M, 1024)), dim3(256), 0, st, l, tags_in, tags, groups_in, groups,
                     bias_in, bias);
  return hipGetLastError();
}
