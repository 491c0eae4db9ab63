// Forward-only pair loss for gfx950: what
//   session.run([model.loss, model.train_acc, binarylogit], feed)            (sse_model.py:290,298,302)
// computes WITHOUT model.train -- loss, binary accuracy and the cosine of every pair row of a held-out batch.  The two
// encoders run on the inference kernels (sse_api.hip: encode_dev_locked, un-normalised); the kernels here take their
// outputs to per-row values and the per-row values to three double sums.  Nothing is written that a train step owns.
#include "train.h"

#include "sse_kernels.h"

// ---------------------------------------------------------------------------
// Staging of the source side of a chunk: out[b][0..T) = rows ? corpus[rows[b * stride]][0..T) : ids[b * stride][0..T).
// stride = 2 is the de-duplicated paired batch (rows 2i, 2i + 1 share their source: one encoder row per pair).
// A row number outside [0, N) raises error flag bit 2 (as gather_id_rows_kernel does) and reads row 0.
__global__ void eval_stage_ids_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ rows, int stride, int B, int T,
                                      int64_t N, int32_t *__restrict__ out, int32_t *err) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= B) return;
  int64_t r = (int64_t)b * stride;
  if (rows) {
    r = rows[r];
    if (r < 0 || r >= N) {
      if (lane == 0) atomicOr(err, 2);
      r = 0;
    }
  }
  const int32_t *src = ids + (size_t)r * T;
  for (int t = lane; t < T; t += 64) out[(size_t)b * T + t] = src[t];
}

// ---------------------------------------------------------------------------
// One wave per pair row, as loss_kernel (train.hip), no gradients.
struct PairEvalArgs {
  const float *src_raw;      // [B >> src_shift][S] un-normalised source encodings of this chunk
  const float *tgt_raw;      // [B][S] un-normalised target encodings -- or, with tgt_rows, the free target matrix [N][S]
  const int32_t *tgt_rows;   // nullptr | [B] rows of the free target matrix
  const float *labels;       // [B]
  float *row_loss, *row_acc, *row_cos;  // [B], at the chunk's position in the whole call
  int32_t *err;
  int32_t B, S, N;
  int32_t src_shift;         // 1: paired batch, row b reads source row b >> 1
};

__global__ __launch_bounds__(256) void pair_eval_kernel(PairEvalArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= a.B) return;
  int64_t trow = row;
  bool ok = true;
  if (a.tgt_rows) {
    trow = a.tgt_rows[row];
    if (trow < 0 || trow >= a.N) {  // (the one atomic of this file: the error flag, never a result)
      if (lane == 0) atomicOr(a.err, 1);
      ok = false;
      trow = 0;
    }
  }
  const float *s = a.src_raw + (size_t)(row >> a.src_shift) * a.S, *t = a.tgt_raw + (size_t)trow * a.S;
  float ss = 0.0f, tt = 0.0f, st = 0.0f;
  for (int d = lane; d < a.S; d += 64) {
    const float x = s[d], y = ok ? t[d] : 0.0f;
    ss += x * x;
    tt += y * y;
    st += x * y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ss += __shfl_xor(ss, o);
    tt += __shfl_xor(tt, o);
    st += __shfl_xor(st, o);
  }
  if (lane != 0) return;
  const float rs = 1.0f / sqrtf(fmaxf(ss, 1e-12f)), rt = 1.0f / sqrtf(fmaxf(tt, 1e-12f));
  const float cosv = st * rs * rt;  // reduce_sum(ns * nt)
  const float x = 64.0f * cosv;
  const float z = a.labels[row];
  const float sg = sse_sigmoid(x);
  // weighted_cross_entropy_with_logits, pos_weight = 1; the accuracy of sse_model.py:302
  a.row_loss[row] = (1.0f - z) * x + log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.0f);
  a.row_acc[row] = z * floorf(sg + 0.1f) + (1.0f - z) * floorf(1.1f - sg);
  a.row_cos[row] = cosv;
}

// ---------------------------------------------------------------------------
// sums[3] = { sum row_loss, sum row_acc, B } in double: ONE workgroup, thread i adds rows i, i + 1024, ... in that order,
// then a fixed tree over the 1024 partial sums -- the order depends on B alone.
#define EVAL_REDUCE_THREADS 1024
__global__ __launch_bounds__(EVAL_REDUCE_THREADS) void eval_reduce_kernel(const float *__restrict__ row_loss,
                                                                          const float *__restrict__ row_acc, int64_t B,
                                                                          double *__restrict__ sums) {
  __shared__ double sl[EVAL_REDUCE_THREADS], sa[EVAL_REDUCE_THREADS];
  double l = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += EVAL_REDUCE_THREADS) {
    l += (double)row_loss[i];
    c += (double)row_acc[i];
  }
  sl[threadIdx.x] = l;
  sa[threadIdx.x] = c;
  __syncthreads();
  for (int o = EVAL_REDUCE_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sl[threadIdx.x] += sl[threadIdx.x + o];
      sa[threadIdx.x] += sa[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sums[0] = sl[0];
    sums[1] = sa[0];
    sums[2] = (double)B;
  }
}

hipError_t launch_eval_stage_ids(const int32_t *ids, const int32_t *rows, int stride, int B, int T, int64_t N, int32_t *out,
                                 int32_t *err, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(eval_stage_ids_kernel, dim3((B + 3) / 4), dim3(256), 0, st, ids, rows, stride, B, T, N, out, err);
  return hipGetLastError();
}

hipError_t launch_pair_eval(const float *src_raw, const float *tgt_raw, const int32_t *tgt_rows, int N, const float *labels,
                            float *row_loss, float *row_acc, float *row_cos, int32_t *err, int B, int S, int paired,
                            hipStream_t st) {
  if (B <= 0) return hipSuccess;
  PairEvalArgs a;
  a.src_raw = src_raw;
  a.tgt_raw = tgt_raw;
  a.tgt_rows = tgt_rows;
  a.labels = labels;
  a.row_loss = row_loss;
  a.row_acc = row_acc;
  a.row_cos = row_cos;
  a.err = err;
  a.B = B;
  a.S = S;
  a.N = N;
  a.src_shift = paired ? 1 : 0;
  hipLaunchKernelGGL(pair_eval_kernel, dim3((B + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_eval_reduce(const float *row_loss, const float *row_acc, int64_t B, double *sums, hipStream_t st) {
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(EVAL_REDUCE_THREADS), 0, st, row_loss, row_acc, B, sums);
  return hipGetLastError();
}
