// Exact top-k of cosine + per-row prior among tag-eligible index rows for gfx950 (MI355X): sse_score_topk_biased*.
//
// The reference ranks every target of a query by the bare dot product (sse_evaluator.py:110-112); an item prior, a class
// log-prior or the hubness correction of cross-lingual retrieval (CSLS: cos(x,t) - 0.5 r_S(t)) is a number per index row added
// to that score BEFORE the cut, which no re-ranking of an unbiased top-k can reproduce.  Here the biased score of row r for
// query p is
//   sb(p, r) = score64(p, r) + (double)w[p] * (double)bias[r]
// (both factors are floats: the product is exact in double, sb is rounded once, contraction to an fma cannot change it) and
// the answer is the best k tag-eligible rows by (sb descending, id ascending) (DESIGN K6l).  The stages are those of
// score_eligible.h, carried out on the biased fp32 value y = fmaf(w, bias[r], x), x the fp32 score of the sweep:
//   0. biased_bounds_kernel: e_b per query (below).
//   1. eligible_sweep_kernel<NQ, BiasedMaxStage>: the running maxima of y over the tag-eligible rows.
//   2. biased_threshold_kernel: theta = the k-th largest maximum (-inf with fewer than k finite ones).  k distinct eligible rows
//      have y >= theta, so sb >= theta - e_b: so has the k-th answer row, and every answer row has y >= theta - 2 e_b.
//   3. eligible_sweep_kernel<NQ, BiasedCollectStage>: every tag-eligible row with y >= rd(theta - 2 e_b).
//   4. eligible_select_kernel<BiasedSelect>: sb formed from the re-scored row before it is keyed, in the buffer and in the
//      float64 sweep of the whole index alike; the bar of the overflow path is a biased key.
//
// The bound.  Let s = score64 (taken as the exact dot product: its own rounding is inside e), m = |q| idx_norm_max >= |s|,
// B = |w| bias_absmax >= |w bias[r]|, and e = eps32 |q| (1 + 2^-20) >= |x - s| (score_rank.hip).
//   y = fmaf(w, b, x) rounds the exact x + w b once: |y - (x + w b)| <= 2^-24 |x + w b| <= 2^-24 (m + e + B)
//     (a subnormal y: <= 2^-150 instead).
//   sb rounds the exact s + w b once in float64: |sb - (s + w b)| <= 2^-53 (m + B).
//   idx_norm_max is the square root of an fp32 sum of squares: it may fall short of the largest norm by a factor
//     1 - S 2^-24 > 1 - 2^-10, which enlarges the m of the first line by less than 2^-9 m.
// So |y - sb| <= e + (2^-24 (1 + 2^-9) + 2^-53) (m + e + B) + 2^-150 < e + u (m + e + B) + 2^-149 with u = 2^-23, and
//   e_b = (e + u (|q| idx_norm_max + e + |w| bias_absmax) + 2^-149) (1 + 2^-20),
// the last factor over the float64 arithmetic of the bound itself (five operations of relative error 2^-53).  A large
// |w| bias_absmax widens the band and sends more rows to float64; the result stays exact.
#include "score_eligible.h"

// bias[N .. NT * 32) = 0; *absmax (float bits, zeroed by the caller) = max |bias[0 .. N)|: non-negative floats order as their bits
__global__ __launch_bounds__(256) void bias_prepare_kernel(float *bias, int64_t N, int64_t NP, unsigned *absmax) {
  float m = 0.0f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < NP; i += (int64_t)gridDim.x * 256) {
    if (i < N) m = fmaxf(m, fabsf(bias[i]));
    else bias[i] = 0.0f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(absmax, __float_as_uint(m));
}
hipError_t launch_bias_prepare(float *bias, int64_t N, int64_t NT, float *absmax, hipStream_t st) {
  if (NT <= 0) return hipSuccess;
  const int64_t blocks = (NT * 32 + 255) / 256;
  hipLaunchKernelGGL(bias_prepare_kernel, dim3((int)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, bias, N, NT * 32,
                     reinterpret_cast<unsigned *>(absmax));
  return hipGetLastError();
}

__device__ __forceinline__ float bs_weight(const BiasedArgs &g, int p) { return g.weight ? g.weight[p] : 1.0f; }

// one workgroup per query: |q| and e_b
__global__ __launch_bounds__(256) void biased_bounds_kernel(BiasedArgs g) {
  __shared__ double s_qn[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  ft_qnorm2_parts(g.f, p, tid, s_qn);
  __syncthreads();
  if (tid == 0) {
    const double e = ft_score_bound(g.f.eps32, s_qn);
    const double qn = sqrt(s_qn[0] + s_qn[1] + s_qn[2] + s_qn[3]);
    const double B = fabs((double)bs_weight(g, p)) * (double)g.bias_absmax[0];
    const double u = 1.0 / 8388608.0;  // 2^-23
    g.eb[p] = (e + u * (qn * (double)g.norm_max + e + B) + 1.4012984643248171e-45) * (1.0 + 1.0 / 1048576.0);
  }
}

// biased max: the running maxima of FilteredMaxStage over y
struct BiasedMaxStage : FilteredMaxStage {
  typedef BiasedArgs Args;
  static constexpr bool COUNT_SKIPS = false, BIASED = true;
  struct Col : FilteredMaxStage::Col {
    float w;
  };
  static __device__ __forceinline__ void init(Col &c, const Args g, int pr, bool live) {
    c.w = live ? bs_weight(g, pr) : 0.0f;
    FilteredMaxStage::init(c, {g.f}, pr, live);
  }
  static __device__ __forceinline__ Slot *slots(const Args g) { return g.f.maxima; }
};

// biased collect: eligible rows with y at or above thr
struct BiasedCollectStage {
  typedef BiasedArgs Args;
  static constexpr bool COLLECT = true, COUNT_SKIPS = false, BIASED = true;
  static constexpr int MAX_NQ = 4;
  struct Col {
    float thr, w;
  };
  static __device__ __forceinline__ void init(Col &c, const Args g, int pr, bool live) {
    c.thr = live ? g.f.thr[pr] : __builtin_inff();
    c.w = live ? bs_weight(g, pr) : 0.0f;
  }
  static __device__ __forceinline__ bool take(const Col &c, float y) { return y >= c.thr; }
};

// one workgroup per query: collect threshold from the k-th largest of its NV maxima
__global__ __launch_bounds__(256) void biased_threshold_kernel(BiasedArgs g) {
  extern __shared__ __attribute__((aligned(16))) uint32_t bt_key[];  // [NV]
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < a.NV; c += 256) bt_key[c] = a.maxima[(size_t)p * a.NV + c];
  ft_sort_u32(bt_key, a.NV, tid, 256);
  if (tid == 0) a.thr[p] = ft_collect_threshold(bt_key, a.NV, a.k, g.eb[p]);
}

// sb = score64 + (double)w * (double)bias[row]; a zero product leaves score64's bits alone (the filtered call's row)
struct BiasedSelect : PlainSelect {
  typedef BiasedArgs Args;
  static constexpr bool BIASED = true;
  struct Query {
    float w;
  };
  static __device__ __forceinline__ Query query(const Args &g, int p) { return Query{bs_weight(g, p)}; }
  static __device__ __forceinline__ double score(const Args &g, const Query &q, double sc, int64_t row) {
    const double add = (double)q.w * (double)g.bias[row];
    return add == 0.0 ? sc : sc + add;
  }
};

hipError_t launch_score_biased(const BiasedArgs &g, hipStream_t st) {
  const FilteredArgs &a = g.f;
  if (a.P <= 0) return hipSuccess;
  if (!eligible_args_ok(a, true)) return hipErrorInvalidValue;
  if (a.k < 1 || a.k > SSE_BIASED_MAX_K || a.n_excl != 0 || a.excl) return hipErrorInvalidValue;
  if (!g.bias || !g.bias_absmax || !g.eb) return hipErrorInvalidValue;
  hipLaunchKernelGGL(biased_bounds_kernel, dim3(a.P), dim3(256), 0, st, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_eligible_sweep<BiasedMaxStage>(g, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(biased_threshold_kernel, dim3(a.P), dim3(256), (size_t)a.NV * sizeof(uint32_t), st, g);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_eligible_sweep<BiasedCollectStage>(g, st);
  if (e != hipSuccess) return e;
  return launch_eligible_select<BiasedSelect>(g, st);
}
