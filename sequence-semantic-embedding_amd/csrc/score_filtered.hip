// Exact top-k among tag-eligible index rows for gfx950 (MI355X): sse_score_topk_filtered*.
//
// The reference ranks every target of a query (sse_evaluator.py:110-112, data_utils.py:263-267) and leaves "only the leaves
// under this meta-category", "not the labelled positives" or "not the row itself" to a filter of the sorted row on the host.
// Here the filter is inside the sweep and the threshold comes from eligible rows only (DESIGN K6g).  The stages are those of
// score_eligible.h; this call adds:
//   1. eligible_sweep_kernel<NQ, FilteredMaxStage>: the plain running maxima (tag-ineligible rows and the zero padding of the
//      tail tile count as -inf).  Exclusion lists play no part here.
//   2. filtered_threshold_kernel: theta = the (k + n_excl)-th largest maximum (-inf with fewer finite ones).  k + n_excl
//      distinct tag-eligible rows have an fp32 score >= theta and at most n_excl of them are excluded, so k eligible rows
//      have score64 >= theta - e, so has the k-th best eligible row, and every row of the exact answer has an fp32 score
//      >= theta - 2 e (e = eps32 |q| (1 + 2^-20), the bound of score_rank.hip, rounded outward).
//   3. eligible_sweep_kernel<NQ, FilteredCollectStage>: every tag-eligible row at or above that.
//   4. eligible_select_kernel<FilteredSelect>: the excluded ids dropped before the re-scoring.
// and the tile summaries of the tile skip (tag_tile_summary_kernel).
#include "score_eligible.h"

__global__ void tag_tile_summary_kernel(const uint64_t *tags, int64_t NT, uint64_t *tile_sum) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= NT) return;
  uint64_t s = 0;
  for (int i = 0; i < 32; ++i) s |= tags[t * 32 + i];
  tile_sum[t] = s;
}
hipError_t launch_tag_tile_summary(const uint64_t *tags, int64_t NT, uint64_t *tile_sum, hipStream_t st) {
  if (NT <= 0) return hipSuccess;
  hipLaunchKernelGGL(tag_tile_summary_kernel, dim3((int)((NT + 255) / 256)), dim3(256), 0, st, tags, NT, tile_sum);
  return hipGetLastError();
}

// one workgroup per query: collect threshold from the (k + n_excl)-th largest of its NV maxima
__global__ __launch_bounds__(256) void filtered_threshold_kernel(FilteredArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t th_key[];  // [NV]
  __shared__ double s_qn[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  ft_qnorm2_parts(a, p, tid, s_qn);
  for (int c = tid; c < a.NV; c += 256) th_key[c] = a.maxima[(size_t)p * a.NV + c];
  ft_sort_u32(th_key, a.NV, tid, 256);
  if (tid == 0) a.thr[p] = ft_collect_threshold(th_key, a.NV, a.k + a.n_excl, ft_score_bound(a.eps32, s_qn));
}

// excluded ids are not re-scored (nor is a wave's group of four none of whose rows is used)
struct FilteredSelect : PlainSelect {
  struct Query {
    const int64_t *ex;
    int n_excl;
  };
  static __device__ __forceinline__ Query query(const Args &g, int p) {
    return Query{g.f.excl ? g.f.excl + (size_t)p * g.f.n_excl : nullptr, g.f.excl ? g.f.n_excl : 0};
  }
  static __device__ __forceinline__ bool use_row(const Query &q, int64_t id, int lane) { return !ft_excluded(q.ex, q.n_excl, id, lane); }
};

hipError_t launch_score_filtered(const FilteredArgs &a, hipStream_t st) {
  if (a.P <= 0) return hipSuccess;
  if (!eligible_args_ok(a, true)) return hipErrorInvalidValue;
  if (a.k < 1 || a.k > SSE_FILTERED_MAX_K || a.n_excl < 0 || a.n_excl > SSE_FILTERED_MAX_EXCL) return hipErrorInvalidValue;
  hipError_t e = launch_eligible_sweep<FilteredMaxStage>({a}, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(filtered_threshold_kernel, dim3(a.P), dim3(256), (size_t)a.NV * sizeof(uint32_t), st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_eligible_sweep<FilteredCollectStage>({a}, st);
  if (e != hipSuccess) return e;
  return launch_eligible_select<FilteredSelect>({a}, st);
}

// the max sweep alone (stage 1), for callers with a threshold stage of their own: sse_score_confusions (score_confusions.hip)
hipError_t launch_filtered_max(const FilteredArgs &a, hipStream_t st) {
  if (a.P <= 0) return hipSuccess;
  if (!eligible_args_ok(a, true)) return hipErrorInvalidValue;
  return launch_eligible_sweep<FilteredMaxStage>({a}, st);
}

// the collect sweep alone (stage 3), for callers with a threshold of their own: sse_score_topk_grouped (score_grouped.hip),
// sse_score_confusions
hipError_t launch_filtered_collect(const FilteredArgs &a, hipStream_t st) {
  if (a.P <= 0) return hipSuccess;
  if (!eligible_args_ok(a, false)) return hipErrorInvalidValue;
  return launch_eligible_sweep<FilteredCollectStage>({a}, st);
}
