// The confusions of a training source for gfx950 (MI355X): sse_score_confusions*.
//
// The reference declares get_hard_learning_train_batch and compute_training_confusion_sampes and leaves both empty
// (data.py:124-129); its negatives are uniform draws (data.py:108-114).  A hard negative is a target that is not verified for
// the source and scores near or above the best verified one.  With P(q) the in-range positives of a query, (m, b) the first of
// {(score64(q, p), p)} in the order of before() and f = m - margin, row r is a CONFUSION of q iff id_base + r is not in P(q)
// and score64(q, r) >= f; the answer is the best k of them (DESIGN K6k).  The stages are those of score_eligible.h, run
// without tags; this call adds:
//   0. confusion_floor_kernel: |q| and e, the float64 dot of q with every in-range positive (wave_exact_dot: the bits
//      sse_score_topk returns), their reduction to (m, b), f and flo = rd(f - e).  No positive in range or margin = +inf:
//      f = flo = -inf, no cut.
//   1. eligible_sweep_kernel<NQ, FilteredMaxStage>: the plain running maxima.  Positives play no part here.
//   2. confusion_threshold_kernel: theta = the (k + n_pos)-th largest maximum, thr = max(rd(theta - 2 e), flo).  Every answer
//      row has score64 >= f, hence an fp32 score >= f - e >= flo; and it is one of the best k non-positives, which the
//      argument of the filtered call (score_filtered.hip, 2.) puts at or above rd(theta - 2 e).
//   3. eligible_sweep_kernel<NQ, FilteredCollectStage>: every row at or above thr.
//   4. eligible_select_kernel<ConfusionSelect>: the positives dropped before the re-scoring, score64 < f after it, in the
//      buffer and in the float64 sweep of the whole index alike.
// Only stage 4 decides membership, in float64: flo merely bounds what is collected.
#include "score_eligible.h"

// one workgroup per query: e, the best positive (m, b) in float64, f = m - margin, flo = rd(f - e)
__global__ __launch_bounds__(256) void confusion_floor_kernel(ConfusionArgs g) {
  __shared__ double s_qn[4], s_m[4];
  __shared__ int64_t s_b[4];
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  ft_qnorm2_parts(a, p, tid, s_qn);
  const float *qrow = a.q + (size_t)p * a.S;
  const int64_t *pos = a.excl + (size_t)p * a.n_excl;
  double m = -(double)__builtin_inff();
  int64_t b = INT64_MAX;
  for (int j = w; j < a.n_excl; j += 4) {  // (wave-uniform)
    const int64_t id = pos[j];
    const uint64_t r = (uint64_t)id - (uint64_t)a.id_base;
    if (r >= (uint64_t)a.N) continue;  // padding, an id of another shard
    const double sc = wave_exact_dot(qrow, a.idxp, a.idx64, (int64_t)r, a.S, a.KG, lane);
    if (before(sc, id, m, b)) {
      m = sc;
      b = id;
    }
  }
  if (lane == 0) {
    s_m[w] = m;
    s_b[w] = b;
  }
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 4; ++i)
      if (before(s_m[i], s_b[i], m, b)) {
        m = s_m[i];
        b = s_b[i];
      }
    const double e = ft_score_bound(a.eps32, s_qn);
    const double f = m - g.margin;
    g.floor64[p] = f;
    g.flo[p] = __double2float_rd(f - e);
    if (g.out_pos_score) g.out_pos_score[p] = m;
    if (g.out_pos_id) g.out_pos_id[p] = b;
  }
}

// one workgroup per query: the filtered call's threshold from the (k + n_pos)-th largest of its NV maxima, raised to flo
__global__ __launch_bounds__(256) void confusion_threshold_kernel(ConfusionArgs g) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cf_key[];  // [NV]
  __shared__ double s_qn[4];
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x;
  ft_qnorm2_parts(a, p, tid, s_qn);
  for (int c = tid; c < a.NV; c += 256) cf_key[c] = a.maxima[(size_t)p * a.NV + c];
  ft_sort_u32(cf_key, a.NV, tid, 256);
  if (tid == 0) {
    const float thr = ft_collect_threshold(cf_key, a.NV, a.k + a.n_excl, ft_score_bound(a.eps32, s_qn));
    const float flo = g.flo[p];
    const bool floor_wins = flo > thr;  // (a NaN floor -- non-finite input, outside the claim -- never wins)
    a.thr[p] = floor_wins ? flo : thr;
    if (floor_wins) atomicAdd(a.counters + 2, 1ull);
  }
}

// positives are not re-scored; re-scored rows below the floor are dropped.  counters[0] receives the number collected
struct ConfusionSelect : PlainSelect {
  typedef ConfusionArgs Args;
  static constexpr bool COUNT_COLLECTED = true;
  struct Query {
    const int64_t *pos;
    int n_pos;
    double f;
  };
  static __device__ __forceinline__ Query query(const Args &g, int p) {
    return Query{g.f.excl + (size_t)p * g.f.n_excl, g.f.n_excl, g.floor64[p]};
  }
  static __device__ __forceinline__ bool use_row(const Query &q, int64_t id, int lane) { return !ft_excluded(q.pos, q.n_pos, id, lane); }
  static __device__ __forceinline__ bool keep(const Query &q, double sc, int64_t) { return sc >= q.f; }
};

hipError_t launch_score_confusions(const ConfusionArgs &g, hipStream_t st) {
  const FilteredArgs &a = g.f;
  if (a.P <= 0) return hipSuccess;
  if (!eligible_args_ok(a, true)) return hipErrorInvalidValue;
  if (a.k < 1 || a.k > SSE_CONFUSIONS_MAX_K || a.n_excl < 1 || a.n_excl > SSE_CONFUSIONS_MAX_POS || !a.excl) return hipErrorInvalidValue;
  if (a.tags || a.q_any || a.q_none || a.skip || !(g.margin > -(double)__builtin_inff())) return hipErrorInvalidValue;
  hipLaunchKernelGGL(confusion_floor_kernel, dim3(a.P), dim3(256), 0, st, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_filtered_max(a, st);  // (the filtered call's own two sweeps: score_filtered.hip holds their code)
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(confusion_threshold_kernel, dim3(a.P), dim3(256), (size_t)a.NV * sizeof(uint32_t), st, g);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_filtered_collect(a, st);
  if (e != hipSuccess) return e;
  return launch_eligible_select<ConfusionSelect>(g, st);
}
