// Exact next page after a (score, id) cursor for gfx950 (MI355X): sse_score_topk_after*.
//
// The reference ranks every target of a query and cuts the sorted row on the host (sse_evaluator.py:110-112,
// webserver.py:144-151: [:nbest]); what follows the rows a caller already holds is another cut of the same row.  Here row r is
// AFTER the cursor (cs, cid) of a query iff score64 < cs, or score64 == cs and id_base + r > cid, and the answer is the best k
// tag-eligible rows after it (DESIGN K6j).  The eligibility depends on the score itself, which the fp32 sweep knows to within
// e = eps32 |q| (1 + 2^-20) only: it brackets the cursor and leaves the rows inside the bracket to float64.  The stages are
// those of score_eligible.h; this call adds:
//   0. after_bounds_kernel: e, lo = rd(cs - e), hi = ru(cs + e) per query.  fp32 score < lo: certainly after; > hi: certainly
//      not.  cs = +inf (or no cursor): lo = hi = +inf, every finite score is below lo.  cs = -inf: nothing is below lo or at
//      most hi.  cs = NaN: every comparison is false.  No special cases.
//   1. eligible_sweep_kernel<NQ, AfterMaxStage>: the maxima taken over the tag-eligible rows with fp32
//      score < lo only.
//   2. after_threshold_kernel: theta = the k-th largest maximum (-inf with fewer than k finite ones).  k distinct eligible rows
//      are certainly after the cursor with an fp32 score >= theta, so with score64 >= theta - e: so has the k-th answer row,
//      and every answer row has an fp32 score >= theta - 2 e.
//   3. eligible_sweep_kernel<NQ, AfterCollectStage>: every tag-eligible row with rd(theta - 2 e) <= fp32
//      score <= hi.  An answer row is after the cursor: score64 <= cs, fp32 score <= cs + e <= hi.
//   4. eligible_select_kernel<AfterSelect>: the re-scored rows that are not after the cursor dropped on (score64, id), in
//      the buffer and in the float64 sweep of the whole index alike.
// No row before the cursor is returned: stage 4 alone decides, in float64.  No answer row is missed: see 2. and 3.
#include "score_eligible.h"

// one workgroup per query: |q|, e and the fp32 bracket of the cursor score
__global__ __launch_bounds__(256) void after_bounds_kernel(AfterArgs g) {
  __shared__ double s_qn[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  ft_qnorm2_parts(g.f, p, tid, s_qn);
  __syncthreads();
  if (tid == 0) {
    const double e = ft_score_bound(g.f.eps32, s_qn);
    const double cs = g.after_score ? g.after_score[p] : (double)__builtin_inff();
    g.eb[p] = e;
    g.lo[p] = __double2float_rd(cs - e);
    g.hi[p] = __double2float_ru(cs + e);
  }
}

// after max: the running maxima of FilteredMaxStage over the eligible rows with score < top = lo only
struct AfterMaxStage : FilteredMaxStage {
  typedef AfterArgs Args;
  static constexpr bool COUNT_SKIPS = false;
  struct Col : FilteredMaxStage::Col {
    float top;
  };
  static __device__ __forceinline__ void init(Col &c, const Args g, int pr, bool live) {
    c.top = live ? g.lo[pr] : -__builtin_inff();
    FilteredMaxStage::init(c, {g.f}, pr, live);
  }
  static __device__ __forceinline__ bool admits(const Col &c, float x) { return x < c.top; }
  static __device__ __forceinline__ Slot *slots(const Args g) { return g.f.maxima; }
};

// after collect: eligible rows with thr <= score <= top = hi
struct AfterCollectStage {
  typedef AfterArgs Args;
  static constexpr bool COLLECT = true, COUNT_SKIPS = false, BIASED = false;
  static constexpr int MAX_NQ = 4;
  struct Col {
    float thr, top;
  };
  static __device__ __forceinline__ void init(Col &c, const Args g, int pr, bool live) {
    c.thr = live ? g.f.thr[pr] : __builtin_inff();
    c.top = live ? g.hi[pr] : -__builtin_inff();
  }
  static __device__ __forceinline__ bool take(const Col &c, float x) { return x >= c.thr && x <= c.top; }
};

// one workgroup per query: collect threshold from the k-th largest of its NV maxima
__global__ __launch_bounds__(256) void after_threshold_kernel(AfterArgs g) {
  extern __shared__ __attribute__((aligned(16))) uint32_t at_key[];  // [NV]
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < a.NV; c += 256) at_key[c] = a.maxima[(size_t)p * a.NV + c];
  ft_sort_u32(at_key, a.NV, tid, 256);
  if (tid == 0) a.thr[p] = ft_collect_threshold(at_key, a.NV, a.k, g.eb[p]);
}

// is (score64, id) after the cursor?  IEEE comparisons: a NaN cursor score has nothing after it
__device__ __forceinline__ bool af_after(double sc, int64_t id, double cs, int64_t cid) { return sc < cs || (sc == cs && id > cid); }

// rows not after the cursor are dropped on (score64, id); counters[0] receives the number collected
struct AfterSelect : PlainSelect {
  typedef AfterArgs Args;
  static constexpr bool COUNT_COLLECTED = true;
  struct Query {
    bool cursor;
    double cs;
    int64_t cid;
  };
  static __device__ __forceinline__ Query query(const Args &g, int p) {
    const bool cursor = g.after_score != nullptr;
    return Query{cursor, cursor ? g.after_score[p] : 0.0, cursor ? g.after_id[p] : 0};
  }
  static __device__ __forceinline__ bool keep(const Query &q, double sc, int64_t id) { return !q.cursor || af_after(sc, id, q.cs, q.cid); }
};

hipError_t launch_score_after(const AfterArgs &g, hipStream_t st) {
  const FilteredArgs &a = g.f;
  if (a.P <= 0) return hipSuccess;
  if (!eligible_args_ok(a, true)) return hipErrorInvalidValue;
  if (a.k < 1 || a.k > SSE_AFTER_MAX_K || a.n_excl != 0 || a.excl) return hipErrorInvalidValue;
  if ((g.after_score == nullptr) != (g.after_id == nullptr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(after_bounds_kernel, dim3(a.P), dim3(256), 0, st, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_eligible_sweep<AfterMaxStage>(g, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(after_threshold_kernel, dim3(a.P), dim3(256), (size_t)a.NV * sizeof(uint32_t), st, g);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_eligible_sweep<AfterCollectStage>(g, st);
  if (e != hipSuccess) return e;
  return launch_eligible_select<AfterSelect>(g, st);
}
