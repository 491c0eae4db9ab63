// Exact top-k DISTINCT GROUPS of index rows for gfx950 (MI355X): sse_score_topk_grouped*.
//
// Several index rows may stand for one thing: the labelled example titles of a leaf category (reference README: "one or
// multiples of the 20,000+ leaf categories"), the listings of one product.  Every row carries an int64 group key
// (sse_index_set_groups); the answer of a query is the k best groups, each represented by its best tag-eligible row (the
// lowest id among equal bests).  The stages are those of score_eligible.h with a threshold from distinct groups (DESIGN K6h);
// this call adds:
//   1. eligible_sweep_kernel<NQ, GroupedMaxStage>: beside each of its 16 running maxima a lane keeps the
//      TILE the maximum came from (register and lane fix the row inside the tile).  A slot holds (order-preserving key of the
//      fp32 score) << 32 | shard-local row: plain stores where a split owns its slots, 64-bit atomicMax where splits fold.
//      NQ <= 2: the sixteen tile numbers per query tile do not fit beside NQ = 4's accumulators.
//   2. grouped_threshold_kernel: groups[row] of every finite maximum, the entries sorted by (group, key descending), the
//      first entry of each group kept: theta = the k-th largest of those (-inf with fewer than k distinct groups).
//   3. the collect sweep of score_filtered.hip, unchanged (launch_filtered_collect).
//   4. eligible_select_kernel<GroupedSelect>: a group beside every entry and gp_reduce as the reduction: one entry per
//      group (best score, lowest row among equals), min(k, groups) entries out with their groups (padding INT64_MAX).  In the
//      float64 sweep of the whole index the k-th group's entry is the bar later rows have to pass.
// Exactness: k distinct groups each own a row with fp32 score >= theta, so k groups have a group score64 >= theta - e and so
// has the k-th best group.  The representative of every answer group has score64 >= theta - e, hence fp32 >= theta - 2 e: it
// is collected, and being its group's best eligible row it is what the reduction keeps for the group.  A group seen only
// through rows that are not its best has a true score below theta - e and is understated: it ranks behind the k answer groups.
#include "score_eligible.h"

// grouped max: the maxima of FilteredMaxStage, strict, with the tile of every maximum; a slot holds key << 32 | row
struct GroupedMaxArgs {
  FilteredArgs f;
  unsigned long long *maxima64;
};
struct GroupedMaxStage : FilteredMaxStage {
  typedef GroupedMaxArgs Args;
  static constexpr bool COUNT_SKIPS = false, KEEP_TILE = true;
  static constexpr int MAX_NQ = 2;
  typedef unsigned long long Slot;
  struct Col : FilteredMaxStage::Col {
    int mt[16];  // tile of mx[r]
  };
  static __device__ __forceinline__ void init(Col &c, const Args g, int pr, bool live) {
    FilteredMaxStage::init(c, {g.f}, pr, live);
#pragma unroll
    for (int r = 0; r < 16; ++r) c.mt[r] = 0;
  }
  static __device__ __forceinline__ Slot *slots(const Args g) { return g.maxima64; }
  static __device__ __forceinline__ Slot slot(const Col &c, int r, int lane) {
    const uint32_t row = (uint32_t)sweep_row(sweep_rbase(c.mt[r], lane), r);
    return ((Slot)ft_key(c.mx[r]) << 32) | row;  // (-inf: FT_KEY_NINF, the row unused)
  }
};

// bitonic sort of n2 (power of two) maxima in LDS by (group ascending, key descending)
__device__ __forceinline__ void gp_sort_maxima(unsigned long long *grp, uint32_t *key, int n2, int tid) {
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (n2 >> 1); i += 256) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool asc = ((lo & size) == 0);
        const unsigned long long gx = grp[lo], gy = grp[hi];
        const uint32_t x = key[lo], y = key[hi];
        const bool x_after_y = (gx > gy) || (gx == gy && x < y);
        if (x_after_y == asc) {
          grp[lo] = gy;
          grp[hi] = gx;
          key[lo] = y;
          key[hi] = x;
        }
      }
    }
  __syncthreads();
}

// one workgroup per query: collect threshold from the k-th largest of the per-group bests among its NV maxima
__global__ __launch_bounds__(256) void grouped_threshold_kernel(FilteredArgs a, const unsigned long long *maxima64, const int64_t *groups) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long gt_smem[];
  __shared__ double s_qn[4];
  unsigned long long *sgrp = gt_smem;                           // [NV]
  uint32_t *skey = reinterpret_cast<uint32_t *>(gt_smem + a.NV);  // [NV]
  const int p = blockIdx.x, tid = threadIdx.x;
  ft_qnorm2_parts(a, p, tid, s_qn);
  for (int c = tid; c < a.NV; c += 256) {
    const unsigned long long m = maxima64[(size_t)p * a.NV + c];
    const uint32_t key = (uint32_t)(m >> 32), row = (uint32_t)m;
    const bool real = key > FT_KEY_NINF && (int64_t)row < a.N;  // (an empty slot, a maximum of -inf: no row)
    skey[c] = real ? key : 0u;
    sgrp[c] = real ? (unsigned long long)groups[row] : 0ull;
  }
  gp_sort_maxima(sgrp, skey, a.NV, tid);
  // the best entry of a group is the first of its run; the others leave (key 0 is below every real key)
  bool head[16];  // (NV <= FT_MAXSPLIT * 256 = 16 * 256)
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = tid + j * 256;
    head[j] = c < a.NV && (c == 0 || sgrp[c - 1] != sgrp[c]);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = tid + j * 256;
    if (c < a.NV && !head[j]) skey[c] = 0u;
  }
  ft_sort_u32(skey, a.NV, tid, 256);
  if (tid == 0) a.thr[p] = ft_collect_threshold(skey, a.NV, a.k, ft_score_bound(a.eps32, s_qn));
}

// bitonic sort of n2 (power of two) entries in LDS.  BY_GROUP: (group ascending, key descending, row ascending): the first
// entry of a group's run is its representative.  Otherwise (key descending, row ascending): the order of before().
template <bool BY_GROUP>
__device__ __forceinline__ void gp_sort_entries(unsigned long long *skey, int *srow, unsigned long long *sgrp, int n2, int tid) {
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < (n2 >> 1); i += 256) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool first = ((lo & size) == 0);
        const unsigned long long x = skey[lo], y = skey[hi], gx = sgrp[lo], gy = sgrp[hi];
        const int rx = srow[lo], ry = srow[hi];
        bool x_after_y = (x < y) || (x == y && rx > ry);
        if (BY_GROUP) x_after_y = (gx > gy) || (gx == gy && x_after_y);
        if (x_after_y == first) {
          skey[lo] = y;
          skey[hi] = x;
          srow[lo] = ry;
          srow[hi] = rx;
          sgrp[lo] = gy;
          sgrp[hi] = gx;
        }
      }
    }
  __syncthreads();
}

// The c entries of the LDS area reduced to one per group -- best key, lowest row among equal keys -- and sorted by before();
// returns the number of groups (uniform).  Every thread of the workgroup calls it; cap is a power of two >= c.
__device__ __forceinline__ int gp_reduce(unsigned long long *skey, int *srow, unsigned long long *sgrp, int c, int tid, int *s_heads) {
  int n2 = 1;
  while (n2 < c) n2 <<= 1;
  for (int i = c + tid; i < n2; i += 256) {
    skey[i] = 0ull;
    srow[i] = FT_PAD_ROW;
    sgrp[i] = 0ull;
  }
  if (tid == 0) *s_heads = 0;
  gp_sort_entries<true>(skey, srow, sgrp, n2, tid);
  int mine = 0;
  for (int i = tid; i < n2; i += 256) {  // (reads the neighbour's group only, which nobody writes here)
    // a padding entry (key 0) follows the real entries of group 0 and never stands for a group
    const bool real = srow[i] != FT_PAD_ROW;
    const bool head = real && (i == 0 || sgrp[i - 1] != sgrp[i]);
    if (real && !head) {
      skey[i] = 0ull;
      srow[i] = FT_PAD_ROW;
    }
    mine += head ? 1 : 0;
  }
  if (mine) atomicAdd(s_heads, mine);
  gp_sort_entries<false>(skey, srow, sgrp, n2, tid);  // (starts with a barrier: the marks and the count are in place)
  return *s_heads;
}

// every entry carries its row's group; the area is reduced to one entry per group
struct GroupedSelectArgs {
  FilteredArgs f;
  const int64_t *groups;
  int64_t *out_groups;
};
struct GroupedSelect : PlainSelect {
  typedef GroupedSelectArgs Args;
  static constexpr bool GROUPED = true;
  static __device__ __forceinline__ int reduce(unsigned long long *skey, int *srow, unsigned long long *sgrp, int c, int tid, int *s_heads) {
    return gp_reduce(skey, srow, sgrp, c, tid, s_heads);
  }
};

hipError_t launch_score_grouped(const GroupedArgs &g, hipStream_t st) {
  const FilteredArgs &m = g.max, &c = g.rest;
  if (c.P <= 0) return hipSuccess;
  if (!g.groups || !g.maxima64 || !g.out_groups || m.P != c.P || m.k != c.k) return hipErrorInvalidValue;
  if (c.col_cap != SSE_COLLECT_CAP || c.k < 1 || c.k > SSE_GROUPED_MAX_K) return hipErrorInvalidValue;
  if (!eligible_args_ok(m, true)) return hipErrorInvalidValue;
  hipError_t e = launch_eligible_sweep<GroupedMaxStage>(GroupedMaxArgs{m, g.maxima64}, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grouped_threshold_kernel, dim3(m.P), dim3(256), (size_t)m.NV * (sizeof(unsigned long long) + sizeof(uint32_t)), st,
                     m, g.maxima64, g.groups);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_filtered_collect(c, st);
  if (e != hipSuccess) return e;
  return launch_eligible_select<GroupedSelect>(GroupedSelectArgs{c, g.groups, g.out_groups}, st);
}
