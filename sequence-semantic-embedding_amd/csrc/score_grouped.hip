// Exact top-k DISTINCT GROUPS of index rows for gfx950 (MI355X): sse_score_topk_grouped*.
//
// Several index rows may stand for one thing: the labelled example titles of a leaf category (reference README: "one or
// multiples of the 20,000+ leaf categories"), the listings of one product.  Every row carries an int64 group key
// (sse_index_set_groups); the answer of a query is the k best groups, each represented by its best tag-eligible row (the
// lowest id among equal bests).  The stages are those of score_filtered.hip with a threshold from distinct groups (DESIGN K6h):
//   1. score_grouped_max_kernel<NQ>: the shared sweep (score_sweep.h), eligible maxima as score_filtered_kernel<NQ, false>; beside each of its 16 running
//      maxima a lane keeps the TILE the maximum came from (register and lane fix the row inside the tile).  A slot holds
//      (order-preserving key of the fp32 score) << 32 | shard-local row: plain stores where a split owns its slots, 64-bit
//      atomicMax where splits fold.  NQ <= 2: the sixteen tile numbers per query tile do not fit beside NQ = 4's accumulators.
//   2. grouped_threshold_kernel: groups[row] of every finite maximum, the entries sorted by (group, key descending), the
//      first entry of each group kept: theta = the k-th largest of those (-inf with fewer than k distinct groups).
//   3. the collect sweep of score_filtered.hip, unchanged: every tag-eligible row with fp32 score >= rd(theta - 2 e).
//   4. grouped_select_kernel: float64 scores (wave_exact_dot_n: score_topk's bits), one entry per group (best score, lowest
//      row among equals), sorted by before(), min(k, groups) entries out, padding (-inf, INT64_MAX, INT64_MAX), count.
//   5. a query whose buffer overflowed: a float64 sweep of the whole index in the same workgroup; the LDS area is reduced by
//      group whenever it fills and cut to the k best groups, whose last entry is the bar later rows have to pass.
// Exactness: k distinct groups each own a row with fp32 score >= theta, so k groups have a group score64 >= theta - e and so
// has the k-th best group.  The representative of every answer group has score64 >= theta - e, hence fp32 >= theta - 2 e: it
// is collected, and being its group's best eligible row it is what the reduction keeps for the group.  A group seen only
// through rows that are not its best has a true score below theta - e and is understated: it ranks behind the k answer groups.
#include "sse_kernels.h"
#include "score_exact.h"
#include "score_filtered_common.h"
#include "score_sweep.h"

// The shared sweep (score_sweep.h) with the eligible-max epilogue of score_filtered_kernel<NQ, false> and the tile of every maximum.
template <int NQ>
__global__ __launch_bounds__(SWEEP_THREADS) void score_grouped_max_kernel(FilteredArgs a, unsigned long long *maxima64) {
  extern __shared__ __attribute__((aligned(16))) float gp_smem[];  // [KG][NQ][256]
  __shared__ unsigned long long s_any;
  __shared__ int s_unres;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KG = a.KG;
  int split, qb;
  sweep_decode(a.NSPLIT, split, qb);
  if (qb * NQ * 32 >= a.P) return;
  if (tid == 0) {
    s_any = 0ull;
    s_unres = 0;
  }
  __syncthreads();
  sweep_stage_queries<NQ, false>(gp_smem, a.q, nullptr, qb, a.P, a.S, KG, tid);
  if (tid < NQ * 32) {
    const int pair = qb * NQ * 32 + tid;
    if (pair < a.P) {
      const unsigned long long an = a.q_any ? (unsigned long long)a.q_any[pair] : 0ull;
      if (an == 0ull) atomicOr(&s_unres, 1);
      else atomicOr(&s_any, an);
    }
  }
  uint64_t qany[NQ], qnone[NQ];
  int pr[NQ];
  bool live[NQ];
  f32x16 mx[NQ];
  int mt[NQ][16];  // tile of mx[q][r]
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    pr[q] = (qb * NQ + q) * 32 + (lane & 31);
    live[q] = pr[q] < a.P;
    qany[q] = (live[q] && a.q_any) ? a.q_any[pr[q]] : 0ull;
    qnone[q] = (live[q] && a.q_none) ? a.q_none[pr[q]] : 0ull;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      mx[q][r] = -__builtin_inff();
      mt[q][r] = 0;
    }
  }
  __syncthreads();
  const bool may_skip = a.skip && a.tags && !s_unres;
  const unsigned long long blk_any = s_any;

  int t0, t1;
  sweep_tile_range(a.NT, a.NSPLIT, split, t0, t1);
  const float *qs = gp_smem + lane * 4;
  const int tail_tile = sweep_tail_tile(a.N);
  const int nlim = (int)a.N;

  for (int tile = t0 + w; tile < t1; tile += SWEEP_THREADS / 64) {
    if (may_skip && (a.tile_sum[tile] & blk_any) == 0ull) continue;  // (wave-uniform) no eligible row for any query of the block
    SWEEP_TILE_MFMA(NQ, a.idxp, tile, KG, qs, lane, acc);

    const int rbase = sweep_rbase(tile, lane);
    // rows of this tile that exist (the index's last tile is zero padded past N)
    const unsigned rowmask = (tile == tail_tile) ? sweep_tail_rowmask(rbase, nlim) : 0xFFFFu;  // (uniform condition)
    unsigned em[NQ];  // eligible rows per query tile
    if (a.tags) {     // (uniform)
      uint64_t tg[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) tg[r] = a.tags[sweep_row(rbase, r)];  // (padded to NT * 32 words)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        unsigned m = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool ok = (qany[q] == 0ull || (tg[r] & qany[q]) != 0ull) && (tg[r] & qnone[q]) == 0ull;
          m |= ok ? (1u << r) : 0u;
        }
        em[q] = live[q] ? (m & rowmask) : 0u;
      }
    } else {
#pragma unroll
      for (int q = 0; q < NQ; ++q) em[q] = live[q] ? rowmask : 0u;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool better = ((em[q] >> r) & 1u) && acc[q][r] > mx[q][r];  // (an ineligible row, a NaN: never a maximum)
        mx[q][r] = better ? acc[q][r] : mx[q][r];
        mt[q][r] = better ? tile : mt[q][r];
      }
  }
  // slot of (split, wave, lane half, register); splits past FT_MAXSPLIT fold onto the slots of split % FT_MAXSPLIT
  const int slot0 = (split & (FT_MAXSPLIT - 1)) * 256 + w * 32 + (lane >> 5) * 16;
  const bool shared_slots = a.NSPLIT > FT_MAXSPLIT;  // (uniform)
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (!live[q]) continue;
    unsigned long long *dst = maxima64 + (size_t)pr[q] * a.NV + slot0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t row = (uint32_t)sweep_row(sweep_rbase(mt[q][r], lane), r);
      const unsigned long long v = ((unsigned long long)ft_key(mx[q][r]) << 32) | row;  // (-inf: FT_KEY_NINF, the row unused)
      if (shared_slots) atomicMax(dst + r, v);
      else dst[r] = v;
    }
  }
}

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
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double v = 0.0;
  for (int d = tid; d < a.S; d += 256) v += (double)a.q[(size_t)p * a.S + d] * a.q[(size_t)p * a.S + d];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) s_qn[w] = v;
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
  if (tid == 0) {
    float thr = -__builtin_inff();
    if (a.k <= a.NV && skey[a.k - 1] > FT_KEY_NINF) {
      const double theta = (double)ft_unkey(skey[a.k - 1]);
      const double e = (double)a.eps32 * sqrt(s_qn[0] + s_qn[1] + s_qn[2] + s_qn[3]) * (1.0 + 1.0 / 1048576.0);
      if (theta == theta) thr = __double2float_rd(theta - 2.0 * e);
    }
    a.thr[p] = thr;
  }
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

// One workgroup per query.  Buffer held: its rows in float64, one entry per group, sort, first k.  Buffer overflowed: every
// eligible row of the index in float64, the best k groups kept in the same LDS area.
__global__ __launch_bounds__(256) void grouped_select_kernel(FilteredArgs a, const int64_t *groups, int64_t *out_groups) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long gs_smem[];
  __shared__ int s_cnt, s_heads;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cap = a.col_cap;
  unsigned long long *skey = gs_smem;                      // [cap]
  unsigned long long *sgrp = gs_smem + cap;                // [cap]
  int *srow = reinterpret_cast<int *>(gs_smem + 2 * cap);  // [cap]
  const float *qrow = a.q + (size_t)p * a.S;
  const int n = a.col_cnt[p];  // (uniform)
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  if (n <= cap) {
    const int32_t *rows = a.col_buf + (size_t)p * cap;
    for (int i0 = w * 4; i0 < n; i0 += 16) {
      int64_t r[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) r[b] = rows[min(i0 + b, n - 1)];
      double sc[4];
      wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, sc);
      if (lane == 0) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (i0 + b < n) {
            const int pos = atomicAdd(&s_cnt, 1);
            skey[pos] = ft_key64(sc[b]);
            srow[pos] = (int)r[b];
            sgrp[pos] = (unsigned long long)groups[r[b]];
          }
      }
    }
    __syncthreads();
    if (tid == 0 && s_cnt) atomicAdd(a.counters, (unsigned long long)s_cnt);
  } else {
    const uint64_t qa = a.q_any ? a.q_any[p] : 0ull, qn = a.q_none ? a.q_none[p] : 0ull;
    bool have_bar = false;
    unsigned long long bar_key = 0ull;
    int bar_row = 0;
    for (int64_t n0 = 0; n0 < a.N; n0 += 64) {
#pragma unroll 1
      for (int g = 0; g < 4; ++g) {
        const int64_t base = n0 + g * 16 + w * 4;
        if (base >= a.N) break;  // (wave-uniform)
        int64_t r[4];
        bool use[4];
        bool any_use = false;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          r[b] = (base + b < a.N) ? base + b : a.N - 1;
          bool ok = base + b < a.N;
          if (ok && a.tags) {
            const uint64_t t = a.tags[r[b]];
            ok = (qa == 0ull || (t & qa) != 0ull) && (t & qn) == 0ull;
          }
          use[b] = ok;
          any_use |= ok;
        }
        if (!any_use) continue;  // (wave-uniform)
        double sc[4];
        wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, sc);
        if (lane == 0) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if (!use[b]) continue;
            const unsigned long long key = ft_key64(sc[b]);
            // below the k-th group's entry: not a new answer group, and no better than the entry its own group may hold
            if (have_bar && !(key > bar_key || (key == bar_key && (int)r[b] < bar_row))) continue;
            const int pos = atomicAdd(&s_cnt, 1);  // (at most 64 appends between two cuts: pos < cap)
            skey[pos] = key;
            srow[pos] = (int)r[b];
            sgrp[pos] = (unsigned long long)groups[r[b]];
          }
        }
      }
      __syncthreads();
      const int c = s_cnt;
      __syncthreads();
      if (c > cap - 64) {  // (uniform) one entry per group, cut back to the k best groups
        const int ng = gp_reduce(skey, srow, sgrp, c, tid, &s_heads);
        if (ng >= a.k) {
          have_bar = true;
          bar_key = skey[a.k - 1];
          bar_row = srow[a.k - 1];
        }
        __syncthreads();
        if (tid == 0) s_cnt = min(ng, a.k);
        __syncthreads();
      }
    }
    __syncthreads();
    if (tid == 0) atomicAdd(a.counters + 1, 1ull);
  }
  const int ng = gp_reduce(skey, srow, sgrp, s_cnt, tid, &s_heads);
  const int cnt = min(ng, a.k);
  for (int j = tid; j < a.k; j += 256) {
    a.out_scores[(size_t)p * a.k + j] = (j < cnt) ? ft_unkey64(skey[j]) : -(double)__builtin_inff();
    a.out_ids[(size_t)p * a.k + j] = (j < cnt) ? a.id_base + srow[j] : INT64_MAX;
    out_groups[(size_t)p * a.k + j] = (j < cnt) ? (int64_t)sgrp[j] : INT64_MAX;
  }
  if (tid == 0) a.out_counts[p] = cnt;
}

// (1 KiB of the workgroup's LDS left to s_any / s_unres)
template <int NQ>
static hipError_t launch_grouped_max(const FilteredArgs &a, unsigned long long *maxima64, hipStream_t st) {
  return launch_sweep(score_grouped_max_kernel<NQ>, a.P, NQ, a.KG, a.NSPLIT, SWEEP_LDS_MAX - 1024, st, a, maxima64);
}

hipError_t launch_score_grouped(const GroupedArgs &g, hipStream_t st) {
  const FilteredArgs &m = g.max, &c = g.rest;
  if (c.P <= 0) return hipSuccess;
  if (!g.groups || !g.maxima64 || !g.out_groups || m.P != c.P || m.k != c.k) return hipErrorInvalidValue;
  if (c.col_cap != SSE_COLLECT_CAP || c.k < 1 || c.k > SSE_GROUPED_MAX_K) return hipErrorInvalidValue;
  if (m.NSPLIT < 1 || (m.NSPLIT & (m.NSPLIT - 1))) return hipErrorInvalidValue;
  if (m.NV != (m.NSPLIT < FT_MAXSPLIT ? m.NSPLIT : FT_MAXSPLIT) * 256) return hipErrorInvalidValue;
  hipError_t e;
  if (m.NQ == 2) e = launch_grouped_max<2>(m, g.maxima64, st);
  else if (m.NQ == 1) e = launch_grouped_max<1>(m, g.maxima64, st);
  else e = hipErrorInvalidValue;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grouped_threshold_kernel, dim3(m.P), dim3(256), (size_t)m.NV * (sizeof(unsigned long long) + sizeof(uint32_t)), st,
                     m, g.maxima64, g.groups);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_filtered_collect(c, st);
  if (e != hipSuccess) return e;
  const size_t lds = (size_t)c.col_cap * (2 * sizeof(unsigned long long) + sizeof(int));
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(grouped_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grouped_select_kernel, dim3(c.P), dim3(256), lds, st, c, g.groups, g.out_groups);
  return hipGetLastError();
}
