// Exact top-k among tag-eligible index rows for gfx950 (MI355X): sse_score_topk_filtered*.
//
// The reference ranks every target of a query (sse_evaluator.py:110-112, data_utils.py:263-267) and leaves "only the leaves
// under this meta-category", "not the labelled positives" or "not the row itself" to a filter of the sorted row on the host.
// Here the filter is inside the sweep and the threshold comes from eligible rows only (DESIGN K6g):
//   1. score_filtered_kernel<NQ, false>: the shared fp32 sweep (score_sweep.h) on v_mfma_f32_32x32x2_f32 (index rows = M, one
//      query per lane column).  A lane reads the 16 tag words of its rows, turns tag-ineligible rows and the zero padding of
//      the tail tile into -inf and keeps a running maximum per accumulator register.  The NSPLIT x 8 waves x 2 halves x 16
//      maxima of a query belong to DISJOINT row sets (folded onto NV = min(NSPLIT, 16) x 256 slots: a slot shared by several
//      splits holds the maximum of their union).  Exclusion lists play no part here.
//   2. filtered_threshold_kernel: theta = the (k + n_excl)-th largest maximum (-inf with fewer finite ones).  k + n_excl
//      distinct tag-eligible rows have an fp32 score >= theta and at most n_excl of them are excluded, so k eligible rows
//      have score64 >= theta - e, so has the k-th best eligible row, and every row of the exact answer has an fp32 score
//      >= theta - 2 e (e = eps32 |q| (1 + 2^-20), the bound of score_rank.hip, rounded outward).
//   3. score_filtered_kernel<NQ, true>: the same template and MFMA chain appends every tag-eligible row at or above that to
//      the query's buffer.
//   4. filtered_select_kernel: excluded ids dropped, the rest re-scored with wave_exact_dot, sorted by before(), first k out,
//      padding (-inf, INT64_MAX), count.  Fewer than k rows is a valid answer (theta = -inf: everything eligible was
//      collected).  A query whose buffer overflowed is served by a float64 sweep of the whole index in the same workgroup.
// Tile skip: a tile whose summary word (OR of its 32 tag words) shares no bit with the OR of q_any over the workgroup's
// query block, none of whose queries is unrestricted, has no eligible row for any of them: the wave moves on.
#include "sse_kernels.h"
#include "score_exact.h"
#include "score_filtered_common.h"
#include "score_sweep.h"

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

// The shared sweep (score_sweep.h), one query per column.  COLLECT: eligible rows at or above thr are appended to the query's
// buffer; otherwise a running maximum per accumulator register.
template <int NQ, bool COLLECT>
__global__ __launch_bounds__(SWEEP_THREADS) void score_filtered_kernel(FilteredArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ft_smem[];  // [KG][NQ][256]
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
  sweep_stage_queries<NQ, false>(ft_smem, a.q, nullptr, qb, a.P, a.S, KG, tid);
  // the block's OR of q_any, and whether one of its queries asks for nothing (the tile skip)
  if (tid < NQ * 32) {
    const int pair = qb * NQ * 32 + tid;
    if (pair < a.P) {
      const unsigned long long an = a.q_any ? (unsigned long long)a.q_any[pair] : 0ull;
      if (an == 0ull) atomicOr(&s_unres, 1);
      else atomicOr(&s_any, an);
    }
  }
  uint64_t qany[NQ], qnone[NQ];
  float thr[NQ];
  int pr[NQ];
  bool live[NQ];
  f32x16 mx[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    pr[q] = (qb * NQ + q) * 32 + (lane & 31);
    live[q] = pr[q] < a.P;
    qany[q] = (live[q] && a.q_any) ? a.q_any[pr[q]] : 0ull;
    qnone[q] = (live[q] && a.q_none) ? a.q_none[pr[q]] : 0ull;
    thr[q] = (COLLECT && live[q]) ? a.thr[pr[q]] : __builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; ++r) mx[q][r] = -__builtin_inff();
  }
  __syncthreads();
  const bool may_skip = a.skip && a.tags && !s_unres;
  const unsigned long long blk_any = s_any;

  int t0, t1;
  sweep_tile_range(a.NT, a.NSPLIT, split, t0, t1);
  const float *qs = ft_smem + lane * 4;
  const int tail_tile = sweep_tail_tile(a.N);
  const int nlim = (int)a.N;
  int skipped = 0;

  for (int tile = t0 + w; tile < t1; tile += SWEEP_THREADS / 64) {
    if (may_skip && (a.tile_sum[tile] & blk_any) == 0ull) {  // (wave-uniform)
      ++skipped;
      continue;
    }
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
    for (int q = 0; q < NQ; ++q) {
      if (COLLECT) {
        unsigned bm = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) bm |= (acc[q][r] >= thr[q]) ? (1u << r) : 0u;
        bm &= em[q];
        while (bm) {
          const int r = __ffs((int)bm) - 1;
          bm &= bm - 1;
          const int row = sweep_row(rbase, r);
          sweep_append(a.col_cnt, a.col_buf, a.col_cap, pr[q], row, row < nlim);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) mx[q][r] = fmaxf(mx[q][r], ((em[q] >> r) & 1u) ? acc[q][r] : -__builtin_inff());
      }
    }
  }
  if (!COLLECT) {
    // slot of (split, wave, lane half, register); splits past FT_MAXSPLIT fold onto the slots of split % FT_MAXSPLIT
    const int slot0 = (split & (FT_MAXSPLIT - 1)) * 256 + w * 32 + (lane >> 5) * 16;
    const bool shared_slots = a.NSPLIT > FT_MAXSPLIT;  // (uniform)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (!live[q]) continue;
      uint32_t *dst = a.maxima + (size_t)pr[q] * a.NV + slot0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t key = ft_key(mx[q][r]);
        if (shared_slots) atomicMax(dst + r, key);
        else dst[r] = key;
      }
    }
    if (skipped && lane == 0) atomicAdd(a.counters + 2, (unsigned long long)skipped);
  }
}

// one workgroup per query: collect threshold from the (k + n_excl)-th largest of its NV maxima
__global__ __launch_bounds__(256) void filtered_threshold_kernel(FilteredArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t th_key[];  // [NV]
  __shared__ double s_qn[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double v = 0.0;
  for (int d = tid; d < a.S; d += 256) v += (double)a.q[(size_t)p * a.S + d] * a.q[(size_t)p * a.S + d];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) s_qn[w] = v;
  for (int c = tid; c < a.NV; c += 256) th_key[c] = a.maxima[(size_t)p * a.NV + c];
  ft_sort_u32(th_key, a.NV, tid, 256);
  if (tid == 0) {
    const int m = a.k + a.n_excl;
    float thr = -__builtin_inff();
    if (m <= a.NV && th_key[m - 1] > FT_KEY_NINF) {
      const double theta = (double)ft_unkey(th_key[m - 1]);
      const double e = (double)a.eps32 * sqrt(s_qn[0] + s_qn[1] + s_qn[2] + s_qn[3]) * (1.0 + 1.0 / 1048576.0);
      if (theta == theta) thr = __double2float_rd(theta - 2.0 * e);
    }
    a.thr[p] = thr;
  }
}

// is id among the query's exclusion list?  One lane per entry (n_excl <= 64); the answer is wave-uniform.
__device__ __forceinline__ bool ft_excluded(const int64_t *ex, int n_excl, int64_t id, int lane) {
  if (n_excl == 0) return false;
  return __ballot(lane < n_excl && ex[lane] == id) != 0ull;
}

// One workgroup per query.  Buffer held: its rows without the excluded ids, float64 scores, sort, first k.  Buffer
// overflowed: every eligible row of the index in float64, the best k kept in the same LDS area (filled to col_cap, then cut
// back to the k best whose last entry becomes the bar later rows have to pass).
__global__ __launch_bounds__(256) void filtered_select_kernel(FilteredArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long fs_smem[];
  __shared__ int s_cnt;
  __shared__ unsigned long long s_bar_key;
  __shared__ int s_bar_row;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cap = a.col_cap;
  unsigned long long *skey = fs_smem;                  // [cap]
  int *srow = reinterpret_cast<int *>(fs_smem + cap);  // [cap]
  const float *qrow = a.q + (size_t)p * a.S;
  const int64_t *ex = a.excl ? a.excl + (size_t)p * a.n_excl : nullptr;
  const int n_excl = a.excl ? a.n_excl : 0;
  const int n = a.col_cnt[p];  // (uniform)
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  int n2 = 1;
  if (n <= cap) {
    const int32_t *rows = a.col_buf + (size_t)p * cap;
    for (int i0 = w * 4; i0 < n; i0 += 16) {
      int64_t r[4];
      bool use[4];
      bool any_use = false;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        r[b] = rows[min(i0 + b, n - 1)];
        use[b] = (i0 + b < n) && !ft_excluded(ex, n_excl, a.id_base + r[b], lane);
        any_use |= use[b];
      }
      if (!any_use) continue;  // (wave-uniform)
      double sc[4];
      wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, sc);
      if (lane == 0) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (use[b]) {
            const int pos = atomicAdd(&s_cnt, 1);
            skey[pos] = ft_key64(sc[b]);
            srow[pos] = (int)r[b];
          }
      }
    }
    __syncthreads();
    const int c = s_cnt;
    while (n2 < c) n2 <<= 1;
    if (tid == 0 && c) atomicAdd(a.counters, (unsigned long long)c);
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
          use[b] = ok && !ft_excluded(ex, n_excl, a.id_base + r[b], lane);
          any_use |= use[b];
        }
        if (!any_use) continue;  // (wave-uniform)
        double sc[4];
        wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, sc);
        if (lane == 0) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if (!use[b]) continue;
            const unsigned long long key = ft_key64(sc[b]);
            if (have_bar && !(key > bar_key || (key == bar_key && (int)r[b] < bar_row))) continue;
            const int pos = atomicAdd(&s_cnt, 1);  // (at most 64 appends between two cuts: pos < cap)
            skey[pos] = key;
            srow[pos] = (int)r[b];
          }
        }
      }
      __syncthreads();
      const int c = s_cnt;
      __syncthreads();
      if (c > cap - 64) {  // (uniform) cut back to the k best
        for (int i = c + tid; i < cap; i += 256) {
          skey[i] = 0ull;
          srow[i] = FT_PAD_ROW;
        }
        ft_sort_entries(skey, srow, cap, tid);
        if (tid == 0) {
          s_cnt = a.k;
          s_bar_key = skey[a.k - 1];
          s_bar_row = srow[a.k - 1];
        }
        __syncthreads();
        have_bar = true;
        bar_key = s_bar_key;
        bar_row = s_bar_row;
      }
    }
    __syncthreads();
    const int c = s_cnt;
    while (n2 < c) n2 <<= 1;
    if (tid == 0) atomicAdd(a.counters + 1, 1ull);
  }
  const int c = s_cnt;
  for (int i = c + tid; i < n2; i += 256) {
    skey[i] = 0ull;
    srow[i] = FT_PAD_ROW;
  }
  ft_sort_entries(skey, srow, n2, tid);
  const int cnt = min(c, a.k);
  for (int j = tid; j < a.k; j += 256) {
    a.out_scores[(size_t)p * a.k + j] = (j < cnt) ? ft_unkey64(skey[j]) : -(double)__builtin_inff();
    a.out_ids[(size_t)p * a.k + j] = (j < cnt) ? a.id_base + srow[j] : INT64_MAX;
  }
  if (tid == 0) a.out_counts[p] = cnt;
}

// (1 KiB of the workgroup's LDS left to s_any / s_unres)
template <int NQ, bool COLLECT>
static hipError_t launch_filtered_sweep(const FilteredArgs &a, hipStream_t st) {
  return launch_sweep(score_filtered_kernel<NQ, COLLECT>, a.P, NQ, a.KG, a.NSPLIT, SWEEP_LDS_MAX - 1024, st, a);
}

hipError_t launch_score_filtered(const FilteredArgs &a, hipStream_t st) {
  if (a.P <= 0) return hipSuccess;
  if (a.col_cap != SSE_COLLECT_CAP) return hipErrorInvalidValue;
  if (a.k < 1 || a.k > SSE_FILTERED_MAX_K || a.n_excl < 0 || a.n_excl > SSE_FILTERED_MAX_EXCL) return hipErrorInvalidValue;
  if (a.NSPLIT < 1 || (a.NSPLIT & (a.NSPLIT - 1))) return hipErrorInvalidValue;  // a power of two: 1, 2, 4, 8, then multiples of 8
  if (a.NV != (a.NSPLIT < FT_MAXSPLIT ? a.NSPLIT : FT_MAXSPLIT) * 256) return hipErrorInvalidValue;
  hipError_t e;
  if (a.NQ == 4) e = launch_filtered_sweep<4, false>(a, st);
  else if (a.NQ == 2) e = launch_filtered_sweep<2, false>(a, st);
  else if (a.NQ == 1) e = launch_filtered_sweep<1, false>(a, st);
  else e = hipErrorInvalidValue;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(filtered_threshold_kernel, dim3(a.P), dim3(256), (size_t)a.NV * sizeof(uint32_t), st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.NQ == 4) e = launch_filtered_sweep<4, true>(a, st);
  else if (a.NQ == 2) e = launch_filtered_sweep<2, true>(a, st);
  else e = launch_filtered_sweep<1, true>(a, st);
  if (e != hipSuccess) return e;
  const size_t lds = (size_t)a.col_cap * (sizeof(unsigned long long) + sizeof(int));
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(filtered_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(filtered_select_kernel, dim3(a.P), dim3(256), lds, st, a);
  return hipGetLastError();
}

// the collect sweep alone (stage 3), for callers with a threshold of their own: sse_score_topk_grouped (score_grouped.hip)
hipError_t launch_filtered_collect(const FilteredArgs &a, hipStream_t st) {
  if (a.P <= 0) return hipSuccess;
  if (a.col_cap != SSE_COLLECT_CAP || a.NSPLIT < 1 || (a.NSPLIT & (a.NSPLIT - 1))) return hipErrorInvalidValue;
  if (a.NQ == 4) return launch_filtered_sweep<4, true>(a, st);
  if (a.NQ == 2) return launch_filtered_sweep<2, true>(a, st);
  if (a.NQ == 1) return launch_filtered_sweep<1, true>(a, st);
  return hipErrorInvalidValue;
}
