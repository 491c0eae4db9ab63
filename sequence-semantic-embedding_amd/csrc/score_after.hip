// Exact next page after a (score, id) cursor for gfx950 (MI355X): sse_score_topk_after*.
//
// The reference ranks every target of a query and cuts the sorted row on the host (sse_evaluator.py:110-112,
// webserver.py:144-151: [:nbest]); what follows the rows a caller already holds is another cut of the same row.  Here row r is
// AFTER the cursor (cs, cid) of a query iff score64 < cs, or score64 == cs and id_base + r > cid, and the answer is the best k
// tag-eligible rows after it (DESIGN K6j).  The eligibility depends on the score itself, which the fp32 sweep knows to within
// e = eps32 |q| (1 + 2^-20) only: it brackets the cursor and leaves the rows inside the bracket to float64.
//   0. after_bounds_kernel: e, lo = rd(cs - e), hi = ru(cs + e) per query.  fp32 score < lo: certainly after; > hi: certainly
//      not.  cs = +inf (or no cursor): lo = hi = +inf, every finite score is below lo.  cs = -inf: nothing is below lo or at
//      most hi.  cs = NaN: every comparison is false.  No special cases.
//   1. score_after_kernel<NQ, false>: the shared fp32 sweep (score_sweep.h) with the eligible maxima over disjoint row sets of
//      score_filtered_kernel<NQ, false>, taken over the tag-eligible rows with fp32 score < lo only.
//   2. after_threshold_kernel: theta = the k-th largest maximum (-inf with fewer than k finite ones).  k distinct eligible rows
//      are certainly after the cursor with an fp32 score >= theta, so with score64 >= theta - e: so has the k-th answer row,
//      and every answer row has an fp32 score >= theta - 2 e.
//   3. score_after_kernel<NQ, true>: every tag-eligible row with rd(theta - 2 e) <= fp32 score <= hi is appended to the query's
//      buffer.  An answer row is after the cursor: score64 <= cs, fp32 score <= cs + e <= hi.
//   4. after_select_kernel: re-scored with wave_exact_dot, rows not after the cursor dropped on (score64, id), the rest sorted
//      by before(), first k out, padding (-inf, INT64_MAX), count.  A query whose buffer overflowed is served by a float64
//      sweep of the whole index in the same workgroup with the same predicate.
// No row before the cursor is returned: stage 4 alone decides, in float64.  No answer row is missed: see 2. and 3.
#include "sse_kernels.h"
#include "score_exact.h"
#include "score_filtered_common.h"
#include "score_sweep.h"

// one workgroup per query: |q|, e and the fp32 bracket of the cursor score
__global__ __launch_bounds__(256) void after_bounds_kernel(AfterArgs g) {
  __shared__ double s_qn[4];
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double v = 0.0;
  for (int d = tid; d < a.S; d += 256) v += (double)a.q[(size_t)p * a.S + d] * a.q[(size_t)p * a.S + d];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (lane == 0) s_qn[w] = v;
  __syncthreads();
  if (tid == 0) {
    const double e = (double)a.eps32 * sqrt(s_qn[0] + s_qn[1] + s_qn[2] + s_qn[3]) * (1.0 + 1.0 / 1048576.0);
    const double cs = g.after_score ? g.after_score[p] : (double)__builtin_inff();
    g.eb[p] = e;
    g.lo[p] = __double2float_rd(cs - e);
    g.hi[p] = __double2float_ru(cs + e);
  }
}

// The shared sweep (score_sweep.h), one query per column.  COLLECT: eligible rows with thr <= score <= hi are appended to the
// query's buffer; otherwise a running maximum per accumulator register over the eligible rows with score < lo.
template <int NQ, bool COLLECT>
__global__ __launch_bounds__(SWEEP_THREADS) void score_after_kernel(AfterArgs g) {
  extern __shared__ __attribute__((aligned(16))) float af_smem[];  // [KG][NQ][256]
  __shared__ unsigned long long s_any;
  __shared__ int s_unres;
  const FilteredArgs &a = g.f;
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
  sweep_stage_queries<NQ, false>(af_smem, a.q, nullptr, qb, a.P, a.S, KG, tid);
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
  float thr[NQ], top[NQ];  // COLLECT: thr <= score <= top = hi; otherwise score < top = lo
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
    top[q] = live[q] ? (COLLECT ? g.hi[pr[q]] : g.lo[pr[q]]) : -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; ++r) mx[q][r] = -__builtin_inff();
  }
  __syncthreads();
  const bool may_skip = a.skip && a.tags && !s_unres;
  const unsigned long long blk_any = s_any;

  int t0, t1;
  sweep_tile_range(a.NT, a.NSPLIT, split, t0, t1);
  const float *qs = af_smem + lane * 4;
  const int tail_tile = sweep_tail_tile(a.N);
  const int nlim = (int)a.N;

  for (int tile = t0 + w; tile < t1; tile += SWEEP_THREADS / 64) {
    if (may_skip && (a.tile_sum[tile] & blk_any) == 0ull) continue;  // (wave-uniform)
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
        for (int r = 0; r < 16; ++r) bm |= (acc[q][r] >= thr[q] && acc[q][r] <= top[q]) ? (1u << r) : 0u;
        bm &= em[q];
        while (bm) {
          const int r = __ffs((int)bm) - 1;
          bm &= bm - 1;
          const int row = sweep_row(rbase, r);
          sweep_append(a.col_cnt, a.col_buf, a.col_cap, pr[q], row, row < nlim);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          mx[q][r] = fmaxf(mx[q][r], (((em[q] >> r) & 1u) && acc[q][r] < top[q]) ? acc[q][r] : -__builtin_inff());
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
  }
}

// one workgroup per query: collect threshold from the k-th largest of its NV maxima
__global__ __launch_bounds__(256) void after_threshold_kernel(AfterArgs g) {
  extern __shared__ __attribute__((aligned(16))) uint32_t at_key[];  // [NV]
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x;
  for (int c = tid; c < a.NV; c += 256) at_key[c] = a.maxima[(size_t)p * a.NV + c];
  ft_sort_u32(at_key, a.NV, tid, 256);
  if (tid == 0) {
    float thr = -__builtin_inff();
    if (a.k <= a.NV && at_key[a.k - 1] > FT_KEY_NINF) {
      const double theta = (double)ft_unkey(at_key[a.k - 1]);
      if (theta == theta) thr = __double2float_rd(theta - 2.0 * g.eb[p]);
    }
    a.thr[p] = thr;
  }
}

// is (score64, id) after the cursor?  IEEE comparisons: a NaN cursor score has nothing after it
__device__ __forceinline__ bool af_after(double sc, int64_t id, double cs, int64_t cid) { return sc < cs || (sc == cs && id > cid); }

// One workgroup per query.  Buffer held: its rows in float64, those after the cursor sorted, first k.  Buffer overflowed: every
// eligible row of the index in float64, the best k after the cursor kept in the same LDS area (filled to col_cap, then cut
// back to the k best whose last entry becomes the bar later rows have to pass), as filtered_select_kernel.
__global__ __launch_bounds__(256) void after_select_kernel(AfterArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long as_smem[];
  __shared__ int s_cnt;
  __shared__ unsigned long long s_bar_key;
  __shared__ int s_bar_row;
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cap = a.col_cap;
  unsigned long long *skey = as_smem;                  // [cap]
  int *srow = reinterpret_cast<int *>(as_smem + cap);  // [cap]
  const float *qrow = a.q + (size_t)p * a.S;
  const bool cursor = g.after_score != nullptr;
  const double cs = cursor ? g.after_score[p] : 0.0;
  const int64_t cid = cursor ? g.after_id[p] : 0;
  const int n = a.col_cnt[p];  // (uniform)
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  int n2 = 1;
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
          if (i0 + b < n && (!cursor || af_after(sc[b], a.id_base + r[b], cs, cid))) {
            const int pos = atomicAdd(&s_cnt, 1);
            skey[pos] = ft_key64(sc[b]);
            srow[pos] = (int)r[b];
          }
      }
    }
    __syncthreads();
    const int c = s_cnt;
    while (n2 < c) n2 <<= 1;
    if (tid == 0 && n) atomicAdd(a.counters, (unsigned long long)n);
  } else {
    const uint64_t qa = a.q_any ? a.q_any[p] : 0ull, qn = a.q_none ? a.q_none[p] : 0ull;
    bool have_bar = false;
    unsigned long long bar_key = 0ull;
    int bar_row = 0;
    for (int64_t n0 = 0; n0 < a.N; n0 += 64) {
#pragma unroll 1
      for (int gq = 0; gq < 4; ++gq) {
        const int64_t base = n0 + gq * 16 + w * 4;
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
            if (!use[b] || (cursor && !af_after(sc[b], a.id_base + r[b], cs, cid))) continue;
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
static hipError_t launch_after_sweep(const AfterArgs &g, hipStream_t st) {
  return launch_sweep(score_after_kernel<NQ, COLLECT>, g.f.P, NQ, g.f.KG, g.f.NSPLIT, SWEEP_LDS_MAX - 1024, st, g);
}

hipError_t launch_score_after(const AfterArgs &g, hipStream_t st) {
  const FilteredArgs &a = g.f;
  if (a.P <= 0) return hipSuccess;
  if (a.col_cap != SSE_COLLECT_CAP) return hipErrorInvalidValue;
  if (a.k < 1 || a.k > SSE_AFTER_MAX_K || a.n_excl != 0 || a.excl) return hipErrorInvalidValue;
  if ((g.after_score == nullptr) != (g.after_id == nullptr)) return hipErrorInvalidValue;
  if (a.NSPLIT < 1 || (a.NSPLIT & (a.NSPLIT - 1))) return hipErrorInvalidValue;  // a power of two: 1, 2, 4, 8, then multiples of 8
  if (a.NV != (a.NSPLIT < FT_MAXSPLIT ? a.NSPLIT : FT_MAXSPLIT) * 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(after_bounds_kernel, dim3(a.P), dim3(256), 0, st, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.NQ == 4) e = launch_after_sweep<4, false>(g, st);
  else if (a.NQ == 2) e = launch_after_sweep<2, false>(g, st);
  else if (a.NQ == 1) e = launch_after_sweep<1, false>(g, st);
  else e = hipErrorInvalidValue;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(after_threshold_kernel, dim3(a.P), dim3(256), (size_t)a.NV * sizeof(uint32_t), st, g);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.NQ == 4) e = launch_after_sweep<4, true>(g, st);
  else if (a.NQ == 2) e = launch_after_sweep<2, true>(g, st);
  else e = launch_after_sweep<1, true>(g, st);
  if (e != hipSuccess) return e;
  const size_t lds = (size_t)a.col_cap * (sizeof(unsigned long long) + sizeof(int));
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(after_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(after_select_kernel, dim3(a.P), dim3(256), lds, st, g);
  return hipGetLastError();
}
