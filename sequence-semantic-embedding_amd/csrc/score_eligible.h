// The stages sse_score_topk_filtered, sse_score_topk_grouped, sse_score_topk_after, sse_score_confusions and
// sse_score_topk_biased share (score_filtered.hip, score_grouped.hip, score_after.hip, score_confusions.hip, score_biased.hip;
// DESIGN K6g / K6h / K6j / K6k / K6l), each written once:
//   eligible_sweep_kernel<NQ, Stage>
//                               the shared fp32 sweep (score_sweep.h) over tag-eligible rows: the block's OR of q_any and the
//                               tile skip, the tail-tile row mask, the 16 tag words and the eligibility masks, then either the
//                               running maxima and their slots or the append to the query's buffer.  A Stage supplies what a
//                               lane holds per column (Col, init), which scores count (admits, KEEP_TILE; take for a collect
//                               stage) and what a slot holds (Slot, slots, slot).
//   ft_qnorm2_parts, ft_score_bound, ft_collect_threshold
//                               |q|^2, e = eps32 |q| (1 + 2^-20), and "m-th largest maximum theta -> thr = rd(theta - 2 e)".
//   eligible_select_kernel<Sel> the buffer re-scored in float64 or -- buffer overflow -- the float64 sweep of the whole index
//                               with its cuts, then the final reduction and the output.  A Sel supplies which rows are used,
//                               which (score64, id) are kept, whether entries carry a group and how the area is reduced
//                               (BIASED: what is added to score64 first).
//   ft_excluded                 is an id among a query's list of at most 64 (exclusions, positives)?
//   eligible_args_ok, launch_eligible_sweep, launch_eligible_select
//                               the launchers' argument checks, the NQ dispatch and the select launch.
#pragma once
#include "sse_kernels.h"
#include "score_exact.h"
#include "score_filtered_common.h"
#include "score_sweep.h"

// ---- sweep stages: the maxima of a column's eligible rows (Slot = what a maxima slot holds) or the collect ----

// The kernel arguments of a stage, Stage::Args, hold the chunk's FilteredArgs as member f (as AfterArgs does) beside what the
// stage needs of its own, and a stage's functions take them BY VALUE.  (With an accessor function for f, or a reference to the
// kernel's arguments crossing a call, some sweep instantiations come out with other register counts than the kernels they
// replace; so they do with the fmaxf of the running maximum in a stage function, which is why the body keeps it and a max
// stage supplies the predicate only: profiles/score_select_refactor.txt.)
struct FilteredStageArgs {
  FilteredArgs f;
};

// filtered max: a running maximum per accumulator register; a slot holds its order-preserving key
struct FilteredMaxStage {
  typedef FilteredStageArgs Args;
  static constexpr bool COLLECT = false, COUNT_SKIPS = true;  // (the one sweep that counts skipped tiles into counters[2])
  static constexpr bool KEEP_TILE = false;  // true: Col has mt[16], the tile of each maximum, and the maximum is strict
  static constexpr bool BIASED = false;     // true: Args has bias [NT * 32], Col has w; a score is fmaf(w, bias[row], dot) (K6l)
  static constexpr int MAX_NQ = 4;
  typedef uint32_t Slot;
  struct Col {
    f32x16 mx;
  };
  static __device__ __forceinline__ void init(Col &c, const Args, int, bool) {
#pragma unroll
    for (int r = 0; r < 16; ++r) c.mx[r] = -__builtin_inff();
  }
  static __device__ __forceinline__ bool admits(const Col &, float) { return true; }  // which eligible scores count
  static __device__ __forceinline__ Slot *slots(const Args g) { return g.f.maxima; }
  static __device__ __forceinline__ Slot slot(const Col &c, int r, int) { return ft_key(c.mx[r]); }
};

// filtered collect: eligible rows at or above thr
struct FilteredCollectStage {
  typedef FilteredStageArgs Args;
  static constexpr bool COLLECT = true, COUNT_SKIPS = false, BIASED = false;
  static constexpr int MAX_NQ = 4;
  struct Col {
    float thr;
  };
  static __device__ __forceinline__ void init(Col &c, const Args g, int pr, bool live) { c.thr = live ? g.f.thr[pr] : __builtin_inff(); }
  static __device__ __forceinline__ bool take(const Col &c, float x) { return x >= c.thr; }
};

// One workgroup = (block of NQ x 32 queries, index split); the dynamic LDS is the block's query fragments [KG][NQ][256].
// Tile skip: a tile whose summary word (OR of its 32 tag words) shares no bit with the OR of q_any over the workgroup's query
// block, none of whose queries is unrestricted, has no eligible row for any of them: the wave moves on.
// !COLLECT: the NSPLIT x 8 waves x 2 halves x 16 maxima of a query belong to DISJOINT row sets, folded onto
// NV = min(NSPLIT, 16) x 256 slots: a slot shared by several splits holds the maximum of their union.
// A kernel, not a function the kernels call: with this text behind a call the compiler gives some instantiations other
// register counts than with it in their bodies, as with SWEEP_TILE_MFMA (profiles/score_select_refactor.txt).
template <int NQ, class Stage>
__global__ __launch_bounds__(SWEEP_THREADS) void eligible_sweep_kernel(typename Stage::Args g) {
  extern __shared__ __attribute__((aligned(16))) float el_smem[];  // [KG][NQ][256]
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
  sweep_stage_queries<NQ, false>(el_smem, a.q, nullptr, qb, a.P, a.S, KG, tid);
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
  int pr[NQ];
  bool live[NQ];
  typename Stage::Col col[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    pr[q] = (qb * NQ + q) * 32 + (lane & 31);
    live[q] = pr[q] < a.P;
    qany[q] = (live[q] && a.q_any) ? a.q_any[pr[q]] : 0ull;
    qnone[q] = (live[q] && a.q_none) ? a.q_none[pr[q]] : 0ull;
    Stage::init(col[q], g, pr[q], live[q]);
  }
  __syncthreads();
  const bool may_skip = a.skip && a.tags && !s_unres;
  const unsigned long long blk_any = s_any;

  int t0, t1;
  sweep_tile_range(a.NT, a.NSPLIT, split, t0, t1);
  const float *qs = el_smem + lane * 4;
  const int tail_tile = sweep_tail_tile(a.N);
  const int nlim = (int)a.N;
  int skipped = 0;

  for (int tile = t0 + w; tile < t1; tile += SWEEP_THREADS / 64) {
    if (may_skip && (a.tile_sum[tile] & blk_any) == 0ull) {  // (wave-uniform) no eligible row for any query of the block
      ++skipped;
      continue;
    }
    SWEEP_TILE_MFMA(NQ, a.idxp, tile, KG, qs, lane, acc);

    const int rbase = sweep_rbase(tile, lane);
    // rows of this tile that exist (the index's last tile is zero padded past N)
    const unsigned rowmask = (tile == tail_tile) ? sweep_tail_rowmask(rbase, nlim) : 0xFFFFu;  // (uniform condition)
    if constexpr (Stage::BIASED) {  // the per-row prior, fused into the tile's scores before anything looks at them
      float bs[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) bs[r] = g.bias[sweep_row(rbase, r)];  // (padded to NT * 32 floats)
#pragma unroll
      for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = fmaf(col[q].w, bs[r], acc[q][r]);
    }
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
      if constexpr (Stage::COLLECT) {
        unsigned bm = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) bm |= Stage::take(col[q], acc[q][r]) ? (1u << r) : 0u;
        bm &= em[q];
        while (bm) {
          const int r = __ffs((int)bm) - 1;
          bm &= bm - 1;
          const int row = sweep_row(rbase, r);
          sweep_append(a.col_cnt, a.col_buf, a.col_cap, pr[q], row, row < nlim);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if constexpr (Stage::KEEP_TILE) {
            const bool better = ((em[q] >> r) & 1u) && acc[q][r] > col[q].mx[r];  // (an ineligible row, a NaN: never a maximum)
            col[q].mx[r] = better ? acc[q][r] : col[q].mx[r];
            col[q].mt[r] = better ? tile : col[q].mt[r];
          } else {
            col[q].mx[r] = fmaxf(col[q].mx[r], (((em[q] >> r) & 1u) && Stage::admits(col[q], acc[q][r])) ? acc[q][r] : -__builtin_inff());
          }
        }
      }
    }
  }
  if constexpr (!Stage::COLLECT) {
    // slot of (split, wave, lane half, register); splits past FT_MAXSPLIT fold onto the slots of split % FT_MAXSPLIT
    const int slot0 = (split & (FT_MAXSPLIT - 1)) * 256 + w * 32 + (lane >> 5) * 16;
    const bool shared_slots = a.NSPLIT > FT_MAXSPLIT;  // (uniform)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (!live[q]) continue;
      typename Stage::Slot *dst = Stage::slots(g) + (size_t)pr[q] * a.NV + slot0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const typename Stage::Slot v = Stage::slot(col[q], r, lane);
        if (shared_slots) atomicMax(dst + r, v);
        else dst[r] = v;
      }
    }
    if (Stage::COUNT_SKIPS && skipped && lane == 0) atomicAdd(a.counters + 2, (unsigned long long)skipped);
  }
}

// ---- thresholds ----

// |q_p|^2 in float64 by the workgroup's 256 threads: s_qn[0 .. 4) hold the four waves' parts after the next barrier
__device__ __forceinline__ void ft_qnorm2_parts(const FilteredArgs &a, int p, int tid, double *s_qn) {
  double v = 0.0;
  for (int d = tid; d < a.S; d += 256) v += (double)a.q[(size_t)p * a.S + d] * a.q[(size_t)p * a.S + d];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((tid & 63) == 0) s_qn[tid >> 6] = v;
}
// e = eps32 |q| (1 + 2^-20): the bound of score_rank.hip on |fp32 score - score64|, rounded outward
__device__ __forceinline__ double ft_score_bound(float eps32, const double *s_qn) {
  return (double)eps32 * sqrt(s_qn[0] + s_qn[1] + s_qn[2] + s_qn[3]) * (1.0 + 1.0 / 1048576.0);
}
// key[]: a query's NV maxima keys sorted descending.  theta = the m-th largest; thr = rd(theta - 2 e), -inf with fewer than m
// finite maxima: everything eligible is collected
__device__ __forceinline__ float ft_collect_threshold(const uint32_t *key, int NV, int m, double e) {
  float thr = -__builtin_inff();
  if (m <= NV && key[m - 1] > FT_KEY_NINF) {
    const double theta = (double)ft_unkey(key[m - 1]);
    if (theta == theta) thr = __double2float_rd(theta - 2.0 * e);
  }
  return thr;
}

// ---- select ----

// c entries padded to a power of two and sorted by before(); returns c
__device__ __forceinline__ int ft_reduce(unsigned long long *skey, int *srow, int c, int tid) {
  int n2 = 1;
  while (n2 < c) n2 <<= 1;
  for (int i = c + tid; i < n2; i += 256) {
    skey[i] = 0ull;
    srow[i] = FT_PAD_ROW;
  }
  ft_sort_entries(skey, srow, n2, tid);
  return c;
}

// is id among the query's exclusion list?  One lane per entry (n_excl <= 64); the answer is wave-uniform.
__device__ __forceinline__ bool ft_excluded(const int64_t *ex, int n_excl, int64_t id, int lane) {
  if (n_excl == 0) return false;
  return __ballot(lane < n_excl && ex[lane] == id) != 0ull;
}

// What a select stage does unless it says otherwise: every tag-eligible row is used, every re-scored row is kept, entries
// carry no group, the area is sorted, counters[0] receives the number of entries kept.
struct PlainSelect {
  typedef FilteredStageArgs Args;
  static constexpr bool GROUPED = false, COUNT_COLLECTED = false;
  static constexpr bool BIASED = false;  // true: Sel::score(args, query, score64, row) is what is kept, keyed and returned (K6l)
  struct Query {};  // what a workgroup holds of its query beside the row
  template <class A>
  static __device__ __forceinline__ Query query(const A &, int) { return Query{}; }
  template <class Q>
  static __device__ __forceinline__ bool use_row(const Q &, int64_t, int) { return true; }  // (wave-uniform)
  template <class Q>
  static __device__ __forceinline__ bool keep(const Q &, double, int64_t) { return true; }
  static __device__ __forceinline__ int reduce(unsigned long long *skey, int *srow, unsigned long long *, int c, int tid, int *) {
    return ft_reduce(skey, srow, c, tid);
  }
};

// One workgroup of 256 threads per query; LDS: [cap] keys, GROUPED: [cap] groups, [cap] rows.  Buffer held: its used rows in
// float64, those kept reduced (sorted by before(); GROUPED: one entry per group), first k out, padding (-inf, INT64_MAX),
// count.  Fewer than k is a valid answer.  Buffer overflowed: every tag-eligible row of the index in float64 with the same
// tests, the best k kept in the same LDS area: whenever it has filled to within 64 entries of col_cap it is reduced and cut
// back to the k best, whose last entry -- once there are k -- becomes the bar later rows have to pass.
template <class Sel>
__global__ __launch_bounds__(256) void eligible_select_kernel(typename Sel::Args g) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long es_smem[];
  __shared__ int s_cnt, s_heads;
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cap = a.col_cap;
  unsigned long long *skey = es_smem;                                           // [cap]
  unsigned long long *sgrp = es_smem + cap;                                     // [cap] (GROUPED)
  int *srow = reinterpret_cast<int *>(es_smem + (Sel::GROUPED ? 2 : 1) * cap);  // [cap]
  const float *qrow = a.q + (size_t)p * a.S;
  const typename Sel::Query qu = Sel::query(g, p);
  const int n = a.col_cnt[p];  // (uniform)
  bool have_bar = false;
  unsigned long long bar_key = 0ull;
  int bar_row = 0;
  // four rows of a wave (use[b]: the row exists and is tag-eligible) in float64; lane 0 appends what passes
  auto rescore = [&](const int64_t(&r)[4], bool(&use)[4]) {
    bool any_use = false;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      use[b] = use[b] && Sel::use_row(qu, a.id_base + r[b], lane);
      any_use |= use[b];
    }
    if (!any_use) return;  // (wave-uniform)
    double sc[4];
    wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, sc);
    if (lane == 0) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (!use[b]) continue;
        if constexpr (Sel::BIASED) sc[b] = Sel::score(g, qu, sc[b], r[b]);
        if (!Sel::keep(qu, sc[b], a.id_base + r[b])) continue;
        const unsigned long long key = ft_key64(sc[b]);
        // below the k-th entry: not a new answer (GROUPED: nor better than the entry its own group may hold)
        if (have_bar && !(key > bar_key || (key == bar_key && (int)r[b] < bar_row))) continue;
        const int pos = atomicAdd(&s_cnt, 1);  // (at most 64 appends between two cuts: pos < cap)
        skey[pos] = key;
        srow[pos] = (int)r[b];
        if constexpr (Sel::GROUPED) sgrp[pos] = (unsigned long long)g.groups[r[b]];
      }
    }
  };
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  if (n <= cap) {
    const int32_t *rows = a.col_buf + (size_t)p * cap;
    for (int i0 = w * 4; i0 < n; i0 += 16) {
      int64_t r[4];
      bool use[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        r[b] = rows[min(i0 + b, n - 1)];
        use[b] = i0 + b < n;
      }
      rescore(r, use);
    }
    __syncthreads();
    const int c = Sel::COUNT_COLLECTED ? n : s_cnt;
    if (tid == 0 && c) atomicAdd(a.counters, (unsigned long long)c);
  } else {
    const uint64_t qa = a.q_any ? a.q_any[p] : 0ull, qn = a.q_none ? a.q_none[p] : 0ull;
    for (int64_t n0 = 0; n0 < a.N; n0 += 64) {
#pragma unroll 1
      for (int g = 0; g < 4; ++g) {
        const int64_t base = n0 + g * 16 + w * 4;
        if (base >= a.N) break;  // (wave-uniform)
        int64_t r[4];
        bool use[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          r[b] = (base + b < a.N) ? base + b : a.N - 1;
          use[b] = base + b < a.N;
          if (use[b] && a.tags) {
            const uint64_t t = a.tags[r[b]];
            use[b] = (qa == 0ull || (t & qa) != 0ull) && (t & qn) == 0ull;
          }
        }
        rescore(r, use);
      }
      __syncthreads();
      const int c = s_cnt;
      __syncthreads();
      if (c > cap - 64) {  // (uniform) reduce, cut back to the k best
        const int ng = Sel::reduce(skey, srow, sgrp, c, tid, &s_heads);
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
  const int cnt = min(Sel::reduce(skey, srow, sgrp, s_cnt, tid, &s_heads), a.k);
  for (int j = tid; j < a.k; j += 256) {
    a.out_scores[(size_t)p * a.k + j] = (j < cnt) ? ft_unkey64(skey[j]) : -(double)__builtin_inff();
    a.out_ids[(size_t)p * a.k + j] = (j < cnt) ? a.id_base + srow[j] : INT64_MAX;
    if constexpr (Sel::GROUPED) g.out_groups[(size_t)p * a.k + j] = (j < cnt) ? (int64_t)sgrp[j] : INT64_MAX;
  }
  if (tid == 0) a.out_counts[p] = cnt;
}

// ---- launchers ----

// what every launcher of the family asks of a chunk; maxima: of one with a max sweep and a threshold stage
inline bool eligible_args_ok(const FilteredArgs &a, bool maxima) {
  if (a.col_cap != SSE_COLLECT_CAP) return false;
  if (a.NSPLIT < 1 || (a.NSPLIT & (a.NSPLIT - 1))) return false;  // a power of two: 1, 2, 4, 8, then multiples of 8
  return !maxima || a.NV == (a.NSPLIT < FT_MAXSPLIT ? a.NSPLIT : FT_MAXSPLIT) * 256;
}

// the sweep of a stage for blocks of NQ = 1, 2 or (MAX_NQ = 4) 4 column tiles
// (1 KiB of the workgroup's LDS left to s_any / s_unres)
template <class Stage>
static hipError_t launch_eligible_sweep(const typename Stage::Args &g, hipStream_t st) {
  const FilteredArgs &a = g.f;
  void (*kernel)(typename Stage::Args) = nullptr;
  if (a.NQ == 1) kernel = eligible_sweep_kernel<1, Stage>;
  if (a.NQ == 2) kernel = eligible_sweep_kernel<2, Stage>;
  if constexpr (Stage::MAX_NQ >= 4)
    if (a.NQ == 4) kernel = eligible_sweep_kernel<4, Stage>;
  if (!kernel) return hipErrorInvalidValue;
  return launch_sweep(kernel, a.P, a.NQ, a.KG, a.NSPLIT, SWEEP_LDS_MAX - 1024, st, g);
}

// one workgroup per query of the chunk
template <class Sel>
static hipError_t launch_eligible_select(const typename Sel::Args &g, hipStream_t st) {
  const FilteredArgs &a = g.f;
  const size_t lds = (size_t)a.col_cap * ((Sel::GROUPED ? 2 : 1) * sizeof(unsigned long long) + sizeof(int));
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(eligible_select_kernel<Sel>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(eligible_select_kernel<Sel>, dim3(a.P), dim3(256), lds, st, g);
  return hipGetLastError();
}
