// Softmax log-partition over the tag-eligible rows of the resident index for gfx950 (MI355X): sse_score_lse* (DESIGN K6m).
//
//   out_lse[p] = log sum_{eligible r} exp(z_r),   z_r = scale (score64(p, r) + (double)w[p] (double)bias[r])
//
// One fp32 MFMA sweep (score_sweep.h) with the eligibility logic and the fused bias of eligible_sweep_kernel and an epilogue
// that keeps, per lane and column tile, a running (m, sum, count):
//   y = fmaf(w, bias[r], fp32 score)            the value sse_score_topk_biased's sweep looks at
//   x = y c, c = scale log2(e)                  the logit in bits
//   m = an INTEGER >= every x seen so far       the reference: 2^m, a power of two
//   sum = sum 2^(x - m)                         float64 across tiles, fp32 over a tile's 16 rows
// A tile whose largest eligible x exceeds m raises m to its ceiling and rescales sum by 2^(m_old - m_new): an exact ldexp,
// so an index sorted by ascending score (the reference rises on every tile) costs no accuracy.  x - m is formed as
//   t = fmaf(y, c_lo, fmaf(y, c_hi, -m)),  c_hi + c_lo = c to 2^-48,
// whose roundings are relative to |t|, not to |x|: the terms that carry the sum have |t| of a few bits whatever the scale.
// Masked rows (tail padding, ineligible rows, columns past P) are SELECTED away, never multiplied: a padded row's 2^(0 - m)
// can be +inf and contributes nothing.  The per (split, wave, lane half) partials go to global memory with one 16-byte
// store each; lse_merge_kernel merges a query's NSPLIT x 16 partials in a fixed order in float64, adds the counts, takes the
// log and forms the bound.  No floating-point atomic anywhere: the same (N, S, Q) gives the same bits.
//
// The bound (derived in DESIGN K6m).  d = scale e_b bounds |scale y - z_r| (e_b of score_biased.hip, = e without a bias), and
// moving every logit by at most d moves the log of the sum by at most d.  The rest is below LSE_REST = 2^-16:
//   argument:  two fma roundings of t, 2^-24 (|t| + 2^-7) each, and |x| 2^-48 of c: < 2^-17.5 bits for |t| <= 64, times
//              ln 2; the terms with t < -64 together weigh < 2^31 2^-64 of a sum that is >= 1/4
//   v_exp_f32: 1 ulp, 2^-23 relative; results below 2^-126 flushed: < 2^31 2^-126 of the sum
//   tile sum:  15 fp32 additions of positive terms, 15 2^-24
//   the float64 additions, the merge, the log and the bound's own arithmetic: < 2^-40
#include "score_eligible.h"

#define LSE_M_EMPTY (-(1 << 24))  // the reference of an empty partial: below every ceil(x) inside the claim (|x| < 2^17)
#define LSE_REST (1.0 / 65536.0)  // the non-dot part of out_bound

struct alignas(16) LsePartial {
  double sum;    // sum of 2^(x - m) over the partial's rows
  int32_t m;     // LSE_M_EMPTY: no row
  int32_t count; // eligible rows
};

// One workgroup = (block of NQ x 32 queries, index split), as eligible_sweep_kernel; the dynamic LDS is the block's query
// fragments [KG][NQ][256].
template <int NQ>
__global__ __launch_bounds__(SWEEP_THREADS) void lse_sweep_kernel(LseArgs g) {
  extern __shared__ __attribute__((aligned(16))) float lse_smem[];  // [KG][NQ][256]
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
  sweep_stage_queries<NQ, false>(lse_smem, a.q, nullptr, qb, a.P, a.S, KG, tid);
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
  int pr[NQ], m[NQ], cnt[NQ];
  bool live[NQ];
  float wt[NQ];
  double sum[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    pr[q] = (qb * NQ + q) * 32 + (lane & 31);
    live[q] = pr[q] < a.P;
    qany[q] = (live[q] && a.q_any) ? a.q_any[pr[q]] : 0ull;
    qnone[q] = (live[q] && a.q_none) ? a.q_none[pr[q]] : 0ull;
    wt[q] = (live[q] && g.weight) ? g.weight[pr[q]] : 0.0f;
    m[q] = LSE_M_EMPTY;
    cnt[q] = 0;
    sum[q] = 0.0;
  }
  __syncthreads();
  const bool may_skip = a.skip && a.tags && !s_unres;
  const unsigned long long blk_any = s_any;

  int t0, t1;
  sweep_tile_range(a.NT, a.NSPLIT, split, t0, t1);
  const float *qs = lse_smem + lane * 4;
  const int tail_tile = sweep_tail_tile(a.N);
  const int nlim = (int)a.N;
  const float c_hi = g.c_hi, c_lo = g.c_lo;
  int skipped = 0;

  for (int tile = t0 + w; tile < t1; tile += SWEEP_THREADS / 64) {
    if (may_skip && (a.tile_sum[tile] & blk_any) == 0ull) {  // (wave-uniform) no eligible row for any query of the block
      ++skipped;
      continue;
    }
    SWEEP_TILE_MFMA(NQ, a.idxp, tile, KG, qs, lane, acc);

    const int rbase = sweep_rbase(tile, lane);
    const unsigned rowmask = (tile == tail_tile) ? sweep_tail_rowmask(rbase, nlim) : 0xFFFFu;  // (uniform condition)
    if (g.weight) {  // (uniform) the per-row prior, fused into the tile's scores as sse_score_topk_biased's sweep fuses it
      float bs[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) bs[r] = g.bias[sweep_row(rbase, r)];  // (padded to NT * 32 floats)
#pragma unroll
      for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = fmaf(wt[q], bs[r], acc[q][r]);
    }
    unsigned em[NQ];  // eligible rows per query tile
    if (a.tags) {     // (uniform)
      uint64_t tg[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) tg[r] = a.tags[sweep_row(rbase, r)];  // (padded to NT * 32 words)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        unsigned mk = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool ok = (qany[q] == 0ull || (tg[r] & qany[q]) != 0ull) && (tg[r] & qnone[q]) == 0ull;
          mk |= ok ? (1u << r) : 0u;
        }
        em[q] = live[q] ? (mk & rowmask) : 0u;
      }
    } else {
#pragma unroll
      for (int q = 0; q < NQ; ++q) em[q] = live[q] ? rowmask : 0u;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      // the reference: raised to the ceiling of the tile's largest eligible logit (x rounded once: any integer within a bit
      // of the maximum serves, the terms below are formed against the integer itself)
      float xmax = -__builtin_inff();
#pragma unroll
      for (int r = 0; r < 16; ++r) xmax = fmaxf(xmax, ((em[q] >> r) & 1u) ? acc[q][r] * c_hi : -__builtin_inff());
      const int mt = (xmax > -__builtin_inff()) ? (int)ceilf(xmax) : LSE_M_EMPTY;  // (a NaN: outside the claim, no fault)
      const int mn = max(m[q], mt);
      const float mf = (float)mn;  // (exact: |mn| <= 2^24)
      float ts = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float t = fmaf(acc[q][r], c_lo, fmaf(acc[q][r], c_hi, -mf));
        const float e = __builtin_amdgcn_exp2f(t);
        ts += ((em[q] >> r) & 1u) ? e : 0.0f;
      }
      sum[q] = ldexp(sum[q], m[q] - mn) + (double)ts;  // (sum == 0 while m is LSE_M_EMPTY; the shift is exact or to zero)
      m[q] = mn;
      cnt[q] += __popc(em[q]);
    }
  }
  // partial of (query, split, wave, lane half): written by every live column, rows or none
  const int slot = split * 16 + w * 2 + (lane >> 5);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (!live[q]) continue;
    LsePartial v;
    v.sum = sum[q];
    v.m = m[q];
    v.count = cnt[q];
    g.part[(size_t)pr[q] * (a.NSPLIT * 16) + slot] = v;
  }
  if (skipped && lane == 0) atomicAdd(a.counters, (unsigned long long)skipped);
}

// (m, sum) of the union of two partials: the larger reference, both sums shifted onto it (exact), one float64 addition.
// Symmetric in its arguments, so the xor tree below leaves every lane with the same bits.
__device__ __forceinline__ void lse_merge(int &m, double &s, int m2, double s2) {
  const int mn = max(m, m2);
  s = ldexp(s, m - mn) + ldexp(s2, m2 - mn);
  m = mn;
}

// One workgroup of 256 threads per query: |q| by all (ft_qnorm2_parts), the query's NSPLIT x 16 partials by wave 0 -- lane l
// takes partials l, l + 64, ... in that order, then the xor tree -- and the three outputs.
__global__ __launch_bounds__(256) void lse_merge_kernel(LseArgs g) {
  __shared__ double s_qn[4];
  const FilteredArgs &a = g.f;
  const int p = blockIdx.x, tid = threadIdx.x;
  ft_qnorm2_parts(a, p, tid, s_qn);
  __syncthreads();
  if (tid >= 64) return;
  const int np = a.NSPLIT * 16;
  const LsePartial *src = g.part + (size_t)p * np;
  int m = LSE_M_EMPTY;
  double s = 0.0;
  long long cnt = 0;
  for (int i = tid; i < np; i += 64) {
    const LsePartial v = src[i];
    lse_merge(m, s, v.m, v.sum);
    cnt += v.count;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int m2 = __shfl_xor(m, o);
    const double s2 = __shfl_xor(s, o);
    lse_merge(m, s, m2, s2);
    cnt += __shfl_xor(cnt, o);
  }
  if (tid != 0) return;
  g.out_count[p] = cnt;
  g.out_lse[p] = cnt > 0 ? (log(s) + (double)m * 0.6931471805599453) : -(double)__builtin_inff();
  if (g.out_bound) {
    const double e = ft_score_bound(a.eps32, s_qn);
    double eb = e;
    if (g.weight) {  // e_b as biased_bounds_kernel forms it
      const double qn = sqrt(s_qn[0] + s_qn[1] + s_qn[2] + s_qn[3]);
      const double B = fabs((double)g.weight[p]) * (double)g.bias_absmax[0];
      const double u = 1.0 / 8388608.0;  // 2^-23
      eb = (e + u * (qn * (double)g.norm_max + e + B) + 1.4012984643248171e-45) * (1.0 + 1.0 / 1048576.0);
    }
    g.out_bound[p] = (double)g.scale * eb * (1.0 + 1.0 / 1048576.0) + LSE_REST;
  }
}

size_t score_lse_part_bytes(int P, int NSPLIT) { return (size_t)P * NSPLIT * 16 * sizeof(LsePartial); }

hipError_t launch_score_lse(const LseArgs &g, hipStream_t st) {
  const FilteredArgs &a = g.f;
  if (a.P <= 0) return hipSuccess;
  if (!sweep_nsplit_ok(a.NSPLIT) || !g.part || !g.out_lse || !g.out_count) return hipErrorInvalidValue;
  if (g.weight && (!g.bias || !g.bias_absmax)) return hipErrorInvalidValue;
  if ((a.q_any || a.q_none) && !a.tags) return hipErrorInvalidValue;
  void (*kernel)(LseArgs) = nullptr;
  if (a.NQ == 1) kernel = lse_sweep_kernel<1>;
  if (a.NQ == 2) kernel = lse_sweep_kernel<2>;
  if (a.NQ == 4) kernel = lse_sweep_kernel<4>;
  if (!kernel) return hipErrorInvalidValue;
  hipError_t e = launch_sweep(kernel, a.P, a.NQ, a.KG, a.NSPLIT, SWEEP_LDS_MAX - 1024, st, g);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lse_merge_kernel, dim3(a.P), dim3(256), 0, st, g);
  return hipGetLastError();
}
