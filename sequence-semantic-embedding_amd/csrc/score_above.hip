// All index rows at or above a score threshold for gfx950 (MI355X): sse_score_above*.
//
// Replaces a FULL row of getSortedResults cut by a confidence threshold (sse_evaluator.py:110-112 ranks every target of a query
// and keeps nbest; data_utils.py:263-267 sorts all N float64 scores per query): the reference can only answer "which targets
// score at least t" by sorting the whole index per query and scanning the sorted row.  Here pair p (query pair_q[p], threshold
// pair_thr[p]) gets exactly the rows r with score64(q, r) >= pair_thr[p] -- the float64 dot product sse_score_topk returns for
// that row -- as a segment of per-pair length, sorted the way sse_score_topk ranks (DESIGN K6f):
//   1. above_prepare_kernel: the threshold narrowed outward to an fp32 interval [lo, hi] (the bound of score_rank.hip).
//   2. score_above_kernel<NQ, false>: the shared sweep (score_sweep.h) on v_mfma_f32_32x32x2_f32: x > hi adds 1 to the
//      pair's sure count, lo <= x <= hi appends the row to the pair's band buffer.
//   3. above_resolve_kernel / above_bruteforce_kernel: band rows decided in float64; a band that outgrew its buffer makes the
//      pair an "overflowed" one, counted (and later listed) by a float64 sweep of the whole index.  Counts are exact.
//   4. above_scan_kernel: offsets = exclusive scan of the counts; offsets[L] is the call's total.
//   5. the emit pass, only when total <= cap (decided on the device: every kernel reads the total first): the SAME sweep
//      (score_above_kernel<NQ, true>: one template, one MFMA chain per accumulator in the same k-order, so a row classifies the
//      same way twice whatever the grid) appends sure rows to the pair's segment through a per-pair cursor; band rows that
//      pass the float64 test and the rows of overflowed pairs are appended by the float64 kernels.  Every append is guarded
//      by the segment's end; a disagreement of the two passes raises the device error word and stores nothing.
//   6. above_score_kernel: float64 scores of the appended rows (wave_exact_dot_n, four rows at a time).
//   7. above_sort_lds_kernel: every run of SSE_ABOVE_SORT_CAP entries of a segment sorted in LDS by (score descending, id
//      ascending); above_merge_kernel: the runs of a longer segment merged pairwise through scratch of the lists' own
//      length (every entry finds its place by a binary search of the sibling run).  Atomics make the append order arbitrary;
//      the total order makes the result deterministic.
#include "sse_kernels.h"
#include "score_exact.h"
#include "score_sweep.h"

#define AB_SORT_THREADS 1024
#define AB_ERR_PAIR 32     // device error word: a pair_q out of range
#define AB_ERR_PASSES 64   // device error word: the emitting pass found other rows than the counting pass

__global__ void above_validate_kernel(const int32_t *pair_q, int64_t L, int Q, int32_t *bad, int32_t *err_flag) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < L; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t pq = pair_q[p];
    if (pq < 0 || pq >= Q) {
      atomicOr(bad, 1);
      atomicOr(err_flag, AB_ERR_PAIR);
    }
  }
}

__device__ __forceinline__ bool above_skip(const AboveArgs &a) {
  if (*a.bad) return true;
  return a.emit && *a.total > a.cap;
}

// guarded append of one global id to pair p's segment
__device__ __forceinline__ void above_append(const AboveArgs &a, int p, int64_t id) {
  const int64_t s0 = a.offsets[p], s1 = a.offsets[p + 1];
  const int64_t pos = s0 + (int64_t)atomicAdd(a.cursor + p, 1ull);
  if (pos < s1 && pos < a.cap) a.out_ids[pos] = id;
  else atomicOr(a.err_flag, AB_ERR_PASSES);
}

// one wave per pair: fp32 interval, zeroed counts.  Emit pass: an overflowed pair gets an interval nothing falls into (the
// float64 sweep lists it).
__global__ __launch_bounds__(256) void above_prepare_kernel(AboveArgs a) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.P) return;
  if (above_skip(a)) return;
  const float *qrow = a.q + (size_t)a.pair_q[p] * a.S;
  double qn = 0.0;
  for (int d = lane; d < a.S; d += 64) qn += (double)qrow[d] * qrow[d];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) qn += __shfl_xor(qn, o);
  if (lane == 0) {
    const double s = a.pair_thr[p];
    const double e = (double)a.eps32 * sqrt(qn) * (1.0 + 1.0 / 1048576.0);
    float lo = __double2float_rd(s - e), hi = __double2float_ru(s + e);
    if (a.emit && a.ovf[p]) lo = hi = __builtin_nanf("");
    a.lo[p] = lo;
    a.hi[p] = hi;
    a.sure[p] = 0ull;
    a.band_cnt[p] = 0;
  }
}

// The shared sweep (score_sweep.h), one (query, threshold) pair per column.  EMIT: rows above hi are appended to the pair's
// segment instead of counted.
template <int NQ, bool EMIT>
__global__ __launch_bounds__(SWEEP_THREADS) void score_above_kernel(AboveArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ab_smem[];  // [KG][NQ][256]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KG = a.KG;
  if (above_skip(a)) return;  // (uniform)
  int split, qb;
  sweep_decode(a.NSPLIT, split, qb);
  if (qb * NQ * 32 >= a.P) return;

  sweep_stage_queries<NQ, true>(ab_smem, a.q, a.pair_q, qb, a.P, a.S, KG, tid);
  float lo[NQ], hi[NQ];
  int pr[NQ], cnt[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    pr[q] = (qb * NQ + q) * 32 + (lane & 31);
    const bool live = pr[q] < a.P;
    lo[q] = live ? a.lo[pr[q]] : __builtin_inff();
    hi[q] = live ? a.hi[pr[q]] : __builtin_inff();
    cnt[q] = 0;
  }
  __syncthreads();

  int t0, t1;
  sweep_tile_range(a.NT, a.NSPLIT, split, t0, t1);
  const float *qs = ab_smem + lane * 4;
  const int tail_tile = sweep_tail_tile(a.N);
  const int nlim = (int)a.N;

  for (int tile = t0 + w; tile < t1; tile += SWEEP_THREADS / 64) {
    SWEEP_TILE_MFMA(NQ, a.idxp, tile, KG, qs, lane, acc);

    const int rbase = sweep_rbase(tile, lane);
    const bool tail = (tile == tail_tile);  // (uniform)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (tail) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = (sweep_row(rbase, r) >= nlim) ? -__builtin_inff() : acc[q][r];
      }
      int cgt = 0, cge = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        cgt += (acc[q][r] > hi[q]) ? 1 : 0;
        cge += (acc[q][r] >= lo[q]) ? 1 : 0;
      }
      if (EMIT) {
        if (cgt) {  // (hi of a pair past the chunk is +inf: pr[q] < P here)
          unsigned sm = 0;
#pragma unroll
          for (int r = 0; r < 16; ++r) sm |= (acc[q][r] > hi[q]) ? (1u << r) : 0u;
          const int64_t s1 = min(a.offsets[pr[q] + 1], a.cap);
          int64_t pos = a.offsets[pr[q]] + (int64_t)atomicAdd(a.cursor + pr[q], (unsigned long long)cgt);
          while (sm) {
            const int r = __ffs((int)sm) - 1;
            sm &= sm - 1;
            const int row = sweep_row(rbase, r);
            if (pos < s1 && row < nlim) a.out_ids[pos] = a.id_base + row;
            else atomicOr(a.err_flag, AB_ERR_PASSES);
            ++pos;
          }
        }
      } else {
        cnt[q] += cgt;
      }
      if (__builtin_expect(cge != cgt, 0)) {
        unsigned bm = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) bm |= (acc[q][r] >= lo[q] && acc[q][r] <= hi[q]) ? (1u << r) : 0u;
        while (bm) {
          const int r = __ffs((int)bm) - 1;
          bm &= bm - 1;
          const int row = sweep_row(rbase, r);
          if (row < nlim && pr[q] < a.P) sweep_append(a.band_cnt, a.band_buf, a.band_cap, pr[q], row);
        }
      }
    }
  }
  if (!EMIT) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int c = cnt[q] + __shfl_xor(cnt[q], 32);
      if (lane < 32 && pr[q] < a.P && c) atomicAdd(a.sure + pr[q], (unsigned long long)c);
    }
  }
}

// one wave per pair: float64 scores of the band rows, four at a time.  Count pass: counts = sure + band rows at or above the
// threshold, ovf = the band outgrew its buffer.  Emit pass: those band rows appended.
__global__ __launch_bounds__(256) void above_resolve_kernel(AboveArgs a) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.P) return;
  if (above_skip(a)) return;
  const int n = a.band_cnt[p];
  if (a.emit) {
    if (a.ovf[p]) return;
    if (n > a.band_cap) {  // (the counting pass held this band)
      if (lane == 0) atomicOr(a.err_flag, AB_ERR_PASSES);
      return;
    }
  } else {
    if (lane == 0) a.ovf[p] = (n > a.band_cap) ? 1 : 0;
    if (n > a.band_cap) return;  // above_bruteforce_kernel
  }
  const float *qrow = a.q + (size_t)a.pair_q[p] * a.S;
  const int32_t *rows = a.band_buf + (size_t)p * a.band_cap;
  const double s = a.pair_thr[p];
  long long c = 0;
  for (int i0 = 0; i0 < n; i0 += 4) {
    int64_t r[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = rows[min(i0 + b, n - 1)];
    double ex[4];
    wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, ex);
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (i0 + b < n && ex[b] >= s) {
        ++c;
        if (a.emit && lane == 0) above_append(a, p, a.id_base + r[b]);
      }
  }
  if (lane == 0 && !a.emit) {
    a.counts[p] = (int64_t)a.sure[p] + c;
    if (n) atomicAdd(a.counters, (unsigned long long)n);
  }
}

// one workgroup per overflowed pair: every row of the index in float64
__global__ __launch_bounds__(256) void above_bruteforce_kernel(AboveArgs a) {
  __shared__ long long s_c[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (above_skip(a)) return;
  if (a.emit ? !a.ovf[p] : a.band_cnt[p] <= a.band_cap) return;  // (uniform)
  const float *qrow = a.q + (size_t)a.pair_q[p] * a.S;
  const double s = a.pair_thr[p];
  long long c = 0;
  for (int64_t n0 = (int64_t)w * 4; n0 < a.N; n0 += 16) {
    int64_t r[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = (n0 + b < a.N) ? n0 + b : a.N - 1;
    double ex[4];
    wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, ex);
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (n0 + b < a.N && ex[b] >= s) {
        ++c;
        if (a.emit && lane == 0) above_append(a, p, a.id_base + r[b]);
      }
  }
  if (a.emit) return;
  if (lane == 0) s_c[w] = c;
  __syncthreads();
  if (tid == 0) {
    a.counts[p] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    atomicAdd(a.counters, (unsigned long long)a.N);
    atomicAdd(a.counters + 1, 1ull);
  }
}

// one workgroup: offsets[1 .. L] hold the counts; inclusive scan in place, offsets[0] = 0.  A thread owns a contiguous slice.
__global__ __launch_bounds__(1024) void above_scan_kernel(int64_t *offsets, int64_t L, const int32_t *bad) {
  __shared__ long long s_sum[1024];
  if (*bad) return;
  const int tid = threadIdx.x;
  const int64_t per = (L + 1023) / 1024;
  const int64_t b = min(L, tid * per), e = min(L, b + per);
  long long t = 0;
  for (int64_t i = b; i < e; ++i) t += offsets[1 + i];
  s_sum[tid] = t;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele over the 1024 slice sums
    const long long v = (tid >= o) ? s_sum[tid - o] : 0;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  long long run = s_sum[tid] - t;
  for (int64_t i = b; i < e; ++i) {
    run += offsets[1 + i];
    offsets[1 + i] = run;
  }
  if (tid == 0) offsets[0] = 0;
}

__device__ __forceinline__ bool lists_skip(const AboveListArgs &a) {
  if (*a.bad) return true;
  return a.offsets[a.L] > a.cap;
}

// the pair whose segment holds entry e (0 <= e < offsets[L]): the last p with offsets[p] <= e
__device__ __forceinline__ int64_t above_find_pair(const int64_t *offsets, int64_t L, int64_t e) {
  int64_t lo = 0, hi = L;  // answer in [lo, hi)
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// a wave scores four consecutive entries: together when they belong to one pair, else one by one (the same sums either way)
__global__ __launch_bounds__(256) void above_score_kernel(AboveListArgs a) {
  if (lists_skip(a)) return;
  const int lane = threadIdx.x & 63;
  const int64_t total = a.offsets[a.L];
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); g * 4 < total; g += nw) {
    const int64_t e0 = g * 4;
    const int nb = (int)min((int64_t)4, total - e0);
    int64_t r[4];
    bool okrow = true;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      r[b] = a.ids[e0 + min(b, nb - 1)] - a.id_base;
      if (r[b] < 0 || r[b] >= a.N) {  // (a slot the emitting pass never filled: flagged there)
        r[b] = 0;
        okrow = false;
      }
    }
    if (!okrow && lane == 0) atomicOr(a.err_flag, AB_ERR_PASSES);
    const int64_t p0 = above_find_pair(a.offsets, a.L, e0), p1 = above_find_pair(a.offsets, a.L, e0 + nb - 1);
    double ex[4];
    if (p0 == p1) {
      wave_exact_dot_n<4>(a.q + (size_t)a.pair_q[p0] * a.S, a.idxp, a.idx64, r, a.S, a.KG, lane, ex);
    } else {
      for (int b = 0; b < nb; ++b) {
        const int64_t p = above_find_pair(a.offsets, a.L, e0 + b);
        ex[b] = wave_exact_dot(a.q + (size_t)a.pair_q[p] * a.S, a.idxp, a.idx64, r[b], a.S, a.KG, lane);
      }
    }
    if (lane == 0)
      for (int b = 0; b < nb; ++b) a.scores[e0 + b] = ex[b];
  }
}

// Runs of SSE_ABOVE_SORT_CAP entries of every segment, sorted in LDS by a bitonic network over the next power of two
// (padding: score -inf, id INT64_MAX -- after every real entry).  blockIdx.x strides the pairs, blockIdx.y a segment's runs.
__global__ __launch_bounds__(AB_SORT_THREADS) void above_sort_lds_kernel(AboveListArgs a) {
  extern __shared__ __attribute__((aligned(16))) double so_smem[];
  if (lists_skip(a)) return;
  double *ks = so_smem;
  int64_t *ki = reinterpret_cast<int64_t *>(so_smem + SSE_ABOVE_SORT_CAP);
  const int tid = threadIdx.x;
  for (int64_t p = blockIdx.x; p < a.L; p += gridDim.x) {
    const int64_t s0 = a.offsets[p], len = a.offsets[p + 1] - s0;
    if (blockIdx.y == 0 && tid == 0) {
      if ((int64_t)a.cursor[p] != len) atomicOr(a.err_flag, AB_ERR_PASSES);
      if (len > SSE_ABOVE_SORT_CAP) atomicAdd(a.counters + 2, 1ull);
    }
    for (int64_t c0 = (int64_t)blockIdx.y * SSE_ABOVE_SORT_CAP; c0 < len; c0 += (int64_t)gridDim.y * SSE_ABOVE_SORT_CAP) {
      const int n = (int)min((int64_t)SSE_ABOVE_SORT_CAP, len - c0);
      if (n < 2) continue;  // (uniform)
      int n2 = 2;
      while (n2 < n) n2 <<= 1;
      for (int i = tid; i < n2; i += AB_SORT_THREADS) {
        ks[i] = (i < n) ? a.scores[s0 + c0 + i] : -(double)__builtin_inff();
        ki[i] = (i < n) ? a.ids[s0 + c0 + i] : INT64_MAX;
      }
      __syncthreads();
      for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int t = tid; t < (n2 >> 1); t += AB_SORT_THREADS) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
            const double si = ks[i], sl = ks[l];
            const int64_t ii = ki[i], il = ki[l];
            const bool fwd = (i & k) == 0;  // this block of k ends up in ranking order / in reverse
            if (fwd ? before(sl, il, si, ii) : before(si, ii, sl, il)) {
              ks[i] = sl;
              ki[i] = il;
              ks[l] = si;
              ki[l] = ii;
            }
          }
          __syncthreads();
        }
      for (int i = tid; i < n; i += AB_SORT_THREADS) {
        a.scores[s0 + c0 + i] = ks[i];
        a.ids[s0 + c0 + i] = ki[i];
      }
      __syncthreads();
    }
  }
}

// One merge pass over every segment: its sorted runs of W entries merged pairwise from src into dst.  An entry's place is its
// index in its own run plus the number of entries of the sibling run ranked before it (the order is total: ids differ); a run
// without a sibling is copied.  Every place lies inside the entry's own pair of runs.
__global__ __launch_bounds__(256) void above_merge_kernel(AboveListArgs a, const double *src_s, const int64_t *src_i, double *dst_s,
                                                          int64_t *dst_i, int64_t W) {
  if (lists_skip(a)) return;
  const int64_t total = a.offsets[a.L];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = above_find_pair(a.offsets, a.L, e);
    const int64_t s0 = a.offsets[p], len = a.offsets[p + 1] - s0, k = e - s0;
    const int64_t run = k / W, a0 = (run >> 1) * 2 * W;       // this pair of runs: [a0, a0 + W) and [a0 + W, b1)
    const int64_t b0 = min(len, a0 + W), b1 = min(len, a0 + 2 * W);
    const bool in_a = (run & 1) == 0;
    const int64_t o0 = in_a ? b0 : a0, on = in_a ? b1 - b0 : W;  // the sibling run
    const double s = src_s[e];
    const int64_t id = src_i[e];
    int64_t lo = 0, hi = on;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (before(src_s[s0 + o0 + mid], src_i[s0 + o0 + mid], s, id)) lo = mid + 1;
      else hi = mid;
    }
    const int64_t pos = a0 + (k - (in_a ? a0 : b0)) + lo;
    if (pos < len) {
      dst_s[s0 + pos] = s;
      dst_i[s0 + pos] = id;
    }
  }
}

hipError_t launch_above_validate(const int32_t *pair_q, int64_t L, int Q, int32_t *bad, int32_t *err_flag, hipStream_t st) {
  if (L <= 0) return hipSuccess;
  const int64_t blocks = (L + 255) / 256;
  hipLaunchKernelGGL(above_validate_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, pair_q, L, Q, bad, err_flag);
  return hipGetLastError();
}

template <int NQ, bool EMIT>
static hipError_t launch_above_sweep(const AboveArgs &a, hipStream_t st) {
  return launch_sweep(score_above_kernel<NQ, EMIT>, a.P, NQ, a.KG, a.NSPLIT, SWEEP_LDS_MAX, st, a);
}

hipError_t launch_score_above(const AboveArgs &a, hipStream_t st) {
  if (a.P <= 0) return hipSuccess;
  if (a.band_cap > SSE_COLLECT_CAP || a.band_cap < 1) return hipErrorInvalidValue;
  if (!sweep_nsplit_ok(a.NSPLIT)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(above_prepare_kernel, dim3((a.P + 3) / 4), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.emit) {
    if (a.NQ == 4) e = launch_above_sweep<4, true>(a, st);
    else if (a.NQ == 2) e = launch_above_sweep<2, true>(a, st);
    else if (a.NQ == 1) e = launch_above_sweep<1, true>(a, st);
    else e = hipErrorInvalidValue;
  } else {
    if (a.NQ == 4) e = launch_above_sweep<4, false>(a, st);
    else if (a.NQ == 2) e = launch_above_sweep<2, false>(a, st);
    else if (a.NQ == 1) e = launch_above_sweep<1, false>(a, st);
    else e = hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(above_resolve_kernel, dim3((a.P + 3) / 4), dim3(256), 0, st, a);
  hipLaunchKernelGGL(above_bruteforce_kernel, dim3(a.P), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_above_scan(int64_t *offsets, int64_t L, const int32_t *bad, hipStream_t st) {
  hipLaunchKernelGGL(above_scan_kernel, dim3(1), dim3(1024), 0, st, offsets, L, bad);
  return hipGetLastError();
}

hipError_t launch_above_lists(const AboveListArgs &a, hipStream_t st) {
  if (a.L <= 0 || a.cap <= 0) return hipSuccess;
  const int64_t groups = (a.cap + 3) / 4, sblocks = (groups + 3) / 4;
  hipLaunchKernelGGL(above_score_kernel, dim3((int)(sblocks < 16384 ? sblocks : 16384)), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t maxlen = a.cap < a.N ? a.cap : a.N;  // no segment is longer
  const int64_t runs = (maxlen + SSE_ABOVE_SORT_CAP - 1) / SSE_ABOVE_SORT_CAP;
  const size_t lds = (size_t)SSE_ABOVE_SORT_CAP * 16;
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(above_sort_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(above_sort_lds_kernel, dim3((int)(a.L < 4096 ? a.L : 4096), (int)(runs < 64 ? runs : 64)), dim3(AB_SORT_THREADS), lds,
                     st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (runs > 1) {
    if (!a.scratch_ids || !a.scratch_scores) return hipErrorInvalidValue;
    const int64_t mblocks = (a.cap + 255) / 256;
    const dim3 mgrid((int)(mblocks < 16384 ? mblocks : 16384));
    int pass = 0;
    // an even number of passes: the lists end where they began (a pass past the last merge copies)
    for (int64_t W = SSE_ABOVE_SORT_CAP; W < maxlen || (pass & 1); W *= 2, ++pass) {
      if (pass & 1) hipLaunchKernelGGL(above_merge_kernel, mgrid, dim3(256), 0, st, a, a.scratch_scores, a.scratch_ids, a.scores, a.ids, W);
      else hipLaunchKernelGGL(above_merge_kernel, mgrid, dim3(256), 0, st, a, a.scores, a.ids, a.scratch_scores, a.scratch_ids, W);
    }
    e = hipGetLastError();
  }
  return e;
}
