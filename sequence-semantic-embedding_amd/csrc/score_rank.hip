// Exact rank of labelled targets over the whole index for gfx950 (MI355X): sse_score_rank*.
//
// Replaces a FULL row of getSortedResults searched for the label (data_utils.py:263-267: np.argsort of all N float64 scores
// of a query, then list.index(label)): the reference can only say where a target landed by sorting the whole index per
// query.  Here the rank of row g for query q is a COUNT -- the number of rows r with before(score64(q, r), r, score64(q, g), g),
// the order sse_score_topk ranks by -- and no list is formed at all:
//   1. rank_prepare_kernel: the float64 threshold score of every (query, row) pair with the re-scorer's own dot product
//      (wave_exact_dot: the bits sse_score_topk returns for that row), narrowed outward to an fp32 interval [lo, hi] that
//      holds every fp32 score the bound eps32 |q| cannot decide.
//   2. score_rank_kernel: [N,S] x [S,P] on v_mfma_f32_32x32x2_f32 from the fragment-order index, the shared sweep of
//      score_sweep.h (index rows = MFMA M, one pair per lane column) with a compare-and-count in place
//      of lists: x > hi adds 1 to the pair's sure count, lo <= x <= hi appends the row to the pair's band buffer, anything
//      else is dropped.  Integer adds: any grid shape gives the same counts.
//   3. rank_resolve_kernel: the band rows re-scored in float64 and counted when before() holds (strict: the label row, which
//      always lands in its own band, is not counted).
//   4. rank_bruteforce_kernel: a pair whose band outgrew its buffer is counted by a float64 sweep of the whole index, one
//      workgroup per pair.  Exact either way.
// Bound: an fp32 MFMA score x of a row differs from its float64 score by at most e = eps32 |q| (eps32 = 2 (S + 2) 5.97e-8
// max|t|, the bound every fp32 candidate pass is certified with, DESIGN K6/K7).  With hi >= s + e and lo <= s - e (both rounded
// outward, e itself inflated by 2^-20): x > hi implies score64 > s (before the label whatever the ids), x < lo implies
// score64 < s (after it), and every row that ties or nearly ties with s sits in [lo, hi].
#include "sse_kernels.h"
#include "score_exact.h"
#include "score_sweep.h"

// pair_q in [0, Q); first form: the label is a row of this index.  One bad pair cancels the whole call: every later kernel
// reads *bad first and writes nothing.
__global__ void rank_validate_kernel(const int32_t *pair_q, const int64_t *pair_id, int64_t L, int Q, int need_row, int64_t id_base,
                                     int64_t N, int32_t *bad, int32_t *err_flag) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < L; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t pq = pair_q[p];
    const int64_t id = pair_id[p];
    if (pq < 0 || pq >= Q || (need_row && (id < id_base || id >= id_base + N))) {
      atomicOr(bad, 1);
      atomicOr(err_flag, 16);
    }
  }
}

// one wave per pair: threshold score, fp32 interval, zeroed counts
__global__ __launch_bounds__(256) void rank_prepare_kernel(RankArgs a) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.P) return;
  if (*a.bad) return;
  const float *qrow = a.q + (size_t)a.pair_q[p] * a.S;
  double qn = 0.0;
  for (int d = lane; d < a.S; d += 64) qn += (double)qrow[d] * qrow[d];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) qn += __shfl_xor(qn, o);
  double s;
  if (a.pair_score_in) s = a.pair_score_in[p];
  else s = wave_exact_dot(qrow, a.idxp, a.idx64, a.pair_id[p] - a.id_base, a.S, a.KG, lane);
  if (lane == 0) {
    const double e = (double)a.eps32 * sqrt(qn) * (1.0 + 1.0 / 1048576.0);
    a.thr64[p] = s;
    if (a.out_score) a.out_score[p] = s;
    a.lo[p] = __double2float_rd(s - e);
    a.hi[p] = __double2float_ru(s + e);
    a.sure[p] = 0ull;
    a.band_cnt[p] = 0;
  }
}

// Count sweep: the shared sweep (score_sweep.h), one (query, label) pair per column.
template <int NQ>
__global__ __launch_bounds__(SWEEP_THREADS) void score_rank_kernel(RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rk_smem[];  // [KG][NQ][256]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KG = a.KG;
  if (*a.bad) return;  // (uniform)
  int split, qb;
  sweep_decode(a.NSPLIT, split, qb);
  if (qb * NQ * 32 >= a.P) return;

  sweep_stage_queries<NQ, true>(rk_smem, a.q, a.pair_q, qb, a.P, a.S, KG, tid);
  // this lane's interval per pair tile (pairs past the chunk: nothing is above +inf, nothing inside an empty interval)
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
  const float *qs = rk_smem + lane * 4;
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
      // rows above hi and rows at or above lo: they differ exactly when a row sits in the band (lo <= hi)
      int cgt = 0, cge = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        cgt += (acc[q][r] > hi[q]) ? 1 : 0;
        cge += (acc[q][r] >= lo[q]) ? 1 : 0;
      }
      cnt[q] += cgt;
      if (__builtin_expect(cge != cgt, 0)) {  // (rare: < 2 rows per pair and sweep on unordered data)
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
  // the two lane halves of a wave hold the same pairs over different rows; one add per (wave, pair)
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = cnt[q] + __shfl_xor(cnt[q], 32);
    if (lane < 32 && pr[q] < a.P && c) atomicAdd(a.sure + pr[q], (unsigned long long)c);
  }
}

// one wave per pair: float64 scores of the band rows, four at a time; out = sure count + the band rows ranked before the label
__global__ __launch_bounds__(256) void rank_resolve_kernel(RankArgs a) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.P) return;
  if (*a.bad) return;
  const int n = a.band_cnt[p];
  if (n > a.band_cap) return;  // overflow: rank_bruteforce_kernel
  const float *qrow = a.q + (size_t)a.pair_q[p] * a.S;
  const int32_t *rows = a.band_buf + (size_t)p * a.band_cap;
  const double s = a.thr64[p];
  const int64_t g = a.pair_id[p];
  long long c = 0;
  for (int i0 = 0; i0 < n; i0 += 4) {
    int64_t r[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = rows[min(i0 + b, n - 1)];
    double ex[4];
    wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, ex);
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (i0 + b < n && before(ex[b], a.id_base + r[b], s, g)) ++c;
  }
  if (lane == 0) {
    a.out_before[p] = (int64_t)a.sure[p] + c;
    if (n) atomicAdd(a.counters, (unsigned long long)n);
  }
}

// one workgroup per overflowed pair: every row of the index in float64 (the manner of exact_topk_kernel)
__global__ __launch_bounds__(256) void rank_bruteforce_kernel(RankArgs a) {
  __shared__ long long s_c[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (*a.bad) return;
  if (a.band_cnt[p] <= a.band_cap) return;  // (uniform)
  const float *qrow = a.q + (size_t)a.pair_q[p] * a.S;
  const double s = a.thr64[p];
  const int64_t g = a.pair_id[p];
  long long c = 0;
  for (int64_t n0 = (int64_t)w * 4; n0 < a.N; n0 += 16) {
    int64_t r[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = (n0 + b < a.N) ? n0 + b : a.N - 1;
    double ex[4];
    wave_exact_dot_n<4>(qrow, a.idxp, a.idx64, r, a.S, a.KG, lane, ex);
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (n0 + b < a.N && before(ex[b], a.id_base + r[b], s, g)) ++c;
  }
  if (lane == 0) s_c[w] = c;
  __syncthreads();
  if (tid == 0) {
    a.out_before[p] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    atomicAdd(a.counters, (unsigned long long)a.N);
    atomicAdd(a.counters + 1, 1ull);
  }
}

hipError_t launch_rank_validate(const int32_t *pair_q, const int64_t *pair_id, int64_t L, int Q, int need_row, int64_t id_base,
                                int64_t N, int32_t *bad, int32_t *err_flag, hipStream_t st) {
  if (L <= 0) return hipSuccess;
  const int64_t blocks = (L + 255) / 256;
  hipLaunchKernelGGL(rank_validate_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, pair_q, pair_id, L, Q,
                     need_row, id_base, N, bad, err_flag);
  return hipGetLastError();
}

template <int NQ>
static hipError_t launch_rank_sweep(const RankArgs &a, hipStream_t st) {
  return launch_sweep(score_rank_kernel<NQ>, a.P, NQ, a.KG, a.NSPLIT, SWEEP_LDS_MAX, st, a);
}

// all four stages of one chunk of a.P pairs
hipError_t launch_score_rank(const RankArgs &a, hipStream_t st) {
  if (a.P <= 0) return hipSuccess;
  if (a.band_cap > SSE_COLLECT_CAP || a.band_cap < 1) return hipErrorInvalidValue;
  if (!sweep_nsplit_ok(a.NSPLIT)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rank_prepare_kernel, dim3((a.P + 3) / 4), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.NQ == 4) e = launch_rank_sweep<4>(a, st);
  else if (a.NQ == 2) e = launch_rank_sweep<2>(a, st);
  else if (a.NQ == 1) e = launch_rank_sweep<1>(a, st);
  else e = hipErrorInvalidValue;
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rank_resolve_kernel, dim3((a.P + 3) / 4), dim3(256), 0, st, a);
  hipLaunchKernelGGL(rank_bruteforce_kernel, dim3(a.P), dim3(256), 0, st, a);
  return hipGetLastError();
}
