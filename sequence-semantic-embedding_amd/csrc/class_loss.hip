// Full-softmax class loss over the free target matrix for gfx950: the third body of the train step's loss stage (option
// train_class_loss = 1) and the kernel behind sse_class_loss_dev.  Definition: include/sse_hip.h (sse_class_loss_dev), DESIGN
// "Class softmax loss".
//
// The rectangular (B x N) sibling of inbatch_loss.hip, on its scheme: no B x N buffer exists.  The normalised source
// encodings ns [Bt][Sp] and the normalised class table nt [Nt][Sp] are staged once (Bt, Nt, Sp: B, N, S rounded up to 32, zero
// padded), then three passes recompute the 32 x 32 logit tiles where they need them:
//   rows pass      own = row i,    walk = class j:  the running (max, sum) of row i, L_{i,y_i}
//   gradient pass  own = row i,    walk = class j:  d(ns_i) = sum_j G_ij nt_j
//   gradient pass  own = class j,  walk = row i:    d(nt_j) = sum_i G_ij ns_i      for EVERY class j
// out of the pieces of softmax_head.h, which explains the register layout (OWN index on the lane, WALK index in the 16
// accumulator registers).  This file adds the exclusion lists, the positive at j = y_i and the split walk.
//
// Split walk.  A workgroup owns 32 own rows (and, in a gradient pass, 128 or 256 columns of S); with few own tiles -- 4 at
// B = 128, 18 at N = 571 -- such a grid leaves most of the machine idle, so the walk tiles are cut into `split` contiguous
// chunks (class_split), one workgroup per (own tile, chunk).  Each chunk leaves a partial: a (max, sum) pair and L_{i,y_i}
// per row, a partial gradient tile per own tile.  class_rows_merge_kernel merges the pairs in chunk order, class_finish_kernel
// adds the gradient partials in chunk order.  Inside a workgroup the 8 waves take the chunk's tiles w, w + 8, .. and are added
// in wave order.  Every order depends on (B, N, S) alone and there are no atomics (the error flag apart): same inputs, same bits.
//
// Exclusion lists.  Column j is no negative of row i when another verified row of i's source names it.  Rows of one source
// share one list, the sorted distinct target rows of its verified rows; class_list_kernel forms the lists on the device, all
// of them inside one [B] array (a source's list starts where the lists of the sources with smaller keys end).  A row keeps
// (begin, length, lowest, highest) and tests membership only for tiles that overlap [lowest, highest].
#include <algorithm>

#include "softmax_head.h"

namespace {

constexpr int CL_TARGET_WGS = 512;  // split the walk until a pass has about this many workgroups (2 per CU of an MI355X)

struct ClassArgs {
  const float *src_raw, *table, *labels;  // [B][S], [N][S], [B]
  const int32_t *tgt_row, *ks;            // [B] target rows, [B] source keys (first row with the same source)
  float *ns, *nt;                         // [Bt][Sp], [Nt][Sp]
  float *dns, *dnt;                       // [split_s][Bt][Sp], [split_t][Nt][Sp]: the chunks' partial un-normalised gradients
  float *rs, *cs, *lse;                   // [Bt]: 1 / norm, clamp flag, log-sum-exp
  float *rt, *ct;                         // [Nt]
  float *pm, *ps, *pl;                    // [split_r][Bt]: a chunk's (max, sum) over the admitted j != y_i, and L_{i,y_i} (-inf: not in it)
  int4 *meta;                             // [Bt]: {y_i or -1, list begin, list length, bits of z_i * scale * inv_rows}
  int2 *range;                            // [Bt]: {lowest, highest} entry of the row's list ({0, -1}: empty)
  int32_t *excl, *first;                  // [B]: the lists; is row r the first verified row of its source naming its class?
  int32_t *err;
  float *d_src, *d_table;                 // [rows_out][S], [N][S]
  float *row_loss, *row_acc;              // [B]
  int32_t B, Bt, N, Nt, rows_out, S, Sp;
  int32_t split_r, tiles_r;               // rows pass: chunks of the class walk, walk tiles per chunk
  int32_t split_s, tiles_s;               // d(ns) pass
  int32_t split_t, tiles_t;               // d(nt) pass: chunks of the row walk
  float scale, coef;                      // coef = scale * inv_rows
};

// one wave per staged row: rows 0 .. Bt-1 are the sources (with their metadata), rows Bt .. Bt+Nt-1 the classes
__global__ __launch_bounds__(256) void class_prep_kernel(ClassArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= a.Bt + a.Nt) return;
  const bool is_src = row < a.Bt;
  const int r = is_src ? row : row - a.Bt, R = is_src ? a.B : a.N;
  float *n = (is_src ? a.ns : a.nt) + (size_t)r * a.Sp;
  if (r >= R) {
    for (int d = lane; d < a.Sp; d += 64) n[d] = 0.0f;
    if (lane == 0) {
      if (is_src) {
        a.meta[r] = make_int4(-1, 0, 0, 0);
        a.range[r] = make_int2(0, -1);
        a.rs[r] = a.cs[r] = a.lse[r] = 0.0f;
      } else {
        a.rt[r] = a.ct[r] = 0.0f;
      }
    }
    return;
  }
  SmxStage st[1] = {{(is_src ? a.src_raw : a.table) + (size_t)r * a.S, n}};
  smx_stage_rows(st, a.S, a.Sp, lane);
  const float rn = st[0].rn, clamped = st[0].clamped;
  if (!is_src) {
    if (lane == 0) {
      a.rt[r] = rn;
      a.ct[r] = clamped;
    }
    return;
  }
  // is this the first verified row of its source that names its class?  The lanes take 64 earlier rows at a time.
  const int y = a.tgt_row[r], k = a.ks[r];
  const bool valid = y >= 0 && y < a.N;
  const bool verified = valid && a.labels[r] != 0.0f;
  bool first = verified;
  for (int j0 = 0; j0 < r && first; j0 += 64) {
    const int j = j0 + lane;
    const bool same = j < r && a.ks[j] == k && a.tgt_row[j] == y && a.labels[j] != 0.0f;
    if (__ballot(same)) first = false;
  }
  if (lane == 0) {
    if (!valid) atomicOr(a.err, 1);  // a target row out of range, as rows_gather reports it; the row contributes nothing
    a.first[r] = first ? 1 : 0;
    a.rs[r] = rn;
    a.cs[r] = clamped;
  }
}

// one wave per row i: where its source's list lies, and -- a first row -- its own entry written at its sorted position
__global__ __launch_bounds__(256) void class_list_kernel(ClassArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (i >= a.B) return;
  const int k = a.ks[i], y = a.tgt_row[i];
  int before = 0, len = 0, below = 0, lo = INT32_MAX, hi = -1;
  for (int r = lane; r < a.B; r += 64) {
    if (!a.first[r]) continue;
    const int kr = a.ks[r], yr = a.tgt_row[r];
    before += kr < k;
    if (kr == k) {
      len += 1;
      below += yr < y;
      lo = min(lo, yr);
      hi = max(hi, yr);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_xor(before, o);
    len += __shfl_xor(len, o);
    below += __shfl_xor(below, o);
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
  }
  if (lane != 0) return;
  const bool valid = y >= 0 && y < a.N;
  a.meta[i] = make_int4(valid ? y : -1, before, len, valid ? __float_as_int(a.labels[i] * a.coef) : 0);
  a.range[i] = len ? make_int2(lo, hi) : make_int2(0, -1);
  if (a.first[i]) a.excl[before + below] = y;  // (first entries of one source carry distinct y: distinct positions, at most B in all)
}

// first position in excl[begin .. begin + len) whose entry is >= j
__device__ __forceinline__ int class_lower_bound(const int32_t *__restrict__ excl, int begin, int len, int j) {
  int lo = begin, hi = begin + len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (excl[mid] < j) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// bit c set: column j0 + c is excluded for the row with metadata (m, rg).  Zero without a search unless the tile overlaps the
// list's range; the row's own target is never excluded.
__device__ __forceinline__ uint32_t class_excluded_mask(const int32_t *__restrict__ excl, const int4 &m, const int2 &rg, int j0) {
  if (rg.y < j0 || rg.x >= j0 + 32) return 0u;
  const int end = m.y + m.z;
  uint32_t mask = 0u;
  for (int p = class_lower_bound(excl, m.y, m.z, j0); p < end; ++p) {
    const int e = excl[p];
    if (e >= j0 + 32) break;
    if (e != m.x) mask |= 1u << (e - j0);
  }
  return mask;
}

// is column j excluded for the row with metadata (m, rg)?
__device__ __forceinline__ bool class_excluded(const int32_t *__restrict__ excl, const int4 &m, const int2 &rg, int j) {
  if (j == m.x || j < rg.x || j > rg.y) return false;
  const int p = class_lower_bound(excl, m.y, m.z, j);
  return p < m.y + m.z && excl[p] == j;
}

// rows pass: block (x = own row tile, y = chunk of the class walk) leaves the chunk's (max, sum) over the admitted j != y_i and
// L_{i,y_i} for its 32 rows
__global__ __launch_bounds__(SMX_NW * 64) void class_rows_kernel(ClassArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int obase = blockIdx.x * 32, i = obase + (lane & 31);
  const int4 mi = a.meta[i];
  const int2 rg = a.range[i];
  const int t0 = blockIdx.y * a.tiles_r, t1 = min(t0 + a.tiles_r, a.Nt / 32);
  float m = SMX_NEG_INF, s = 0.0f, lyy = SMX_NEG_INF;
  for (int wt = t0 + w; wt < t1; wt += SMX_NW) {
    const f32x16 acc = smx_logit_tile(a.nt, wt * 32, a.ns, obase, a.Sp, lane);
    const uint32_t ex = class_excluded_mask(a.excl, mi, rg, wt * 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = mfma_row(r, lane), j = wt * 32 + c;
      const float x = a.scale * acc[r];
      if (j == mi.x) {
        lyy = x;
      } else if (j < a.N && !((ex >> c) & 1u)) {
        smx_update(m, s, x);
      }
    }
  }
  if (!smx_rows_reduce(m, s, lyy, lane, w)) return;
  const size_t at = (size_t)blockIdx.y * a.Bt + i;
  a.pm[at] = m;
  a.ps[at] = s;
  a.pl[at] = lyy;
}

// the chunks of a row in chunk order: lse_i, row_loss_i, row_acc_i; one thread per row
__global__ __launch_bounds__(256) void class_rows_merge_kernel(ClassArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.B) return;
  float m = a.pm[i], s = a.ps[i], lyy = a.pl[i];
  for (int c = 1; c < a.split_r; ++c) {
    const size_t at = (size_t)c * a.Bt + i;
    smx_merge(m, s, a.pm[at], a.ps[at]);
    lyy = fmaxf(lyy, a.pl[at]);
  }
  if (a.meta[i].x < 0) {  // target row out of range (flagged by class_prep_kernel): nothing
    a.lse[i] = 0.0f;
    a.row_loss[i] = 0.0f;
    a.row_acc[i] = 0.0f;
    return;
  }
  smx_row_close(m, s, lyy, a.labels[i], a.lse[i], a.row_loss[i], a.row_acc[i]);
}

// gradient pass, block (x = own tile, y = tile of S, z = chunk of the walk).  COLS == false: own = row i, walk = class j, out =
// a partial of d(ns); COLS == true: own = class j, walk = row i, out = a partial of d(nt).
template <bool COLS, int ST>
__global__ __launch_bounds__(SMX_NW * 64) void class_grad_kernel(ClassArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int obase = blockIdx.x * 32, o = obase + (lane & 31);
  const int sbase = blockIdx.y * (32 * ST);
  const int nst = min(ST, (a.Sp - sbase) / 32);
  const float *__restrict__ ownN = COLS ? a.nt : a.ns;
  const float *__restrict__ walkN = COLS ? a.ns : a.nt;
  const int own_rows = COLS ? a.Nt : a.Bt, walk_tiles = (COLS ? a.Bt : a.Nt) / 32;
  const int per = COLS ? a.tiles_t : a.tiles_s;
  const int t0 = blockIdx.z * per, t1 = min(t0 + per, walk_tiles);
  int4 mo = make_int4(-1, 0, 0, 0);
  int2 ro = make_int2(0, -1);
  float lse_o = 0.0f;
  if (!COLS) {
    mo = a.meta[o];
    ro = a.range[o];
    lse_o = a.lse[o];
  }
  f32x16 out[ST];
  smx_grad_zero(out);
  for (int wt = t0 + w; wt < t1; wt += SMX_NW) {
    f32x16 g = smx_logit_tile(walkN, wt * 32, ownN, obase, a.Sp, lane);
    uint32_t ex = 0u;
    if (!COLS) ex = class_excluded_mask(a.excl, mo, ro, wt * 32);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = mfma_row(r, lane), wi = wt * 32 + c;
      float v = 0.0f;
      if (COLS) {  // walk row i = wi (rows B .. Bt-1 carry coefficient 0), own class j = o
        const int4 mi = a.meta[wi];
        const float coef = __int_as_float(mi.w);  // z_i * scale * inv_rows
        if (coef != 0.0f && o < a.N && !class_excluded(a.excl, mi, a.range[wi], o))
          v = smx_grad_entry(coef, a.scale, g[r], a.lse[wi], o == mi.x);
      } else {     // own row i = o, walk class j = wi
        const float coef = __int_as_float(mo.w);
        if (coef != 0.0f && wi < a.N && !((ex >> c) & 1u)) v = smx_grad_entry(coef, a.scale, g[r], lse_o, wi == mo.x);
      }
      g[r] = v;
    }
    SMX_GRAD_ACCUMULATE(ST, out, g, walkN + (size_t)(wt * 32) * a.Sp + sbase, a.Sp, nst, lane)
  }
  float *dst = (COLS ? a.dnt : a.dns) + (size_t)blockIdx.z * own_rows * a.Sp;  // this chunk's partial
  smx_grad_reduce_store(out, dst + (size_t)obase * a.Sp + sbase, a.Sp, nst, lane, w);
}

// one wave per output row (rows_out source rows, then N classes): the chunks' partials added in chunk order, then the
// l2_normalize backward; source rows B .. rows_out-1 zeroed
__global__ __launch_bounds__(256) void class_finish_kernel(ClassArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= a.rows_out + a.N) return;
  const bool is_src = row < a.rows_out;
  const int r = is_src ? row : row - a.rows_out;
  float *out = (is_src ? a.d_src : a.d_table) + (size_t)r * a.S;
  if (is_src && r >= a.B) {
    for (int d = lane; d < a.S; d += 64) out[d] = 0.0f;
    return;
  }
  const float *n = (is_src ? a.ns : a.nt) + (size_t)r * a.Sp;
  float *dn = (is_src ? a.dns : a.dnt) + (size_t)r * a.Sp;
  const int split = is_src ? a.split_s : a.split_t;
  const size_t stride = (size_t)(is_src ? a.Bt : a.Nt) * a.Sp;
  if (split > 1) {
    for (int d = lane; d < a.S; d += 64) {
      float v = dn[d];
      for (int c = 1; c < split; ++c) v += dn[c * stride + d];
      dn[d] = v;  // (this lane's own element: the lane reads it back below)
    }
  }
  const SmxUnstage un[1] = {{n, dn, is_src ? a.rs[r] : a.rt[r], is_src ? a.cs[r] : a.ct[r], out}};
  smx_normalize_backward(un, a.S, lane);
}

// the walk of `walk_tiles` tiles in chunks of `per` tiles (the result): one chunk when the own side fills the machine by itself,
// else as many as bring the pass to about CL_TARGET_WGS workgroups, a chunk never below one tile per wave
inline int class_split(int own_wgs, int walk_tiles, int *split) {
  int want = own_wgs >= CL_TARGET_WGS / 2 ? 1 : (CL_TARGET_WGS + own_wgs - 1) / own_wgs;
  want = std::max(1, std::min(want, (walk_tiles + SMX_NW - 1) / SMX_NW));
  const int per = (walk_tiles + want - 1) / want;
  *split = (walk_tiles + per - 1) / per;
  return per;
}

struct ClassPlan {
  size_t Bt, Nt, Sp;
  int s_tiles;  // gradient workgroups along S
  bool wide;
  int split_r, tiles_r, split_s, tiles_s, split_t, tiles_t;
};

inline ClassPlan class_plan(int B, int N, int S) {
  ClassPlan p;
  p.Bt = smx_round32(B);
  p.Nt = smx_round32(N);
  p.Sp = smx_round32(S);
  p.wide = smx_wide(p.Sp);
  p.s_tiles = (int)smx_s_tiles(p.Sp);
  const int bt = (int)(p.Bt / 32), nt = (int)(p.Nt / 32);
  p.tiles_r = class_split(bt, nt, &p.split_r);
  p.tiles_s = class_split(bt * p.s_tiles, nt, &p.split_s);
  p.tiles_t = class_split(nt * p.s_tiles, bt, &p.split_t);
  return p;
}

}  // namespace

// [ns | dns x split_s] (Bt * Sp each), [nt | dnt x split_t] (Nt * Sp each), [rs | cs | lse | (pm | ps | pl) x split_r] (Bt each),
// [rt | ct] (Nt each), meta (Bt int4), range (Bt int2), [excl | first] (Bt ints each).  split * own tiles stays below
// CL_TARGET_WGS + own tiles, so the partials add at most CL_TARGET_WGS * 32 * Sp floats per gradient to (B + N) * Sp.
size_t class_loss_scratch_bytes(int B, int N, int S) {
  const ClassPlan p = class_plan(B, N, S);
  return ((1 + p.split_s) * p.Bt * p.Sp + (1 + p.split_t) * p.Nt * p.Sp + (3 + 3 * p.split_r) * p.Bt + 2 * p.Nt) * sizeof(float) +
         p.Bt * (sizeof(int4) + sizeof(int2) + 2 * sizeof(int32_t));
}

hipError_t launch_class_loss(const float *src_raw, const float *table, const int32_t *tgt_row, const float *labels, const int32_t *src_key,
                             int B, int rows_out, int N, int S, float scale, float inv_rows, void *scratch, int32_t *err, float *d_src,
                             float *d_table, float *row_loss, float *row_acc, hipStream_t st) {
  const ClassPlan p = class_plan(B, N, S);
  const size_t Bt = p.Bt, Nt = p.Nt, Sp = p.Sp;
  ClassArgs a;
  a.src_raw = src_raw;  a.table = table;  a.labels = labels;  a.tgt_row = tgt_row;  a.ks = src_key;
  // (every block below is a multiple of 32 floats long: the int4 / int2 blocks stay 16-byte aligned)
  float *q = (float *)scratch;
  a.ns = q;  q += Bt * Sp;
  a.dns = q;  q += p.split_s * Bt * Sp;
  a.nt = q;  q += Nt * Sp;
  a.dnt = q;  q += p.split_t * Nt * Sp;
  a.rs = q;  a.cs = q + Bt;  a.lse = q + 2 * Bt;  q += 3 * Bt;
  a.pm = q;  a.ps = q + p.split_r * Bt;  a.pl = q + 2 * p.split_r * Bt;  q += 3 * p.split_r * Bt;
  a.rt = q;  a.ct = q + Nt;  q += 2 * Nt;
  a.meta = (int4 *)q;  q += 4 * Bt;
  a.range = (int2 *)q;  q += 2 * Bt;
  a.excl = (int32_t *)q;  a.first = (int32_t *)(q + Bt);
  a.err = err;
  a.d_src = d_src;  a.d_table = d_table;  a.row_loss = row_loss;  a.row_acc = row_acc;
  a.B = B;  a.Bt = (int32_t)Bt;  a.N = N;  a.Nt = (int32_t)Nt;  a.rows_out = rows_out;  a.S = S;  a.Sp = (int32_t)Sp;
  a.split_r = p.split_r;  a.tiles_r = p.tiles_r;  a.split_s = p.split_s;  a.tiles_s = p.tiles_s;  a.split_t = p.split_t;  a.tiles_t = p.tiles_t;
  a.scale = scale;  a.coef = scale * inv_rows;
  const unsigned bt = (unsigned)(Bt / 32), nt = (unsigned)(Nt / 32);
  hipLaunchKernelGGL(class_prep_kernel, dim3((unsigned)((Bt + Nt + 3) / 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(class_list_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(class_rows_kernel, dim3(bt, (unsigned)p.split_r), dim3(SMX_NW * 64), 0, st, a);
  hipLaunchKernelGGL(class_rows_merge_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, a);
  if (d_src && d_table) {
    const dim3 gs(bt, (unsigned)p.s_tiles, (unsigned)p.split_s), gt(nt, (unsigned)p.s_tiles, (unsigned)p.split_t);
    if (!p.wide) {
      hipLaunchKernelGGL((class_grad_kernel<false, SMX_ST>), gs, dim3(SMX_NW * 64), 0, st, a);
      hipLaunchKernelGGL((class_grad_kernel<true, SMX_ST>), gt, dim3(SMX_NW * 64), 0, st, a);
    } else {
      hipLaunchKernelGGL((class_grad_kernel<false, SMX_ST_WIDE>), gs, dim3(SMX_NW * 64), 0, st, a);
      hipLaunchKernelGGL((class_grad_kernel<true, SMX_ST_WIDE>), gt, dim3(SMX_NW * 64), 0, st, a);
    }
    hipLaunchKernelGGL(class_finish_kernel, dim3((unsigned)(((size_t)rows_out + N + 3) / 4)), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}
