// In-batch softmax loss (multiple-negatives ranking loss) for gfx950: the second body of the train step's loss stage and
// the kernel behind sse_inbatch_loss_dev.  Definition: include/sse_hip.h (sse_inbatch_loss_dev), DESIGN "In-batch softmax loss".
//
// No B x B buffer exists.  The normalised encodings are staged once ([Bt][Sp], zero padded: Bt = B rounded up to 32 rows, Sp = S
// rounded up to 32 columns), then three passes recompute the 32 x 32 logit tiles where they need them:
//   rows pass      a workgroup owns 32 rows i and walks the column tiles: lse_i, L_ii, the accuracy bit
//   gradient pass  (own = i, walk = j) d(ns_i) = sum_j G_ij nt_j      a workgroup owns a [32 rows][128 or 256 columns of S]
//   gradient pass  (own = j, walk = i) d(nt_j) = sum_i G_ij ns_i      tile of its output and walks the other batch dimension
// The tile, the running (max, sum), the reductions, the gradient product and the row staging are the pieces of softmax_head.h,
// shared with class_loss.hip; that header explains the register layout (OWN index on the lane, WALK index in the 16 accumulator
// registers) and why every order depends on (B, S) alone.  This file adds the keys, the admission rule (inbatch_admits) and the
// positive on the diagonal.
//
// The head can be cut to a window of rows [row_lo, row_hi) of the batch (sse_inbatch_loss_window_dev; the global closing of a
// data-parallel step, where a rank owns a window of the gathered global batch).  The staging and the rows pass still cover every
// row -- d(nt_j) of a window column needs lse_i of every row i -- while the two gradient passes, the finish kernel and the loss
// outputs shrink to the 32-row tiles of the batch's own numbering that meet the window: a workgroup owns the same tile, walks the
// same tiles in the same order and adds its waves up the same way as in the full head, so a row's bits do not depend on the
// window.  The window [0, B) is the full head, launch for launch.
#include "softmax_head.h"

namespace {

struct InbatchArgs {
  const float *src_raw, *tgt_raw, *labels;  // [B][S], [B][S], [B]
  const int32_t *ks, *kt;                   // [B] keys >= 0
  float *ns, *nt, *dns, *dnt;               // [Bt][Sp]
  float *rs, *rt, *cs, *ct, *lse;           // [Bt]: 1 / norm, clamp flag (sum of squares below 1e-12), log-sum-exp
  int4 *meta;                               // [Bt]: {target key, source key, source key or -1 when the label is 0, bits of z * scale * inv_rows}
  float *d_src, *d_tgt;                     // [rows_out][S]: row r is batch row row_lo + r
  float *row_loss, *row_acc;                // [row_hi - row_lo]
  int32_t B, Bt, rows_out, S, Sp;
  int32_t row_lo, row_hi;                   // the window of batch rows whose outputs are written; tile_lo = row_lo / 32
  int32_t tile_lo;
  float scale, coef;                        // coef = scale * inv_rows
};

// one wave per row of the staged operands; rows B .. Bt-1 and columns S .. Sp-1 are zero
__global__ __launch_bounds__(256) void inbatch_prep_kernel(InbatchArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= a.Bt) return;
  float *ns = a.ns + (size_t)row * a.Sp, *nt = a.nt + (size_t)row * a.Sp;
  if (row >= a.B) {
    for (int d = lane; d < a.Sp; d += 64) {
      ns[d] = 0.0f;
      nt[d] = 0.0f;
    }
    if (lane == 0) {
      a.meta[row] = make_int4(-1, -1, -1, 0);
      a.rs[row] = a.rt[row] = a.cs[row] = a.ct[row] = a.lse[row] = 0.0f;
    }
    return;
  }
  SmxStage r[2] = {{a.src_raw + (size_t)row * a.S, ns}, {a.tgt_raw + (size_t)row * a.S, nt}};
  smx_stage_rows(r, a.S, a.Sp, lane);
  if (lane == 0) {
    const float z = a.labels[row];
    const int ks = a.ks[row];
    a.meta[row] = make_int4(a.kt[row], ks, z != 0.0f ? ks : -1, __float_as_int(z * a.coef));
    a.rs[row] = r[0].rn;
    a.rt[row] = r[1].rn;
    a.cs[row] = r[0].clamped;
    a.ct[row] = r[1].clamped;
  }
}

// is column j (meta mj) admitted for row i (meta mi), i != j?  Tail columns (j >= B) never are.
__device__ __forceinline__ bool inbatch_admits(const int4 &mi, const int4 &mj, int j, int B) {
  return j < B && mj.x != mi.x && mj.z != mi.y;
}

// rows pass: lse_i, row_loss_i, row_acc_i of the 32 rows a workgroup owns
__global__ __launch_bounds__(SMX_NW * 64) void inbatch_rows_kernel(InbatchArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int obase = blockIdx.x * 32, i = obase + (lane & 31);
  const int4 mi = a.meta[i];
  float m = SMX_NEG_INF, s = 0.0f;  // over the admitted columns j != i this lane has seen
  float lii = SMX_NEG_INF;          // L_ii, on the one lane that meets it
  for (int wt = w; wt < a.Bt / 32; wt += SMX_NW) {
    const f32x16 acc = smx_logit_tile(a.nt, wt * 32, a.ns, obase, a.Sp, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = wt * 32 + mfma_row(r, lane);
      const float x = a.scale * acc[r];
      if (j == i) {
        lii = x;
      } else if (inbatch_admits(mi, a.meta[j], j, a.B)) {
        smx_update(m, s, x);
      }
    }
  }
  if (!smx_rows_reduce(m, s, lii, lane, w) || i >= a.B) return;
  float row_loss, row_acc;
  smx_row_close(m, s, lii, a.labels[i], a.lse[i], row_loss, row_acc);
  if (i >= a.row_lo && i < a.row_hi) {
    a.row_loss[i - a.row_lo] = row_loss;
    a.row_acc[i - a.row_lo] = row_acc;
  }
}

// gradient pass.  COLS == false: own = row i, walk = column j, out = d(ns); COLS == true: own = column j, walk = row i, out = d(nt).
// Workgroup x owns tile tile_lo + x of the batch: the grid covers the tiles that meet the window.
template <bool COLS, int ST>
__global__ __launch_bounds__(SMX_NW * 64) void inbatch_grad_kernel(InbatchArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int obase = (a.tile_lo + blockIdx.x) * 32, o = obase + (lane & 31);
  const int sbase = blockIdx.y * (32 * ST);
  const int nst = min(ST, (a.Sp - sbase) / 32);
  const float *__restrict__ ownN = COLS ? a.nt : a.ns;
  const float *__restrict__ walkN = COLS ? a.ns : a.nt;
  const int4 mo = a.meta[o];
  const float lse_o = a.lse[o];
  f32x16 out[ST];
  smx_grad_zero(out);
  for (int wt = w; wt < a.Bt / 32; wt += SMX_NW) {
    f32x16 g = smx_logit_tile(walkN, wt * 32, ownN, obase, a.Sp, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int wi = wt * 32 + mfma_row(r, lane);
      const int4 mw = a.meta[wi];
      const int i = COLS ? wi : o, j = COLS ? o : wi;
      const int4 &mi = COLS ? mw : mo;
      const int4 &mj = COLS ? mo : mw;
      const float coef = __int_as_float(mi.w);  // z_i * scale * inv_rows; 0 on tail rows and rows with label 0
      float v = 0.0f;
      if (coef != 0.0f && (i == j || inbatch_admits(mi, mj, j, a.B))) {
        const float lse_i = COLS ? a.lse[wi] : lse_o;
        v = smx_grad_entry(coef, a.scale, g[r], lse_i, i == j);
      }
      g[r] = v;
    }
    SMX_GRAD_ACCUMULATE(ST, out, g, walkN + (size_t)(wt * 32) * a.Sp + sbase, a.Sp, nst, lane)
  }
  smx_grad_reduce_store(out, (COLS ? a.dnt : a.dns) + (size_t)obase * a.Sp + sbase, a.Sp, nst, lane, w);
}

// l2_normalize backward of both sides, one wave per output row (batch row row_lo + output row); the output rows behind the
// window, up to rows_out, zeroed
__global__ __launch_bounds__(256) void inbatch_finish_kernel(InbatchArgs a) {
  const int lane = threadIdx.x & 63;
  const int orow = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (orow >= a.rows_out) return;
  float *ds = a.d_src + (size_t)orow * a.S, *dt = a.d_tgt + (size_t)orow * a.S;
  const int row = a.row_lo + orow;
  if (row >= a.row_hi) {
    for (int d = lane; d < a.S; d += 64) {
      ds[d] = 0.0f;
      dt[d] = 0.0f;
    }
    return;
  }
  const SmxUnstage r[2] = {{a.ns + (size_t)row * a.Sp, a.dns + (size_t)row * a.Sp, a.rs[row], a.cs[row], ds},
                           {a.nt + (size_t)row * a.Sp, a.dnt + (size_t)row * a.Sp, a.rt[row], a.ct[row], dt}};
  smx_normalize_backward(r, a.S, lane);
}

// ---- keys
__global__ __launch_bounds__(256) void inbatch_token_hash_kernel(const int32_t *__restrict__ ids, int B, int T, uint32_t *__restrict__ hash) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int32_t *p = ids + (size_t)b * T;
  uint32_t hsh = 2166136261u;  // FNV-1a over the token words
  for (int t = 0; t < T; ++t) hsh = (hsh ^ (uint32_t)p[t]) * 16777619u;
  hash[b] = hsh;
}

// key[b] = the first row with b's tokens.  One wave per row b: its lanes take 64 earlier rows at a time, a row of equal hash is
// compared token by token, the lowest matching lane ends the search (no match: row b itself).
__global__ __launch_bounds__(256) void inbatch_token_key_kernel(const int32_t *__restrict__ ids, const uint32_t *__restrict__ hash, int B,
                                                                int T, int32_t *__restrict__ key) {
  const int lane = threadIdx.x & 63;
  const int b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (b >= B) return;
  const uint32_t hb = hash[b];
  const int32_t *p = ids + (size_t)b * T;
  int k = b;
  for (int j0 = 0; j0 < b; j0 += 64) {
    const int j = j0 + lane;
    bool same = j < b && hash[j] == hb;
    if (same) {
      const int32_t *q = ids + (size_t)j * T;
      for (int t = 0; t < T && same; ++t) same = p[t] == q[t];
    }
    const unsigned long long hit = __ballot(same);
    if (hit) {
      k = j0 + __ffsll((long long)hit) - 1;
      break;
    }
  }
  if (lane == 0) key[b] = k;
}

// the same search over one key word per row (keys == nullptr: every row distinct)
template <typename K>
__global__ __launch_bounds__(256) void inbatch_value_key_kernel(const K *__restrict__ keys, int B, int32_t *__restrict__ key) {
  const int lane = threadIdx.x & 63;
  const int b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (b >= B) return;
  int k = b;
  if (keys) {
    const K kb = keys[b];
    for (int j0 = 0; j0 < b; j0 += 64) {
      const int j = j0 + lane;
      const unsigned long long hit = __ballot(j < b && keys[j] == kb);
      if (hit) {
        k = j0 + __ffsll((long long)hit) - 1;
        break;
      }
    }
  }
  if (lane == 0) key[b] = k;
}

}  // namespace

hipError_t launch_inbatch_token_keys(const int32_t *ids, int B, int T, uint32_t *hash, int32_t *key, hipStream_t st) {
  hipLaunchKernelGGL(inbatch_token_hash_kernel, dim3((B + 255) / 256), dim3(256), 0, st, ids, B, T, hash);
  hipLaunchKernelGGL(inbatch_token_key_kernel, dim3((B + 3) / 4), dim3(256), 0, st, ids, hash, B, T, key);
  return hipGetLastError();
}

hipError_t launch_inbatch_value_keys(const void *keys, int width, int B, int32_t *key, hipStream_t st) {
  if (width == 64)
    hipLaunchKernelGGL(inbatch_value_key_kernel<int64_t>, dim3((B + 3) / 4), dim3(256), 0, st, (const int64_t *)keys, B, key);
  else
    hipLaunchKernelGGL(inbatch_value_key_kernel<int32_t>, dim3((B + 3) / 4), dim3(256), 0, st, (const int32_t *)keys, B, key);
  return hipGetLastError();
}

// [ns | nt | dns | dnt] (Bt * Sp floats each), [rs | rt | cs | ct | lse] (Bt floats each), meta (Bt int4)
size_t inbatch_scratch_bytes(int B, int S) {
  const size_t Bt = smx_round32(B), Sp = smx_round32(S);
  return (4 * Bt * Sp + 5 * Bt) * sizeof(float) + Bt * sizeof(int4);
}

hipError_t launch_inbatch_loss_window(const float *src_raw, const float *tgt_raw, const float *labels, const int32_t *src_key,
                                      const int32_t *tgt_key, int B, int row_lo, int row_hi, int rows_out, int S, float scale,
                                      float inv_rows, void *scratch, float *d_src, float *d_tgt, float *row_loss, float *row_acc,
                                      hipStream_t st) {
  const size_t Bt = smx_round32(B), Sp = smx_round32(S);
  InbatchArgs a;
  a.src_raw = src_raw;  a.tgt_raw = tgt_raw;  a.labels = labels;  a.ks = src_key;  a.kt = tgt_key;
  float *p = (float *)scratch;
  a.ns = p;  a.nt = p + Bt * Sp;  a.dns = p + 2 * Bt * Sp;  a.dnt = p + 3 * Bt * Sp;
  p += 4 * Bt * Sp;
  a.rs = p;  a.rt = p + Bt;  a.cs = p + 2 * Bt;  a.ct = p + 3 * Bt;  a.lse = p + 4 * Bt;
  a.meta = (int4 *)(p + 5 * Bt);  // (Bt % 32 == 0: 16-byte aligned)
  a.d_src = d_src;  a.d_tgt = d_tgt;  a.row_loss = row_loss;  a.row_acc = row_acc;
  a.B = B;  a.Bt = (int32_t)Bt;  a.rows_out = rows_out;  a.S = S;  a.Sp = (int32_t)Sp;
  a.scale = scale;  a.coef = scale * inv_rows;
  a.row_lo = row_lo;  a.row_hi = row_hi;  a.tile_lo = row_lo / 32;
  const int NT = (int)(Bt / 32), NTw = (row_hi - 1) / 32 - a.tile_lo + 1;
  hipLaunchKernelGGL(inbatch_prep_kernel, dim3((unsigned)((Bt + 3) / 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(inbatch_rows_kernel, dim3(NT), dim3(SMX_NW * 64), 0, st, a);
  if (d_src && d_tgt) {
    const dim3 grid(NTw, smx_s_tiles(Sp));
    if (!smx_wide(Sp)) {
      hipLaunchKernelGGL((inbatch_grad_kernel<false, SMX_ST>), grid, dim3(SMX_NW * 64), 0, st, a);
      hipLaunchKernelGGL((inbatch_grad_kernel<true, SMX_ST>), grid, dim3(SMX_NW * 64), 0, st, a);
    } else {
      hipLaunchKernelGGL((inbatch_grad_kernel<false, SMX_ST_WIDE>), grid, dim3(SMX_NW * 64), 0, st, a);
      hipLaunchKernelGGL((inbatch_grad_kernel<true, SMX_ST_WIDE>), grid, dim3(SMX_NW * 64), 0, st, a);
    }
    hipLaunchKernelGGL(inbatch_finish_kernel, dim3((rows_out + 3) / 4), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_inbatch_loss(const float *src_raw, const float *tgt_raw, const float *labels, const int32_t *src_key,
                               const int32_t *tgt_key, int B, int rows_out, int S, float scale, float inv_rows, void *scratch,
                               float *d_src, float *d_tgt, float *row_loss, float *row_acc, hipStream_t st) {
  return launch_inbatch_loss_window(src_raw, tgt_raw, labels, src_key, tgt_key, B, 0, B, rows_out, S, scale, inv_rows, scratch, d_src,
                                    d_tgt, row_loss, row_acc, st);
}
