// In-batch softmax loss (multiple-negatives ranking loss) for gfx950: the second body of the train step's loss stage and
// the kernel behind sse_inbatch_loss_dev.  Definition: include/sse_hip.h (sse_inbatch_loss_dev), DESIGN "In-batch softmax loss".
//
// No B x B buffer exists.  The normalised encodings are staged once ([Bt][Sp], zero padded: Bt = B rounded up to 32 rows, Sp = S
// rounded up to 32 columns), then three passes recompute the 32 x 32 logit tiles on v_mfma_f32_32x32x2_f32 where they need them:
//   rows pass      a workgroup owns 32 rows i and walks the column tiles: lse_i, L_ii, the accuracy bit
//   gradient pass  (own = i, walk = j) d(ns_i) = sum_j G_ij nt_j      a workgroup owns a [32 rows][128 or 256 columns of S]
//   gradient pass  (own = j, walk = i) d(nt_j) = sum_i G_ij ns_i      tile of its output and walks the other batch dimension
// A logit tile is always formed with the OWN index on the lane and the WALK index in the 16 accumulator registers
// (A operand = walk rows, B operand = own rows), so that
//   - a lane of the rows pass carries one row's running (max, sum) instead of sixteen, and
//   - the gradient tile G, written over the accumulator, is already the A operand of the product that sums over the walk
//     index: register r of lane l holds walk row mfma_row(r, l), which is k = 0 for the lower lane half and k = 1 (4 rows
//     further) for the upper one; the B operand is row mfma_row(r, l) of the walked encodings, one float per lane.
// The waves of a workgroup take walk tiles w, w + NW, ..; their partial results are added in wave order through LDS.  Every
// order depends on (B, S) alone and there are no atomics: the same inputs give the same bits.
#include <cmath>

#include "sse_kernels.h"

namespace {

constexpr int IB_NW = 8;         // waves per workgroup
constexpr int IB_ST = 4;         // 32-column tiles of S per gradient workgroup: 4 up to 128 staged columns, 8 above (half the
constexpr int IB_ST_WIDE = 8;    // logit recomputation per column of S, for 64 more accumulator registers)
constexpr float IB_NEG_INF = -INFINITY;

struct InbatchArgs {
  const float *src_raw, *tgt_raw, *labels;  // [B][S], [B][S], [B]
  const int32_t *ks, *kt;                   // [B] keys >= 0
  float *ns, *nt, *dns, *dnt;               // [Bt][Sp]
  float *rs, *rt, *cs, *ct, *lse;           // [Bt]: 1 / norm, clamp flag (sum of squares below 1e-12), log-sum-exp
  int4 *meta;                               // [Bt]: {target key, source key, source key or -1 when the label is 0, bits of z * scale * inv_rows}
  float *d_src, *d_tgt;                     // [rows_out][S]
  float *row_loss, *row_acc;                // [B]
  int32_t B, Bt, rows_out, S, Sp;
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
  const float *s = a.src_raw + (size_t)row * a.S, *t = a.tgt_raw + (size_t)row * a.S;
  float ss = 0.0f, tt = 0.0f;
  for (int d = lane; d < a.S; d += 64) {
    const float x = s[d], y = t[d];
    ss += x * x;
    tt += y * y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ss += __shfl_xor(ss, o);
    tt += __shfl_xor(tt, o);
  }
  const float rs = 1.0f / sqrtf(fmaxf(ss, 1e-12f)), rt = 1.0f / sqrtf(fmaxf(tt, 1e-12f));  // the clamp of loss_kernel (train.hip)
  for (int d = lane; d < a.Sp; d += 64) {
    ns[d] = d < a.S ? s[d] * rs : 0.0f;
    nt[d] = d < a.S ? t[d] * rt : 0.0f;
  }
  if (lane == 0) {
    const float z = a.labels[row];
    const int ks = a.ks[row];
    a.meta[row] = make_int4(a.kt[row], ks, z != 0.0f ? ks : -1, __float_as_int(z * a.coef));
    a.rs[row] = rs;
    a.rt[row] = rt;
    a.cs[row] = ss < 1e-12f ? 1.0f : 0.0f;
    a.ct[row] = tt < 1e-12f ? 1.0f : 0.0f;
  }
}

// acc[r] = sum_k walk[wbase + mfma_row(r, lane)][k] * own[obase + (lane & 31)][k] over the Sp staged columns.  Lane (row, k half)
// reads one float4 of its row per 8 columns; component e of the two halves is the k pair of one MFMA (both operands permute k
// alike).  Every row read exists (Bt rows) and is 16-byte aligned (Sp % 32 == 0).
__device__ __forceinline__ f32x16 inbatch_logit_tile(const float *__restrict__ walk, int wbase, const float *__restrict__ own, int obase,
                                                     int Sp, int lane) {
  const float *pa = walk + (size_t)(wbase + (lane & 31)) * Sp + 4 * (lane >> 5);
  const float *pb = own + (size_t)(obase + (lane & 31)) * Sp + 4 * (lane >> 5);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int s0 = 0; s0 < Sp; s0 += 32) {
    f32x4 av[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = *reinterpret_cast<const f32x4 *>(pa + s0 + 8 * u);
      bv[u] = *reinterpret_cast<const f32x4 *>(pb + s0 + 8 * u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][e], bv[u][e], acc, 0, 0, 0);
  }
  return acc;
}

// is column j (meta mj) admitted for row i (meta mi), i != j?  Tail columns (j >= B) never are.
__device__ __forceinline__ bool inbatch_admits(const int4 &mi, const int4 &mj, int j, int B) {
  return j < B && mj.x != mi.x && mj.z != mi.y;
}

// (m, s) <- the running (max, sum of exp(. - max)) of two disjoint sets; an empty set is (-inf, 0)
__device__ __forceinline__ void inbatch_merge(float &m, float &s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  if (M == IB_NEG_INF) {
    s = 0.0f;
  } else {
    s = s * expf(m - M) + s2 * expf(m2 - M);
  }
  m = M;
}

// rows pass: lse_i, row_loss_i, row_acc_i of the 32 rows a workgroup owns
__global__ __launch_bounds__(IB_NW * 64) void inbatch_rows_kernel(InbatchArgs a) {
  __shared__ float sh_m[IB_NW][32], sh_s[IB_NW][32], sh_d[IB_NW][32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int obase = blockIdx.x * 32, i = obase + (lane & 31);
  const int4 mi = a.meta[i];
  float m = IB_NEG_INF, s = 0.0f;  // over the admitted columns j != i this lane has seen
  float lii = IB_NEG_INF;          // L_ii, on the one lane that meets it
  for (int wt = w; wt < a.Bt / 32; wt += IB_NW) {
    const f32x16 acc = inbatch_logit_tile(a.nt, wt * 32, a.ns, obase, a.Sp, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = wt * 32 + mfma_row(r, lane);
      const float x = a.scale * acc[r];
      if (j == i) {
        lii = x;
      } else if (inbatch_admits(mi, a.meta[j], j, a.B)) {
        if (x > m) {
          s = s * expf(m - x) + 1.0f;
          m = x;
        } else {
          s += expf(x - m);
        }
      }
    }
  }
  // the two lane halves of a row, then the waves in order
  inbatch_merge(m, s, __shfl_xor(m, 32), __shfl_xor(s, 32));
  lii = fmaxf(lii, __shfl_xor(lii, 32));
  if (lane < 32) {
    sh_m[w][lane] = m;
    sh_s[w][lane] = s;
    sh_d[w][lane] = lii;
  }
  __syncthreads();
  if (w != 0 || lane >= 32 || i >= a.B) return;
  m = sh_m[0][lane];
  s = sh_s[0][lane];
  lii = sh_d[0][lane];
  for (int ww = 1; ww < IB_NW; ++ww) {
    inbatch_merge(m, s, sh_m[ww][lane], sh_s[ww][lane]);
    lii = fmaxf(lii, sh_d[ww][lane]);
  }
  const float M = fmaxf(m, lii);
  const float tot = (m == IB_NEG_INF ? 0.0f : s * expf(m - M)) + expf(lii - M);
  const float lse = M + logf(tot);
  const float z = a.labels[i];
  a.lse[i] = lse;
  a.row_loss[i] = z * (lse - lii);
  a.row_acc[i] = (z != 0.0f && !(m > lii)) ? 1.0f : 0.0f;
}

// gradient pass.  COLS == false: own = row i, walk = column j, out = d(ns); COLS == true: own = column j, walk = row i, out = d(nt).
template <bool COLS, int ST>
__global__ __launch_bounds__(IB_NW * 64) void inbatch_grad_kernel(InbatchArgs a) {
  __shared__ float red[ST][16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int obase = blockIdx.x * 32, o = obase + (lane & 31);
  const int sbase = blockIdx.y * (32 * ST);
  const int nst = min(ST, (a.Sp - sbase) / 32);
  const float *__restrict__ ownN = COLS ? a.nt : a.ns;
  const float *__restrict__ walkN = COLS ? a.ns : a.nt;
  const int4 mo = a.meta[o];
  const float lse_o = a.lse[o];
  f32x16 out[ST];
#pragma unroll
  for (int t = 0; t < ST; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[t][r] = 0.0f;
  for (int wt = w; wt < a.Bt / 32; wt += IB_NW) {
    f32x16 g = inbatch_logit_tile(walkN, wt * 32, ownN, obase, a.Sp, lane);
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
        v = coef * (expf(a.scale * g[r] - lse_i) - (i == j ? 1.0f : 0.0f));
      }
      g[r] = v;
    }
#pragma unroll
    for (int t = 0; t < ST; ++t) {
      if (t < nst) {
        const float *pb = walkN + (size_t)(wt * 32) * a.Sp + sbase + 32 * t + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          out[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], pb[(size_t)mfma_row(r, lane) * a.Sp], out[t], 0, 0, 0);
      }
    }
  }
  // the waves' partial tiles, added in wave order
  for (int ww = 0; ww < IB_NW; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int t = 0; t < ST; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[t][r][lane] = ww == 0 ? out[t][r] : red[t][r][lane] + out[t][r];
    }
    __syncthreads();
  }
  float *dst = COLS ? a.dnt : a.dns;
  for (int e = threadIdx.x; e < nst * 16 * 64; e += IB_NW * 64) {
    const int t = e >> 10, r = (e >> 6) & 15, l = e & 63;
    dst[(size_t)(obase + mfma_row(r, l)) * a.Sp + sbase + 32 * t + (l & 31)] = red[t][r][l];
  }
}

// l2_normalize backward of both sides, one wave per output row: d raw = r * (dn - n * (n . dn)), no n . dn term below the clamp
// (as loss_kernel); rows B .. rows_out-1 zeroed
__global__ __launch_bounds__(256) void inbatch_finish_kernel(InbatchArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= a.rows_out) return;
  float *ds = a.d_src + (size_t)row * a.S, *dt = a.d_tgt + (size_t)row * a.S;
  if (row >= a.B) {
    for (int d = lane; d < a.S; d += 64) {
      ds[d] = 0.0f;
      dt[d] = 0.0f;
    }
    return;
  }
  const float *ns = a.ns + (size_t)row * a.Sp, *nt = a.nt + (size_t)row * a.Sp;
  const float *dns = a.dns + (size_t)row * a.Sp, *dnt = a.dnt + (size_t)row * a.Sp;
  float ps = 0.0f, pt = 0.0f;
  for (int d = lane; d < a.S; d += 64) {
    ps += ns[d] * dns[d];
    pt += nt[d] * dnt[d];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ps += __shfl_xor(ps, o);
    pt += __shfl_xor(pt, o);
  }
  const float rs = a.rs[row], rt = a.rt[row];
  if (a.cs[row] != 0.0f) ps = 0.0f;
  if (a.ct[row] != 0.0f) pt = 0.0f;
  for (int d = lane; d < a.S; d += 64) {
    ds[d] = rs * (dns[d] - ns[d] * ps);
    dt[d] = rt * (dnt[d] - nt[d] * pt);
  }
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

inline size_t inbatch_bt(int B) { return (size_t)round_up(B, 32); }
inline size_t inbatch_sp(int S) { return (size_t)round_up(S, 32); }

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
  const size_t Bt = inbatch_bt(B), Sp = inbatch_sp(S);
  return (4 * Bt * Sp + 5 * Bt) * sizeof(float) + Bt * sizeof(int4);
}

hipError_t launch_inbatch_loss(const float *src_raw, const float *tgt_raw, const float *labels, const int32_t *src_key,
                               const int32_t *tgt_key, int B, int rows_out, int S, float scale, float inv_rows, void *scratch,
                               float *d_src, float *d_tgt, float *row_loss, float *row_acc, hipStream_t st) {
  const size_t Bt = inbatch_bt(B), Sp = inbatch_sp(S);
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
  const int NT = (int)(Bt / 32);
  hipLaunchKernelGGL(inbatch_prep_kernel, dim3((unsigned)((Bt + 3) / 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(inbatch_rows_kernel, dim3(NT), dim3(IB_NW * 64), 0, st, a);
  if (d_src && d_tgt) {
    if (Sp <= 32 * IB_ST) {
      const dim3 grid(NT, 1);
      hipLaunchKernelGGL((inbatch_grad_kernel<false, IB_ST>), grid, dim3(IB_NW * 64), 0, st, a);
      hipLaunchKernelGGL((inbatch_grad_kernel<true, IB_ST>), grid, dim3(IB_NW * 64), 0, st, a);
    } else {
      const dim3 grid(NT, (unsigned)((Sp + 32 * IB_ST_WIDE - 1) / (32 * IB_ST_WIDE)));
      hipLaunchKernelGGL((inbatch_grad_kernel<false, IB_ST_WIDE>), grid, dim3(IB_NW * 64), 0, st, a);
      hipLaunchKernelGGL((inbatch_grad_kernel<true, IB_ST_WIDE>), grid, dim3(IB_NW * 64), 0, st, a);
    }
    hipLaunchKernelGGL(inbatch_finish_kernel, dim3((rows_out + 3) / 4), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}
