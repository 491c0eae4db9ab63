// C-ABI layer of libsse_hip.so (see include/sse_hip.h): handle, variables,
// lazy weight re-layout, scratch management, kernel orchestration.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <dlfcn.h>
#include <link.h>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/sse_hip.h"
#include "sse_kernels.h"
#include "train.h"
#include "train_step.h"

namespace {

thread_local std::string g_create_error;

struct Variable {
  std::string name;
  int rows = 0, cols = 0;  // logical 2-D view (count = rows*cols)
  int64_t count = 0;
  float *dev = nullptr;     // master copy, row-major, TF shape
  float *slot = nullptr;    // '<name>/Adagrad' accumulator
  float *grad = nullptr;    // gradient of the current step (allocated by the first train step)
};

// pad-prefix table: state after p leading PAD steps, p = 0..T ([T+1][width] each), recorded by the kernel that reads it.
// T is what the latest recording covers; the buffers hold cap + 1 rows (cap >= T: a shorter re-recording keeps them).
struct PadTable {
  float *h = nullptr, *c = nullptr;
  int T = 0, cap = 0;
  bool valid = false;
  void release() {
    if (h) (void)hipFree(h);
    if (c) (void)hipFree(c);
    h = c = nullptr;
  }
};

struct Encoder {
  int kernel = -1, bias = -1, proj = -1;  // variable indices
  int H = 0, Hp = 0, UB = 0, KGx = 0, KGh = 0, Ep = 0;
  float *Wp = nullptr, *Mp = nullptr;
  float *Waug = nullptr;      // few-sequences kernel: kernel rows in its k space incl. the bias row
  bool waug_valid = false;
  float *Wc = nullptr;        // cluster kernel (lstm_cluster.hip): weight fragments per workgroup of a cluster
  bool wc_valid = false;
  unsigned short *Wx3 = nullptr;  // option lstm_x3: hi / lo bf16 fragment copies of the kernel matrix
  bool x3_valid = false;
  unsigned short *Wx3t = nullptr;  // option train_fwd_x3: the same copies with the h part in unit order (training forward)
  int shares_lstm_with = -1;  // shared-encoder: target reuses the source LSTM packing
  bool generic = false;       // shape outside the fused kernels' layouts: every encode / train step of this encoder runs lstm_generic.hip
  // pad-prefix tables of the LSTM owner: matrix kernel (lstm_fwd.hip, Hp wide), few-sequences kernel (lstm_small.hip, H wide;
  // the two cluster kernels share its arithmetic and read it too), lstm_x3 path (Hp wide)
  PadTable pad_fwd, pad_small, pad_x3;
  // x-projection table of the LSTM owner (lstm_xtable.hip): per token, the gate accumulators after the x k-groups; read by
  // lstm_fwd_kernel's table path (Hp = 256 / 512 inference)
  float *xtab = nullptr;
  bool xtab_valid = false;
};

}  // namespace

// sse_handle::lstm_path_calls: one entry per kernel an encode can be sent to, then what the matrix kernel's launcher picked
enum { PATH_PERSIST, PATH_CLUSTER, PATH_SMALL, PATH_X3, PATH_GENERIC, PATH_FWD, PATH_FWD_ROWS32, PATH_FWD_ROWS64, PATH_FWD_GS, PATH_FWD_XT,
       PATH_COUNT };

struct sse_handle {
  sse_config cfg;
  std::mutex mu;
  std::string err;
  std::vector<Variable> vars;
  Encoder enc[2];
  bool packed_dirty = true;
  uint64_t weights_version = 1;  // bumped with every change of a variable: the any-shape path's packs (lstm_generic.hip) are cached against it
  bool mp_fresh = false;     // the packed projections match the variables although packed_dirty is set (ensure_proj_packed)
  int pad_skip = 1;      // option "pad_skip": exact left-pad prefix skip in inference encodes
  // option "pad_sort_dev": PAD-prefix bucketing of device-resident id matrices (sse_encode_dev) by two small kernels (pack.hip):
  // 0 off | 1 adaptive: every eligible call measures its batch; rows are bucketed while the latest completed call of that side
  // saw any padding, 32-row tiles while it saw a mean prefix >= T / 4 (no host round trip: an index build's batches look alike)
  // | 2 always bucket + 32-row tiles (deterministic: tests, tools)
  int pad_sort_dev = 1;
  // options "score_two_pass_min_rows" / "score_two_pass_rows": indexes of min .. max rows under >= 1024 queries (k <= 16, bf16
  // candidates) are ranked by a max-only sweep + a collect sweep instead of the list sweep (exact, same ids and scores); max 0 = off.
  // Window measured on well-spread unit vectors, S = 256 (tools/bench_c3.py, tools/bench_score.py, profiles/r06_notes.txt), two-pass /
  // list sweep in ms: 16,491 queries x 32 k rows 1.19 / 1.03, 64 k 1.58 / 1.72, 128 k 2.39 / 3.07, 256 k 4.13 / 5.51, 512 k 7.61 / 10.17;
  // 1024 x 300 k 0.44 / 0.57; but 8192 x 1.25 M 7.83 / 4.91 (a list-free sweep runs at 0.54 of the bf16 peak there, the list sweep at 0.43)
  int score_two_pass_min_rows = 49152, score_two_pass_rows = 524288;
  int64_t two_pass_calls = 0;  // counter "score_two_pass_calls"
  DevBuf s_lmax;
  int lstm_gate_split = 1;  // option "lstm_gate_split": small cells (H <= 128) at 64-row tiles on lstm_fwd_gs.hip (bit-identical)
  DevBuf s_padzero, s_padwork, s_padorder;
  int32_t *pad_stat = nullptr;  // pinned host words the device stores to: [side] {call number, class 0 / 1 / 2}
  int32_t pad_seq = 0;
  int64_t pad_sorted_calls = 0;  // counter "pad_sorted_calls"
  // counters "lstm_path_*" / "lstm_fwd_*": LSTM inference encodes by the kernel they were sent to (PATH_* order)
  int64_t lstm_path_calls[PATH_COUNT] = {};
  int lstm_x3 = 0;       // option "lstm_x3": large inference encodes (Hp = 256) on the bf16 matrix pipe with split operands
  unsigned short *emb16 = nullptr;  // split embedding table of that path
  bool emb16_valid = false;
  int lstm_persist_rows = 32; // option "lstm_persist_rows": batches up to this many rows (<= 32) take the weights-in-LDS cluster kernel
  uint32_t persist_epoch = 0; // tag epoch of the cluster kernel's exchange buffers
  hipStream_t stream = nullptr;  // sse_set_stream: the stream the train-step entry points enqueue on (default: the null stream)
  int persist_inject = 0;   // testing aid (option lstm_persist_inject_miss): report a missing cluster workgroup after every cluster launch
  int64_t persist_fallbacks = 0; // host-buffer encodes re-run on lstm_small because a cluster workgroup did not arrive
  int cu_count = 0;           // compute units of the device (co-residency check of the cluster kernel)
  int lstm_cluster_rows = 1024; // option "lstm_cluster_rows": batches above lstm_persist_rows up to this many rows (<= 1024) take the MFMA cluster kernel
  uint32_t cluster_epoch = 0;   // tag epoch of that kernel's exchange buffers
  int lstm_cluster_chunks = 3;  // option "lstm_cluster_chunks": batches of up to this many times lstm_cluster_rows go through that kernel in launches of lstm_cluster_rows
  int cluster_backoff = -1;     // option "lstm_cluster_backoff": after a cluster-kernel launch gave up, this many following eligible calls go straight to the kernels that need no co-residency.  -1 (default) = automatic: no back-off is ARMED until a give-up has been observed (cooperative launches make co-residency the runtime's promise), but an observed give-up -- another process on the device, or a cooperative launch the runtime refused (counter lstm_coop_refused) -- arms 16 calls, so a busy device pays the 10 ms give-up once in 17 calls, not on every call
  int cluster_skip[2] = {0, 0}; // calls still to skip: [0] single-query kernel (lstm_persist), [1] mid-batch kernel (lstm_cluster)
  int lstm_cluster_coop = 1;    // option "lstm_cluster_coop" (default 1): the cluster kernels are launched with hipLaunchCooperativeKernel (co-residency guaranteed by the runtime; +20 us per launch measured); 0 = plain launches
  int lstm_cluster_wt = 0;      // option "lstm_cluster_write_through": force the any-placement publish path (tests)
  int lstm_cluster_drop = 0;    // option "lstm_cluster_drop_wg": one workgroup of the cluster kernel exits at once (tests)
  int lstm_small_rows = 1024; // option "lstm_small_rows": batches up to this many rows take the few-sequences LSTM kernel
  // option "lstm_x_table": encodes on the matrix kernel at Hp = 256 / 512 start every step's gate accumulators from a per-token
  // table of x projections instead of recomputing them (bit-identical).  1 (default): the table is (re)built when a batch
  // brings at least as many tokens as the vocabulary (B * T >= V), so small batches between weight updates never pay for a
  // rebuild; 2: always built; 0: off.  Option "lstm_x_table_mb": the largest table built, in MiB (default 256, the Infinity
  // Cache of an MI355X); larger ones take the embedding-gather path.  Counter "lstm_x_table_builds".
  int lstm_x_table = 1;
  int lstm_x_table_mb = 256;
  int64_t x_table_builds = 0;
  int score_small_index = 1;  // option "score_small_index": many queries against <= 1024 rows skip the list sweep (launch_score_small_index)
  int score_small_x3 = 1;     // option "score_small_x3": the small-index scorer forms its candidates from split-bf16 operands (idx_x3; wider r.eps)
  int score_bf16 = 1;    // option "score_bf16" (default on): candidate pass on the bf16 matrix pipe; results stay exact
  void *idxp16 = nullptr;    // bf16 fragment copy of the index (built on demand)
  size_t idxp16_cap = 0;
  bool idxp16_valid = false;
  bool fb_cnt_init = false;
  int uncert_word = 0;       // which word of the pair behind the counters the current scoring call counts its uncertified queries in
  bool cnn_bf16 = false;     // option "cnn_bf16": source_only_cnn inference with bf16 storage / fp32 accumulation
  unsigned short *emb_bf16 = nullptr, *cnn_Wc16 = nullptr, *cnn_Mx3 = nullptr;
  int lstm_train_rows = 0;   // option "lstm_train_rows": 0 = automatic, 32 / 64 = rows per workgroup of the training forward (Hp = 256)
  // The train step computes in fp32 like the reference (tf.float32 graph, sse_model.py:355-364): the three split-operand
  // options below are OPT-IN (a default narrower than the reference's arithmetic earns no credit).
  int train_bwd_x3 = 0;  // option "train_bwd_x3": recurrent GEMM of BPTT on the bf16 matrix pipe with split operands (needs train_dk_x3)
  int train_fwd_x3 = 0;  // option "train_fwd_x3": forward of the LSTM train step on the bf16 matrix pipe with split operands
  int train_dk_x3 = 0;   // option "train_dk_x3": weight-gradient GEMM of the LSTM train step on the bf16 matrix pipe with split operands
  int train_generic = 0;  // option "train_generic": the LSTM train step on the any-shape path (lstm_generic.hip) whatever the shape (tests, A/B)
  int train_gen1 = 0;    // option "train_gen1": the fp32 train step on the first-generation kernels (lstm_bwd_kernel + dx_kernel + db partials; A/B timing and tests)
  int train_pair_dedup = 1; // option "train_pair_dedup": run the source encoder once per (pos, neg) pair of rows that share it
  int train_serial = 0; // option "train_serial": both encoders on one stream (profiling: isolated kernel times)
  int train_loss = 0;         // option "train_loss": 0 = the reference's pair loss, 1 = in-batch softmax (inbatch_loss.hip)
  int train_loss_scale = 64;  // option "train_loss_scale": logit scale of the in-batch and class losses (the pair loss keeps the reference's 64)
  int train_class_loss = 0;   // option "train_class_loss": 1 = softmax over every row of the free target matrix (class_loss.hip)
  float *emb_pad = nullptr;  // [V][Ep]
  // source_only_cnn
  int cnn_W[4] = {-1, -1, -1, -1}, cnn_b[4] = {-1, -1, -1, -1}, cnn_M = -1, tgt_table = -1;
  float *cnn_Wc = nullptr, *cnn_bias = nullptr, *cnn_Mp = nullptr;
  int32_t *err_flag = nullptr;
  // index
  float *idxp = nullptr;
  size_t idxp_cap = 0;
  double *idx64 = nullptr;
  DevBuf idx_rm;            // row-major f32 copy of a SMALL index (re-scoring gathers, RescoreArgs::idx_rm); valid: idx_rm_valid
  bool idx_rm_valid = false;
  DevBuf idx_x3;            // split-bf16 image of idxp for the small-index scorer (SmallIndexArgs::idx_x3), rebuilt with every index
  bool idx_x3_valid = false;  // that score_small_index_applies can serve (<= 1024 rows: <= 1 MiB); valid: idx_x3_valid
  int64_t idx_N = 0, idx_base = 0;
  int idx_S = 0;
  float idx_norm_max = 1.0f;
  // in-place updates (sse_index_update* / sse_index_append*, DESIGN K6n): the per-row sums of squares behind idx_norm_max
  // (built from idxp by the first update after an upload; valid: idx_norm2_valid), which of the two pack paths formed that
  // bound (idx_norm_vec: pack_rows_vec_kernel), the bytes idx64 was allocated with, the staged operands of the host forms,
  // the counters "index_update_calls" / "index_update_rows" / "index_append_rows" / "index_grow_copies"
  DevBuf idx_norm2, s_upd;
  bool idx_norm2_valid = false, idx_norm_vec = false;
  size_t idx64_cap = 0;
  int64_t index_update_calls = 0, index_update_rows = 0, index_append_rows = 0, index_grow_copies = 0;
  // scratch
  DevBuf s_ids, s_out, s_q, s_qp, s_ps, s_pi, s_cert, s_os, s_oi, s_tmp, s_tmp2, s_feat, s_zero, s_map;
  DevBuf s_qmap, s_qc;     // fp32 second chance of the bf16 candidate pass: the uncertified queries as a dense set
  DevBuf s_qp32, s_fb_cnt;  // fp32 second chance of the bf16 candidate pass: fp32 query fragments, counter
  DevBuf g_A, g_G, g_c, g_hl, g_raw;  // any-shape LSTM encode (lstm_generic.hip)
  DevBuf g_KT[2], g_Kq[2], g_MT[2];    // ... its packed weights per side, valid while g_ver[side] == weights_version (they
  uint64_t g_ver[2] = {0, 0};          //     were rebuilt by every call)
  DevBuf s_xchg;     // sse_score_topk_sharded_dev: [local lists | gathered lists] of the RCCL exchange
  DevBuf s_persist;  // lstm_persist.hip: h_t / raw-encoding exchange buffers and arrival counters
  DevBuf s_cluster;  // lstm_cluster.hip: h_t / sum-of-squares exchange buffers
  int32_t *pin_small = nullptr;  // 64 pinned host words: error flag / loss read-backs (a pageable target makes the copy a blocking one)
  void *pin = nullptr;  // pinned host staging of the host-buffer scoring entry points: [scores | ids | certificates]
  size_t pin_cap = 0;
  int32_t score_seq = 0;  // call number the re-scoring pass stores into the pinned completion flags (ScoreMirror)
  DevBuf s_pb, s_cthr, s_cslot, s_ccnt, s_cbuf;  // per-split bounds; collect path: thresholds, slots, counters, row buffers
  // exact rank of labelled rows (sse_score_rank*, score_rank.hip): per-pair scratch of a chunk (thresholds, fp32 intervals, sure
  // counts, the call's "bad pair" word), the two counters "score_rank_band_rows" / "score_rank_bruteforce_pairs" on the
  // device.  The band buffers are the collect path's (s_ccnt, s_cbuf).
  DevBuf s_rk, s_rk_cnt;
  bool rk_cnt_init = false;
  // rows at or above a threshold (sse_score_above*, score_above.hip): per-pair cursors and overflow marks of a call, merge
  // scratch of the lists' length, the three "score_above_*" counters, the lists of the host form.
  // Per-chunk scratch is the rank count's (s_rk, s_ccnt, s_cbuf).
  DevBuf s_ab, s_ab_sort, s_ab_cnt, s_ab_out;
  bool ab_cnt_init = false;
  // top-k among tag-eligible rows (sse_score_topk_filtered*, score_filtered.hip): the tags of the resident index (one word per
  // row, zero padded to whole tiles) and their per-tile OR, valid while tags_set; the maxima of a chunk, the three
  // "score_filtered_*" counters.  Thresholds and row buffers are the collect path's (s_cthr, s_ccnt, s_cbuf).
  DevBuf idx_tags, idx_tag_sum, s_ft_max, s_ft_cnt;
  bool tags_set = false, ft_cnt_init = false;
  int score_filtered_skip = 1;  // option "score_filtered_skip": the sweeps skip index tiles no query of a block can use
  // top-k distinct groups (sse_score_topk_grouped*, score_grouped.hip): one int64 key per row of the resident index, valid
  // while groups_set; the (key, row) maxima of a chunk, the two "score_grouped_*" counters
  DevBuf idx_groups, s_gp_max, s_gp_cnt;
  bool groups_set = false, gp_cnt_init = false;
  // next page after a cursor (sse_score_topk_after*, score_after.hip): the bracket of a chunk's cursor scores ([P] e as double,
  // [P] lo, [P] hi), the two "score_after_*" counters.  Maxima, thresholds and row buffers are the filtered call's.
  DevBuf s_af_bnd, s_af_cnt;
  bool af_cnt_init = false;
  // top-k of cosine + per-row prior (sse_score_topk_biased*, score_biased.hip): one float per row of the resident index (zero
  // padded to whole tiles) and bias_absmax = max |bias| beside it as one device word (as idx_norm_max is kept, but on the
  // device: the _dev setter computes it there and never waits), valid while bias_set; e_b of a chunk ([P] double), the two
  // "score_biased_*" counters.  Maxima, thresholds and row buffers are the filtered call's.
  DevBuf idx_bias, idx_bias_absmax, s_bs_bnd, s_bs_cnt;
  bool bias_set = false, bs_cnt_init = false;
  // confusions of a query (sse_score_confusions*, score_confusions.hip): the floors of a chunk ([P] f as double, [P] flo), the
  // three "score_confusions_*" counters.  Maxima, thresholds and row buffers are the filtered call's.
  DevBuf s_cf_bnd, s_cf_cnt;
  bool cf_cnt_init = false;
  // softmax log-partition (sse_score_lse*, score_lse.hip): the (m, sum, count) partials of a chunk, the device word of
  // "score_lse_tiles_skipped", and "score_lse_calls": calls that passed their checks (host and _dev forms alike)
  DevBuf s_lse_part, s_lse_cnt;
  bool lse_cnt_init = false;
  int64_t score_lse_calls = 0;
  // staging of the host forms of the six calls above (stage_in): they hold the handle's mutex and finish all device work
  // before they return, so one buffer serves them all
  DevBuf s_stage;
  // forward-only pair loss (sse_eval_loss*, eval_loss.hip).  Option "eval_chunk_rows": pair rows staged and encoded per chunk (even).
  // Scratch of its own: a gradient result pending between sse_train_grads and sse_train_apply lives in TrainState and the arena.
  int eval_chunk_rows = 65536;
  int64_t eval_paired_calls = 0;  // counter "eval_paired_calls": calls that ran the source encoder once per pair of rows
  DevBuf ev_ids[2], ev_stage, ev_rows[2], ev_labels, ev_raw[2], ev_row, ev_sums;
  // training
  float lr = 0.9f;
  int64_t global_step = 0;
  TrainState *train = nullptr;
  // counters "train_path_*", "train_paired_steps", "train_*_repacks": the route of every train step and what it rebuilt
  int64_t train_path_fused = 0, train_path_generic = 0, train_path_cnn = 0, train_paired_steps = 0;
  int64_t train_fp32_repacks = 0, train_split_repacks = 0, train_generic_repacks = 0;
  int64_t train_inbatch_steps = 0;  // counter "train_inbatch_steps": steps whose loss stage ran the in-batch softmax head
  int64_t train_open_steps = 0;            // counter "train_open_steps": sse_train_forward* calls that left a step open
  int64_t train_global_inbatch_steps = 0;  // counter "train_global_inbatch_steps": steps closed by sse_train_backward_inbatch_global
  // in-batch softmax loss (sse_inbatch_loss_dev and the train step under option train_loss = 1): staged operands, row
  // statistics, un-normalised gradients (launch_inbatch_loss); the row keys [source | target | hash scratch] of a call
  DevBuf s_inbatch, s_inbatch_keys;
  int64_t train_class_steps = 0;  // counter "train_class_steps": steps whose loss stage ran the class softmax head
  // class softmax loss (sse_class_loss_dev and the train step under option train_class_loss = 1): the scratch of
  // launch_class_loss; the source keys [keys | hash scratch] of a call
  DevBuf s_class, s_class_keys;
  std::vector<hipEvent_t> events;
};

namespace {

int fail(sse_handle *h, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_error = buf;
  return 1;
}

#define HIPCHECK(h, expr)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return fail(h, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// how most entry points open: null handle, the handle's mutex for the rest of the call, its device current
#define SSE_ENTER(h)                       \
  if (!(h)) return 1;                      \
  std::lock_guard<std::mutex> lk((h)->mu); \
  HIPCHECK(h, hipSetDevice((h)->cfg.device))

// Wait for a stream: poll for up to ~3 ms (the latency-critical calls finish in 0.1 - 0.5 ms; the runtime's blocking wait
// was seen to add 1 - 2 ms to some of them: an 8-token query against a 1.25 M-row index took 2.0 ms end to end with 0.3 ms
// of device work), then block.
hipError_t sync_stream(hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(st);
    if (e != hipErrorNotReady) return e;
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(3)) return hipStreamSynchronize(st);
  }
}

int reserve(sse_handle *h, DevBuf &b, size_t bytes) {
  if (bytes <= b.cap) return 0;
  if (b.p) HIPCHECK(h, hipFree(b.p));
  b.p = nullptr;
  b.cap = 0;
  const size_t cap = bytes + bytes / 4 + 256;
  HIPCHECK(h, hipMalloc(&b.p, cap));
  b.cap = cap;
  return 0;
}

int add_var(sse_handle *h, const std::string &name, int rows, int cols) {
  Variable v;
  v.name = name;
  v.rows = rows;
  v.cols = cols;
  v.count = (int64_t)rows * cols;
  h->vars.push_back(v);
  return (int)h->vars.size() - 1;
}

int find_var(sse_handle *h, const char *name, bool *is_slot) {
  std::string n(name);
  *is_slot = false;
  const std::string suffix = "/Adagrad";
  if (n.size() > suffix.size() && n.compare(n.size() - suffix.size(), suffix.size(), suffix) == 0) {
    n.resize(n.size() - suffix.size());
    *is_slot = true;
  }
  for (size_t i = 0; i < h->vars.size(); ++i)
    if (h->vars[i].name == n) return (int)i;
  return -1;
}

int setup_encoder(sse_handle *h, Encoder &e, const std::string &scope, const std::string &proj, int H, int proj_rows) {
  const sse_config &c = h->cfg;
  e.H = H;
  e.kernel = add_var(h, scope + "/rnn/basic_lstm_cell/kernel", c.embedding_size + H, 4 * H);
  e.bias = add_var(h, scope + "/rnn/basic_lstm_cell/bias", 1, 4 * H);
  e.proj = add_var(h, proj, proj_rows, c.encoding_size);
  return 0;
}

int geometry(sse_handle *h, Encoder &e) {
  const sse_config &c = h->cfg;
  if (e.H <= 0) return 0;
  e.Hp = e.H <= 128 ? 128 : e.H <= 256 ? 256 : round_up(e.H, 512);
  e.UB = e.Hp / 128;
  e.Ep = round_up(c.embedding_size + 1, 8);  // at least one padding column: it holds the constant 1 of the bias row
  e.KGx = e.Ep / 8;
  e.KGh = e.Hp / 8;
  // Shapes the fused kernels are not laid out for -- cell size > 512, an embedding too wide for the LDS tile, encoding_size >
  // 512 -- run the any-shape path (lstm_generic.hip) instead of being rejected (round 5; the reference accepts any size,
  // sse_train.py:60-74).  (The scorer's own limit, index dimension <= 1024, is separate.)
  e.generic = e.H > 512 || c.encoding_size > 512 || lstm_fwd_lds_bytes(e.KGx, e.KGh, e.Hp == 512 ? 1 : 2) > 160 * 1024;
  return 0;
}

// row stride of the padded embedding table: the LSTM kernels consume k in groups of 8 and need one padding column
// for the constant 1 that carries the bias; the CNN only needs 16-byte aligned window starts (E = 50: 52 instead of
// 56 -> 7 % fewer MFMAs)
static int emb_cols(const sse_config &c) {
  return c.network_mode == SSE_MODE_SOURCE_ONLY_CNN ? round_up(c.embedding_size, 4) : round_up(c.embedding_size + 1, 8);
}

Encoder &lstm_owner(sse_handle *h, Encoder &e) { return e.shares_lstm_with >= 0 ? h->enc[e.shares_lstm_with] : e; }

// the layouts and pad-prefix tables made from the LSTM weights on demand: stale once the weights change
void invalidate_derived(Encoder &e) {
  e.waug_valid = e.wc_valid = e.x3_valid = false;
  e.pad_fwd.valid = e.pad_small.valid = e.pad_x3.valid = false;
  e.xtab_valid = false;
}

// (re)build the kernel-facing layouts from the master variables
// the packed projections alone (what a train step whose LSTM kernels all run on split operands reads of these layouts):
// the embedding pad, the fp32 kernel fragments and the CNN layouts stay stale (packed_dirty) until an encode needs them
int ensure_proj_packed(sse_handle *h, hipStream_t st) {
  if (!h->packed_dirty || h->mp_fresh) return 0;
  const sse_config &c = h->cfg;
  for (int s = 0; s < 2; ++s) {
    Encoder &e = h->enc[s];
    if (e.H <= 0 || e.kernel < 0 || e.generic) continue;
    const int NTS = (c.encoding_size + 31) / 32;
    if (!e.Mp) HIPCHECK(h, hipMalloc((void **)&e.Mp, (size_t)NTS * e.KGh * 256 * sizeof(float)));
    HIPCHECK(h, launch_pack_kn(h->vars[e.proj].dev, e.H, c.encoding_size, e.KGh, e.Mp, st));
  }
  h->mp_fresh = true;
  return 0;
}

int ensure_packed(sse_handle *h, hipStream_t st) {
  if (!h->packed_dirty) return 0;
  const sse_config &c = h->cfg;
  const int Ep = emb_cols(c);
  h->emb16_valid = false;
  if (!h->emb_pad) HIPCHECK(h, hipMalloc((void **)&h->emb_pad, (size_t)c.vocab_size * Ep * sizeof(float)));
  HIPCHECK(h, launch_pad_rows(h->vars[0].dev, c.vocab_size, c.embedding_size, Ep,
                              c.network_mode == SSE_MODE_SOURCE_ONLY_CNN ? -1 : c.embedding_size, h->emb_pad, st));
  for (int s = 0; s < 2; ++s) {
    Encoder &e = h->enc[s];
    if (e.H <= 0 || e.kernel < 0 || e.generic) continue;
    invalidate_derived(e);
    const int KG = e.KGx + e.KGh;
    if (e.shares_lstm_with < 0) {
      if (!e.Wp) HIPCHECK(h, hipMalloc((void **)&e.Wp, (size_t)(e.Hp / 32) * KG * 4 * 256 * sizeof(float)));
      HIPCHECK(h, launch_pack_lstm(h->vars[e.kernel].dev, h->vars[e.bias].dev, c.embedding_size, e.H, e.Ep, e.Hp, e.UB,
                                   e.Wp, st));
    } else {
      e.Wp = h->enc[e.shares_lstm_with].Wp;
    }
    const int NTS = (c.encoding_size + 31) / 32;
    if (!e.Mp) HIPCHECK(h, hipMalloc((void **)&e.Mp, (size_t)NTS * e.KGh * 256 * sizeof(float)));
    HIPCHECK(h, launch_pack_kn(h->vars[e.proj].dev, e.H, c.encoding_size, e.KGh, e.Mp, st));
  }
  if (c.network_mode == SSE_MODE_SOURCE_ONLY_CNN) {
    if (c.encoding_size > 512) return fail(h, "encoding_size %d > 512 not supported", c.encoding_size);
    if (!h->cnn_Wc) HIPCHECK(h, hipMalloc((void **)&h->cnn_Wc, cnn_packed_weight_floats(Ep) * sizeof(float)));
    if (!h->cnn_bias) HIPCHECK(h, hipMalloc((void **)&h->cnn_bias, 576 * sizeof(float)));
    const int NTS = (c.encoding_size + 31) / 32;
    if (!h->cnn_Mp) HIPCHECK(h, hipMalloc((void **)&h->cnn_Mp, (size_t)NTS * 72 * 256 * sizeof(float)));
    const float *W[4];
    static const int foff[4] = {0, 256, 384, 512}, nf[4] = {256, 128, 128, 64};
    for (int i = 0; i < 4; ++i) {
      W[i] = h->vars[h->cnn_W[i]].dev;
      HIPCHECK(h, hipMemcpyAsync(h->cnn_bias + foff[i], h->vars[h->cnn_b[i]].dev, nf[i] * sizeof(float),
                                 hipMemcpyDeviceToDevice, st));
    }
    HIPCHECK(h, launch_pack_conv(W, c.embedding_size, Ep, h->cnn_Wc, st));
    if (h->cnn_bf16) {
      const int Ep8 = round_up(c.embedding_size, 8);
      if (!h->emb_bf16) HIPCHECK(h, hipMalloc((void **)&h->emb_bf16, (size_t)c.vocab_size * Ep8 * sizeof(unsigned short)));
      if (!h->cnn_Wc16) HIPCHECK(h, hipMalloc((void **)&h->cnn_Wc16, cnn_bf16_packed_weight_elems(Ep8) * sizeof(unsigned short)));
      HIPCHECK(h, launch_cnn_bf16_pack(h->vars[0].dev, c.vocab_size, c.embedding_size, Ep8, h->emb_bf16, W, h->cnn_Wc16, st));
      if (!h->cnn_Mx3) HIPCHECK(h, hipMalloc((void **)&h->cnn_Mx3, cnn_proj_x3_elems(c.encoding_size) * sizeof(unsigned short)));
      HIPCHECK(h, launch_pack_cnn_proj_x3(h->vars[h->cnn_M].dev, c.encoding_size, h->cnn_Mx3, st));
    }
    HIPCHECK(h, launch_pack_kn(h->vars[h->cnn_M].dev, 576, c.encoding_size, 72, h->cnn_Mp, st));
  }
  h->packed_dirty = false;
  h->mp_fresh = true;
  return 0;
}

// The layouts a pure fp32 LSTM train step reads -- padded embedding table, packed kernels and projections (what ensure_packed
// builds for the LSTM modes) and the fp32 Kh^T / Kx^T fragment copies of the BPTT kernel -- in ONE launch (launch_pack_multi).
int pack_train_fp32(sse_handle *h, TrainState &ts, int nside, hipStream_t st) {
  const sse_config &c = h->cfg;
  PackJobs js;
  if (h->packed_dirty) {
    const int Ep = emb_cols(c);
    h->emb16_valid = false;
    if (!h->emb_pad) HIPCHECK(h, hipMalloc((void **)&h->emb_pad, (size_t)c.vocab_size * Ep * sizeof(float)));
    pack_job_pad_rows(js, h->vars[0].dev, c.vocab_size, c.embedding_size, Ep, c.embedding_size, h->emb_pad);
    for (int s = 0; s < 2; ++s) {
      Encoder &e = h->enc[s];
      if (e.H <= 0 || e.kernel < 0) continue;
      invalidate_derived(e);
      const int KG = e.KGx + e.KGh;
      if (e.shares_lstm_with < 0) {
        if (!e.Wp) HIPCHECK(h, hipMalloc((void **)&e.Wp, (size_t)(e.Hp / 32) * KG * 4 * 256 * sizeof(float)));
        pack_job_lstm(js, h->vars[e.kernel].dev, h->vars[e.bias].dev, c.embedding_size, e.H, e.Ep, e.Hp, e.Wp);
      } else {
        e.Wp = h->enc[e.shares_lstm_with].Wp;
      }
      const int NTS = (c.encoding_size + 31) / 32;
      if (!e.Mp) HIPCHECK(h, hipMalloc((void **)&e.Mp, (size_t)NTS * e.KGh * 256 * sizeof(float)));
      pack_job_kn(js, h->vars[e.proj].dev, e.H, c.encoding_size, e.KGh, e.Mp);
    }
  }
  if (ts.fp32_dirty) {
    h->train_fp32_repacks += 1;
    for (int s = 0; s < nside; ++s) {
      Encoder &e = h->enc[s];
      if (e.shares_lstm_with >= 0) {
        ts.KhT[s] = ts.KhT[e.shares_lstm_with];
        ts.KxT[s] = ts.KxT[e.shares_lstm_with];
        continue;
      }
      if (!ts.KhT[s]) HIPCHECK(h, hipMalloc((void **)&ts.KhT[s], (size_t)(e.Hp / 32) * (e.Hp / 2) * 256 * sizeof(float)));
      if (!ts.KxT[s]) HIPCHECK(h, hipMalloc((void **)&ts.KxT[s], (size_t)2 * (e.Hp / 2) * 256 * sizeof(float)));
      pack_job_kT(js, h->vars[e.kernel].dev, c.embedding_size, e.H, e.Hp / 32, e.H, e.Hp, ts.KhT[s]);
      pack_job_kT(js, h->vars[e.kernel].dev, 0, c.embedding_size, 2, e.H, e.Hp, ts.KxT[s]);
    }
  }
  HIPCHECK(h, launch_pack_multi(js, st));
  h->packed_dirty = false;
  h->mp_fresh = true;
  ts.fp32_dirty = false;
  return 0;
}

void fill_fwd_args(sse_handle *h, Encoder &e, LstmFwdArgs &a) {
  const sse_config &c = h->cfg;
  a.emb = h->emb_pad;
  a.Wp = e.Wp;
  a.Mp = e.Mp;
  a.err = h->err_flag;
  a.V = c.vocab_size;
  a.Ep = e.Ep;
  a.KGx = e.KGx;
  a.KGh = e.KGh;
  a.H = e.H;
  a.KGhe = (e.H + 7) / 8;
  a.S = c.encoding_size;
  a.NTS = (c.encoding_size + 31) / 32;
  a.gate_split = h->lstm_gate_split ? 1 : 0;
  a.cu_count = h->cu_count;  // (set by sse_create)
}

// State after p leading PAD steps for p = 0..T: one all-PAD row through the kernel that reads the table (bit-identical
// arithmetic), recorded step by step.  record(ids, out, Tt) launches that row: Tt zero ids, scratch output, rec_h / rec_c = t.
template <class Record>
int ensure_pad_table(sse_handle *h, PadTable &t, int width, int T, hipStream_t st, Record record) {
  if (t.valid && t.T >= T) return 0;
  const int Tt = T > h->cfg.max_seq_length ? T : h->cfg.max_seq_length;
  const size_t bytes = (size_t)(Tt + 1) * width * sizeof(float);
  t.valid = false;
  if (t.cap < Tt || !t.h) {
    if (t.h) HIPCHECK(h, hipFree(t.h));
    if (t.c) HIPCHECK(h, hipFree(t.c));
    t.h = t.c = nullptr;
    t.cap = 0;
    HIPCHECK(h, hipMalloc((void **)&t.h, bytes));
    HIPCHECK(h, hipMalloc((void **)&t.c, bytes));
    t.cap = Tt;
  }
  HIPCHECK(h, hipMemsetAsync(t.h, 0, bytes, st));
  HIPCHECK(h, hipMemsetAsync(t.c, 0, bytes, st));
  if (reserve(h, h->s_zero, (size_t)Tt * sizeof(int32_t) + (size_t)h->cfg.encoding_size * sizeof(float))) return 1;
  HIPCHECK(h, hipMemsetAsync(h->s_zero.p, 0, (size_t)Tt * sizeof(int32_t), st));
  if (record((const int32_t *)h->s_zero.p, (float *)((char *)h->s_zero.p + (size_t)Tt * sizeof(int32_t)), Tt)) return 1;
  t.T = Tt;  // rows beyond Tt (an earlier, longer recording) are stale: a later, longer T records again
  t.valid = true;
  return 0;
}

int ensure_waug(sse_handle *h, Encoder &own, hipStream_t st) {
  if (own.waug_valid) return 0;
  const int E = h->cfg.embedding_size;
  if (!own.Waug) HIPCHECK(h, hipMalloc((void **)&own.Waug, lstm_small_waug_floats(E, own.H) * sizeof(float)));
  HIPCHECK(h, launch_pack_lstm_small(h->vars[own.kernel].dev, h->vars[own.bias].dev, E, own.H, own.Waug, st));
  own.waug_valid = true;
  return 0;
}

// LstmSmallArgs / LstmPersistArgs: the few-sequences kernel and the single-query cluster kernel read the same operands
template <class Args>
void fill_small_args(sse_handle *h, Encoder &e, Args &a) {
  const sse_config &c = h->cfg;
  a.emb = h->vars[0].dev;
  a.Waug = lstm_owner(h, e).Waug;
  a.M = h->vars[e.proj].dev;
  a.err = h->err_flag;
  a.V = c.vocab_size;
  a.E = c.embedding_size;
  a.H = e.H;
  a.S = c.encoding_size;
  a.pad_stride = e.H;
}

// pad-prefix table of the few-sequences kernel (lstm_small.hip); both cluster kernels share its arithmetic and read it too
int ensure_pad_table_small(sse_handle *h, Encoder &own, int T, hipStream_t st) {
  return ensure_pad_table(h, own.pad_small, own.H, T, st, [&](const int32_t *ids, float *out, int Tt) {
    if (ensure_waug(h, own, st)) return 1;
    LstmSmallArgs a;
    fill_small_args(h, own, a);  // the LSTM of `own` with any projection of that cell size (the table only records h, c)
    a.ids = ids;
    a.out = out;
    a.B = 1;
    a.T = Tt;
    a.normalize = 0;
    a.rec_h = own.pad_small.h;
    a.rec_c = own.pad_small.c;
    HIPCHECK(h, launch_lstm_small(a, st));
    return 0;
  });
}

// Batches the MFMA cluster kernel (lstm_cluster.hip) takes: 33 rows up to lstm_cluster_chunks launches of lstm_cluster_rows
// (<= 1024) rows.  A launch costs about the same 0.3 ms whatever it holds (T = 32), a 32-row tile of the matrix kernel 1.2 ms
// whether 33 or 8192 rows run beside it: three launches are still ahead of it, four are not.
// With the split-bf16 matrix kernel opted in (lstm_x3: ~0.45 ms for anything up to 8192 rows, ~1e-5 from fp32) a second
// launch no longer pays: one launch only.
static bool x3_applies(const sse_handle *h, const Encoder &e) {
  return h->lstm_x3 && e.Hp <= 256 && e.H >= 64 && h->cfg.embedding_size < 64;
}
static int cluster_row_limit(const sse_handle *h, const Encoder &e) {
  const int per = std::min(h->lstm_cluster_rows, lstm_cluster_max_rows());
  return per * (x3_applies(h, e) ? 1 : std::max(1, h->lstm_cluster_chunks));
}

static int ensure_cu_count(sse_handle *h) {
  if (h->cu_count == 0) {
    hipDeviceProp_t prop;
    HIPCHECK(h, hipGetDeviceProperties(&prop, h->cfg.device));
    h->cu_count = prop.multiProcessorCount;
  }
  return 0;
}

enum class LstmPath { Unset, Persist, Cluster, Small, X3, Fwd, Error /* h->err is set */ };

// what the caller of one inference encode knows beyond the ids
struct EncodeRequest {
  const int32_t *row_map = nullptr;  // host pad-prefix row sort (encode_host_ids_locked): row b of the kernels is caller row row_map[b]
  bool padded_hint = false;          // ... with it: the batch's mean leading-PAD count is >= T / 4
  bool allow_cluster = true;         // false: the re-run of a batch whose cluster-kernel launch gave up (encode_fallback_locked)
  LstmPath path = LstmPath::Unset;   // set: choose_lstm_path already ran for this call (encode_host_ids_locked, before its sort)
};

// The LSTM kernel that runs an inference encode of B x T ids of encoder e, first match wins.  The only reader of the
// back-off after a give-up (cluster_skip): an eligible call of a backed-off kernel counts it down and goes on to the next
// candidate.  Called once per encode: the host-side pad-prefix row sort asks before it sorts, because the cluster kernel
// takes rows as they come (shape, back-off, the device's CU count and the LDS fit all enter), and hands the
// answer on in EncodeRequest::path; every other encode asks in encode_dev_locked.
LstmPath choose_lstm_path(sse_handle *h, const Encoder &e, int B, int T, const EncodeRequest &rq) {
  const sse_config &c = h->cfg;
  const bool small_ok = !rq.row_map && lstm_small_lds_bytes(c.embedding_size, e.H, c.encoding_size) <= 160 * 1024;
  // one to a few queries: the single-query cluster kernel, with every workgroup of the launch resident at once (at most half
  // the CUs are asked for)
  if (rq.allow_cluster && small_ok && B <= h->lstm_persist_rows && B <= lstm_persist_max_rows() && T <= lstm_persist_max_steps()) {
    if (h->cluster_skip[0] > 0) {
      --h->cluster_skip[0];
    } else {
      const int nwg = lstm_persist_nwg(c.embedding_size, e.H, c.encoding_size);
      if (ensure_cu_count(h)) return LstmPath::Error;
      if (nwg > 0 && 8 * nwg * 2 <= h->cu_count) return LstmPath::Persist;
    }
  }
  // mid-size batches: the MFMA cluster kernel, one CU per workgroup (a failed CU-count query is a silent "no" here)
  if (rq.allow_cluster && small_ok && B > 32 && B <= cluster_row_limit(h, e) && T <= lstm_persist_max_steps() &&
      lstm_cluster_ok(c.embedding_size, e.H, c.encoding_size)) {
    if (h->cluster_skip[1] > 0) {
      --h->cluster_skip[1];
    } else if (!ensure_cu_count(h)) {
      const int ncl = (std::min(B, std::min(h->lstm_cluster_rows, lstm_cluster_max_rows())) + 63) / 64;
      if ((ncl <= 8 ? 128 : 256) <= h->cu_count) return LstmPath::Cluster;
    }
  }
  if (B <= h->lstm_small_rows && small_ok) return LstmPath::Small;
  if (x3_applies(h, e)) return LstmPath::X3;
  return LstmPath::Fwd;
}

// Inference encode of an encoder whose shape is outside the fused kernels' layouts: lstm_generic.hip, row chunks sized so
// that the per-step operand matrix A [T][rows][E + H] stays below ~1 GiB.  Same arithmetic, device ids [B][T] in, [B][S] out.
static int encode_generic_locked(sse_handle *h, Encoder &e, const int32_t *ids, int B, int T, int normalize, float *out, hipStream_t st) {
  const sse_config &c = h->cfg;
  const int E = c.embedding_size, S = c.encoding_size;
  const GenLstmDims d0 = gen_lstm_dims(32, T, E, e.H);
  const size_t per_row = (size_t)T * d0.Kp * sizeof(float);
  int rows = (int)std::min<size_t>(8192, std::max<size_t>(32, (((size_t)1 << 30) / per_row) / 32 * 32));
  const GenLstmDims dm = gen_lstm_dims(std::min(rows, B), T, E, e.H);
  if (reserve(h, h->g_A, gen_lstm_a_floats(dm) * sizeof(float)) || reserve(h, h->g_G, (size_t)dm.Bp * 4 * dm.Hq * sizeof(float)) ||
      reserve(h, h->g_c, (size_t)dm.Bp * dm.Hq * sizeof(float)) || reserve(h, h->g_hl, (size_t)dm.Bp * dm.Hq * sizeof(float)) ||
      reserve(h, h->g_raw, (size_t)dm.Bp * S * sizeof(float)))
    return 1;
  const int side = (&e == &h->enc[1]) ? 1 : 0;
  if (h->g_ver[side] != h->weights_version || !h->g_KT[side].p) {
    if (reserve(h, h->g_KT[side], gen_lstm_kt_floats(dm) * sizeof(float)) || reserve(h, h->g_Kq[side], gen_lstm_kt_floats(dm) * sizeof(float)) ||
        reserve(h, h->g_MT[side], (size_t)S * dm.Hq * sizeof(float)))
      return 1;
    HIPCHECK(h, launch_gen_pack(h->vars[e.kernel].dev, h->vars[e.proj].dev, dm, S, (float *)h->g_KT[side].p, (float *)h->g_Kq[side].p,
                                (float *)h->g_MT[side].p, st));
    h->g_ver[side] = h->weights_version;
  }
  for (int b0 = 0; b0 < B; b0 += rows) {
    const int nb = std::min(rows, B - b0);
    const GenLstmDims d = gen_lstm_dims(nb, T, E, e.H);
    HIPCHECK(h, launch_gen_forward(ids + (size_t)b0 * T, h->vars[0].dev, c.vocab_size, (const float *)h->g_KT[side].p, h->vars[e.bias].dev, d,
                                   (float *)h->g_A.p, (float *)h->g_G.p, (float *)h->g_c.p, nullptr, (float *)h->g_hl.p, h->err_flag, st));
    HIPCHECK(h, launch_gen_project((const float *)h->g_hl.p, (const float *)h->g_MT[side].p, d, S, (float *)h->g_raw.p, st));
    if (normalize) HIPCHECK(h, launch_l2_normalize((const float *)h->g_raw.p, out + (size_t)b0 * S, nb, S, st));
    else HIPCHECK(h, hipMemcpyAsync(out + (size_t)b0 * S, h->g_raw.p, (size_t)nb * S * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

// PAD-prefix bucketing for ids that are already on the device (sse_index.py:79-85 left-pads every row):
// what encode_host_ids_locked does with a host counting sort, as two launches on the caller's stream.  *row_map / *padded
// keep the caller's values when the batch is not bucketed.
static int device_pad_sort(sse_handle *h, int side, const int32_t *ids, int B, int T, hipStream_t st, const int32_t **row_map,
                           bool *padded) {
  if (*row_map || !h->pad_skip || h->pad_sort_dev == 0 || T < 2 || T > SSE_PAD_SORT_MAX_T || B <= 64) return 0;
  volatile int32_t *stat = h->pad_stat + 2 * side;
  const int seen = h->pad_sort_dev == 2 ? 2 : (stat[0] != 0 ? (int)stat[1] : 1);  // nothing seen yet: bucket, keep the tile policy
  const bool scatter = seen != 0;
  if (!h->s_padzero.p) {
    if (reserve(h, h->s_padzero, pad_sort_zeroed_words() * sizeof(int32_t))) return 1;
    HIPCHECK(h, hipMemsetAsync(h->s_padzero.p, 0, h->s_padzero.cap, st));
  }
  if (reserve(h, h->s_padwork, pad_sort_work_words(B, T) * sizeof(int32_t))) return 1;
  if (scatter && reserve(h, h->s_padorder, (size_t)B * sizeof(int32_t))) return 1;
  h->pad_seq = h->pad_seq == INT32_MAX ? 1 : h->pad_seq + 1;
  HIPCHECK(h, launch_pad_sort(ids, B, T, (int32_t *)h->s_padzero.p, (int32_t *)h->s_padwork.p, (int32_t *)h->s_padorder.p,
                              h->pad_stat + 2 * side, h->pad_seq, scatter, st));
  if (scatter) {
    *row_map = (const int32_t *)h->s_padorder.p;
    *padded = seen == 2;
    h->pad_sorted_calls += 1;
  }
  return 0;
}

// Tag epoch of the next launch of a cluster kernel on its exchange buffer (need bytes): a fresh or re-sized buffer, or a 20-bit
// epoch that ran out, first has all its tags set to "never written".
int next_epoch(sse_handle *h, DevBuf &xchg, uint32_t &epoch, size_t need, hipStream_t st, uint32_t *next) {
  if (epoch == 0 || epoch >= (1u << 20) - 1 || need > xchg.cap) {
    if (reserve(h, xchg, need)) return 1;
    HIPCHECK(h, hipMemsetAsync(xchg.p, 0, xchg.cap, st));
    epoch = 0;
  }
  *next = ++epoch;
  return 0;
}

// testing aid (option lstm_persist_inject_miss): after a cluster-kernel launch, pretend a workgroup never arrived
int inject_miss(sse_handle *h, hipStream_t st) {
  static const int32_t four = 4;
  if (h->persist_inject) HIPCHECK(h, hipMemcpyAsync(h->err_flag, &four, sizeof four, hipMemcpyHostToDevice, st));
  return 0;
}

// one to a few queries (sse_demo / webserver): a cluster of workgroups with the weights resident in LDS, see lstm_persist.hip
int encode_persist(sse_handle *h, int side, const int32_t *ids, int B, int T, int normalize, float *out, hipStream_t st) {
  Encoder &e = h->enc[side], &own = lstm_owner(h, e);
  if (ensure_waug(h, own, st)) return 1;
  LstmPersistArgs pa;
  fill_small_args(h, e, pa);
  pa.ids = ids;
  pa.out = out;
  pa.B = B;
  pa.T = T;
  pa.normalize = normalize ? 1 : 0;
  if (h->pad_skip && T > 1) {
    if (ensure_pad_table_small(h, own, T, st)) return 1;  // same arithmetic, same table
    pa.pad_h = own.pad_small.h;
    pa.pad_c = own.pad_small.c;
  }
  const size_t nhx = lstm_persist_hx_words(e.H), nraw = lstm_persist_raw_words(h->cfg.encoding_size);
  if (next_epoch(h, h->s_persist, h->persist_epoch, (nhx + nraw) * sizeof(unsigned long long), st, &pa.epoch)) return 1;
  pa.write_through = h->lstm_cluster_wt;
  pa.plain_launch = h->lstm_cluster_coop ? 0 : 1;
  pa.hx = (unsigned long long *)h->s_persist.p;
  pa.rawx = pa.hx + nhx;
  HIPCHECK(h, launch_lstm_persist(pa, st));
  return inject_miss(h, st);
}

// mid-size batches (the evaluator's 600, the index builder's 1000): the hidden units of every 64-row tile spread over a
// cluster of 16 compute units, weights in LDS, h_t exchanged per step (lstm_cluster.hip); launches of lstm_cluster_rows rows
int encode_cluster(sse_handle *h, int side, const int32_t *ids, int B, int T, int normalize, float *out, hipStream_t st) {
  const sse_config &c = h->cfg;
  Encoder &e = h->enc[side], &own = lstm_owner(h, e);
  if (!own.wc_valid) {
    if (!own.Wc) HIPCHECK(h, hipMalloc((void **)&own.Wc, lstm_cluster_weight_floats(c.embedding_size, own.H) * sizeof(float)));
    HIPCHECK(h, launch_pack_lstm_cluster(h->vars[own.kernel].dev, h->vars[own.bias].dev, c.embedding_size, own.H, own.Wc, st));
    own.wc_valid = true;
  }
  LstmClusterArgs ca;
  ca.emb = h->emb_pad;
  ca.Wc = own.Wc;
  ca.Mp = e.Mp;
  ca.err = h->err_flag;
  ca.T = T;
  ca.V = c.vocab_size;
  ca.E = c.embedding_size;
  ca.Ep = e.Ep;
  ca.KGx = e.KGx;
  ca.H = e.H;
  ca.Hp = e.H <= 128 ? 128 : 256;
  ca.KGh = ca.Hp / 8;
  ca.S = c.encoding_size;
  ca.NTS = (c.encoding_size + 31) / 32;
  ca.normalize = normalize ? 1 : 0;
  if (h->pad_skip && T > 1) {
    if (ensure_pad_table_small(h, own, T, st)) return 1;  // lstm_small's table: the same arithmetic
    ca.pad_h = own.pad_small.h;
    ca.pad_c = own.pad_small.c;
    ca.pad_stride = e.H;
  }
  ca.write_through = h->lstm_cluster_wt;
  ca.plain_launch = h->lstm_cluster_coop ? 0 : 1;
  ca.drop_wg = h->lstm_cluster_drop;
  const int per = std::min(h->lstm_cluster_rows, lstm_cluster_max_rows());
  const size_t nhx = lstm_cluster_hx_words(e.H), nsx = lstm_cluster_sx_words();
  for (int c0 = 0; c0 < B; c0 += per) {  // launches of the same stream reuse the exchange buffers under new epochs
    if (next_epoch(h, h->s_cluster, h->cluster_epoch, (nhx + nsx) * sizeof(unsigned long long), st, &ca.epoch)) return 1;
    ca.hx = (unsigned long long *)h->s_cluster.p;
    ca.sx = ca.hx + nhx;
    ca.ids = ids + (size_t)c0 * T;
    ca.out = out + (size_t)c0 * c.encoding_size;
    ca.B = std::min(per, B - c0);
    HIPCHECK(h, launch_lstm_cluster(ca, st));
  }
  return inject_miss(h, st);
}

// a handful of sequences (demo / web query, last batch of an index build): GEMV on the vector ALUs, see lstm_small.hip
int encode_small(sse_handle *h, int side, const int32_t *ids, int B, int T, int normalize, float *out, hipStream_t st) {
  Encoder &e = h->enc[side], &own = lstm_owner(h, e);
  if (ensure_waug(h, own, st)) return 1;
  LstmSmallArgs sa;
  fill_small_args(h, e, sa);
  sa.ids = ids;
  sa.out = out;
  sa.B = B;
  sa.T = T;
  sa.normalize = normalize ? 1 : 0;
  if (h->pad_skip && T > 1) {
    if (ensure_pad_table_small(h, own, T, st)) return 1;
    sa.pad_h = own.pad_small.h;
    sa.pad_c = own.pad_small.c;
  }
  HIPCHECK(h, launch_lstm_small(sa, st));
  return 0;
}

// opt-in: the gate GEMMs on the bf16 matrix pipe with hi + lo split operands (lstm_fwd_x3.hip); ~1e-5 from the fp32 path
int encode_x3(sse_handle *h, int side, const int32_t *ids, int B, int T, int normalize, float *out, const EncodeRequest &rq,
              hipStream_t st) {
  const sse_config &c = h->cfg;
  Encoder &e = h->enc[side], &own = lstm_owner(h, e);
  const int E = c.embedding_size;
  if (!own.x3_valid || !h->emb16_valid) {
    if (!own.Wx3) HIPCHECK(h, hipMalloc((void **)&own.Wx3, lstm_x3_weight_elems(E, own.Hp) * sizeof(unsigned short)));
    if (!h->emb16) HIPCHECK(h, hipMalloc((void **)&h->emb16, lstm_x3_emb_elems(c.vocab_size, E) * sizeof(unsigned short)));
    HIPCHECK(h, launch_pack_lstm_x3(h->vars[own.kernel].dev, h->vars[own.bias].dev, h->vars[0].dev, c.vocab_size, E, own.H,
                                    own.Hp, own.Wx3, h->emb16_valid ? nullptr : h->emb16, 0, st));
    own.x3_valid = true;
    h->emb16_valid = true;
  }
  LstmX3Args xa;
  xa.ids = ids;
  xa.emb16 = h->emb16;
  xa.Wx3 = own.Wx3;
  xa.Mp = e.Mp;
  xa.out = out;
  xa.err = h->err_flag;
  xa.B = B;
  xa.T = T;
  xa.V = c.vocab_size;
  xa.KGX = lstm_x3_kgx(E);
  xa.H = e.H;
  xa.S = c.encoding_size;
  xa.NTS = (c.encoding_size + 31) / 32;
  xa.normalize = normalize ? 1 : 0;
  xa.row_map = rq.row_map;
  bool padded = false;
  if (device_pad_sort(h, side, ids, B, T, st, &xa.row_map, &padded)) return 1;
  if (h->pad_skip && T > 1) {
    if (ensure_pad_table(h, own.pad_x3, own.Hp, T, st, [&](const int32_t *zero_ids, float *scratch, int Tt) {
          LstmX3Args ta = xa;
          ta.ids = zero_ids;
          ta.out = scratch;
          ta.B = 1;
          ta.T = Tt;
          ta.normalize = 0;
          ta.row_map = nullptr;
          ta.rec_h = own.pad_x3.h;
          ta.rec_c = own.pad_x3.c;
          HIPCHECK(h, launch_lstm_fwd_x3(ta, st));
          return 0;
        }))
      return 1;
    xa.pad_h = own.pad_x3.h;
    xa.pad_c = own.pad_x3.c;
  }
  HIPCHECK(h, launch_lstm_fwd_x3(xa, st));
  return 0;
}

// *use = the x-projection table of the LSTM owner serves this B x T batch: the lstm_x_table policy wants it and it is valid or
// has just been (re)built on st.  Otherwise the caller takes the embedding-gather path.
int ensure_x_table(sse_handle *h, Encoder &own, int B, int T, hipStream_t st, bool *use) {
  *use = false;
  if (h->lstm_x_table == 0 || own.Hp < 256) return 0;
  const int64_t V = h->cfg.vocab_size;
  const int UBt = (own.H + 31) / 32;
  const size_t bytes = lstm_xtable_floats(V, UBt) * sizeof(float);
  if (bytes > ((size_t)h->lstm_x_table_mb << 20) || bytes > (size_t)INT32_MAX) return 0;  // (lstm_fwd reads it with 32-bit offsets)
  if (own.xtab_valid) {
    *use = true;
    return 0;
  }
  if (h->lstm_x_table == 1 && (int64_t)B * T < V) return 0;
  if (!own.xtab && hipMalloc((void **)&own.xtab, bytes) != hipSuccess) {
    (void)hipGetLastError();  // out of device memory: the embedding-gather path needs no table
    own.xtab = nullptr;
    return 0;
  }
  HIPCHECK(h, launch_lstm_xtable(h->emb_pad, own.Wp, V, own.Ep, own.KGx, own.KGh, UBt, own.xtab, st));
  own.xtab_valid = true;
  h->x_table_builds += 1;
  *use = true;
  return 0;
}

// the MFMA matrix kernel (lstm_fwd.hip / lstm_fwd_gs.hip): any batch
int encode_fwd(sse_handle *h, int side, const int32_t *ids, int B, int T, int normalize, float *out, const EncodeRequest &rq,
               hipStream_t st) {
  Encoder &e = h->enc[side], &own = lstm_owner(h, e);
  LstmFwdArgs a;
  fill_fwd_args(h, e, a);
  a.ids = ids;
  a.out = out;
  a.B = B;
  a.T = T;
  a.normalize = normalize ? 1 : 0;
  a.row_map = rq.row_map;
  bool padded_hint = rq.padded_hint;
  if (device_pad_sort(h, side, ids, B, T, st, &a.row_map, &padded_hint)) return 1;
  if (h->pad_skip && T > 1) {
    if (ensure_pad_table(h, own.pad_fwd, own.Hp, T, st, [&](const int32_t *zero_ids, float *scratch, int Tt) {
          LstmFwdArgs ta;
          fill_fwd_args(h, own, ta);
          ta.ids = zero_ids;
          ta.out = scratch;
          ta.B = 1;
          ta.T = Tt;
          ta.normalize = 0;
          ta.rec_h = own.pad_fwd.h;
          ta.rec_c = own.pad_fwd.c;
          HIPCHECK(h, launch_lstm_fwd(ta, own.Hp, st));
          return 0;
        }))
      return 1;
    a.pad_h = own.pad_fwd.h;
    a.pad_c = own.pad_fwd.c;
    // a heavily left-padded batch sorted by pad count (sse_encode's host path knows both): tiles differ in length, the finer
    // 32-row granularity with two workgroups per CU balances them better -- crosslingual index build 2.96 -> 2.64 ms, queries
    // 1.24 -> 0.84 ms (profiles/r05_notes.txt)
    if (padded_hint && a.row_map && e.Hp <= 256) a.force_rows = 32;
  }
  bool use_xt = false;
  if (ensure_x_table(h, own, B, T, st, &use_xt)) return 1;
  if (use_xt) {
    a.xtab = own.xtab;
    a.xtab_ub = (own.H + 31) / 32;
  }
  const int variant = lstm_fwd_variant(a, e.Hp);
  h->lstm_path_calls[(variant & 64) ? PATH_FWD_ROWS64 : PATH_FWD_ROWS32] += 1;
  if (variant & LSTM_FWD_GATE_SPLIT) h->lstm_path_calls[PATH_FWD_GS] += 1;
  if (variant & LSTM_FWD_X_TABLE) h->lstm_path_calls[PATH_FWD_XT] += 1;
  HIPCHECK(h, launch_lstm_fwd(a, e.Hp, st));
  return 0;
}

int encode_dev_locked(sse_handle *h, int side, const int32_t *ids, int B, int T, int normalize, float *out, hipStream_t st,
                      const EncodeRequest &rq = EncodeRequest()) {
  const sse_config &c = h->cfg;
  if (side != SSE_SIDE_SOURCE && side != SSE_SIDE_TARGET) return fail(h, "side must be 0 (source) or 1 (target)");
  if (B < 0 || T < 1) return fail(h, "bad batch shape B=%d T=%d", B, T);
  if (B == 0) return 0;
  if (side == SSE_SIDE_TARGET && h->tgt_table >= 0) {
    // source-encoder-only / source_only_cnn: the "target encoder" is the free matrix
    // tgt_seq_embedding [N,S] (sse_model.py:214,233); norm_tgt_seq_embedding ignores the feed
    // and yields all N rows.  Honour that contract when the caller asks for exactly N rows.
    const Variable &tv = h->vars[h->tgt_table];
    if (B != tv.rows)
      return fail(h, "network mode has no target sequence encoder: tgt_seq_embedding is a [%d,%d] variable "
                     "(sse_model.py:214,233); request exactly %d rows", tv.rows, tv.cols, tv.rows);
    if (normalize) HIPCHECK(h, launch_l2_normalize(tv.dev, out, tv.rows, tv.cols, st));
    else HIPCHECK(h, hipMemcpyAsync(out, tv.dev, tv.count * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
  }
  if (c.network_mode == SSE_MODE_SOURCE_ONLY_CNN) {
    if (ensure_packed(h, st)) return 1;
    const int Ep = emb_cols(c);
    if (T < 5) return fail(h, "source_only_cnn needs max_seq_length >= 5 (widest filter)");
    if (cnn_lds_bytes(T, Ep, 0) > 160 * 1024)
      return fail(h, "source_only_cnn: T*E = %d*%d does not fit the LDS tile of the gfx950 kernel", T, c.embedding_size);
    if (reserve(h, h->s_feat, (size_t)((B + 31) / 32) * 72 * 256 * sizeof(float))) return 1;
    if (h->cnn_bf16) {
      const int Ep8 = round_up(c.embedding_size, 8);
      if (cnn_bf16_lds_bytes(T, Ep8, 0) > 160 * 1024)
        return fail(h, "source_only_cnn (bf16): T*E = %d*%d does not fit the LDS tile of the gfx950 kernel", T, c.embedding_size);
      HIPCHECK(h, launch_cnn_fwd_bf16(ids, h->emb_bf16, h->cnn_Wc16, h->cnn_bias, (float *)h->s_feat.p, h->err_flag, B, T,
                                      c.vocab_size, Ep8, nullptr, nullptr, st));
      HIPCHECK(h, launch_cnn_proj_x3((const float *)h->s_feat.p, h->cnn_Mx3, out, B, c.encoding_size, normalize ? 1 : 0, st));
      return 0;
    }
    HIPCHECK(h, launch_cnn_fwd(ids, h->emb_pad, h->cnn_Wc, h->cnn_bias, h->cnn_Mp, (float *)h->s_feat.p, out, h->err_flag, B,
                               T, c.vocab_size, Ep, c.encoding_size, normalize ? 1 : 0, nullptr, nullptr, st));
    return 0;
  }
  Encoder &e = h->enc[side];
  if (e.kernel < 0) return fail(h, "network mode has no %s sequence encoder (sse_model.py:231-233)", side ? "target" : "source");
  if (e.generic) {
    h->lstm_path_calls[PATH_GENERIC] += 1;
    return encode_generic_locked(h, e, ids, B, T, normalize, out, st);
  }
  if (ensure_packed(h, st)) return 1;
  switch (rq.path != LstmPath::Unset ? rq.path : choose_lstm_path(h, e, B, T, rq)) {
    case LstmPath::Persist: h->lstm_path_calls[PATH_PERSIST] += 1; return encode_persist(h, side, ids, B, T, normalize, out, st);
    case LstmPath::Cluster: h->lstm_path_calls[PATH_CLUSTER] += 1; return encode_cluster(h, side, ids, B, T, normalize, out, st);
    case LstmPath::Small: h->lstm_path_calls[PATH_SMALL] += 1; return encode_small(h, side, ids, B, T, normalize, out, st);
    case LstmPath::X3: h->lstm_path_calls[PATH_X3] += 1; return encode_x3(h, side, ids, B, T, normalize, out, rq, st);
    case LstmPath::Fwd: h->lstm_path_calls[PATH_FWD] += 1; return encode_fwd(h, side, ids, B, T, normalize, out, rq, st);
    case LstmPath::Unset:
    case LstmPath::Error: break;
  }
  return 1;
}

// bits: (optional) receives the raw flag; a flag that is exactly bit 2 (cluster kernel: a workgroup did not arrive) is then
// cleared and reported through *bits with rc 0, so that the caller can re-run the batch on another kernel
int check_err_flag(sse_handle *h, hipStream_t st, int32_t *bits = nullptr) {
  HIPCHECK(h, hipMemcpyAsync(h->pin_small, h->err_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHECK(h, sync_stream(st));
  const int32_t flag = h->pin_small[0];
  if (bits) *bits = flag;
  if (flag) {
    HIPCHECK(h, hipMemsetAsync(h->err_flag, 0, sizeof(int32_t), st));
    if (bits && flag == 4) return 0;
    if (flag & 1) return fail(h, "token id out of range [0, %d) (tf.gather would raise; sse_model.py:163-164)", h->cfg.vocab_size);
    if (flag & 2) return fail(h, "corpus row out of range in a train step by rows");
    if (flag & 8) return fail(h, "data-parallel embedding-gradient exchange: more touched rows than the packed buffer holds, or a row id "
                                 "out of range in a gathered buffer (sse_train_pack_embedding_grad / sse_train_unpack_embedding_grad)");
    if (flag & 16) return fail(h, "sse_score_rank_dev: a pair_q out of [0, Q) or, without pair scores, a pair_id that is not a row of "
                                  "this index; the call wrote no output");
    if (flag & 32) return fail(h, "sse_score_above_dev: a pair_q out of [0, Q); the call wrote no output");
    if (flag & 64) return fail(h, "sse_score_above: the emitting pass found other rows than the counting pass; the lists of the call are not valid");
    if (flag & SSE_ERR_INDEX_IDS) return fail(h, "sse_index_update_dev: an id outside the index, or ids not strictly increasing; the "
                                                 "call changed nothing");
    if (flag & 4) return fail(h, "LSTM cluster kernel: a workgroup of a cluster did not arrive (device oversubscribed?); the "
                                 "host-buffer entry points fall back to the few-sequences kernel by themselves, for "
                                 "sse_encode_dev set option lstm_persist_rows to 0");
    return fail(h, "device error flag 0x%x", flag);
  }
  return 0;
}

// The shapes an index can have.  The upload entry points ask this BEFORE they free, allocate or invalidate anything: a refused
// upload leaves the resident index, its float64 rows, tags and group keys as they were.
int index_shape_check(sse_handle *h, int64_t N, int64_t S) {
  if (N <= 0 || S <= 0) return fail(h, "empty index");
  if (S > SSE_MAX_INDEX_DIM) return fail(h, "index dimension %lld > %d not supported by the scoring kernel", (long long)S, SSE_MAX_INDEX_DIM);
  if (N > (int64_t)2147483000) return fail(h, "index shard too large for int32 row ids");
  return 0;
}

int index_from_dev_rows(sse_handle *h, const float *rows_dev, int64_t N, int S, int64_t id_base, hipStream_t st) {
  if (index_shape_check(h, N, S)) return 1;
  const int KG = (S + 7) / 8;
  const int64_t NT = (N + 31) / 32;
  h->tags_set = false;  // (tags belong to the rows they were set for)
  h->groups_set = false;  // (and so do group keys)
  h->bias_set = false;    // (and the bias)
  // fragment-order copy of the index: grow-only (re-indexing with the same or a smaller shard reuses the allocation)
  const size_t need = (size_t)NT * KG * 256 * sizeof(float);
  if (need > h->idxp_cap) {
    if (h->idxp) HIPCHECK(h, hipFree(h->idxp));
    h->idxp = nullptr;
    h->idxp_cap = 0;
    HIPCHECK(h, hipMalloc((void **)&h->idxp, need));
    h->idxp_cap = need;
  }
  if (reserve(h, h->s_tmp2, 16)) return 1;
  HIPCHECK(h, hipMemsetAsync(h->s_tmp2.p, 0, 4, st));
  HIPCHECK(h, launch_pack_rows_norm(rows_dev, N, S, h->idxp, (float *)h->s_tmp2.p, st));
  h->idx_norm_vec = (S & 3) == 0 && (reinterpret_cast<uintptr_t>(rows_dev) & 15) == 0;  // (the path launch_pack_rows_norm took)
  h->idx_norm2_valid = false;
  // the small-index scorer's split-bf16 image: once per index, from the fragment copy just written (the index is resident
  // and constant from call to call); an index it cannot serve leaves no image behind
  h->idx_x3_valid = false;
  if (score_small_index_applies(1024, KG, NT)) {
    if (reserve(h, h->idx_x3, (size_t)NT * ((KG + 1) / 2) * 2048)) return 1;
    HIPCHECK(h, launch_frag32_to_split_bf16(h->idxp, NT, KG, h->idx_x3.p, st));
    h->idx_x3_valid = true;
  }
  float n2 = 0;
  HIPCHECK(h, hipMemcpyAsync(&n2, h->s_tmp2.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHECK(h, hipStreamSynchronize(st));
  h->idx_norm_max = std::sqrt(n2);
  // small indexes (the evaluator's 571 targets, anything up to 64 MiB) also keep their rows as they came: the float64
  // re-scoring of 16384 queries x 10 rows gathered every row from 64 cache lines of the fragment copy
  h->idx_rm_valid = false;
  if ((S & 3) == 0 && (size_t)N * S * sizeof(float) <= ((size_t)64 << 20) && (reinterpret_cast<uintptr_t>(rows_dev) & 15) == 0) {
    if (reserve(h, h->idx_rm, (size_t)N * S * sizeof(float))) return 1;
    HIPCHECK(h, hipMemcpyAsync(h->idx_rm.p, rows_dev, (size_t)N * S * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHECK(h, hipStreamSynchronize(st));  // (rows_dev may be the caller's, or scratch that is reused)
    h->idx_rm_valid = true;
  }
  h->idxp16_valid = false;
  h->idx_N = N;
  h->idx_S = S;
  h->idx_base = id_base;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// sse_index_update* / sse_index_append* (DESIGN K6n).  After any sequence of them the handle answers as a fresh handle given
// the final rows, tags, keys and bias.

// an allocation of at least `need` bytes that still holds its first `used` bytes (reserve() drops the contents); the growth
// is geometric; *grew reports a reallocation
int grow_keep(sse_handle *h, void **p, size_t *cap, size_t used, size_t need, hipStream_t st, bool *grew = nullptr) {
  if (need <= *cap) return 0;
  const size_t ncap = std::max(need, *cap * 2) + 256;
  void *np = nullptr;
  HIPCHECK(h, hipMalloc(&np, ncap));
  if (*p && used) {
    const hipError_t e = hipMemcpyAsync(np, *p, used, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
      (void)hipFree(np);
      return fail(h, "index growth: copy failed: %s", hipGetErrorString(e));
    }
  }
  HIPCHECK(h, hipStreamSynchronize(st));
  if (*p) HIPCHECK(h, hipFree(*p));
  *p = np;
  *cap = ncap;
  if (grew) *grew = true;
  return 0;
}
int grow_keep(sse_handle *h, DevBuf &b, size_t used, size_t need, hipStream_t st) { return grow_keep(h, &b.p, &b.cap, used, need, st); }

struct IndexDelta {
  const char *name;        // the entry point, for messages
  bool append;
  const int64_t *ids;      // update: [M] global ids on the device (already checked, or checked on the device: check_ids)
  bool check_ids;
  const float *rows32;     // [M][S] on the device; at most one of the two
  const double *rows64;
  int64_t M;
  const uint64_t *tags;    // [M] on the device, or nullptr
  const int64_t *groups;
  const float *bias;
};

// every refusal that needs no look at the operands' contents; nothing has been touched when one fires
int index_delta_check(sse_handle *h, const char *name, bool append, bool f64, bool has_rows, int64_t M, const void *tags,
                      const void *groups, const void *bias) {
  if (!h->idxp || h->idx_N <= 0) return fail(h, "%s: no index uploaded", name);
  if (M < 0) return fail(h, "%s: M = %lld", name, (long long)M);
  if (has_rows && f64 != (h->idx64 != nullptr))
    return fail(h, f64 ? "%s: the resident index holds no float64 rows (it was not uploaded with sse_index_upload_f64); use the float form"
                       : "%s: the resident index holds float64 rows (sse_index_upload_f64); use the _f64 form", name);
  if (append) {
    if (!has_rows) return fail(h, "%s: rows must not be NULL", name);
    if ((tags != nullptr) != h->tags_set || (groups != nullptr) != h->groups_set || (bias != nullptr) != h->bias_set)
      return fail(h, "%s: tags, groups and bias must be given exactly when the resident index has them set (tags %s, groups %s, bias %s); "
                     "the index is unchanged", name, h->tags_set ? "set" : "not set", h->groups_set ? "set" : "not set",
                  h->bias_set ? "set" : "not set");
    if (h->idx_N + M > (int64_t)2147483000) return fail(h, "%s: %lld + %lld rows: index shard too large for int32 row ids", name,
                                                         (long long)h->idx_N, (long long)M);
  } else {
    if (!has_rows && !tags && !groups && !bias) return fail(h, "%s: rows is NULL and so is every column: nothing to update", name);
    if ((tags && !h->tags_set) || (groups && !h->groups_set) || (bias && !h->bias_set))
      return fail(h, "%s: a column was given that is not set on the resident index (sse_index_set_tags / _groups / _bias first); "
                     "the index is unchanged", name);
  }
  return 0;
}

// room for `newN` rows in every per-index buffer, contents kept; new tiles of idxp, the tags and the bias start as zeros
int index_grow(sse_handle *h, int64_t newN, hipStream_t st) {
  const int64_t N = h->idx_N, NT = (N + 31) / 32, newNT = (newN + 31) / 32;
  const size_t S = (size_t)h->idx_S, KG = (S + 7) / 8, KB = (KG + 1) / 2;
  bool grew = false;
  if (grow_keep(h, (void **)&h->idxp, &h->idxp_cap, (size_t)NT * KG * 1024, (size_t)newNT * KG * 1024, st, &grew)) return 1;
  if (grew) h->index_grow_copies += 1;
  if (newNT > NT) HIPCHECK(h, hipMemsetAsync(h->idxp + (size_t)NT * KG * 256, 0, (size_t)(newNT - NT) * KG * 1024, st));
  // (an upload of that many rows keeps no row-major copy / no split image; the two flags fall only after the last
  // allocation that can fail, so a refused append leaves the routes as they were)
  const bool drop_rm = h->idx_rm_valid && (size_t)newN * S * sizeof(float) > ((size_t)64 << 20);
  const bool drop_x3 = h->idx_x3_valid && !score_small_index_applies(1024, (int)KG, newNT);
  if (h->idx_rm_valid && !drop_rm && grow_keep(h, h->idx_rm, (size_t)N * S * 4, (size_t)newN * S * 4, st)) return 1;
  if (h->idx64) {
    if (h->idx64_cap < (size_t)N * S * 8) h->idx64_cap = (size_t)N * S * 8;
    if (grow_keep(h, (void **)&h->idx64, &h->idx64_cap, (size_t)N * S * 8, (size_t)newN * S * 8, st)) return 1;
  }
  if (h->idx_x3_valid && !drop_x3 && grow_keep(h, h->idx_x3, (size_t)NT * KB * 2048, (size_t)newNT * KB * 2048, st)) return 1;
  if (h->idxp16_valid && grow_keep(h, &h->idxp16, &h->idxp16_cap, (size_t)NT * KB * 1024, (size_t)newNT * KB * 1024, st)) return 1;
  if (h->tags_set) {
    if (grow_keep(h, h->idx_tags, (size_t)NT * 32 * 8, (size_t)newNT * 32 * 8, st)) return 1;
    if (grow_keep(h, h->idx_tag_sum, (size_t)NT * 8, (size_t)newNT * 8, st)) return 1;
    if (newNT > NT) HIPCHECK(h, hipMemsetAsync((uint64_t *)h->idx_tags.p + NT * 32, 0, (size_t)(newNT - NT) * 32 * 8, st));
  }
  if (h->groups_set && grow_keep(h, h->idx_groups, (size_t)N * 8, (size_t)newN * 8, st)) return 1;
  if (h->bias_set && grow_keep(h, h->idx_bias, (size_t)NT * 32 * 4, (size_t)newNT * 32 * 4, st)) return 1;  // (launch_bias_prepare zeroes the padding)
  if (grow_keep(h, h->idx_norm2, h->idx_norm2_valid ? (size_t)N * 4 : 0, (size_t)newN * 4, st)) return 1;
  if (drop_rm) h->idx_rm_valid = false;
  if (drop_x3) h->idx_x3_valid = false;
  return 0;
}

// the device half of every form: operands on the device, index_delta_check passed.  One synchronisation of `st` at the end
// (idx_norm_max lives on the host, and the device's verdict on the ids is read with it).
int index_apply_delta(sse_handle *h, const IndexDelta &d, hipStream_t st) {
  if (d.M == 0) return 0;
  const int S = h->idx_S, KG = (S + 7) / 8;
  const int64_t N = h->idx_N, newN = d.append ? N + d.M : N;
  const bool rows = d.rows32 || d.rows64;
  if (d.append) {
    if (index_grow(h, newN, st)) return 1;
  } else if (rows && reserve(h, h->idx_norm2, (size_t)N * sizeof(float))) {  // (not valid yet whenever this reallocates)
    return 1;
  }
  if (reserve(h, h->s_tmp2, 16)) return 1;
  if (d.check_ids) HIPCHECK(h, launch_index_ids_check(d.ids, d.M, h->idx_base, h->idx_base + N, h->err_flag, st));
  const IndexRowList rl{d.append ? nullptr : d.ids, h->idx_base, N, d.M, d.check_ids ? h->err_flag : nullptr};
  if (rows) {
    float *norm2 = (float *)h->idx_norm2.p;
    if (!h->idx_norm2_valid) {  // first update after an upload: every row's sum from the fragment copy, as the pack formed it
      const IndexRowList all{nullptr, h->idx_base, 0, N, nullptr};
      HIPCHECK(h, launch_index_row_norms(all, h->idxp, S, h->idx_norm_vec, norm2, st));
      h->idx_norm2_valid = true;
    }
    HIPCHECK(h, launch_index_scatter_rows(rl, d.rows32, d.rows64, S, h->idxp, h->idx_rm_valid ? (float *)h->idx_rm.p : nullptr,
                                          h->idx64, st));
    HIPCHECK(h, launch_index_row_norms(rl, h->idxp, S, h->idx_norm_vec, norm2, st));
    HIPCHECK(h, hipMemsetAsync(h->s_tmp2.p, 0, 4, st));
    HIPCHECK(h, launch_index_norm_max(norm2, newN, rl.err, (float *)h->s_tmp2.p, st));
    if (h->idx_x3_valid) HIPCHECK(h, launch_frag32_to_split_bf16_rows(rl, h->idxp, KG, h->idx_x3.p, st));
    if (h->idxp16_valid) HIPCHECK(h, launch_frag32_to_bf16_rows(rl, h->idxp, KG, h->idxp16, st));
  }
  if (d.tags || d.groups || d.bias) {
    const int64_t newNT = (newN + 31) / 32;
    HIPCHECK(h, launch_index_scatter_cols(rl, d.tags, (uint64_t *)h->idx_tags.p, d.groups, (int64_t *)h->idx_groups.p, d.bias,
                                          (float *)h->idx_bias.p, st));
    // the touched tiles' ORs and max |bias| fall as well as rise: both are formed again from the columns (O(N) words)
    if (d.tags) HIPCHECK(h, launch_tag_tile_summary((const uint64_t *)h->idx_tags.p, newNT, (uint64_t *)h->idx_tag_sum.p, st));
    if (d.bias) {
      HIPCHECK(h, hipMemsetAsync(h->idx_bias_absmax.p, 0, sizeof(float), st));
      HIPCHECK(h, launch_bias_prepare((float *)h->idx_bias.p, newN, newNT, (float *)h->idx_bias_absmax.p, st));
    }
  }
  if (rows) HIPCHECK(h, hipMemcpyAsync(h->pin_small + 1, h->s_tmp2.p, 4, hipMemcpyDeviceToHost, st));
  if (d.check_ids) {
    int32_t bits = 0;
    if (check_err_flag(h, st, &bits)) return 1;
  } else {
    HIPCHECK(h, sync_stream(st));
  }
  if (rows) {
    float n2;
    memcpy(&n2, h->pin_small + 1, 4);
    h->idx_norm_max = std::sqrt(n2);
  }
  h->idx_N = newN;
  if (d.append) h->index_append_rows += d.M;
  else h->index_update_calls += 1, h->index_update_rows += d.M;
  return 0;
}

// the host forms: ids in range and strictly increasing, a finite bias (both before anything is touched), then every operand
// staged on the device in one buffer
template <typename T>
int index_delta_host(sse_handle *h, const char *name, bool append, const int64_t *ids, const T *rows, int64_t M,
                     const uint64_t *tags, const int64_t *groups, const float *bias) {
  if (index_delta_check(h, name, append, sizeof(T) == 8, rows != nullptr, M, tags, groups, bias)) return 1;
  if (M == 0) return 0;
  if (!append) {
    if (!ids) return fail(h, "%s: ids must not be NULL", name);
    for (int64_t m = 0; m < M; ++m) {
      if (ids[m] < h->idx_base || ids[m] >= h->idx_base + h->idx_N)
        return fail(h, "%s: ids[%lld] = %lld is outside the index [%lld, %lld); the index is unchanged", name, (long long)m,
                    (long long)ids[m], (long long)h->idx_base, (long long)(h->idx_base + h->idx_N));
      if (m > 0 && ids[m - 1] >= ids[m])
        return fail(h, "%s: ids must be strictly increasing (ids[%lld] = %lld after %lld); the index is unchanged", name, (long long)m,
                    (long long)ids[m], (long long)ids[m - 1]);
    }
  }
  if (bias)
    for (int64_t m = 0; m < M; ++m)
      if (!std::isfinite(bias[m]))
        return fail(h, "%s: bias[%lld] = %g is not finite; the index is unchanged", name, (long long)m, (double)bias[m]);
  const size_t S = (size_t)h->idx_S;
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_rows = rows ? pad((size_t)M * S * sizeof(T)) : 0, b8 = pad((size_t)M * 8), b4 = pad((size_t)M * 4);
  if (reserve(h, h->s_upd, b_rows + 3 * b8 + b4)) return 1;
  char *base = (char *)h->s_upd.p;
  auto put = [&](size_t off, const void *src, size_t bytes) -> const void * {
    if (!src) return nullptr;
    return hipMemcpy(base + off, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? base + off : (const void *)-1;
  };
  IndexDelta d{};
  d.name = name;
  d.append = append;
  d.M = M;
  const void *r = put(0, rows, (size_t)M * S * sizeof(T));
  d.ids = (const int64_t *)put(b_rows, append ? nullptr : ids, (size_t)M * 8);
  d.tags = (const uint64_t *)put(b_rows + b8, tags, (size_t)M * 8);
  d.groups = (const int64_t *)put(b_rows + 2 * b8, groups, (size_t)M * 8);
  d.bias = (const float *)put(b_rows + 3 * b8, bias, (size_t)M * 4);
  const void *bad = (const void *)-1;
  if (r == bad || d.ids == bad || d.tags == bad || d.groups == bad || d.bias == bad) return fail(h, "%s: staging copy failed", name);
  if (sizeof(T) == 8) d.rows64 = (const double *)r;
  else d.rows32 = (const float *)r;
  return index_apply_delta(h, d, nullptr);
}

// splits of the index range for a candidate / collect sweep (see score_dev_locked)
static int choose_nsplit(int NQ, int QB, int64_t NT) {
  // enough workgroups to fill the 256 CUs (2 waves of them when the sweep is long), at least 16 n-tiles (2 per
  // wave) per split
  int nsplit = 1;
  const int max_split = (NQ == 1) ? 256 : 128;  // 16 candidates per split, at most RS_MAXNC = 4096 per query
  while (nsplit < max_split && QB * nsplit < 512 && NT / (nsplit * 2) >= 16) nsplit *= 2;
  if (nsplit <= 8) {
    nsplit = 1;
    while (nsplit < 8 && QB * nsplit < 256 && NT / (nsplit * 2) >= 8) nsplit *= 2;
  }
  // one workgroup per CU is resident (the query block fills LDS): the launch runs in ceil(WGs/256) rounds and the
  // last round may be nearly empty (782 query blocks = 3.05 rounds ran at 76 % of the 64-block rate).  Split
  // further while that evens the rounds out by more than the extra per-split cost (~1 % per doubling).
  if (NQ >= 2) {
    auto eff = [&](int ns) {
      const double r = (double)QB * ns / 256.0;
      return r / std::ceil(r);
    };
    int best = nsplit;
    double best_score = eff(nsplit);
    // (splits down to 200 n-tiles -- 256 before round 5: the crosslingual index, 1002 tiles x 129 query blocks, stopped at 2 splits = 258
    // workgroups = one full round + one of 2 workgroups, and its 32 candidates per query left 3,850 of 16,491 crowded random-init
    // queries to the fp32 second chance: 1.60 ms per pass; 4 splits: 1.17 ms, no second chance; 8 splits 1.18; on well-spread
    // vectors 0.97 / 1.07 / 1.38 ms -- tools/bench_c3.py, profiles/r05_notes.txt)
    static const int min_tiles = getenv("SSE_SPLIT_MIN_TILES") ? atoi(getenv("SSE_SPLIT_MIN_TILES")) : 200;  // (env: measurement aid)
    for (int ns = nsplit * 2, d = 1; ns <= 128 && NT / ns >= min_tiles; ns *= 2, ++d) {
      const double sc = eff(ns) - 0.01 * d;
      if (sc > best_score + 0.01) {
        best = ns;
        best_score = sc;
      }
    }
    nsplit = best;
  }
  return nsplit;
}

// Splits of the two list-free sweeps of the two-pass route: the list sweep's choice (nsplit) weighs list warm-up against rounds;
// without lists only the rounds count -- workgroups are one per CU (VGPRs), so QB x splits should sit just below a multiple of
// the CU count: 129 query blocks x 4 splits = 2.02 rounds run as 3, x 16 = 8.06 run as 9.  At most 16 (the threshold kernel
// takes 16 x 16 lane maxima per query), at least 32 tiles per split.
static int choose_two_pass_splits(const sse_handle *h, int QB, int64_t NT, int nsplit) {
  static const int force = getenv("SSE_TWO_PASS_SPLITS") ? atoi(getenv("SSE_TWO_PASS_SPLITS")) : 0;  // (env: measurement aid)
  if (force == 1 || force == 2 || force == 4 || force == 8 || force == 16) return force;
  int ns2 = std::min(nsplit, 16);
  const int cus = h->cu_count > 0 ? h->cu_count : 256;
  double best = 0.0;
  for (int ns = 1; ns <= 16; ns *= 2) {
    if (ns > 1 && NT / ns < 32) break;
    const double r = (double)QB * ns / cus, eff = r / std::ceil(r);
    if (eff > best + 0.02) {
      best = eff;
      ns2 = ns;
    }
  }
  return ns2;
}

// query tiles per workgroup of a sweep for P columns of the resident index; the one place that refuses a dimension whose
// query block does not fit LDS
static int pick_nq(sse_handle *h, int P, bool bf, int &NQ) {
  NQ = score_pick_nq(P, h->idx_S, bf ? 1 : 0);
  if (NQ == 0) return fail(h, "index dimension %d does not fit the scoring kernel's LDS query block", h->idx_S);
  return 0;
}

// NQ, query blocks and base split count of one sweep over P columns (queries or pairs) of the resident index
struct SweepChunk {
  int NQ, QB, nsplit;
};
static int sweep_chunk(sse_handle *h, int P, SweepChunk &c, bool bf = false) {
  if (pick_nq(h, P, bf, c.NQ)) return 1;
  c.QB = (P + c.NQ * 32 - 1) / (c.NQ * 32);
  c.nsplit = choose_nsplit(c.NQ, c.QB, (h->idx_N + 31) / 32);
  return 0;
}

// The three bounds on |candidate score - float64 score| / |q| over the rows of the resident index (DESIGN K6/K7).
// fp32 MFMA candidates: |fp32 fma-chain dot - exact| <= S * 2^-24 * |q||t| (+ the f32 rounding of f64 rows); use 2x margin
static float score_eps32(const sse_handle *h) { return (float)(2.0 * (h->idx_S + 2) * 5.97e-8 * h->idx_norm_max); }
// bf16 operands: |q^.t^ - q.t| <= ((1+u)^2 - 1) sum|q_i t_i| <= (2^-8 + 2^-18) |q||t|, u = 2^-9 (round to nearest), on top of
// the fp32 accumulation's bound
static float score_eps_bf16(const sse_handle *h) {
  return score_eps32(h) + (float)(1.02 * (1.0 / 256.0 + 1.0 / 262144.0) * h->idx_norm_max);
}
// split-bf16 candidates of the small-index scorer (DESIGN K6).  bf16 keeps 8 significant bits: hi = rne(x) leaves
// |x - hi| <= 2^-8 |x|, lo = rne(x - hi) leaves e = x - hi - lo with |e| <= 2^-17 |x| (and |lo| <= 2^-8 (1 + 2^-9) |x|).  The
// dropped terms ql.tl + eq.t + (q - eq).et are <= (2^-16 + 2 * 2^-17)(1 + 2^-7) sum|q_i t_i| <= 2^-15 (1 + 2^-6) |q||t| -- reached
// to 2 % by mantissas that sit halfway in both roundings.  The 3 S kept products are exact in fp32 and are added in an order
// the matrix pipe chooses: (3 S + 2) additions of <= 2^-24 sum|terms| each (+ the f32 rounding of f64 rows), sum|terms| <=
// (1 + 2^-5) sum|q_i t_i|, with the fp32 bound's 2x margin.  1.26e-4 at S = 256 (fp32: 3.1e-5); rows or queries of norm
// below 2^-100 are outside the claim (a lo part may underflow bf16's range).
static float score_eps_split_bf16(const sse_handle *h) {
  return (float)(((1.0 + 1.0 / 64.0) / 32768.0 + 2.0 * (3 * h->idx_S + 2) * 5.97e-8 * (1.0 + 1.0 / 32.0)) * h->idx_norm_max);
}

// n_words device counters in b, zeroed when they are first reserved (they accumulate over the handle's life)
static int ensure_zeroed_once(sse_handle *h, DevBuf &b, bool &init, int n_words, hipStream_t st) {
  if (reserve(h, b, n_words * sizeof(unsigned long long))) return 1;
  if (!init) {
    HIPCHECK(h, hipMemsetAsync(b.p, 0, n_words * sizeof(unsigned long long), st));
    init = true;
  }
  return 0;
}

// diagnostic counters on the device: [0] queries whose bf16-candidate result missed its certificate, [1] queries served
// by the collect path, [2] queries that fell through to the float64 brute force
static int ensure_counters(sse_handle *h, hipStream_t st) {
  // four diagnostic counters, then the pair of "queries left uncertified" words (RescoreArgs::uncert)
  return ensure_zeroed_once(h, h->s_fb_cnt, h->fb_cnt_init, 6, st);
}

// Staging of a host-buffer entry point in h->s_stage, reserved once.  A piece is `bytes` of device memory with the host data
// that goes in before the call (src) and the host buffer its content comes back to after it (dst), either may be null.
struct StagePiece {
  size_t bytes;
  const void *src;
  void *dst;
  char *dev;  // set by stage_in: the 8-byte-aligned start of the piece
  // the piece as a kernel argument; null for an optional input the caller left out
  template <class T>
  T *as() const { return src || dst ? (T *)dev : nullptr; }
};
template <size_t N>
static int stage_in(sse_handle *h, StagePiece (&p)[N]) {
  size_t total = 0;
  for (const StagePiece &x : p) total += (x.bytes + 7) & ~(size_t)7;
  if (reserve(h, h->s_stage, total)) return 1;
  total = 0;
  for (StagePiece &x : p) {
    x.dev = (char *)h->s_stage.p + total;
    total += (x.bytes + 7) & ~(size_t)7;
    if (x.src) HIPCHECK(h, hipMemcpy(x.dev, x.src, x.bytes, hipMemcpyHostToDevice));
  }
  return 0;
}
template <size_t N>
static int stage_out(sse_handle *h, const StagePiece (&p)[N]) {
  for (const StagePiece &x : p)
    if (x.dst) HIPCHECK(h, hipMemcpy(x.dst, x.dev, x.bytes, hipMemcpyDeviceToHost));
  return 0;
}

// collect-path scratch: thresholds, slots, counters (+1: the slot allocator), row buffers
static int reserve_collect(sse_handle *h, int Q, int slots) {
  if (reserve(h, h->s_cthr, (size_t)Q * sizeof(float))) return 1;
  if (reserve(h, h->s_cslot, (size_t)Q * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_ccnt, (size_t)(slots + 1) * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_cbuf, (size_t)slots * SSE_COLLECT_CAP * sizeof(int32_t))) return 1;
  return 0;
}

// sse_score_rank*: every stage of the call queued on `st` (device pointers throughout).  Pairs go in chunks of RANK_POOL: a
// chunk's pairs are the columns of one count sweep (a pair = one query row of the sweep, so a query with several labels is
// staged once per label) and own one band buffer each.  Validation runs over ALL pairs first: one bad pair and no kernel of
// the call writes anything (the flag reaches the host through the device error word, bit 16).
static int score_rank_dev_locked(sse_handle *h, const float *q, int Q, const int32_t *pair_q, const int64_t *pair_id, int64_t L,
                                 const double *pair_score_in, int64_t *out_before, double *out_score, hipStream_t st) {
  if (!h->idxp) return fail(h, "no index uploaded");
  if (Q < 0 || L < 0) return fail(h, "bad arguments to sse_score_rank");
  if (L == 0) return 0;
  if (!q || !pair_q || !pair_id || !out_before || Q == 0) return fail(h, "bad arguments to sse_score_rank");
  const int RANK_POOL = 4096;
  const int S = h->idx_S, KG = (S + 7) / 8;
  const int64_t NT = (h->idx_N + 31) / 32;
  const int Pmax = (int)std::min<int64_t>(L, RANK_POOL);
  // per-pair scratch: thr64 [Pmax] | sure [Pmax] | lo [Pmax] | hi [Pmax] | bad
  if (reserve(h, h->s_rk, (size_t)Pmax * 24 + 16)) return 1;
  if (reserve(h, h->s_ccnt, (size_t)(Pmax + 1) * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_cbuf, (size_t)Pmax * SSE_COLLECT_CAP * sizeof(int32_t))) return 1;
  if (ensure_zeroed_once(h, h->s_rk_cnt, h->rk_cnt_init, 2, st)) return 1;
  char *base = (char *)h->s_rk.p;
  int32_t *bad = (int32_t *)(base + (size_t)Pmax * 24);
  HIPCHECK(h, hipMemsetAsync(bad, 0, sizeof(int32_t), st));
  HIPCHECK(h, launch_rank_validate(pair_q, pair_id, L, Q, pair_score_in ? 0 : 1, h->idx_base, h->idx_N, bad, h->err_flag, st));
  RankArgs a;
  a.q = q;
  a.idxp = h->idxp;
  a.idx64 = h->idx64;
  a.thr64 = (double *)base;
  a.sure = (unsigned long long *)(base + (size_t)Pmax * 8);
  a.lo = (float *)(base + (size_t)Pmax * 16);
  a.hi = (float *)(base + (size_t)Pmax * 20);
  a.band_cnt = (int32_t *)h->s_ccnt.p;
  a.band_buf = (int32_t *)h->s_cbuf.p;
  a.band_cap = SSE_COLLECT_CAP;
  a.bad = bad;
  a.counters = (unsigned long long *)h->s_rk_cnt.p;
  a.id_base = h->idx_base;
  a.N = h->idx_N;
  a.S = S;
  a.KG = KG;
  a.NT = (int)NT;
  a.eps32 = score_eps32(h);
  for (int64_t p0 = 0; p0 < L; p0 += RANK_POOL) {
    const int P = (int)std::min<int64_t>(RANK_POOL, L - p0);
    SweepChunk ck;
    if (sweep_chunk(h, P, ck)) return 1;
    a.pair_q = pair_q + p0;
    a.pair_id = pair_id + p0;
    a.pair_score_in = pair_score_in ? pair_score_in + p0 : nullptr;
    a.out_before = out_before + p0;
    a.out_score = out_score ? out_score + p0 : nullptr;
    a.P = P;
    a.NQ = ck.NQ;
    a.NSPLIT = ck.nsplit;
    HIPCHECK(h, launch_score_rank(a, st));
  }
  return 0;
}

// sse_score_above*, first half: exact counts of all L pairs into offsets[1 .. L], then the scan.  Pairs go in chunks of
// ABOVE_POOL as score_rank_dev_locked chunks them (same per-chunk scratch); ovf [L] keeps which pairs the float64 sweep took.
struct AboveCall {
  AboveArgs a;
  int64_t *offsets;
  int32_t *ovf;
  unsigned long long *cursor;
};
static const int ABOVE_POOL = 4096;
static int score_above_chunks(sse_handle *h, AboveCall &c, const int32_t *pair_q, const double *pair_thr, int64_t L, int emit, hipStream_t st) {
  AboveArgs &a = c.a;
  a.emit = emit;
  for (int64_t p0 = 0; p0 < L; p0 += ABOVE_POOL) {
    const int P = (int)std::min<int64_t>(ABOVE_POOL, L - p0);
    SweepChunk ck;
    if (sweep_chunk(h, P, ck)) return 1;
    a.pair_q = pair_q + p0;
    a.pair_thr = pair_thr + p0;
    a.counts = c.offsets + 1 + p0;
    a.offsets = c.offsets + p0;
    a.ovf = c.ovf + p0;
    a.cursor = c.cursor + p0;
    a.P = P;
    a.NQ = ck.NQ;
    a.NSPLIT = ck.nsplit;
    HIPCHECK(h, launch_score_above(a, st));
  }
  return 0;
}

static int score_above_setup(sse_handle *h, AboveCall &c, const float *q, int64_t L, int64_t *offsets, hipStream_t st) {
  const int S = h->idx_S, KG = (S + 7) / 8;
  const int Pmax = (int)std::min<int64_t>(L, ABOVE_POOL);
  // per-chunk scratch (the rank count's buffers): sure [Pmax] | lo [Pmax] | hi [Pmax] | bad
  if (reserve(h, h->s_rk, (size_t)Pmax * 24 + 16)) return 1;
  if (reserve(h, h->s_ccnt, (size_t)(Pmax + 1) * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_cbuf, (size_t)Pmax * SSE_COLLECT_CAP * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_ab, (size_t)L * 12 + 16)) return 1;  // cursor [L] | ovf [L]
  if (ensure_zeroed_once(h, h->s_ab_cnt, h->ab_cnt_init, 3, st)) return 1;
  char *base = (char *)h->s_rk.p;
  AboveArgs &a = c.a;
  a.q = q;
  a.idxp = h->idxp;
  a.idx64 = h->idx64;
  a.sure = (unsigned long long *)base;
  a.lo = (float *)(base + (size_t)Pmax * 16);
  a.hi = (float *)(base + (size_t)Pmax * 20);
  a.band_cnt = (int32_t *)h->s_ccnt.p;
  a.band_buf = (int32_t *)h->s_cbuf.p;
  a.band_cap = SSE_COLLECT_CAP;
  a.bad = (int32_t *)(base + (size_t)Pmax * 24);
  a.err_flag = h->err_flag;
  a.counters = (unsigned long long *)h->s_ab_cnt.p;
  a.total = offsets + L;
  a.out_ids = nullptr;
  a.cap = 0;
  a.id_base = h->idx_base;
  a.N = h->idx_N;
  a.S = S;
  a.KG = KG;
  a.NT = (int)((h->idx_N + 31) / 32);
  a.eps32 = score_eps32(h);
  c.offsets = offsets;
  c.cursor = (unsigned long long *)h->s_ab.p;
  c.ovf = (int32_t *)((char *)h->s_ab.p + (size_t)L * 8);
  return 0;
}

static int score_above_count_locked(sse_handle *h, AboveCall &c, const float *q, int Q, const int32_t *pair_q, const double *pair_thr,
                                    int64_t L, int64_t *offsets, hipStream_t st) {
  if (score_above_setup(h, c, q, L, offsets, st)) return 1;
  int32_t *bad = const_cast<int32_t *>(c.a.bad);
  HIPCHECK(h, hipMemsetAsync(bad, 0, sizeof(int32_t), st));
  HIPCHECK(h, launch_above_validate(pair_q, L, Q, bad, h->err_flag, st));
  if (score_above_chunks(h, c, pair_q, pair_thr, L, 0, st)) return 1;
  HIPCHECK(h, launch_above_scan(offsets, L, bad, st));
  return 0;
}

// second half: the lists, queued behind the count; every kernel leaves when the total on the device exceeds cap
static int score_above_emit_locked(sse_handle *h, AboveCall &c, const int32_t *pair_q, const double *pair_thr, int64_t L, int64_t cap,
                                   int64_t *ids, double *scores, hipStream_t st) {
  if (cap <= 0) return 0;  // (only an empty total fits: nothing to write)
  const bool long_runs = std::min<int64_t>(cap, h->idx_N) > SSE_ABOVE_SORT_CAP;
  if (long_runs && reserve(h, h->s_ab_sort, (size_t)cap * 16)) return 1;
  HIPCHECK(h, hipMemsetAsync(c.cursor, 0, (size_t)L * sizeof(unsigned long long), st));
  c.a.out_ids = ids;
  c.a.cap = cap;
  if (score_above_chunks(h, c, pair_q, pair_thr, L, 1, st)) return 1;
  AboveListArgs l;
  l.q = c.a.q;
  l.pair_q = pair_q;
  l.idxp = h->idxp;
  l.idx64 = h->idx64;
  l.offsets = c.offsets;
  l.cursor = c.cursor;
  l.ids = ids;
  l.scores = scores;
  l.scratch_ids = long_runs ? (int64_t *)h->s_ab_sort.p : nullptr;
  l.scratch_scores = long_runs ? (double *)((char *)h->s_ab_sort.p + (size_t)cap * 8) : nullptr;
  l.bad = c.a.bad;
  l.err_flag = h->err_flag;
  l.counters = c.a.counters;
  l.L = L;
  l.cap = cap;
  l.id_base = h->idx_base;
  l.N = h->idx_N;
  l.S = c.a.S;
  l.KG = c.a.KG;
  HIPCHECK(h, launch_above_lists(l, st));
  return 0;
}

// sse_index_set_tags*: the words copied behind the index (device to device on `st`, or from the host), zero padded to whole
// tiles, and the per-tile OR.  Nothing changes before every check and allocation has passed.
static int index_set_tags_locked(sse_handle *h, const uint64_t *tags, int64_t N, bool from_host, hipStream_t st) {
  if (!tags) {
    h->tags_set = false;
    return 0;
  }
  if (!h->idxp) return fail(h, "sse_index_set_tags: no index uploaded");
  if (N != h->idx_N) return fail(h, "sse_index_set_tags: %lld tags for an index of %lld rows; the tags are unchanged", (long long)N, (long long)h->idx_N);
  const int64_t NT = (N + 31) / 32;
  if (!h->tags_set) {  // (live tags are never reallocated: the sizes are the index's)
    if (reserve(h, h->idx_tags, (size_t)NT * 32 * sizeof(uint64_t))) return 1;
    if (reserve(h, h->idx_tag_sum, (size_t)NT * sizeof(uint64_t))) return 1;
  }
  uint64_t *d = (uint64_t *)h->idx_tags.p;
  if (NT * 32 > N) HIPCHECK(h, hipMemsetAsync(d + N, 0, (size_t)(NT * 32 - N) * sizeof(uint64_t), st));
  if (from_host) HIPCHECK(h, hipMemcpy(d, tags, (size_t)N * sizeof(uint64_t), hipMemcpyHostToDevice));
  else HIPCHECK(h, hipMemcpyAsync(d, tags, (size_t)N * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  HIPCHECK(h, launch_tag_tile_summary(d, NT, (uint64_t *)h->idx_tag_sum.p, st));
  h->tags_set = true;
  return 0;
}

// The three top-k calls that sweep the index with the filtered call's machinery: the name their messages carry, the largest k,
// whether they need group keys
struct TopkCall {
  const char *name;
  int max_k;
  bool grouped;
};
static const TopkCall CALL_FILTERED = {"sse_score_topk_filtered", SSE_FILTERED_MAX_K, false};
static const TopkCall CALL_GROUPED = {"sse_score_topk_grouped", SSE_GROUPED_MAX_K, true};
static const TopkCall CALL_AFTER = {"sse_score_topk_after", SSE_AFTER_MAX_K, false};

// what a call reads and writes per query (device pointers), beyond what only one of the three takes
struct TopkIo {
  const float *q;
  const uint64_t *q_any, *q_none;
  double *out_s;
  int64_t *out_i;
  int32_t *out_c;
};

// argument errors of the three calls, all decidable on the host.  excl / n_excl: the filtered call's; after_score / after_id:
// the after call's cursor.
static int score_topk_check(sse_handle *h, const TopkCall &c, int Q, int k, const void *q_any, const void *q_none, const void *excl = nullptr,
                            int n_excl = 0, const void *after_score = nullptr, const void *after_id = nullptr) {
  if (!h->idxp) return fail(h, "%s: no index uploaded", c.name);
  if (c.grouped && !h->groups_set) return fail(h, "%s: the index has no group keys (sse_index_set_groups)", c.name);
  if (Q < 0) return fail(h, "bad arguments to %s", c.name);
  if (k < 1 || k > c.max_k) return fail(h, "%s: k = %d is not in [1, %d]", c.name, k, c.max_k);
  if (n_excl < 0 || n_excl > SSE_FILTERED_MAX_EXCL) return fail(h, "%s: n_excl = %d is not in [0, %d]", c.name, n_excl, SSE_FILTERED_MAX_EXCL);
  if (n_excl > 0 && !excl) return fail(h, "%s: n_excl = %d without excl_ids", c.name, n_excl);
  if ((after_score == nullptr) != (after_id == nullptr))
    return fail(h, "%s: after_score and after_id are both given or both NULL (%s is missing)", c.name, after_score ? "after_id" : "after_score");
  if ((q_any || q_none) && !h->tags_set) return fail(h, "%s: tag masks given but the index has no tags (sse_index_set_tags)", c.name);
  return 0;
}

// the fields of FilteredArgs that the three calls fill alike, for every chunk of a call
static void fill_filtered_common(sse_handle *h, FilteredArgs &a, int k, int n_excl, const DevBuf &counters) {
  a.idxp = h->idxp;
  a.idx64 = h->idx64;
  a.tags = h->tags_set ? (const uint64_t *)h->idx_tags.p : nullptr;
  a.tile_sum = h->tags_set ? (const uint64_t *)h->idx_tag_sum.p : nullptr;
  a.col_cap = SSE_COLLECT_CAP;
  a.counters = (unsigned long long *)counters.p;
  a.id_base = h->idx_base;
  a.N = h->idx_N;
  a.S = h->idx_S;
  a.KG = (h->idx_S + 7) / 8;
  a.NT = (int)((h->idx_N + 31) / 32);
  a.k = k;
  a.n_excl = n_excl;
  a.skip = h->score_filtered_skip ? 1 : 0;
  a.eps32 = score_eps32(h);
}

// queries per chunk of the three calls
static const int TOPK_POOL = 4096;

// nsplit doubled until a query gets at least `need` maxima (256 per split) where every wave of a split still has a tile of its own
static int split_for_maxima(int nsplit, int need, int64_t NT) {
  while (nsplit < 128 && nsplit * 256 < need && NT / (nsplit * 2) >= 8) nsplit *= 2;
  return nsplit;
}

// One chunk, P queries from q0, of any of the three calls: reserves the chunk scratch -- the maxima (in `maxima`, max_bytes:
// each call's own shape), then the rank count's thresholds and row buffers [P][SSE_COLLECT_CAP] (DESIGN K6e), then `extra` --
// clears the maxima and the row counts on `st`, and points `a` at the chunk's queries, scratch and outputs.
static int topk_chunk(sse_handle *h, FilteredArgs &a, const TopkIo &io, int q0, int P, int NQ, int nsplit, DevBuf &maxima, size_t max_bytes,
                      hipStream_t st, DevBuf *extra = nullptr, size_t extra_bytes = 0) {
  if (reserve(h, maxima, max_bytes)) return 1;
  if (reserve(h, h->s_cthr, (size_t)P * sizeof(float))) return 1;
  if (reserve(h, h->s_ccnt, (size_t)(P + 1) * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_cbuf, (size_t)P * SSE_COLLECT_CAP * sizeof(int32_t))) return 1;
  if (extra && reserve(h, *extra, extra_bytes)) return 1;
  HIPCHECK(h, hipMemsetAsync(maxima.p, 0, max_bytes, st));
  HIPCHECK(h, hipMemsetAsync(h->s_ccnt.p, 0, (size_t)P * sizeof(int32_t), st));
  a.q = io.q + (size_t)q0 * h->idx_S;
  a.q_any = io.q_any ? io.q_any + q0 : nullptr;
  a.q_none = io.q_none ? io.q_none + q0 : nullptr;
  a.thr = (float *)h->s_cthr.p;
  a.col_cnt = (int32_t *)h->s_ccnt.p;
  a.col_buf = (int32_t *)h->s_cbuf.p;
  a.out_scores = io.out_s + (size_t)q0 * a.k;
  a.out_ids = io.out_i + (size_t)q0 * a.k;
  a.out_counts = io.out_c + q0;
  a.P = P;
  a.NQ = NQ;
  a.NSPLIT = nsplit;
  a.NV = std::min(nsplit, 16) * 256;
  return 0;
}

// sse_score_topk_filtered*: every stage queued on `st` (device pointers throughout), queries in chunks of 4096; maxima [P][NV]
static int score_filtered_dev_locked(sse_handle *h, const TopkIo &io, int Q, int k, const int64_t *excl, int n_excl, hipStream_t st) {
  const int64_t NT = (h->idx_N + 31) / 32;
  if (ensure_zeroed_once(h, h->s_ft_cnt, h->ft_cnt_init, 3, st)) return 1;
  FilteredArgs a;
  fill_filtered_common(h, a, k, excl ? n_excl : 0, h->s_ft_cnt);
  for (int q0 = 0; q0 < Q; q0 += TOPK_POOL) {
    const int P = std::min(TOPK_POOL, Q - q0);
    SweepChunk ck;
    if (sweep_chunk(h, P, ck)) return 1;
    const int nsplit = split_for_maxima(ck.nsplit, 2 * (k + a.n_excl), NT);
    if (topk_chunk(h, a, io, q0, P, ck.NQ, nsplit, h->s_ft_max, (size_t)P * std::min(nsplit, 16) * 256 * sizeof(uint32_t), st)) return 1;
    a.excl = excl ? excl + (size_t)q0 * n_excl : nullptr;
    a.maxima = (uint32_t *)h->s_ft_max.p;
    HIPCHECK(h, launch_score_filtered(a, st));
  }
  return 0;
}

// sse_score_topk_after*: the filtered call's chunks with the cursor brackets beside them (DESIGN K6j): [P] e as double, [P] lo, [P] hi
static int score_after_dev_locked(sse_handle *h, const TopkIo &io, int Q, int k, const double *after_s, const int64_t *after_i, hipStream_t st) {
  const int64_t NT = (h->idx_N + 31) / 32;
  if (ensure_zeroed_once(h, h->s_af_cnt, h->af_cnt_init, 3, st)) return 1;
  AfterArgs g;
  FilteredArgs &a = g.f;
  fill_filtered_common(h, a, k, 0, h->s_af_cnt);
  a.excl = nullptr;
  for (int q0 = 0; q0 < Q; q0 += TOPK_POOL) {
    const int P = std::min(TOPK_POOL, Q - q0);
    SweepChunk ck;
    if (sweep_chunk(h, P, ck)) return 1;
    const int nsplit = split_for_maxima(ck.nsplit, 2 * k, NT);
    if (topk_chunk(h, a, io, q0, P, ck.NQ, nsplit, h->s_ft_max, (size_t)P * std::min(nsplit, 16) * 256 * sizeof(uint32_t), st, &h->s_af_bnd,
                   (size_t)P * (sizeof(double) + 2 * sizeof(float))))
      return 1;
    a.maxima = (uint32_t *)h->s_ft_max.p;
    g.after_score = after_s ? after_s + q0 : nullptr;
    g.after_id = after_i ? after_i + q0 : nullptr;
    g.eb = (double *)h->s_af_bnd.p;
    g.lo = (float *)(g.eb + P);
    g.hi = g.lo + P;
    HIPCHECK(h, launch_score_after(g, st));
  }
  return 0;
}

static const TopkCall CALL_BIASED = {"sse_score_topk_biased", SSE_BIASED_MAX_K, false};

// sse_index_set_bias*: the floats copied behind the index (device to device on `st`, or from the host after one pass that
// refuses a non-finite value), zero padded to whole tiles, and max |bias| formed on the device beside them.  Nothing changes
// before every check and allocation has passed.
static int index_set_bias_locked(sse_handle *h, const float *bias, int64_t N, bool from_host, hipStream_t st) {
  if (!bias) {
    h->bias_set = false;
    return 0;
  }
  if (!h->idxp) return fail(h, "sse_index_set_bias: no index uploaded");
  if (N != h->idx_N) return fail(h, "sse_index_set_bias: %lld values for an index of %lld rows; the bias is unchanged", (long long)N, (long long)h->idx_N);
  if (from_host)
    for (int64_t i = 0; i < N; ++i)
      if (!std::isfinite(bias[i])) return fail(h, "sse_index_set_bias: bias[%lld] = %g is not finite; the bias is unchanged", (long long)i, (double)bias[i]);
  const int64_t NT = (N + 31) / 32;
  if (!h->bias_set) {  // (a live bias is never reallocated: the sizes are the index's)
    if (reserve(h, h->idx_bias, (size_t)NT * 32 * sizeof(float))) return 1;
    if (reserve(h, h->idx_bias_absmax, sizeof(float))) return 1;
  }
  float *d = (float *)h->idx_bias.p;
  if (from_host) HIPCHECK(h, hipMemcpy(d, bias, (size_t)N * sizeof(float), hipMemcpyHostToDevice));
  else HIPCHECK(h, hipMemcpyAsync(d, bias, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIPCHECK(h, hipMemsetAsync(h->idx_bias_absmax.p, 0, sizeof(float), st));
  HIPCHECK(h, launch_bias_prepare(d, N, NT, (float *)h->idx_bias_absmax.p, st));
  h->bias_set = true;
  return 0;
}

// sse_score_topk_biased*: the filtered call's chunks with e_b beside them (DESIGN K6l): [P] double
static int score_biased_dev_locked(sse_handle *h, const TopkIo &io, int Q, int k, const float *weight, hipStream_t st) {
  const int64_t NT = (h->idx_N + 31) / 32;
  if (ensure_zeroed_once(h, h->s_bs_cnt, h->bs_cnt_init, 3, st)) return 1;
  BiasedArgs g;
  FilteredArgs &a = g.f;
  fill_filtered_common(h, a, k, 0, h->s_bs_cnt);
  a.excl = nullptr;
  g.bias = (const float *)h->idx_bias.p;
  g.bias_absmax = (const float *)h->idx_bias_absmax.p;
  g.norm_max = h->idx_norm_max;
  for (int q0 = 0; q0 < Q; q0 += TOPK_POOL) {
    const int P = std::min(TOPK_POOL, Q - q0);
    SweepChunk ck;
    if (sweep_chunk(h, P, ck)) return 1;
    const int nsplit = split_for_maxima(ck.nsplit, 2 * k, NT);
    if (topk_chunk(h, a, io, q0, P, ck.NQ, nsplit, h->s_ft_max, (size_t)P * std::min(nsplit, 16) * 256 * sizeof(uint32_t), st, &h->s_bs_bnd,
                   (size_t)P * sizeof(double)))
      return 1;
    a.maxima = (uint32_t *)h->s_ft_max.p;
    g.weight = weight ? weight + q0 : nullptr;
    g.eb = (double *)h->s_bs_bnd.p;
    HIPCHECK(h, launch_score_biased(g, st));
  }
  return 0;
}

// argument errors of sse_score_topk_biased*, all decidable on the host
static int score_biased_check(sse_handle *h, int Q, int k, const void *q_any, const void *q_none) {
  if (!h->idxp) return fail(h, "%s: no index uploaded", CALL_BIASED.name);
  if (!h->bias_set) return fail(h, "%s: the index has no bias (sse_index_set_bias)", CALL_BIASED.name);
  return score_topk_check(h, CALL_BIASED, Q, k, q_any, q_none);
}

// sse_score_lse*: one sweep and one merge per chunk of 4096 queries, queued on `st` (device pointers throughout); the partials
// [P][nsplit * 16] are the only scratch
static int score_lse_dev_locked(sse_handle *h, const float *q, int Q, float scale, const float *weight, const uint64_t *q_any,
                                const uint64_t *q_none, double *out_lse, int64_t *out_count, double *out_bound, hipStream_t st) {
  if (ensure_zeroed_once(h, h->s_lse_cnt, h->lse_cnt_init, 1, st)) return 1;
  LseArgs g{};  // (of FilteredArgs the sweep reads what fill_filtered_common and the chunk loop set; the rest stays null)
  FilteredArgs &a = g.f;
  fill_filtered_common(h, a, 0, 0, h->s_lse_cnt);
  g.bias = weight ? (const float *)h->idx_bias.p : nullptr;
  g.bias_absmax = weight ? (const float *)h->idx_bias_absmax.p : nullptr;
  g.norm_max = h->idx_norm_max;
  const double c = (double)scale * 1.4426950408889634;
  g.scale = scale;
  g.c_hi = (float)c;
  g.c_lo = (float)(c - (double)g.c_hi);
  for (int q0 = 0; q0 < Q; q0 += TOPK_POOL) {
    const int P = std::min(TOPK_POOL, Q - q0);
    SweepChunk ck;
    if (sweep_chunk(h, P, ck)) return 1;
    if (reserve(h, h->s_lse_part, score_lse_part_bytes(P, ck.nsplit))) return 1;
    a.q = q + (size_t)q0 * h->idx_S;
    a.q_any = q_any ? q_any + q0 : nullptr;
    a.q_none = q_none ? q_none + q0 : nullptr;
    a.P = P;
    a.NQ = ck.NQ;
    a.NSPLIT = ck.nsplit;
    g.weight = weight ? weight + q0 : nullptr;
    g.part = (LsePartial *)h->s_lse_part.p;
    g.out_lse = out_lse + q0;
    g.out_count = out_count + q0;
    g.out_bound = out_bound ? out_bound + q0 : nullptr;
    HIPCHECK(h, launch_score_lse(g, st));
  }
  h->score_lse_calls += 1;
  return 0;
}

// argument errors of sse_score_lse*, all decidable on the host
static int score_lse_check(sse_handle *h, int Q, float scale, const void *weight, const void *q_any, const void *q_none) {
  if (!h->idxp) return fail(h, "sse_score_lse: no index uploaded");
  if (Q < 0) return fail(h, "bad arguments to sse_score_lse");
  if (!(scale > 0.0f && scale <= 256.0f)) return fail(h, "sse_score_lse: scale = %g is not in (0, 256]", (double)scale);
  if (weight && !h->bias_set) return fail(h, "sse_score_lse: q_weight given but the index has no bias (sse_index_set_bias)");
  if ((q_any || q_none) && !h->tags_set) return fail(h, "sse_score_lse: tag masks given but the index has no tags (sse_index_set_tags)");
  return 0;
}

static const TopkCall CALL_CONFUSIONS = {"sse_score_confusions", SSE_CONFUSIONS_MAX_K, false};

// argument errors of sse_score_confusions*, all decidable on the host
static int score_confusions_check(sse_handle *h, int Q, int k, const void *pos_ids, int n_pos, double margin) {
  if (score_topk_check(h, CALL_CONFUSIONS, Q, k, nullptr, nullptr)) return 1;
  if (n_pos < 1 || n_pos > SSE_CONFUSIONS_MAX_POS)
    return fail(h, "%s: n_pos = %d is not in [1, %d]", CALL_CONFUSIONS.name, n_pos, SSE_CONFUSIONS_MAX_POS);
  if (!(margin > -INFINITY)) return fail(h, "%s: margin = %g is neither finite nor +inf", CALL_CONFUSIONS.name, margin);
  if (!pos_ids) return fail(h, "%s: pos_ids is NULL", CALL_CONFUSIONS.name);
  return 0;
}

// sse_score_confusions*: the filtered call's chunks, run without tags, with the floors beside them (DESIGN K6k): [P] f as
// double, [P] flo.  The positives take the place of the exclusion list.
static int score_confusions_dev_locked(sse_handle *h, const TopkIo &io, int Q, int k, const int64_t *pos, int n_pos, double margin,
                                       double *out_ps, int64_t *out_pi, hipStream_t st) {
  const int64_t NT = (h->idx_N + 31) / 32;
  if (ensure_zeroed_once(h, h->s_cf_cnt, h->cf_cnt_init, 3, st)) return 1;
  ConfusionArgs g;
  FilteredArgs &a = g.f;
  fill_filtered_common(h, a, k, n_pos, h->s_cf_cnt);
  a.tags = a.tile_sum = nullptr;  // every row is tag-eligible
  a.skip = 0;
  g.margin = margin;
  for (int q0 = 0; q0 < Q; q0 += TOPK_POOL) {
    const int P = std::min(TOPK_POOL, Q - q0);
    SweepChunk ck;
    if (sweep_chunk(h, P, ck)) return 1;
    const int nsplit = split_for_maxima(ck.nsplit, 2 * (k + n_pos), NT);
    if (topk_chunk(h, a, io, q0, P, ck.NQ, nsplit, h->s_ft_max, (size_t)P * std::min(nsplit, 16) * 256 * sizeof(uint32_t), st, &h->s_cf_bnd,
                   (size_t)P * (sizeof(double) + sizeof(float))))
      return 1;
    a.excl = pos + (size_t)q0 * n_pos;
    a.maxima = (uint32_t *)h->s_ft_max.p;
    g.floor64 = (double *)h->s_cf_bnd.p;
    g.flo = (float *)(g.floor64 + P);
    g.out_pos_score = out_ps ? out_ps + q0 : nullptr;
    g.out_pos_id = out_pi ? out_pi + q0 : nullptr;
    HIPCHECK(h, launch_score_confusions(g, st));
  }
  return 0;
}

// sse_index_set_groups*: the keys copied behind the index (device to device on `st`, or from the host).  Nothing changes
// before every check and allocation has passed.
static int index_set_groups_locked(sse_handle *h, const int64_t *groups, int64_t N, bool from_host, hipStream_t st) {
  if (!groups) {
    h->groups_set = false;
    return 0;
  }
  if (!h->idxp) return fail(h, "sse_index_set_groups: no index uploaded");
  if (N != h->idx_N) return fail(h, "sse_index_set_groups: %lld keys for an index of %lld rows; the keys are unchanged", (long long)N, (long long)h->idx_N);
  if (!h->groups_set) {  // (live keys are never reallocated: the size is the index's)
    if (reserve(h, h->idx_groups, (size_t)N * sizeof(int64_t))) return 1;
  }
  if (from_host) HIPCHECK(h, hipMemcpy(h->idx_groups.p, groups, (size_t)N * sizeof(int64_t), hipMemcpyHostToDevice));
  else HIPCHECK(h, hipMemcpyAsync(h->idx_groups.p, groups, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  h->groups_set = true;
  return 0;
}

// sse_score_topk_grouped*: the filtered call's chunks with (key, row) maxima [P][NV] of its own (DESIGN K6h), found by a sweep
// of its own shape
static int score_grouped_dev_locked(sse_handle *h, const TopkIo &io, int Q, int k, int64_t *out_g, hipStream_t st) {
  const int64_t NT = (h->idx_N + 31) / 32;
  if (ensure_zeroed_once(h, h->s_gp_cnt, h->gp_cnt_init, 3, st)) return 1;
  GroupedArgs g;
  FilteredArgs &a = g.rest;
  fill_filtered_common(h, a, k, 0, h->s_gp_cnt);
  a.excl = nullptr;
  a.maxima = nullptr;
  g.groups = (const int64_t *)h->idx_groups.p;
  for (int q0 = 0; q0 < Q; q0 += TOPK_POOL) {
    const int P = std::min(TOPK_POOL, Q - q0);
    SweepChunk ck;
    if (sweep_chunk(h, P, ck)) return 1;
    // the eligible-max sweep: at most 2 query tiles per workgroup (the tile of every maximum costs 16 registers per query
    // tile) and at least 4 k maxima per query: the maxima of several row sets share groups, and theta needs k DISTINCT groups
    // among them (DESIGN K6h)
    const int NQM = std::min(ck.NQ, 2);
    const int msplit = split_for_maxima(choose_nsplit(NQM, (P + NQM * 32 - 1) / (NQM * 32), NT), 4 * k, NT);
    const int NV = std::min(msplit, 16) * 256;
    if (topk_chunk(h, a, io, q0, P, ck.NQ, ck.nsplit, h->s_gp_max, (size_t)P * NV * sizeof(unsigned long long), st)) return 1;
    g.max = a;
    g.max.NQ = NQM;
    g.max.NSPLIT = msplit;
    g.max.NV = NV;
    g.maxima64 = (unsigned long long *)h->s_gp_max.p;
    g.out_groups = out_g + (size_t)q0 * k;
    HIPCHECK(h, launch_score_grouped(g, st));
  }
  return 0;
}

// ---- sse_score_topk*: plan -> prepare -> route (DESIGN K6/K7) ----
// Paging: k > SSE_MAX_SELECT_K, exact float64 paging.  Select: 16 < k <= SSE_MAX_SELECT_K.  TwoPass: mid-size indexes under
// many queries.  Lists: everything else, in two stages (lists_first, lists_rest).  None: no queries.
enum class TopkRoute { None, Paging, Select, TwoPass, Lists };

// What one call does, decided once from (handle, Q, k) by topk_plan and const afterwards.  Paging and Select use the fields
// down to eps32 only (Select shapes its sweeps per pool of queries).
struct TopkPlan {
  TopkRoute route;
  int Q, k, S, KG, KG16, QT;
  int64_t NT;
  float eps32, eps_bf16, eps_split;  // score_eps32 / score_eps_bf16 / score_eps_split_bf16
  bool bf;           // bf16 candidate pass
  int NQ, QB;        // query tiles per workgroup, query blocks
  int nsplit;        // splits of the candidate sweep: 16 candidates each
  int nsplit2;       // splits of the bf16 route's fp32 second chance
  int two_pass_splits;
  bool small_idx, small_x3;  // the small-index scorer instead of the list sweep; on split-bf16 operands
  bool rows_direct;  // the sweeps build their query fragments from the rows themselves: no pack launch
  int NC, NCmax;     // candidates per query of the first stage; of the larger of the two sweeps
  int POOL;          // collect-buffer slots for uncertified queries (the rest: float64 brute force)
  bool own_slots;    // every query has a collect slot of its own: the re-scoring pass hands them out
  bool has_rest;     // a second stage exists: what the first one left uncertified is served by lists_rest
  float cand_eps() const { return small_x3 ? eps_split : bf ? eps_bf16 : eps32; }
};

static int topk_plan(sse_handle *h, int Q, int k, TopkPlan &p) {
  p = TopkPlan{};
  p.route = TopkRoute::None;
  if (!h->idxp) return fail(h, "no index uploaded");
  if (Q < 0) return fail(h, "bad Q");
  if (Q == 0) return 0;
  if (k < 1 || k > h->idx_N) return fail(h, "k=%d must be in [1, N=%lld]", k, (long long)h->idx_N);
  const int S = h->idx_S;
  p.Q = Q;
  p.k = k;
  p.S = S;
  p.KG = (S + 7) / 8;
  p.KG16 = (S + 15) / 16;
  p.QT = (Q + 31) / 32;
  p.NT = (h->idx_N + 31) / 32;
  p.eps32 = score_eps32(h);
  p.eps_bf16 = score_eps_bf16(h);
  p.eps_split = score_eps_split_bf16(h);
  if (k > 16) {
    p.route = k > SSE_MAX_SELECT_K ? TopkRoute::Paging : TopkRoute::Select;
    return 0;
  }
  // bf16 candidate pass (option score_bf16): 16x the matrix rate for the 128-query-block variant, half the index
  // bytes for the HBM-bound few-queries sweep
  // (small indexes stay on the fp32 pass: nothing to win, and no bf16 copy / second-chance launches to pay for)
  p.bf = h->score_bf16 && h->idx_N >= 8192;
  // <= 32 queries (demo / web): single query tile, HBM-bound sweep; else 128-query blocks while they fit LDS (index
  // dimension <= 296), 64-query blocks up to 616 (configs[4]: 512), 32-query blocks beyond.
  // The 16 lane lists of a workgroup are always merged in-kernel (a few tens of microseconds per workgroup): the
  // re-scoring pass ranks 16 candidates per split
  SweepChunk ck;
  if (sweep_chunk(h, Q, ck, p.bf)) return 1;
  p.NQ = ck.NQ;
  p.QB = ck.QB;
  p.nsplit = ck.nsplit;
  // Mid-size indexes under many queries: the two-pass route.  (A host call of few queries, the only kind with a mirror,
  // never comes here: a mirror needs Q <= 64, this route Q >= 1024.)
  if (p.bf && p.NQ == 4 && Q >= 1024 && h->idx_N >= h->score_two_pass_min_rows && h->idx_N <= h->score_two_pass_rows) {
    p.route = TopkRoute::TwoPass;
    p.two_pass_splits = choose_two_pass_splits(h, p.QB, p.NT, p.nsplit);
    return 0;
  }
  p.route = TopkRoute::Lists;
  p.has_rest = true;
  // the fp32 second chance of the bf16 pass sweeps for a dense set of FEW queries (typically a handful of query blocks): it
  // takes its parallelism from the index instead -- up to 128 splits -- or three workgroups would walk 1.25 M rows alone
  // (up to 128 since round 6: with 32, the 30 uncertified of 16384 random queries against 1.25 M rows -- one query block -- kept 32
  // workgroups busy for 4 ms on an otherwise idle chip: 13.5 ms per pass, 9.75 with 128; env: measurement aid)
  static const int split2_max = getenv("SSE_SPLIT2_MAX") ? atoi(getenv("SSE_SPLIT2_MAX")) : 128;
  p.nsplit2 = p.nsplit;
  while (p.nsplit2 < split2_max && p.NT / (p.nsplit2 * 2 * 2) >= 16) p.nsplit2 *= 2;
  // many queries against a small index (the evaluator's 16384 x 571): one launch forms all N scores per query and selects the
  // 16 best exactly (launch_score_small_index) instead of the list sweep
  p.small_idx = h->score_small_index && !p.bf && score_small_index_applies(Q, p.KG, p.NT);
  p.small_x3 = p.small_idx && h->score_small_x3 && h->idx_x3_valid;
  p.rows_direct = p.NQ == 1;  // <= 32 queries (the latency path)
  p.NC = p.small_idx ? 16 : p.nsplit * 16;
  p.NCmax = std::max(p.nsplit, p.nsplit2) * 16;
  p.POOL = std::min(Q, 1024);
  p.own_slots = Q <= p.POOL;
  return 0;
}

// what every route but Paging needs before its first launch: the bf16 image of the index, built when the first bf16 call asks
// for it, and the device counters
static int topk_prepare(sse_handle *h, const TopkPlan &p, hipStream_t st) {
  if (p.bf && !h->idxp16_valid) {
    const size_t need = (size_t)p.NT * p.KG16 * 1024;
    if (need > h->idxp16_cap) {
      if (h->idxp16) HIPCHECK(h, hipFree(h->idxp16));
      h->idxp16 = nullptr;
      h->idxp16_cap = 0;
      HIPCHECK(h, hipMalloc(&h->idxp16, need));
      h->idxp16_cap = need;
    }
    HIPCHECK(h, launch_frag32_to_bf16(h->idxp, p.NT, p.KG, h->idxp16, st));
    h->idxp16_valid = true;
  }
  return ensure_counters(h, st);
}

static unsigned long long *topk_counters(const sse_handle *h) { return (unsigned long long *)h->s_fb_cnt.p; }

// the caller's side of a call: query rows [Q][S] and results [Q][k], all on the device
struct TopkBufs {
  const float *q;
  double *out_s;
  int64_t *out_i;
};

// The fields every sweep of this driver shares: Q queries in blocks of NQ tiles against the fp32 or the bf16 image of the
// index in nsplit splits, fragments from s_qp, candidate lists in s_ps / s_pi / s_pb.
static ScoreArgs sweep_args(const sse_handle *h, bool bf, int Q, int NQ, int nsplit) {
  ScoreArgs a;
  a.BF = bf ? 1 : 0;
  a.idxp = bf ? (const float *)h->idxp16 : h->idxp;
  a.qp = (const float *)h->s_qp.p;
  a.part_scores = (float *)h->s_ps.p;
  a.part_ids = (int32_t *)h->s_pi.p;
  a.part_bnd = (float *)h->s_pb.p;
  a.N = h->idx_N;
  a.Q = Q;
  a.KG = bf ? (h->idx_S + 15) / 16 : (h->idx_S + 7) / 8;
  a.NT = (int)((h->idx_N + 31) / 32);
  a.QT = (Q + 31) / 32;
  a.NSPLIT = nsplit;
  a.KC = 16;
  a.NQ = NQ;
  return a;
}

// What the collect tails of the three routes differ in (besides the sweep they start from)
struct CollectTail {
  int cap;                              // rows one query may collect: SSE_COLLECT_CAP, or the two-pass route's MID_CAP
  unsigned long long *served, *brute;   // counter words of the select and of the float64 brute force (null: not counted)
  const int32_t *uncert;                // RescoreArgs::uncert of the call or null: the launches are sized for all queries
  int follow_grid;
};
// The end of every route: `c` as a collect sweep of every row at or above a query's threshold (s_cthr) into its slot (s_cslot,
// s_ccnt, s_cbuf), the float64 select of those rows, and the float64 brute force for whatever overflowed its buffer, saw fewer
// than k rows or had no slot (pages of 16).  The caller has reserved and cleared the buffers and s_cert.
static int collect_tail(sse_handle *h, ScoreArgs c, const TopkBufs &io, int k, const CollectTail &t, hipStream_t st) {
  const int S = h->idx_S;
  int32_t *cert = (int32_t *)h->s_cert.p;
  c.COLLECT = 1;
  c.col_thr = (const float *)h->s_cthr.p;
  c.col_slot = (const int32_t *)h->s_cslot.p;
  c.col_cnt = (int32_t *)h->s_ccnt.p;
  c.col_buf = (int32_t *)h->s_cbuf.p;
  c.col_cap = t.cap;
  c.uncert = t.uncert;
  HIPCHECK(h, launch_score_topk(c, st));
  SelectArgs sel{io.q, h->idxp, h->idx64, c.col_slot, c.col_cnt, c.col_buf, t.cap, io.out_s, io.out_i, cert, h->idx_base, c.Q, S, k,
                 t.served, t.uncert, t.follow_grid};
  HIPCHECK(h, launch_select_topk(sel, st));
  HIPCHECK(h, launch_exact_topk(io.q, h->idxp, h->idx64, cert, io.out_s, io.out_i, h->idx_base, h->idx_N, c.Q, S, k, st, t.brute,
                                t.uncert, t.follow_grid));
  return 0;
}

// k > SSE_MAX_SELECT_K, beyond the collect path's buffers: exact float64 paging (correct for any k <= N, one workgroup per query)
static int topk_paging(sse_handle *h, const TopkPlan &p, const TopkBufs &io, hipStream_t st) {
  HIPCHECK(h, launch_exact_topk(io.q, h->idxp, h->idx64, nullptr, io.out_s, io.out_i, h->idx_base, h->idx_N, p.Q, p.S, p.k, st));
  return 0;
}

// 16 < k <= SSE_MAX_SELECT_K (sse_demo.py:128-134 and webserver.py take a user-chosen nbest): candidate sweep with enough
// per-split lists that the k-th best candidate is a tight lower bound of the k-th best row, then a collect sweep of every row
// that can still be in the exact top-k and a float64 sort of those -- two grid-wide sweeps instead of the
// one-workgroup-per-query float64 brute force (which stays as the fallback: more than SSE_COLLECT_CAP rows within the bound of
// the k-th score).  Pools of 2048 queries, each a sweep shape of its own.
static int topk_select(sse_handle *h, const TopkPlan &p, const TopkBufs &io, hipStream_t st) {
  const int POOL = 2048, k = p.k;
  unsigned long long *counters = topk_counters(h);
  for (int q0 = 0; q0 < p.Q; q0 += POOL) {
    const int Qc = std::min(POOL, p.Q - q0);
    const TopkBufs ioc{io.q + (size_t)q0 * p.S, io.out_s + (size_t)q0 * k, io.out_i + (size_t)q0 * k};
    SweepChunk ck;
    if (sweep_chunk(h, Qc, ck)) return 1;
    int nsplit = ck.nsplit;
    // at least 4k candidates (k-th candidate close to the k-th row), at most RS_MAXNC = 4096, >= 2 tiles per split
    const int max_split = (ck.NQ == 1) ? 256 : 128;
    while (nsplit < max_split && nsplit * 16 < 4 * k && p.NT / (nsplit * 2) >= 2) nsplit *= 2;
    const int NC = nsplit * 16;
    if (reserve(h, h->s_qp, (size_t)ck.QB * ck.NQ * p.KG * 256 * sizeof(float))) return 1;
    if (reserve(h, h->s_ps, (size_t)Qc * NC * sizeof(float))) return 1;
    if (reserve(h, h->s_pi, (size_t)Qc * NC * sizeof(int32_t))) return 1;
    if (reserve(h, h->s_pb, (size_t)Qc * nsplit * sizeof(float))) return 1;
    if (reserve(h, h->s_cert, (size_t)Qc * sizeof(int32_t))) return 1;
    if (reserve_collect(h, Qc, Qc)) return 1;
    HIPCHECK(h, launch_pack_rows(ioc.q, Qc, p.S, (float *)h->s_qp.p, st));
    const ScoreArgs a = sweep_args(h, false, Qc, ck.NQ, nsplit);
    HIPCHECK(h, launch_score_topk(a, st));
    HIPCHECK(h, launch_kth_bound(ioc.q, a.part_scores, a.part_ids, Qc, p.S, NC, k, p.eps32, (float *)h->s_cthr.p,
                                 (int32_t *)h->s_cslot.p, st));
    HIPCHECK(h, hipMemsetAsync(h->s_ccnt.p, 0, (size_t)(Qc + 1) * sizeof(int32_t), st));
    HIPCHECK(h, hipMemsetAsync(h->s_cert.p, 0, (size_t)Qc * sizeof(int32_t), st));
    if (collect_tail(h, a, ioc, k, {SSE_COLLECT_CAP, counters + 1, counters + 2, nullptr, 0}, st)) return 1;
  }
  return 0;
}

// Mid-size indexes under many queries: max-only sweep -> per-query threshold -> collect sweep -> float64 select (see
// lane_max_threshold_kernel in score_topk.hip for the argument), all on the bf16 image.  Everything is final after it: no
// certificates to follow up.
static int topk_two_pass(sse_handle *h, const TopkPlan &p, const TopkBufs &io, hipStream_t st) {
  constexpr int MID_CAP = 512;  // rows one query may collect (typically 20 - 30); more: float64 brute force for that query
  const int Q = p.Q, ns2 = p.two_pass_splits;
  h->two_pass_calls += 1;
  if (reserve(h, h->s_qp, (size_t)p.QB * p.NQ * p.KG * 256 * sizeof(float))) return 1;
  if (reserve(h, h->s_lmax, (size_t)Q * ns2 * 16 * sizeof(float))) return 1;
  if (reserve(h, h->s_cert, (size_t)Q * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_cthr, (size_t)Q * sizeof(float)) || reserve(h, h->s_cslot, (size_t)Q * sizeof(int32_t)) ||
      reserve(h, h->s_ccnt, (size_t)(Q + 1) * sizeof(int32_t)) || reserve(h, h->s_cbuf, (size_t)Q * MID_CAP * sizeof(int32_t)))
    return 1;
  HIPCHECK(h, launch_pack_rows_bf16(io.q, Q, p.S, h->s_qp.p, st));
  HIPCHECK(h, hipMemsetAsync(h->s_ccnt.p, 0, (size_t)(Q + 1) * sizeof(int32_t), st));
  HIPCHECK(h, hipMemsetAsync(h->s_cert.p, 0, (size_t)Q * sizeof(int32_t), st));
  const ScoreArgs sweep = sweep_args(h, true, Q, p.NQ, ns2);
  ScoreArgs m1 = sweep;
  m1.COLLECT = 1;
  m1.lane_max = (float *)h->s_lmax.p;
  HIPCHECK(h, launch_score_topk(m1, st));
  HIPCHECK(h, launch_lane_max_threshold(io.q, m1.lane_max, Q, p.S, ns2 * 16, p.eps_bf16, (float *)h->s_cthr.p, (int32_t *)h->s_cslot.p, st));
  // (the select does not count: a query it cannot serve -- buffer overflowed, fewer than k rows -- goes to the brute force)
  return collect_tail(h, sweep, io, p.k, {MID_CAP, nullptr, topk_counters(h) + 2, nullptr, 0}, st);
}

// Host mirror of the first stage of a call of few queries (see RescoreArgs): pinned, device-visible host pointers the
// re-scoring pass stores results, certificates, the error flag of the encoder in front of it and -- last, released at system
// scope -- one completion word per query through.  The host polls the words: no read-back copies, no stream synchronisation.
struct ScoreMirror {
  double *scores;
  int64_t *ids;
  int32_t *cert, *err, *flag;
  int32_t seq;
};

// The word the follow-up launches of the Lists route read first (RescoreArgs::uncert): they are queued unconditionally by
// the all-queued form, and the word lets their workgroups leave at once (and their grids stay small) when the re-scoring pass
// certified every query -- the usual call.  Two words, used in turn (lists_first flips): a call's re-scoring pass zeroes the one
// the next call will count in.
static int32_t *lists_uncert(const sse_handle *h, int other = 0) { return (int32_t *)(topk_counters(h) + 4) + (h->uncert_word ^ other); }
static int follow_grid(const sse_handle *h) { return 2 * (h->cu_count > 0 ? h->cu_count : 256); }

// the candidate sweep of the Lists route
static ScoreArgs lists_sweep_args(const sse_handle *h, const TopkPlan &p, const float *q) {
  ScoreArgs a = sweep_args(h, p.bf, p.Q, p.NQ, p.nsplit);
  if (p.rows_direct) {
    a.q_rows = q;
    a.S = p.S;
  }
  return a;
}

// the float64 re-scoring of the first stage's candidates, as both stages of the Lists route see it
static RescoreArgs lists_rescore_args(const sse_handle *h, const TopkPlan &p, const TopkBufs &io) {
  RescoreArgs r;
  r.q = io.q;
  r.idx32 = h->idxp;
  r.idx64 = h->idx64;
  r.idx_rm = h->idx_rm_valid ? (const float *)h->idx_rm.p : nullptr;
  r.part_scores = (const float *)h->s_ps.p;
  r.part_ids = (const int32_t *)h->s_pi.p;
  r.part_bnd = (const float *)h->s_pb.p;
  r.out_scores = io.out_s;
  r.out_ids = io.out_i;
  r.cert = (int32_t *)h->s_cert.p;
  r.id_base = h->idx_base;
  r.N = h->idx_N;
  r.Q = p.Q;
  r.S = p.S;
  r.NC = p.NC;
  r.k = p.k;
  r.eps = p.cand_eps();
  r.eps32 = p.eps32;
  r.col_thr = (float *)h->s_cthr.p;
  r.uncert = lists_uncert(h);
  r.uncert_clear = lists_uncert(h, 1);
  // every query has a collect slot of its own (the usual call): the re-scoring pass hands them out (slot = query for an
  // uncertified one) and zeroes their counters -- no memset / launch_assign_slots between the passes
  if (p.own_slots) {
    r.col_slot = (int32_t *)h->s_cslot.p;
    r.col_cnt = (int32_t *)h->s_ccnt.p;
  }
  return r;
}

// Lists route, first stage: candidate sweep (or the small-index scorer) + float64 re-scoring.  Results and certificates are
// final for every certified query.  mirror (host form of few queries, else null): the re-scoring pass reports through it.
static int lists_first(sse_handle *h, const TopkPlan &p, const TopkBufs &io, const ScoreMirror *mirror, hipStream_t st) {
  const int Q = p.Q;
  if (reserve(h, h->s_qp, (size_t)p.QB * p.NQ * p.KG * 256 * sizeof(float))) return 1;
  if (reserve(h, h->s_ps, (size_t)Q * (p.bf ? p.NCmax : p.NC) * sizeof(float))) return 1;
  if (reserve(h, h->s_pi, (size_t)Q * (p.bf ? p.NCmax : p.NC) * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_pb, (size_t)Q * (p.bf ? p.NCmax / 16 : p.nsplit) * sizeof(float))) return 1;
  if (reserve(h, h->s_cert, (size_t)Q * sizeof(int32_t))) return 1;
  if (reserve_collect(h, Q, p.POOL)) return 1;
  if (p.small_idx) {
    SmallIndexArgs si{io.q, h->idxp, (float *)h->s_ps.p, (int32_t *)h->s_pi.p, (float *)h->s_pb.p, h->idx_N, Q, p.S, p.KG, (int)p.NT};
    if (p.small_x3) si.idx_x3 = h->idx_x3.p;
    HIPCHECK(h, launch_score_small_index(si, st));
  } else {
    if (!p.rows_direct) {
      if (p.bf) HIPCHECK(h, launch_pack_rows_bf16(io.q, Q, p.S, h->s_qp.p, st));
      else HIPCHECK(h, launch_pack_rows(io.q, Q, p.S, (float *)h->s_qp.p, st));
    }
    HIPCHECK(h, launch_score_topk(lists_sweep_args(h, p, io.q), st));
  }
  h->uncert_word ^= 1;
  RescoreArgs r = lists_rescore_args(h, p, io);
  if (mirror) {
    r.host_scores = mirror->scores;
    r.host_ids = mirror->ids;
    r.host_cert = mirror->cert;
    r.host_err = mirror->err;
    r.host_flag = mirror->flag;
    r.err_in = h->err_flag;
    r.seq = mirror->seq;
  }
  HIPCHECK(h, launch_rescore(r, st));
  return 0;
}

// Second chance of the bf16 candidates, entirely on the device (the call stays asynchronous): queries whose bf16-candidate
// result missed its certificate (top scores packed closer than the bf16 bound) are swept again with fp32 candidates -- the same
// kernels, where a workgroup whose whole query block is certified returns at once and a certified query is left alone --
// before anything falls through to the collect path.
static int lists_second_chance(sse_handle *h, const TopkPlan &p, const TopkBufs &io, hipStream_t st) {
  const int Q = p.Q;
  if (reserve(h, h->s_qp32, (size_t)p.QB * p.NQ * p.KG * 256 * sizeof(float))) return 1;
  if (reserve(h, h->s_qmap, (size_t)(Q + 1) * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_qc, (size_t)p.QT * 32 * p.S * sizeof(float))) return 1;
  const RescoreArgs r = lists_rescore_args(h, p, io);
  HIPCHECK(h, launch_count_uncert(r.cert, Q, topk_counters(h), st));
  // the uncertified queries as a dense set: the sweep and the re-scoring below cost what THEY cost (launches sized for all
  // Q; workgroups past the set return at once)
  int32_t *qmap = (int32_t *)h->s_qmap.p, *qcount = qmap + Q;
  HIPCHECK(h, launch_compact_uncert(io.q, r.cert, Q, p.S, qmap, qcount, (float *)h->s_qc.p, st));
  if (!p.rows_direct) HIPCHECK(h, launch_pack_rows((const float *)h->s_qc.p, Q, p.S, (float *)h->s_qp32.p, st));
  ScoreArgs a2 = lists_sweep_args(h, p, (const float *)h->s_qc.p);
  a2.BF = 0;
  a2.idxp = h->idxp;
  a2.qp = (const float *)h->s_qp32.p;
  a2.KG = p.KG;
  a2.q_count = qcount;
  a2.NSPLIT = p.nsplit2;
  HIPCHECK(h, launch_score_topk(a2, st));
  RescoreArgs r2 = r;
  r2.q = (const float *)h->s_qc.p;
  r2.NC = p.nsplit2 * 16;
  r2.eps = p.eps32;
  r2.qmap = qmap;
  r2.q_count = qcount;
  r2.uncert = r2.uncert_clear = nullptr;  // (the word keeps the first pass's count: an upper bound, zero only if nothing is left)
  HIPCHECK(h, launch_rescore(r2, st));
  return 0;
}

// Lists route, second stage, for what the first left uncertified: the second chance of bf16 candidates, then the collect
// tail.  What is still uncertified there has its k-th score tied with (or within the fp32 bound of) rows outside the candidate
// lists -- e.g. an index holding many exact duplicates of a query's best rows: every row whose fp32 score reaches (exact k-th
// of the candidates) - bound is gathered by a grid-wide sweep and sorted in float64: provably the exact top-k, at the cost of
// one more fp32 sweep for the query blocks concerned.  The all-queued form launches this unconditionally (no host sync); with
// everything certified all workgroups return at once.
static int lists_rest(sse_handle *h, const TopkPlan &p, const TopkBufs &io, hipStream_t st) {
  // (<= 32 queries skip the second chance: for one query block it is the same fp32 sweep of the whole index as the collect
  // pass, which is final)
  const bool second = p.bf && p.Q > 32;
  if (second && lists_second_chance(h, p, io, st)) return 1;
  if (!p.own_slots) {
    HIPCHECK(h, hipMemsetAsync(h->s_ccnt.p, 0, (size_t)(p.POOL + 1) * sizeof(int32_t), st));
    HIPCHECK(h, launch_assign_slots((const int32_t *)h->s_cert.p, p.Q, p.POOL, (int32_t *)h->s_cslot.p, (int32_t *)h->s_ccnt.p + p.POOL, st));
  }
  ScoreArgs c = sweep_args(h, false, p.Q, p.NQ, p.nsplit);
  if (second) c.qp = (const float *)h->s_qp32.p;  // (unused: the collect sweep builds its fp32 fragments from the rows, nothing packed for it)
  c.q_rows = io.q;
  c.S = p.S;
  unsigned long long *counters = topk_counters(h);
  // brute force: the last resort (more than SSE_COLLECT_CAP rows within the bound of the k-th score, or no buffer slot left)
  return collect_tail(h, c, io, p.k, {SSE_COLLECT_CAP, counters + 1, counters + 2, lists_uncert(h), follow_grid(h)}, st);
}

// Everything of a call up to the point where the Lists route's certificates decide whether anything is left (p.has_rest); the
// other routes are complete after it.
static int topk_first(sse_handle *h, const TopkPlan &p, const TopkBufs &io, const ScoreMirror *mirror, hipStream_t st) {
  if (p.route == TopkRoute::None) return 0;
  if (p.route == TopkRoute::Paging) return topk_paging(h, p, io, st);
  if (topk_prepare(h, p, st)) return 1;
  if (p.route == TopkRoute::Select) return topk_select(h, p, io, st);
  if (p.route == TopkRoute::TwoPass) return topk_two_pass(h, p, io, st);
  return lists_first(h, p, io, mirror, st);
}

// sse_score_topk*_dev: every stage queued (no host sync; the follow-up stage returns at once when every query is certified).
// The host-buffer entry points (score_to_host_locked) look at the certificates in between and usually skip the second stage:
// the common call saves five to nine empty launches (~4.5 us each: a third of a single-query call,
// profiles/r02z_demo_kernel_stats.csv).
int score_dev_locked(sse_handle *h, const float *q, int Q, int k, double *out_s, int64_t *out_i, hipStream_t st) {
  TopkPlan p;
  if (topk_plan(h, Q, k, p)) return 1;
  const TopkBufs io{q, out_s, out_i};
  if (topk_first(h, p, io, nullptr, st)) return 1;
  return p.has_rest ? lists_rest(h, p, io, st) : 0;
}

}  // namespace

extern "C" {

const char *sse_last_error(sse_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int sse_create(const sse_config *cfg, sse_handle **out) {
  if (!cfg || !out) return fail(nullptr, "sse_create: null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, "no HIP device available");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, "device %d out of range (have %d)", cfg->device, ndev);
  if (cfg->vocab_size < 2 || cfg->embedding_size < 1 || cfg->encoding_size < 1)
    return fail(nullptr, "bad model sizes V=%d E=%d S=%d", cfg->vocab_size, cfg->embedding_size, cfg->encoding_size);
  sse_handle *h = new sse_handle();
  h->cfg = *cfg;
  h->lr = cfg->learning_rate;
#define CREATE_FAIL(...)        \
  do {                          \
    fail(nullptr, __VA_ARGS__); \
    sse_destroy(h);             \
    return 1;                   \
  } while (0)
  if (hipSetDevice(cfg->device) != hipSuccess) CREATE_FAIL("hipSetDevice(%d) failed", cfg->device);
  add_var(h, "word_embedding", cfg->vocab_size, cfg->embedding_size);
  switch (cfg->network_mode) {
    case SSE_MODE_DUAL_ENCODER:
      setup_encoder(h, h->enc[0], "source_encoder", "source_encoder/src_M", cfg->src_cell_size, cfg->src_cell_size);
      setup_encoder(h, h->enc[1], "target_encoder", "target_encoder/tgt_M", cfg->tgt_cell_size, cfg->tgt_cell_size);
      break;
    case SSE_MODE_SHARED_ENCODER:
      setup_encoder(h, h->enc[0], "shared_encoder", "shared_encoder/src_M", cfg->src_cell_size, cfg->src_cell_size);
      h->enc[1] = h->enc[0];
      h->enc[1].proj = add_var(h, "shared_encoder/tgt_M", cfg->src_cell_size, cfg->encoding_size);
      h->enc[1].shares_lstm_with = 0;
      break;
    case SSE_MODE_SOURCE_ENCODER_ONLY:
      setup_encoder(h, h->enc[0], "source_only_encoder", "source_only_encoder/src_M", cfg->src_cell_size, cfg->src_cell_size);
      h->tgt_table = add_var(h, "target_embedding/tgt_seq_embedding", cfg->target_space_size, cfg->encoding_size);
      break;
    case SSE_MODE_SOURCE_ONLY_CNN: {
      static const int fs[4] = {2, 3, 4, 5}, nf[4] = {256, 128, 128, 64};
      for (int i = 0; i < 4; ++i) {
        char nm[96];
        snprintf(nm, sizeof nm, "source_only_cnn/conv-maxpool-%d/W", fs[i]);
        h->cnn_W[i] = add_var(h, nm, fs[i] * cfg->embedding_size, nf[i]);
        snprintf(nm, sizeof nm, "source_only_cnn/conv-maxpool-%d/b", fs[i]);
        h->cnn_b[i] = add_var(h, nm, 1, nf[i]);
      }
      h->cnn_M = add_var(h, "source_only_cnn/src_M", 576, cfg->encoding_size);
      h->tgt_table = add_var(h, "target_embedding/tgt_seq_embedding", cfg->target_space_size, cfg->encoding_size);
      break;
    }
    default:
      CREATE_FAIL("Unsupported network mode %d (sse_model.py:175-177)", cfg->network_mode);
  }
  for (int s = 0; s < 2; ++s)
    if (h->enc[s].kernel >= 0 && geometry(h, h->enc[s])) {
      g_create_error = h->err;
      sse_destroy(h);
      return 1;
    }
  for (auto &v : h->vars) {
    if (hipMalloc((void **)&v.dev, v.count * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&v.slot, v.count * sizeof(float)) != hipSuccess)
      CREATE_FAIL("hipMalloc failed for variable %s", v.name.c_str());
    hipMemset(v.dev, 0, v.count * sizeof(float));
    launch_fill(v.slot, v.count, 0.1f, nullptr);  // AdagradOptimizer initial_accumulator_value
  }
  if (hipMalloc((void **)&h->err_flag, sizeof(int32_t)) != hipSuccess) CREATE_FAIL("hipMalloc failed");
  if (hipHostMalloc((void **)&h->pin_small, 64 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) CREATE_FAIL("hipHostMalloc failed");
  hipMemset(h->err_flag, 0, sizeof(int32_t));
  if (hipHostMalloc((void **)&h->pad_stat, 8 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) CREATE_FAIL("hipHostMalloc failed");
  {  // compute units of the device: the tile policy of the matrix LSTM kernel counts rounds of them, the cluster kernels check co-residency
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) h->cu_count = prop.multiProcessorCount;
  }
  if (const char *ev = getenv("SSE_PAD_SORT_DEV")) {  // measurement aid: the option's initial value
    const int v = atoi(ev);
    if (v >= 0 && v <= 2) h->pad_sort_dev = v;
  }
  memset(h->pad_stat, 0, 8 * sizeof(int32_t));
  if (hipDeviceSynchronize() != hipSuccess) CREATE_FAIL("device initialisation failed");
#undef CREATE_FAIL
  *out = h;
  return 0;
}

void sse_destroy(sse_handle *h) {
  if (!h) return;
  hipSetDevice(h->cfg.device);
  hipDeviceSynchronize();
  for (auto &v : h->vars) {
    if (v.dev) hipFree(v.dev);
    if (v.slot) hipFree(v.slot);
  }
  if (h->train && h->train->arena && !h->train->arena_external) hipFree(h->train->arena);
  for (int s = 0; s < 2; ++s) {
    Encoder &e = h->enc[s];
    if (e.shares_lstm_with < 0) {
      if (e.Wp) hipFree(e.Wp);
      if (e.Waug) (void)hipFree(e.Waug);
      if (e.Wc) (void)hipFree(e.Wc);
      if (e.Wx3) (void)hipFree(e.Wx3);
      if (e.Wx3t) (void)hipFree(e.Wx3t);
      e.pad_fwd.release();
      e.pad_small.release();
      e.pad_x3.release();
      if (e.xtab) (void)hipFree(e.xtab);
    }
    if (e.Mp) hipFree(e.Mp);
  }
  if (h->pin) (void)hipHostFree(h->pin);
  if (h->pin_small) (void)hipHostFree(h->pin_small);
  if (h->pad_stat) (void)hipHostFree(h->pad_stat);
  if (h->emb_pad) hipFree(h->emb_pad);
  if (h->emb16) (void)hipFree(h->emb16);
  if (h->err_flag) hipFree(h->err_flag);
  if (h->idxp) hipFree(h->idxp);
  if (h->idxp16) (void)hipFree(h->idxp16);
  if (h->idx64) hipFree(h->idx64);
  if (h->cnn_Wc) (void)hipFree(h->cnn_Wc);
  if (h->emb_bf16) (void)hipFree(h->emb_bf16);
  if (h->cnn_Wc16) (void)hipFree(h->cnn_Wc16);
  if (h->cnn_Mx3) (void)hipFree(h->cnn_Mx3);
  if (h->cnn_bias) (void)hipFree(h->cnn_bias);
  if (h->cnn_Mp) (void)hipFree(h->cnn_Mp);
  if (h->train) {
    TrainState *t = h->train;
    for (int s = 0; s < 2; ++s) {
      if (t->side[s]) (void)hipStreamDestroy(t->side[s]);
      if (t->ev_join[s]) (void)hipEventDestroy(t->ev_join[s]);
      if (t->KhT[s] && (s == 0 || t->KhT[s] != t->KhT[0])) (void)hipFree(t->KhT[s]);
      if (t->KxT[s] && (s == 0 || t->KxT[s] != t->KxT[0])) (void)hipFree(t->KxT[s]);
      if (t->KhT16[s] && (s == 0 || t->KhT16[s] != t->KhT16[0])) (void)hipFree(t->KhT16[s]);
      if (t->KxT16[s] && (s == 0 || t->KxT16[s] != t->KxT16[0])) (void)hipFree(t->KxT16[s]);
    }
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    delete t;
  }
  for (hipEvent_t e : h->events)
    if (e) (void)hipEventDestroy(e);
  delete h;
}

int sse_num_variables(sse_handle *h) { return h ? (int)h->vars.size() : 0; }

int sse_variable_info(sse_handle *h, int index, const char **name, int64_t *count, int32_t *rows, int32_t *cols) {
  if (!h) return 1;
  if (index < 0 || index >= (int)h->vars.size()) return fail(h, "variable index %d out of range", index);
  const Variable &v = h->vars[index];
  if (name) *name = v.name.c_str();
  if (count) *count = v.count;
  if (rows) *rows = v.rows;
  if (cols) *cols = v.cols;
  return 0;
}

int sse_set_variable(sse_handle *h, const char *name, const float *host, int64_t count) {
  if (!h || !name || !host) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  bool slot;
  const int i = find_var(h, name, &slot);
  if (i < 0) return fail(h, "unknown variable '%s'", name);
  if (count != h->vars[i].count) return fail(h, "variable '%s' has %lld elements, got %lld", name, (long long)h->vars[i].count, (long long)count);
  HIPCHECK(h, hipMemcpy(slot ? h->vars[i].slot : h->vars[i].dev, host, count * sizeof(float), hipMemcpyHostToDevice));
  if (!slot) {
    h->packed_dirty = true;
    h->weights_version += 1;
    h->mp_fresh = false;
    if (h->train) h->train->packed_dirty = h->train->fp32_dirty = true;
  }
  return 0;
}

int sse_get_variable(sse_handle *h, const char *name, float *host, int64_t count) {
  if (!h || !name || !host) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  bool slot;
  const int i = find_var(h, name, &slot);
  if (i < 0) return fail(h, "unknown variable '%s'", name);
  if (count != h->vars[i].count) return fail(h, "variable '%s' has %lld elements, got %lld", name, (long long)h->vars[i].count, (long long)count);
  HIPCHECK(h, hipDeviceSynchronize());
  HIPCHECK(h, hipMemcpy(host, slot ? h->vars[i].slot : h->vars[i].dev, count * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int sse_encode_dev(sse_handle *h, int side, const int32_t *ids_dev, int32_t B, int32_t T, int32_t normalize,
                   float *out_dev, void *stream) {
  SSE_ENTER(h);
  return encode_dev_locked(h, side, ids_dev, B, T, normalize, out_dev, (hipStream_t)stream);
}

// host ids -> encodings [B][S] in h->s_out (device); the handle mutex is held by the caller
// the handle's pinned read-back buffer, grown on demand
static int ensure_pin(sse_handle *h, size_t need) {
  if (need <= h->pin_cap) return 0;
  if (h->pin) HIPCHECK(h, hipHostFree(h->pin));
  h->pin = nullptr;
  h->pin_cap = 0;
  HIPCHECK(h, hipHostMalloc(&h->pin, need + need / 2 + 4096, hipHostMallocCoherent));  // (the device stores into it: ScoreMirror)
  h->pin_cap = need + need / 2 + 4096;
  memset(h->pin, 0, h->pin_cap);  // (the completion words of ScoreMirror must not hold a call number by accident)
  return 0;
}

// Re-run of a batch whose cluster-kernel launch reported a missing workgroup (error bit 2), on the kernels that need no
// co-residency.  The cluster kernels need their 16 - 32 workgroups per cluster resident together; a device busy with other
// work (a train step on another handle, four serving routes at once) can keep one from arriving within the give-up time.
// Nothing was written that the other kernels do not overwrite; results are bit-identical.
static int encode_fallback_locked(sse_handle *h, int side, int32_t B, int32_t T, int32_t normalize, hipStream_t st) {
  h->persist_fallbacks += 1;
  h->cluster_skip[B <= 32 ? 0 : 1] = h->cluster_backoff >= 0 ? h->cluster_backoff : 16;  // a time-out costs 10 ms: do not pay it on every call of a busy device
  EncodeRequest rq;
  rq.allow_cluster = false;
  if (encode_dev_locked(h, side, (const int32_t *)h->s_ids.p, B, T, normalize, (float *)h->s_out.p, st, rq)) return 1;
  return check_err_flag(h, st);
}

// defer_check: leave the device error flag unread (no synchronisation here); the caller reads it with its own read-back
static int encode_host_ids_locked(sse_handle *h, int side, const int32_t *ids_host, int32_t B, int32_t T, int32_t normalize,
                                  bool defer_check = false) {
  const size_t S = h->cfg.encoding_size;
  if (reserve(h, h->s_ids, (size_t)B * T * sizeof(int32_t))) return 1;
  if (reserve(h, h->s_out, (size_t)B * S * sizeof(float))) return 1;
  hipStream_t st = nullptr;
  // Group rows by their leading-PAD count (left-padded inputs, sse_index.py:79-85) so that every
  // 64-row tile can skip its whole common PAD prefix; results are scattered back in caller order.
  const bool lstm_side = h->cfg.network_mode != SSE_MODE_SOURCE_ONLY_CNN && !(side == SSE_SIDE_TARGET && h->tgt_table >= 0);
  EncodeRequest rq;
  const Encoder &e = h->enc[side];
  if (lstm_side && e.kernel >= 0 && !e.generic) {  // the kernel, chosen once: the cluster kernel takes rows as they come
    rq.path = choose_lstm_path(h, e, B, T, rq);
    if (rq.path == LstmPath::Error) return 1;
  }
  if (h->pad_skip && lstm_side && B > 64 && B > h->lstm_small_rows && rq.path != LstmPath::Cluster && !e.generic) {
    // counting sort of the row numbers by leading-PAD count, shortest prefix first (the tiles with the most steps left are
    // dispatched first; see pack.hip, pad_lead_kernel)
    std::vector<int32_t> lead(B), start(T + 2, 0), order(B);
    for (int b = 0; b < B; ++b) {
      const int32_t *row = ids_host + (size_t)b * T;
      int t = 0;
      while (t < T && row[t] == 0) ++t;
      lead[b] = t;
      ++start[t + 1];
    }
    for (int i = 1; i <= T + 1; ++i) start[i] += start[i - 1];
    for (int b = 0; b < B; ++b) order[start[lead[b]]++] = b;
    int64_t lead_sum = 0;
    for (int b = 0; b < B; ++b) lead_sum += lead[b];
    rq.padded_hint = lead_sum * 4 >= (int64_t)B * T;
    if (reserve(h, h->s_map, (size_t)B * sizeof(int32_t))) return 1;
    HIPCHECK(h, hipMemcpyAsync(h->s_map.p, order.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(h, hipStreamSynchronize(st));  // `order` is a local
    rq.row_map = (const int32_t *)h->s_map.p;
  }
  HIPCHECK(h, hipMemcpyAsync(h->s_ids.p, ids_host, (size_t)B * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (encode_dev_locked(h, side, (const int32_t *)h->s_ids.p, B, T, normalize, (float *)h->s_out.p, st, rq)) return 1;
  if (defer_check) return 0;
  int32_t bits = 0;
  if (check_err_flag(h, st, &bits)) return 1;
  if (bits == 4) return encode_fallback_locked(h, side, B, T, normalize, st);
  return 0;
}

int sse_encode(sse_handle *h, int side, const int32_t *ids_host, int32_t B, int32_t T, int32_t normalize,
               float *out_host) {
  SSE_ENTER(h);
  if (B == 0) return 0;
  if (B < 0 || T < 1 || !ids_host || !out_host) return fail(h, "bad arguments to sse_encode");
  const size_t nbytes = (size_t)B * h->cfg.encoding_size * sizeof(float);
  if (nbytes <= (64u << 10)) {
    // small results (a few queries): the encodings and the error flag come back in ONE pinned read-back with one
    // synchronisation, 0.155 -> 0.144 ms for a query.  (Measured the other way for larger ones: 600 x 256 floats 0.340 ->
    // 0.364 ms, 1024 rows 0.364 -> 0.440 ms -- the runtime's staged copy into a pageable target beats pinned + memcpy.)
    if (encode_host_ids_locked(h, side, ids_host, B, T, normalize, /*defer_check=*/true)) return 1;
    const size_t need = nbytes + sizeof(int32_t);
    if (ensure_pin(h, need)) return 1;
    char *pin = (char *)h->pin;
    hipStream_t st = nullptr;
    HIPCHECK(h, hipMemcpyAsync(pin, h->s_out.p, nbytes, hipMemcpyDeviceToHost, st));
    HIPCHECK(h, hipMemcpyAsync(pin + nbytes, h->err_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHECK(h, sync_stream(st));
    int32_t bits = *(const int32_t *)(pin + nbytes);
    if (bits == 0) {
      memcpy(out_host, pin, nbytes);
      return 0;
    }
    if (check_err_flag(h, st, &bits)) return 1;  // reports what is reportable, resets the flag
    if (bits == 4 && encode_fallback_locked(h, side, B, T, normalize, st)) return 1;
  } else if (encode_host_ids_locked(h, side, ids_host, B, T, normalize)) {
    return 1;
  }
  HIPCHECK(h, hipMemcpy(out_host, h->s_out.p, nbytes, hipMemcpyDeviceToHost));
  return 0;
}

// The pinned block of one host-form scoring call: [scores | ids | certificates | error flag | completion words]
struct ScorePin {
  char *base;
  size_t nb;  // bytes of the scores, and of the ids
  int32_t *cert, *flag, *done;
};

// First results through the mirror: the host polls the completion words the re-scoring pass stores last; scores, ids,
// certificates and the error flag are in the block when they are all there
static int poll_mirror(sse_handle *h, const ScorePin &pin, int Q, int32_t seq, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  bool synced = false;
  for (;;) {
    bool all = true;
    for (int i = 0; i < Q && all; ++i) all = __atomic_load_n(pin.done + i, __ATOMIC_ACQUIRE) == seq;
    if (all) return 0;
    if (synced) return fail(h, "the re-scoring pass did not report completion");
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(3)) {
      HIPCHECK(h, hipStreamSynchronize(st));  // (a launch that failed shows up here)
      synced = true;
    }
  }
}

// Results by copies: scores and ids, with them (certs / err) the certificates and the device error flag, one synchronisation
static int copy_back(sse_handle *h, const ScorePin &pin, int Q, bool certs, bool err, hipStream_t st) {
  HIPCHECK(h, hipMemcpyAsync(pin.base, h->s_os.p, pin.nb, hipMemcpyDeviceToHost, st));
  HIPCHECK(h, hipMemcpyAsync(pin.base + pin.nb, h->s_oi.p, pin.nb, hipMemcpyDeviceToHost, st));
  if (certs) HIPCHECK(h, hipMemcpyAsync(pin.cert, h->s_cert.p, (size_t)Q * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (err) HIPCHECK(h, hipMemcpyAsync(pin.flag, h->err_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHECK(h, sync_stream(st));
  return 0;
}

// Scores + ids of Q queries (device rows q_dev) into host buffers: the first stage, its results, certificates and error flag
// read back at once (polled through the mirror for few queries, else one pinned read-back with one synchronisation), and the
// second stage with a read-back of its own only when some query is not certified.
// err_bits: (optional) the device error flag rides along with the first results (an encoder launched just before on the
// same stream with its check deferred); when it comes back non-zero the outputs are not written.
static int score_to_host_locked(sse_handle *h, const float *q_dev, int Q, int k, double *out_scores, int64_t *out_ids,
                                int32_t *err_bits = nullptr) {
  hipStream_t st = nullptr;
  if (reserve(h, h->s_os, (size_t)Q * k * sizeof(double))) return 1;
  if (reserve(h, h->s_oi, (size_t)Q * k * sizeof(int64_t))) return 1;
  const size_t nb = (size_t)Q * k * 8, need = 2 * nb + (size_t)(2 * Q + 1) * sizeof(int32_t);
  if (ensure_pin(h, need)) return 1;
  char *base = (char *)h->pin;
  int32_t *cert = (int32_t *)(base + 2 * nb);
  const ScorePin pin{base, nb, cert, cert + Q, cert + Q + 1};
  // few queries (the demo / web call): the re-scoring pass stores its results through the pinned pointers itself and the
  // host polls the completion words -- three read-back copies and the stream synchronisation were ~40 us of a 0.19 ms call
  const bool use_mirror = Q <= 64 && k <= 16;
  ScoreMirror hm{(double *)base, (int64_t *)(base + nb), pin.cert, pin.flag, pin.done, 0};
  if (use_mirror) {
    h->score_seq = (h->score_seq == INT32_MAX) ? 1 : h->score_seq + 1;
    hm.seq = h->score_seq;
    // The completion words move inside the pinned block with (Q, k), and the block is shared with earlier calls of other
    // shapes (scores, int64 ids, certificates) and with sse_encode's read-back: a stale word could equal this call's
    // sequence number.  Nothing of this handle is in flight here (the previous call returned after its last poll / sync),
    // so the host clears them before the launch.
    for (int i = 0; i < Q; ++i) __atomic_store_n(pin.done + i, 0, __ATOMIC_RELAXED);
    __atomic_store_n(pin.flag, 0, __ATOMIC_RELEASE);
  }
  TopkPlan p;
  if (topk_plan(h, Q, k, p)) return 1;
  const TopkBufs io{q_dev, (double *)h->s_os.p, (int64_t *)h->s_oi.p};
  if (topk_first(h, p, io, use_mirror ? &hm : nullptr, st)) return 1;
  const bool polled = use_mirror && p.has_rest;  // (the mirror belongs to lists_first)
  if (polled ? poll_mirror(h, pin, Q, hm.seq, st) : copy_back(h, pin, Q, p.has_rest, err_bits != nullptr, st)) return 1;
  if (err_bits) {
    *err_bits = *pin.flag;
    if (*pin.flag) return 0;  // the queries were not what the caller meant: it looks at the flag first
  }
  bool open_q = false;
  for (int i = 0; i < Q && p.has_rest && !open_q; ++i) open_q = pin.cert[i] == 0;
  if (open_q) {
    // rare: ties / near-ties at the k-th score, or scores packed closer than the bf16 bound
    if (lists_rest(h, p, io, st)) return 1;
    if (copy_back(h, pin, Q, false, false, st)) return 1;
  }
  memcpy(out_scores, pin.base, nb);
  memcpy(out_ids, pin.base + nb, nb);
  return 0;
}

int sse_encode_score_topk(sse_handle *h, int side, const int32_t *ids_host, int32_t B, int32_t T, int32_t normalize,
                          int32_t k, double *out_scores, int64_t *out_ids, float *enc_out_host) {
  SSE_ENTER(h);
  if (B == 0) return 0;
  if (B < 0 || T < 1 || !ids_host || !out_scores || !out_ids) return fail(h, "bad arguments to sse_encode_score_topk");
  if (!h->idxp) return fail(h, "no index uploaded");
  if (h->cfg.encoding_size != h->idx_S)
    return fail(h, "index dimension %d != encoding_size %d", h->idx_S, h->cfg.encoding_size);
  // One synchronisation for the whole call: the encoder's error flag (token id out of range, a cluster workgroup that did
  // not arrive) is not waited for before the scorer is launched -- it comes back with the scores.
  if (encode_host_ids_locked(h, side, ids_host, B, T, normalize, /*defer_check=*/true)) return 1;
  // the encodings never leave the device between the encoder and the scorer
  int32_t bits = 0;
  if (score_to_host_locked(h, (const float *)h->s_out.p, B, k, out_scores, out_ids, &bits)) return 1;
  if (bits) {
    if (check_err_flag(h, nullptr, &bits)) return 1;  // reports what is reportable, resets the flag
    if (bits == 4) {
      if (encode_fallback_locked(h, side, B, T, normalize, nullptr)) return 1;
      if (score_to_host_locked(h, (const float *)h->s_out.p, B, k, out_scores, out_ids)) return 1;
    }
  }
  if (enc_out_host)
    HIPCHECK(h, hipMemcpy(enc_out_host, h->s_out.p, (size_t)B * h->cfg.encoding_size * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

namespace {

// Counters whose words live on the device, one group per family of scoring calls: the words accumulate over the handle's life
// (ensure_zeroed_once) and read as 0 until the first call of the family has reserved and cleared them.
struct DevCounters {
  DevBuf sse_handle::*buf;
  bool sse_handle::*init;
  int words;  // read back together
};
enum { CG_RANK, CG_ABOVE, CG_FILTERED, CG_GROUPED, CG_AFTER, CG_CONFUSIONS, CG_BIASED, CG_TOPK, CG_LSE, CG_DEV_COUNT, CG_HOST = CG_DEV_COUNT, CG_PATH, CG_COOP };
const DevCounters DEV_COUNTERS[CG_DEV_COUNT] = {
    {&sse_handle::s_rk_cnt, &sse_handle::rk_cnt_init, 2}, {&sse_handle::s_ab_cnt, &sse_handle::ab_cnt_init, 3},
    {&sse_handle::s_ft_cnt, &sse_handle::ft_cnt_init, 3}, {&sse_handle::s_gp_cnt, &sse_handle::gp_cnt_init, 3},
    {&sse_handle::s_af_cnt, &sse_handle::af_cnt_init, 3}, {&sse_handle::s_cf_cnt, &sse_handle::cf_cnt_init, 3},
    {&sse_handle::s_bs_cnt, &sse_handle::bs_cnt_init, 3}, {&sse_handle::s_fb_cnt, &sse_handle::fb_cnt_init, 4},
    {&sse_handle::s_lse_cnt, &sse_handle::lse_cnt_init, 1}};
int64_t sse_handle::*const HOST_COUNTERS[] = {&sse_handle::persist_fallbacks, &sse_handle::two_pass_calls, &sse_handle::pad_sorted_calls,
                                              &sse_handle::eval_paired_calls, &sse_handle::x_table_builds,
                                              &sse_handle::train_path_fused, &sse_handle::train_path_generic, &sse_handle::train_path_cnn,
                                              &sse_handle::train_paired_steps, &sse_handle::train_fp32_repacks,
                                              &sse_handle::train_split_repacks, &sse_handle::train_generic_repacks,
                                              &sse_handle::train_inbatch_steps, &sse_handle::score_lse_calls,
                                              &sse_handle::train_class_steps, &sse_handle::train_open_steps,
                                              &sse_handle::train_global_inbatch_steps,
                                              &sse_handle::index_update_calls, &sse_handle::index_update_rows,
                                              &sse_handle::index_append_rows, &sse_handle::index_grow_copies};

// every name sse_get_counter answers: its group and its word there (CG_HOST: entry of HOST_COUNTERS; CG_PATH: entry of
// sse_handle::lstm_path_calls; a device group: the word the kernels of that family count in)
const struct {
  const char *name;
  int group, word;
} COUNTERS[] = {
    {"lstm_persist_fallbacks", CG_HOST, 0},
    {"score_two_pass_calls", CG_HOST, 1},  // sse_score_topk* calls ranked by the two-pass path for mid-size indexes
    {"pad_sorted_calls", CG_HOST, 2},      // encodes of device-resident ids whose rows were bucketed by PAD prefix on the device
    {"eval_paired_calls", CG_HOST, 3},     // sse_eval_loss* calls whose source encoder ran once per (positive, negative) pair
    {"lstm_x_table_builds", CG_HOST, 4},   // x-projection tables built (option lstm_x_table)
    // train steps (sse_train_grads*, sse_train_step*) by path, the fused path's paired steps, and the layouts a step rebuilt
    {"train_path_fused", CG_HOST, 5},
    {"train_path_generic", CG_HOST, 6},
    {"train_path_cnn", CG_HOST, 7},
    {"train_paired_steps", CG_HOST, 8},
    {"train_fp32_repacks", CG_HOST, 9},     // the fp32 Kh^T / Kx^T fragment copies of the BPTT kernels
    {"train_split_repacks", CG_HOST, 10},   // their split-operand forms KhT16 / KxT16
    {"train_generic_repacks", CG_HOST, 11}, // the any-shape path's packs, once per side
    {"train_inbatch_steps", CG_HOST, 12},   // steps whose loss stage ran the in-batch softmax head (option train_loss = 1)
    {"train_class_steps", CG_HOST, 14},     // steps whose loss stage ran the class softmax head (option train_class_loss = 1)
    {"train_open_steps", CG_HOST, 15},      // sse_train_forward* calls that left a step open
    {"train_global_inbatch_steps", CG_HOST, 16},  // steps closed by sse_train_backward_inbatch_global
    // LSTM inference encodes by kernel
    {"lstm_path_persist", CG_PATH, PATH_PERSIST},
    {"lstm_path_cluster", CG_PATH, PATH_CLUSTER},
    {"lstm_path_small", CG_PATH, PATH_SMALL},
    {"lstm_path_x3", CG_PATH, PATH_X3},
    {"lstm_path_generic", CG_PATH, PATH_GENERIC},
    {"lstm_path_fwd", CG_PATH, PATH_FWD},
    {"lstm_fwd_rows32", CG_PATH, PATH_FWD_ROWS32},
    {"lstm_fwd_rows64", CG_PATH, PATH_FWD_ROWS64},
    {"lstm_fwd_gate_split", CG_PATH, PATH_FWD_GS},
    {"lstm_fwd_x_table", CG_PATH, PATH_FWD_XT},
    {"lstm_coop_refused", CG_COOP, 0},  // process-wide: cooperative launches refused by the runtime (plain launch taken)
    // sse_score_rank* (score_rank.hip): rows that needed float64, pairs whose band outgrew its buffer
    {"score_rank_band_rows", CG_RANK, 0},
    {"score_rank_bruteforce_pairs", CG_RANK, 1},
    // sse_score_above* (score_above.hip): rows decided in float64, pairs listed by the float64 sweep, segments merged in global memory
    {"score_above_band_rows", CG_ABOVE, 0},
    {"score_above_bruteforce_pairs", CG_ABOVE, 1},
    {"score_above_long_segments", CG_ABOVE, 2},
    // sse_score_topk_filtered* (score_filtered.hip): rows re-scored by the select stage, queries of the float64 sweep, tiles skipped
    {"score_filtered_collected_rows", CG_FILTERED, 0},
    {"score_filtered_bruteforce_queries", CG_FILTERED, 1},
    {"score_filtered_tiles_skipped", CG_FILTERED, 2},
    // sse_score_topk_grouped* (score_grouped.hip) and sse_score_topk_after* (score_after.hip): rows re-scored by the select
    // stage, queries of the float64 sweep
    {"score_grouped_collected_rows", CG_GROUPED, 0},
    {"score_grouped_bruteforce_queries", CG_GROUPED, 1},
    {"score_after_collected_rows", CG_AFTER, 0},
    {"score_after_bruteforce_queries", CG_AFTER, 1},
    // sse_score_confusions* (score_confusions.hip): rows collected for the select stage, queries of the float64 sweep, queries
    // whose stored collect threshold is the floor term
    {"score_confusions_collected_rows", CG_CONFUSIONS, 0},
    {"score_confusions_bruteforce_queries", CG_CONFUSIONS, 1},
    {"score_confusions_floor_queries", CG_CONFUSIONS, 2},
    // sse_score_topk_biased* (score_biased.hip): rows re-scored by the select stage, queries of the float64 sweep
    {"score_biased_collected_rows", CG_BIASED, 0},
    {"score_biased_bruteforce_queries", CG_BIASED, 1},
    // sse_score_topk* (score_topk.hip): queries whose bf16-candidate result missed its certificate, queries served by the
    // collect path, queries that fell through to the float64 brute force
    {"score_bf16_second_chance_queries", CG_TOPK, 0},
    {"score_collect_queries", CG_TOPK, 1},
    {"score_bruteforce_queries", CG_TOPK, 2},
    // sse_score_lse* (score_lse.hip): calls that passed their checks, index tiles its sweep skipped
    {"score_lse_calls", CG_HOST, 13},
    {"score_lse_tiles_skipped", CG_LSE, 0},
    // sse_index_update* / sse_index_append*: update calls and the rows they named, rows appended, appends that reallocated
    // the fragment copy
    {"index_update_calls", CG_HOST, 17},
    {"index_update_rows", CG_HOST, 18},
    {"index_append_rows", CG_HOST, 19},
    {"index_grow_copies", CG_HOST, 20},
};

static int read_dev_counter(sse_handle *h, const DevCounters &g, int word, int64_t *value) {
  unsigned long long v[4] = {0, 0, 0, 0};
  if ((h->*g.buf).p && h->*g.init) {
    HIPCHECK(h, hipSetDevice(h->cfg.device));
    HIPCHECK(h, hipDeviceSynchronize());
    HIPCHECK(h, hipMemcpy(v, (h->*g.buf).p, g.words * sizeof v[0], hipMemcpyDeviceToHost));
  }
  *value = (int64_t)v[word];
  return 0;
}

// The options that are one int of the handle: a switch (message null; stored as value != 0) or a value in [min, max], refused
// with `message` outside.  What each one does stands beside its member in struct sse_handle (above).
const struct {
  const char *name;
  int sse_handle::*member;
  int min, max;
  const char *message;
} OPTIONS[] = {
    {"score_small_index", &sse_handle::score_small_index},
    {"score_small_x3", &sse_handle::score_small_x3},
    {"score_filtered_skip", &sse_handle::score_filtered_skip},
    {"score_bf16", &sse_handle::score_bf16},
    {"train_bwd_x3", &sse_handle::train_bwd_x3},
    {"train_fwd_x3", &sse_handle::train_fwd_x3},
    {"train_dk_x3", &sse_handle::train_dk_x3},
    {"train_generic", &sse_handle::train_generic},
    {"train_gen1", &sse_handle::train_gen1},
    {"train_pair_dedup", &sse_handle::train_pair_dedup},
    {"train_serial", &sse_handle::train_serial},
    {"pad_skip", &sse_handle::pad_skip},
    {"lstm_gate_split", &sse_handle::lstm_gate_split},
    {"lstm_x3", &sse_handle::lstm_x3},
    {"lstm_persist_inject_miss", &sse_handle::persist_inject},  // testing aid for the fallback path of the host-buffer encodes
    {"lstm_cluster_drop_wg", &sse_handle::lstm_cluster_drop},
    {"lstm_cluster_coop", &sse_handle::lstm_cluster_coop},
    {"lstm_cluster_write_through", &sse_handle::lstm_cluster_wt},
    {"score_two_pass_min_rows", &sse_handle::score_two_pass_min_rows, 0, INT32_MAX, "score_two_pass_min_rows must be >= 0"},
    {"score_two_pass_rows", &sse_handle::score_two_pass_rows, 0, INT32_MAX, "score_two_pass_rows must be >= 0"},
    {"pad_sort_dev", &sse_handle::pad_sort_dev, 0, 2, "pad_sort_dev must be 0 (off), 1 (adaptive) or 2 (always)"},
    {"lstm_persist_rows", &sse_handle::lstm_persist_rows, 0, INT32_MAX, "lstm_persist_rows must be >= 0"},
    {"lstm_cluster_chunks", &sse_handle::lstm_cluster_chunks, 1, INT32_MAX, "lstm_cluster_chunks must be >= 1"},
    {"lstm_cluster_rows", &sse_handle::lstm_cluster_rows, 0, INT32_MAX, "lstm_cluster_rows must be >= 0"},
    {"lstm_small_rows", &sse_handle::lstm_small_rows, 0, INT32_MAX, "lstm_small_rows must be >= 0"},
    {"lstm_x_table", &sse_handle::lstm_x_table, 0, 2, "lstm_x_table must be 0 (off), 1 (batches with B * T >= vocab_size) or 2 (always)"},
    {"lstm_x_table_mb", &sse_handle::lstm_x_table_mb, 0, INT32_MAX, "lstm_x_table_mb must be >= 0"},
    {"train_loss", &sse_handle::train_loss, 0, 1, "train_loss must be 0 (pair) or 1 (in-batch softmax)"},
    {"train_loss_scale", &sse_handle::train_loss_scale, 1, 256, "train_loss_scale must be in 1 .. 256"},
    {"train_class_loss", &sse_handle::train_class_loss, 0, 1, "train_class_loss must be 0 (off) or 1 (softmax over the free target matrix)"},
};

}  // namespace

int sse_get_counter(sse_handle *h, const char *name, int64_t *value) {
  if (!h || !name || !value) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  for (const auto &c : COUNTERS) {
    if (strcmp(name, c.name) != 0) continue;
    if (c.group < CG_DEV_COUNT) return read_dev_counter(h, DEV_COUNTERS[c.group], c.word, value);
    *value = c.group == CG_HOST ? h->*HOST_COUNTERS[c.word] : c.group == CG_PATH ? h->lstm_path_calls[c.word] : (int64_t)lstm_coop_refused();
    return 0;
  }
  return fail(h, "unknown counter '%s'", name);
}

int sse_set_option(sse_handle *h, const char *name, int32_t value) {
  if (!h || !name) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  for (const auto &o : OPTIONS) {
    if (strcmp(name, o.name) != 0) continue;
    if (o.message && (value < o.min || value > o.max)) return fail(h, "%s", o.message);
    h->*o.member = o.message ? value : value != 0;
    return 0;
  }
  // the options that do more than store one int
  if (strcmp(name, "cnn_bf16") == 0) {
    if (h->cfg.network_mode != SSE_MODE_SOURCE_ONLY_CNN) return fail(h, "option cnn_bf16 needs network_mode source_only_cnn");
    h->cnn_bf16 = value != 0;
    h->packed_dirty = true;  // (re)build the bf16 copies with the next encode
    h->mp_fresh = false;
    return 0;
  }
  if (strcmp(name, "lstm_train_rows") == 0) {
    if (value != 0 && value != 32 && value != 64) return fail(h, "lstm_train_rows must be 0, 32 or 64");
    h->lstm_train_rows = (int)value;
    return 0;
  }
  if (strcmp(name, "eval_chunk_rows") == 0) {
    if (value < 2) return fail(h, "eval_chunk_rows must be >= 2");
    h->eval_chunk_rows = (int)(value & ~1);  // even: a chunk never splits a (positive, negative) pair of rows
    return 0;
  }
  if (strcmp(name, "lstm_persist_epoch") == 0) {  // testing aid: move the cluster kernel's 20-bit tag epoch (wrap-around path)
    if (value < 0 || value >= (1 << 20)) return fail(h, "lstm_persist_epoch must be in [0, 2^20)");
    h->persist_epoch = (uint32_t)value;
    return 0;
  }
  if (strcmp(name, "lstm_cluster_backoff") == 0) {
    if (value < -1) return fail(h, "lstm_cluster_backoff must be >= 0 (or -1: automatic)");
    h->cluster_backoff = (int)value;
    h->cluster_skip[0] = h->cluster_skip[1] = 0;
    return 0;
  }
  return fail(h, "unknown option '%s'", name);
}

int sse_l2_normalize_dev(sse_handle *h, const float *x_dev, float *out_dev, int64_t rows, int32_t cols, void *stream) {
  SSE_ENTER(h);
  HIPCHECK(h, launch_l2_normalize(x_dev, out_dev, rows, cols, (hipStream_t)stream));
  return 0;
}

// the handle's scratch of one in-batch loss call over B rows of S columns; keys: [source keys | target keys | hash words], B each
static int reserve_inbatch(sse_handle *h, int B, int S) {
  return reserve(h, h->s_inbatch, inbatch_scratch_bytes(B, S)) || reserve(h, h->s_inbatch_keys, (size_t)3 * B * sizeof(int32_t));
}

int sse_inbatch_loss_dev(sse_handle *h, const float *src_raw_dev, const float *tgt_raw_dev, const float *labels_dev,
                         const int64_t *src_key_dev, const int64_t *tgt_key_dev, int32_t B, int32_t S, float scale, float inv_rows,
                         float *d_src_dev, float *d_tgt_dev, float *row_loss_dev, float *row_acc_dev, void *stream) {
  SSE_ENTER(h);
  if (B < 1 || S < 1) return fail(h, "sse_inbatch_loss_dev: B and S must be >= 1");
  if (!src_raw_dev || !tgt_raw_dev || !labels_dev || !row_loss_dev || !row_acc_dev)
    return fail(h, "sse_inbatch_loss_dev: encodings, labels, row_loss and row_acc must not be NULL");
  if ((d_src_dev == nullptr) != (d_tgt_dev == nullptr))
    return fail(h, "sse_inbatch_loss_dev: d_src and d_tgt must both be given, or both be NULL (forward only)");
  if (!(scale > 0.0f && scale <= 256.0f)) return fail(h, "sse_inbatch_loss_dev: scale must be in (0, 256]");
  if (reserve_inbatch(h, B, S)) return 1;
  hipStream_t st = (hipStream_t)stream;
  int32_t *ks = (int32_t *)h->s_inbatch_keys.p, *kt = ks + B;
  HIPCHECK(h, launch_inbatch_value_keys(src_key_dev, 64, B, ks, st));
  HIPCHECK(h, launch_inbatch_value_keys(tgt_key_dev, 64, B, kt, st));
  HIPCHECK(h, launch_inbatch_loss(src_raw_dev, tgt_raw_dev, labels_dev, ks, kt, B, B, S, scale, inv_rows, h->s_inbatch.p, d_src_dev,
                                  d_tgt_dev, row_loss_dev, row_acc_dev, st));
  return 0;
}

int sse_inbatch_loss_window_dev(sse_handle *h, const float *src_raw_dev, const float *tgt_raw_dev, const float *labels_dev,
                                const int64_t *src_key_dev, const int64_t *tgt_key_dev, int32_t B, int32_t S, int32_t row_lo,
                                int32_t row_hi, float scale, float inv_rows, float *d_src_dev, float *d_tgt_dev, float *row_loss_dev,
                                float *row_acc_dev, void *stream) {
  SSE_ENTER(h);
  if (B < 1 || S < 1) return fail(h, "sse_inbatch_loss_window_dev: B and S must be >= 1");
  if (row_lo < 0) return fail(h, "sse_inbatch_loss_window_dev: row_lo = %d is negative", row_lo);
  if (row_hi > B) return fail(h, "sse_inbatch_loss_window_dev: row_hi = %d lies behind the %d rows of the batch", row_hi, B);
  if (row_lo >= row_hi) return fail(h, "sse_inbatch_loss_window_dev: the window [%d, %d) is empty or inverted", row_lo, row_hi);
  if (!src_raw_dev || !tgt_raw_dev || !labels_dev || !row_loss_dev || !row_acc_dev)
    return fail(h, "sse_inbatch_loss_window_dev: encodings, labels, row_loss and row_acc must not be NULL");
  if ((d_src_dev == nullptr) != (d_tgt_dev == nullptr))
    return fail(h, "sse_inbatch_loss_window_dev: d_src and d_tgt must both be given, or both be NULL (forward only)");
  if (!(scale > 0.0f && scale <= 256.0f)) return fail(h, "sse_inbatch_loss_window_dev: scale must be in (0, 256]");
  if (reserve_inbatch(h, B, S)) return 1;
  hipStream_t st = (hipStream_t)stream;
  int32_t *ks = (int32_t *)h->s_inbatch_keys.p, *kt = ks + B;
  HIPCHECK(h, launch_inbatch_value_keys(src_key_dev, 64, B, ks, st));
  HIPCHECK(h, launch_inbatch_value_keys(tgt_key_dev, 64, B, kt, st));
  HIPCHECK(h, launch_inbatch_loss_window(src_raw_dev, tgt_raw_dev, labels_dev, ks, kt, B, row_lo, row_hi, row_hi - row_lo, S, scale, inv_rows,
                                         h->s_inbatch.p, d_src_dev, d_tgt_dev, row_loss_dev, row_acc_dev, st));
  return 0;
}

// the handle's scratch of one class loss call; keys: [source keys | hash words], B each
static int reserve_class(sse_handle *h, int B, int N, int S) {
  return reserve(h, h->s_class, class_loss_scratch_bytes(B, N, S)) || reserve(h, h->s_class_keys, (size_t)2 * B * sizeof(int32_t));
}

int sse_class_loss_dev(sse_handle *h, const float *src_raw_dev, const float *table_dev, const int32_t *tgt_row_dev,
                       const float *labels_dev, const int64_t *src_key_dev, int32_t B, int32_t N, int32_t S, float scale,
                       float inv_rows, float *d_src_dev, float *d_table_dev, float *row_loss_dev, float *row_acc_dev, void *stream) {
  SSE_ENTER(h);
  if (B < 1 || N < 1 || S < 1) return fail(h, "sse_class_loss_dev: B, N and S must be >= 1");
  if (!src_raw_dev || !table_dev || !tgt_row_dev || !labels_dev || !row_loss_dev || !row_acc_dev)
    return fail(h, "sse_class_loss_dev: encodings, table, target rows, labels, row_loss and row_acc must not be NULL");
  if ((d_src_dev == nullptr) != (d_table_dev == nullptr))
    return fail(h, "sse_class_loss_dev: d_src and d_table must both be given, or both be NULL (forward only)");
  if (!(scale > 0.0f && scale <= 256.0f)) return fail(h, "sse_class_loss_dev: scale must be in (0, 256]");
  if (reserve_class(h, B, N, S)) return 1;
  hipStream_t st = (hipStream_t)stream;
  int32_t *ks = (int32_t *)h->s_class_keys.p;
  HIPCHECK(h, launch_inbatch_value_keys(src_key_dev, 64, B, ks, st));
  HIPCHECK(h, launch_class_loss(src_raw_dev, table_dev, tgt_row_dev, labels_dev, ks, B, B, N, S, scale, inv_rows, h->s_class.p,
                                h->err_flag, d_src_dev, d_table_dev, row_loss_dev, row_acc_dev, st));
  return 0;
}

int sse_index_set_dev(sse_handle *h, const float *rows_dev, int64_t N, int32_t S, int64_t id_base, void *stream) {
  SSE_ENTER(h);
  if (index_shape_check(h, N, S)) return 1;
  if (h->idx64) {
    HIPCHECK(h, hipFree(h->idx64));
    h->idx64 = nullptr;
  }
  return index_from_dev_rows(h, rows_dev, N, S, id_base, (hipStream_t)stream);
}

int sse_index_upload(sse_handle *h, const float *rows_host, int64_t N, int32_t S, int64_t id_base) {
  if (!h || !rows_host) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (index_shape_check(h, N, S)) return 1;
  if (reserve(h, h->s_tmp, (size_t)N * S * sizeof(float))) return 1;
  HIPCHECK(h, hipMemcpy(h->s_tmp.p, rows_host, (size_t)N * S * sizeof(float), hipMemcpyHostToDevice));
  if (h->idx64) {
    HIPCHECK(h, hipFree(h->idx64));
    h->idx64 = nullptr;
  }
  return index_from_dev_rows(h, (const float *)h->s_tmp.p, N, S, id_base, nullptr);
}

int sse_index_upload_f64(sse_handle *h, const double *rows_host, int64_t N, int32_t S, int64_t id_base) {
  if (!h || !rows_host) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if (index_shape_check(h, N, S)) return 1;
  if (h->idx64) {
    HIPCHECK(h, hipFree(h->idx64));
    h->idx64 = nullptr;
  }
  HIPCHECK(h, hipMalloc((void **)&h->idx64, (size_t)N * S * sizeof(double)));
  h->idx64_cap = (size_t)N * S * sizeof(double);
  HIPCHECK(h, hipMemcpy(h->idx64, rows_host, (size_t)N * S * sizeof(double), hipMemcpyHostToDevice));
  if (reserve(h, h->s_tmp, (size_t)N * S * sizeof(float))) return 1;
  HIPCHECK(h, launch_f64_to_f32(h->idx64, (float *)h->s_tmp.p, N * S, nullptr));
  return index_from_dev_rows(h, (const float *)h->s_tmp.p, N, S, id_base, nullptr);
}

int sse_index_shape(sse_handle *h, int64_t *N, int32_t *S, int64_t *id_base, float *norm_max) {
  SSE_ENTER(h);
  const bool resident = h->idxp != nullptr && h->idx_N > 0;
  if (N) *N = resident ? h->idx_N : 0;
  if (S) *S = resident ? h->idx_S : 0;
  if (id_base) *id_base = resident ? h->idx_base : 0;
  if (norm_max) *norm_max = resident ? h->idx_norm_max : 0.0f;
  return 0;
}

int sse_index_update(sse_handle *h, const int64_t *ids, const float *rows, int64_t M, const uint64_t *tags, const int64_t *groups,
                     const float *bias) {
  SSE_ENTER(h);
  return index_delta_host<float>(h, "sse_index_update", false, ids, rows, M, tags, groups, bias);
}

int sse_index_update_f64(sse_handle *h, const int64_t *ids, const double *rows, int64_t M, const uint64_t *tags,
                         const int64_t *groups, const float *bias) {
  SSE_ENTER(h);
  return index_delta_host<double>(h, "sse_index_update_f64", false, ids, rows, M, tags, groups, bias);
}

int sse_index_append(sse_handle *h, const float *rows, int64_t M, const uint64_t *tags, const int64_t *groups, const float *bias) {
  SSE_ENTER(h);
  return index_delta_host<float>(h, "sse_index_append", true, nullptr, rows, M, tags, groups, bias);
}

int sse_index_append_f64(sse_handle *h, const double *rows, int64_t M, const uint64_t *tags, const int64_t *groups,
                         const float *bias) {
  SSE_ENTER(h);
  return index_delta_host<double>(h, "sse_index_append_f64", true, nullptr, rows, M, tags, groups, bias);
}

int sse_index_update_dev(sse_handle *h, const int64_t *ids_dev, const float *rows_dev, int64_t M, const uint64_t *tags_dev,
                         const int64_t *groups_dev, const float *bias_dev, void *stream) {
  SSE_ENTER(h);
  if (index_delta_check(h, "sse_index_update_dev", false, false, rows_dev != nullptr, M, tags_dev, groups_dev, bias_dev)) return 1;
  if (M > 0 && !ids_dev) return fail(h, "sse_index_update_dev: ids must not be NULL");
  IndexDelta d{"sse_index_update_dev", false, ids_dev, true, rows_dev, nullptr, M, tags_dev, groups_dev, bias_dev};
  return index_apply_delta(h, d, (hipStream_t)stream);
}

int sse_index_append_dev(sse_handle *h, const float *rows_dev, int64_t M, const uint64_t *tags_dev, const int64_t *groups_dev,
                         const float *bias_dev, void *stream) {
  SSE_ENTER(h);
  if (index_delta_check(h, "sse_index_append_dev", true, false, rows_dev != nullptr, M, tags_dev, groups_dev, bias_dev)) return 1;
  IndexDelta d{"sse_index_append_dev", true, nullptr, false, rows_dev, nullptr, M, tags_dev, groups_dev, bias_dev};
  return index_apply_delta(h, d, (hipStream_t)stream);
}

int sse_score_topk_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, double *out_scores_dev,
                       int64_t *out_ids_dev, void *stream) {
  SSE_ENTER(h);
  return score_dev_locked(h, q_dev, Q, k, out_scores_dev, out_ids_dev, (hipStream_t)stream);
}

int sse_score_topk(sse_handle *h, const float *q_host, int32_t Q, int32_t k, double *out_scores, int64_t *out_ids) {
  SSE_ENTER(h);
  if (Q == 0) return 0;
  if (Q < 0 || !q_host || !out_scores || !out_ids) return fail(h, "bad arguments to sse_score_topk");
  if (!h->idxp) return fail(h, "no index uploaded");
  const size_t S = h->idx_S;
  if (reserve(h, h->s_q, (size_t)Q * S * sizeof(float))) return 1;
  HIPCHECK(h, hipMemcpy(h->s_q.p, q_host, (size_t)Q * S * sizeof(float), hipMemcpyHostToDevice));
  return score_to_host_locked(h, (const float *)h->s_q.p, Q, k, out_scores, out_ids);
}

int sse_score_rank_dev(sse_handle *h, const float *q_dev, int32_t Q, const int32_t *pair_q_dev, const int64_t *pair_id_dev, int64_t L,
                       const double *pair_score_in_dev, int64_t *out_before_dev, double *out_score_dev, void *stream) {
  SSE_ENTER(h);
  return score_rank_dev_locked(h, q_dev, Q, pair_q_dev, pair_id_dev, L, pair_score_in_dev, out_before_dev, out_score_dev,
                               (hipStream_t)stream);
}

int sse_score_rank(sse_handle *h, const float *q_host, int32_t Q, const int32_t *pair_q, const int64_t *pair_id, int64_t L,
                   const double *pair_score_in, int64_t *out_before, double *out_score) {
  SSE_ENTER(h);
  if (!h->idxp) return fail(h, "no index uploaded");
  if (Q < 0 || L < 0) return fail(h, "bad arguments to sse_score_rank");
  if (L == 0) return 0;
  if (!q_host || !pair_q || !pair_id || !out_before || Q == 0) return fail(h, "bad arguments to sse_score_rank");
  // the host has the pairs: checked here, with the offending pair in the message, before anything is queued
  for (int64_t p = 0; p < L; ++p) {
    if (pair_q[p] < 0 || pair_q[p] >= Q) return fail(h, "sse_score_rank: pair_q[%lld] = %d is not in [0, Q = %d)", (long long)p, pair_q[p], Q);
    if (!pair_score_in && (pair_id[p] < h->idx_base || pair_id[p] >= h->idx_base + h->idx_N))
      return fail(h, "sse_score_rank: pair_id[%lld] = %lld is not a row of this index [%lld, %lld)", (long long)p, (long long)pair_id[p],
                  (long long)h->idx_base, (long long)(h->idx_base + h->idx_N));
  }
  const size_t l8 = (size_t)L * 8;
  StagePiece p[] = {{(size_t)Q * h->idx_S * sizeof(float), q_host}, {l8, pair_id}, {l8, pair_score_in}, {l8, nullptr, out_score},
                    {l8, nullptr, out_before}, {(size_t)L * 4, pair_q}};
  if (stage_in(h, p)) return 1;
  // (the scores are always computed: out_score only decides whether they come back)
  if (score_rank_dev_locked(h, p[0].as<float>(), Q, p[5].as<int32_t>(), p[1].as<int64_t>(), L, p[2].as<double>(), p[4].as<int64_t>(),
                            (double *)p[3].dev, nullptr))
    return 1;
  if (check_err_flag(h, nullptr)) return 1;
  return stage_out(h, p);
}

int sse_score_above_dev(sse_handle *h, const float *q_dev, int32_t Q, const int32_t *pair_q_dev, const double *pair_thr_dev,
                        int64_t L, int64_t cap, int64_t *out_offsets_dev, int64_t *out_ids_dev, double *out_scores_dev,
                        void *stream) {
  SSE_ENTER(h);
  hipStream_t st = (hipStream_t)stream;
  if (!h->idxp) return fail(h, "sse_score_above: no index uploaded");
  const bool lists = out_ids_dev != nullptr;
  if (Q < 0 || L < 0 || !out_offsets_dev || (out_ids_dev == nullptr) != (out_scores_dev == nullptr) || (lists && cap < 0))
    return fail(h, "bad arguments to sse_score_above");
  if (L == 0) {
    HIPCHECK(h, hipMemsetAsync(out_offsets_dev, 0, sizeof(int64_t), st));
    return 0;
  }
  if (!q_dev || !pair_q_dev || !pair_thr_dev || Q == 0) return fail(h, "bad arguments to sse_score_above");
  AboveCall c;
  if (score_above_count_locked(h, c, q_dev, Q, pair_q_dev, pair_thr_dev, L, out_offsets_dev, st)) return 1;
  if (lists && score_above_emit_locked(h, c, pair_q_dev, pair_thr_dev, L, cap, out_ids_dev, out_scores_dev, st)) return 1;
  return 0;
}

int sse_score_above(sse_handle *h, const float *q_host, int32_t Q, const int32_t *pair_q, const double *pair_thr, int64_t L,
                    int64_t cap, int64_t *out_offsets, int64_t *out_ids, double *out_scores) {
  SSE_ENTER(h);
  if (!h->idxp) return fail(h, "sse_score_above: no index uploaded");
  const bool lists = out_ids != nullptr;
  if (Q < 0 || L < 0 || !out_offsets || (out_ids == nullptr) != (out_scores == nullptr) || (lists && cap < 0))
    return fail(h, "bad arguments to sse_score_above");
  if (L == 0) {
    out_offsets[0] = 0;
    return 0;
  }
  if (!q_host || !pair_q || !pair_thr || Q == 0) return fail(h, "bad arguments to sse_score_above");
  for (int64_t p = 0; p < L; ++p)
    if (pair_q[p] < 0 || pair_q[p] >= Q) return fail(h, "sse_score_above: pair_q[%lld] = %d is not in [0, Q = %d)", (long long)p, pair_q[p], Q);
  StagePiece p[] = {{(size_t)Q * h->idx_S * sizeof(float), q_host}, {(size_t)L * 8, pair_thr}, {(size_t)L * 8 + 8, nullptr, out_offsets},
                    {(size_t)L * 4, pair_q}};
  if (stage_in(h, p)) return 1;
  const double *d_thr = p[1].as<double>();
  const int32_t *d_pq = p[3].as<int32_t>();
  AboveCall c;
  if (score_above_count_locked(h, c, p[0].as<float>(), Q, d_pq, d_thr, L, p[2].as<int64_t>(), nullptr)) return 1;
  if (check_err_flag(h, nullptr)) return 1;
  if (stage_out(h, p)) return 1;
  // the host knows the total now: the lists are staged at exactly that length, and skipped when the caller's do not hold it
  const int64_t total = out_offsets[L];
  if (!lists || total > cap || total == 0) return 0;
  if (reserve(h, h->s_ab_out, (size_t)total * 16)) return 1;
  int64_t *d_ids = (int64_t *)h->s_ab_out.p;
  double *d_sc = (double *)((char *)h->s_ab_out.p + (size_t)total * 8);
  if (score_above_emit_locked(h, c, d_pq, d_thr, L, total, d_ids, d_sc, nullptr)) return 1;
  if (check_err_flag(h, nullptr)) return 1;
  HIPCHECK(h, hipMemcpy(out_ids, d_ids, (size_t)total * 8, hipMemcpyDeviceToHost));
  HIPCHECK(h, hipMemcpy(out_scores, d_sc, (size_t)total * 8, hipMemcpyDeviceToHost));
  return 0;
}

int sse_index_set_tags(sse_handle *h, const uint64_t *tags_host, int64_t N) {
  SSE_ENTER(h);
  if (index_set_tags_locked(h, tags_host, N, true, nullptr)) return 1;
  HIPCHECK(h, hipStreamSynchronize(nullptr));
  return 0;
}

int sse_index_set_tags_dev(sse_handle *h, const uint64_t *tags_dev, int64_t N, void *stream) {
  SSE_ENTER(h);
  return index_set_tags_locked(h, tags_dev, N, false, (hipStream_t)stream);
}

int sse_score_topk_filtered_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const uint64_t *q_any_dev,
                                const uint64_t *q_none_dev, const int64_t *excl_ids_dev, int32_t n_excl,
                                double *out_scores_dev, int64_t *out_ids_dev, int32_t *out_counts_dev, void *stream) {
  SSE_ENTER(h);
  if (score_topk_check(h, CALL_FILTERED, Q, k, q_any_dev, q_none_dev, excl_ids_dev, n_excl)) return 1;
  if (Q == 0) return 0;
  if (!q_dev || !out_scores_dev || !out_ids_dev || !out_counts_dev) return fail(h, "bad arguments to sse_score_topk_filtered");
  const TopkIo io{q_dev, q_any_dev, q_none_dev, out_scores_dev, out_ids_dev, out_counts_dev};
  return score_filtered_dev_locked(h, io, Q, k, excl_ids_dev, n_excl, (hipStream_t)stream);
}

int sse_score_topk_filtered(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const uint64_t *q_any,
                            const uint64_t *q_none, const int64_t *excl_ids, int32_t n_excl, double *out_scores,
                            int64_t *out_ids, int32_t *out_counts) {
  SSE_ENTER(h);
  if (score_topk_check(h, CALL_FILTERED, Q, k, q_any, q_none, excl_ids, n_excl)) return 1;
  if (Q == 0) return 0;
  if (!q_host || !out_scores || !out_ids || !out_counts) return fail(h, "bad arguments to sse_score_topk_filtered");
  const size_t o8 = (size_t)Q * k * 8, m8 = (size_t)Q * 8;
  StagePiece p[] = {{o8, nullptr, out_scores}, {o8, nullptr, out_ids}, {m8, q_any}, {m8, q_none}, {m8 * n_excl, n_excl > 0 ? excl_ids : nullptr},
                    {(size_t)Q * h->idx_S * sizeof(float), q_host}, {(size_t)Q * 4, nullptr, out_counts}};
  if (stage_in(h, p)) return 1;
  const TopkIo io{p[5].as<float>(), p[2].as<uint64_t>(), p[3].as<uint64_t>(), p[0].as<double>(), p[1].as<int64_t>(), p[6].as<int32_t>()};
  if (score_filtered_dev_locked(h, io, Q, k, p[4].as<int64_t>(), n_excl, nullptr)) return 1;
  HIPCHECK(h, sync_stream(nullptr));
  return stage_out(h, p);
}

int sse_index_set_groups(sse_handle *h, const int64_t *groups_host, int64_t N) {
  SSE_ENTER(h);
  if (index_set_groups_locked(h, groups_host, N, true, nullptr)) return 1;
  HIPCHECK(h, hipStreamSynchronize(nullptr));
  return 0;
}

int sse_index_set_groups_dev(sse_handle *h, const int64_t *groups_dev, int64_t N, void *stream) {
  SSE_ENTER(h);
  return index_set_groups_locked(h, groups_dev, N, false, (hipStream_t)stream);
}

int sse_score_topk_grouped_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const uint64_t *q_any_dev,
                               const uint64_t *q_none_dev, double *out_scores_dev, int64_t *out_ids_dev,
                               int64_t *out_groups_dev, int32_t *out_counts_dev, void *stream) {
  SSE_ENTER(h);
  if (score_topk_check(h, CALL_GROUPED, Q, k, q_any_dev, q_none_dev)) return 1;
  if (Q == 0) return 0;
  if (!q_dev || !out_scores_dev || !out_ids_dev || !out_groups_dev || !out_counts_dev) return fail(h, "bad arguments to sse_score_topk_grouped");
  const TopkIo io{q_dev, q_any_dev, q_none_dev, out_scores_dev, out_ids_dev, out_counts_dev};
  return score_grouped_dev_locked(h, io, Q, k, out_groups_dev, (hipStream_t)stream);
}

int sse_score_topk_grouped(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const uint64_t *q_any,
                           const uint64_t *q_none, double *out_scores, int64_t *out_ids, int64_t *out_groups,
                           int32_t *out_counts) {
  SSE_ENTER(h);
  if (score_topk_check(h, CALL_GROUPED, Q, k, q_any, q_none)) return 1;
  if (Q == 0) return 0;
  if (!q_host || !out_scores || !out_ids || !out_groups || !out_counts) return fail(h, "bad arguments to sse_score_topk_grouped");
  const size_t o8 = (size_t)Q * k * 8, m8 = (size_t)Q * 8;
  StagePiece p[] = {{o8, nullptr, out_scores}, {o8, nullptr, out_ids}, {o8, nullptr, out_groups}, {m8, q_any}, {m8, q_none},
                    {(size_t)Q * h->idx_S * sizeof(float), q_host}, {(size_t)Q * 4, nullptr, out_counts}};
  if (stage_in(h, p)) return 1;
  const TopkIo io{p[5].as<float>(), p[3].as<uint64_t>(), p[4].as<uint64_t>(), p[0].as<double>(), p[1].as<int64_t>(), p[6].as<int32_t>()};
  if (score_grouped_dev_locked(h, io, Q, k, p[2].as<int64_t>(), nullptr)) return 1;
  HIPCHECK(h, sync_stream(nullptr));
  return stage_out(h, p);
}

int sse_score_topk_after_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const double *after_score_dev,
                             const int64_t *after_id_dev, const uint64_t *q_any_dev, const uint64_t *q_none_dev,
                             double *out_scores_dev, int64_t *out_ids_dev, int32_t *out_counts_dev, void *stream) {
  SSE_ENTER(h);
  if (score_topk_check(h, CALL_AFTER, Q, k, q_any_dev, q_none_dev, nullptr, 0, after_score_dev, after_id_dev)) return 1;
  if (Q == 0) return 0;
  if (!q_dev || !out_scores_dev || !out_ids_dev || !out_counts_dev) return fail(h, "bad arguments to sse_score_topk_after");
  const TopkIo io{q_dev, q_any_dev, q_none_dev, out_scores_dev, out_ids_dev, out_counts_dev};
  return score_after_dev_locked(h, io, Q, k, after_score_dev, after_id_dev, (hipStream_t)stream);
}

int sse_score_topk_after(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const double *after_score,
                         const int64_t *after_id, const uint64_t *q_any, const uint64_t *q_none, double *out_scores,
                         int64_t *out_ids, int32_t *out_counts) {
  SSE_ENTER(h);
  if (score_topk_check(h, CALL_AFTER, Q, k, q_any, q_none, nullptr, 0, after_score, after_id)) return 1;
  if (Q == 0) return 0;
  if (!q_host || !out_scores || !out_ids || !out_counts) return fail(h, "bad arguments to sse_score_topk_after");
  const size_t o8 = (size_t)Q * k * 8, m8 = (size_t)Q * 8;
  StagePiece p[] = {{o8, nullptr, out_scores}, {o8, nullptr, out_ids}, {m8, after_score}, {m8, after_id}, {m8, q_any}, {m8, q_none},
                    {(size_t)Q * h->idx_S * sizeof(float), q_host}, {(size_t)Q * 4, nullptr, out_counts}};
  if (stage_in(h, p)) return 1;
  const TopkIo io{p[6].as<float>(), p[4].as<uint64_t>(), p[5].as<uint64_t>(), p[0].as<double>(), p[1].as<int64_t>(), p[7].as<int32_t>()};
  if (score_after_dev_locked(h, io, Q, k, p[2].as<double>(), p[3].as<int64_t>(), nullptr)) return 1;
  HIPCHECK(h, sync_stream(nullptr));
  return stage_out(h, p);
}

int sse_index_set_bias(sse_handle *h, const float *bias_host, int64_t N) {
  SSE_ENTER(h);
  if (index_set_bias_locked(h, bias_host, N, true, nullptr)) return 1;
  HIPCHECK(h, hipStreamSynchronize(nullptr));
  return 0;
}

int sse_index_set_bias_dev(sse_handle *h, const float *bias_dev, int64_t N, void *stream) {
  SSE_ENTER(h);
  return index_set_bias_locked(h, bias_dev, N, false, (hipStream_t)stream);
}

int sse_score_topk_biased_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const float *q_weight_dev,
                              const uint64_t *q_any_dev, const uint64_t *q_none_dev, double *out_scores_dev,
                              int64_t *out_ids_dev, int32_t *out_counts_dev, void *stream) {
  SSE_ENTER(h);
  if (score_biased_check(h, Q, k, q_any_dev, q_none_dev)) return 1;
  if (Q == 0) return 0;
  if (!q_dev || !out_scores_dev || !out_ids_dev || !out_counts_dev) return fail(h, "bad arguments to sse_score_topk_biased");
  const TopkIo io{q_dev, q_any_dev, q_none_dev, out_scores_dev, out_ids_dev, out_counts_dev};
  return score_biased_dev_locked(h, io, Q, k, q_weight_dev, (hipStream_t)stream);
}

int sse_score_topk_biased(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const float *q_weight, const uint64_t *q_any,
                          const uint64_t *q_none, double *out_scores, int64_t *out_ids, int32_t *out_counts) {
  SSE_ENTER(h);
  if (score_biased_check(h, Q, k, q_any, q_none)) return 1;
  if (Q == 0) return 0;
  if (!q_host || !out_scores || !out_ids || !out_counts) return fail(h, "bad arguments to sse_score_topk_biased");
  const size_t o8 = (size_t)Q * k * 8, m8 = (size_t)Q * 8;
  StagePiece p[] = {{o8, nullptr, out_scores}, {o8, nullptr, out_ids}, {m8, q_any}, {m8, q_none}, {(size_t)Q * sizeof(float), q_weight},
                    {(size_t)Q * h->idx_S * sizeof(float), q_host}, {(size_t)Q * 4, nullptr, out_counts}};
  if (stage_in(h, p)) return 1;
  const TopkIo io{p[5].as<float>(), p[2].as<uint64_t>(), p[3].as<uint64_t>(), p[0].as<double>(), p[1].as<int64_t>(), p[6].as<int32_t>()};
  if (score_biased_dev_locked(h, io, Q, k, p[4].as<float>(), nullptr)) return 1;
  HIPCHECK(h, sync_stream(nullptr));
  return stage_out(h, p);
}

int sse_score_lse_dev(sse_handle *h, const float *q_dev, int32_t Q, float scale, const float *q_weight_dev, const uint64_t *q_any_dev,
                      const uint64_t *q_none_dev, double *out_lse_dev, int64_t *out_count_dev, double *out_bound_dev, void *stream) {
  SSE_ENTER(h);
  if (score_lse_check(h, Q, scale, q_weight_dev, q_any_dev, q_none_dev)) return 1;
  if (Q == 0) return 0;
  if (!q_dev || !out_lse_dev || !out_count_dev) return fail(h, "bad arguments to sse_score_lse");
  return score_lse_dev_locked(h, q_dev, Q, scale, q_weight_dev, q_any_dev, q_none_dev, out_lse_dev, out_count_dev, out_bound_dev,
                              (hipStream_t)stream);
}

int sse_score_lse(sse_handle *h, const float *q_host, int32_t Q, float scale, const float *q_weight, const uint64_t *q_any,
                  const uint64_t *q_none, double *out_lse, int64_t *out_count, double *out_bound) {
  SSE_ENTER(h);
  if (score_lse_check(h, Q, scale, q_weight, q_any, q_none)) return 1;
  if (Q == 0) return 0;
  if (!q_host || !out_lse || !out_count) return fail(h, "bad arguments to sse_score_lse");
  const size_t m8 = (size_t)Q * 8;
  StagePiece p[] = {{m8, nullptr, out_lse}, {m8, nullptr, out_count}, {m8, nullptr, out_bound}, {m8, q_any}, {m8, q_none},
                    {(size_t)Q * sizeof(float), q_weight}, {(size_t)Q * h->idx_S * sizeof(float), q_host}};
  if (stage_in(h, p)) return 1;
  if (score_lse_dev_locked(h, p[6].as<float>(), Q, scale, p[5].as<float>(), p[3].as<uint64_t>(), p[4].as<uint64_t>(), p[0].as<double>(),
                           p[1].as<int64_t>(), p[2].as<double>(), nullptr))
    return 1;
  HIPCHECK(h, sync_stream(nullptr));
  return stage_out(h, p);
}

int sse_score_confusions_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const int64_t *pos_ids_dev, int32_t n_pos,
                             double margin, double *out_scores_dev, int64_t *out_ids_dev, int32_t *out_counts_dev,
                             double *out_pos_score_dev, int64_t *out_pos_id_dev, void *stream) {
  SSE_ENTER(h);
  if (score_confusions_check(h, Q, k, pos_ids_dev, n_pos, margin)) return 1;
  if (Q == 0) return 0;
  if (!q_dev || !out_scores_dev || !out_ids_dev || !out_counts_dev) return fail(h, "bad arguments to sse_score_confusions");
  const TopkIo io{q_dev, nullptr, nullptr, out_scores_dev, out_ids_dev, out_counts_dev};
  return score_confusions_dev_locked(h, io, Q, k, pos_ids_dev, n_pos, margin, out_pos_score_dev, out_pos_id_dev, (hipStream_t)stream);
}

int sse_score_confusions(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const int64_t *pos_ids, int32_t n_pos,
                         double margin, double *out_scores, int64_t *out_ids, int32_t *out_counts, double *out_pos_score,
                         int64_t *out_pos_id) {
  SSE_ENTER(h);
  if (score_confusions_check(h, Q, k, pos_ids, n_pos, margin)) return 1;
  if (Q == 0) return 0;
  if (!q_host || !out_scores || !out_ids || !out_counts) return fail(h, "bad arguments to sse_score_confusions");
  const size_t o8 = (size_t)Q * k * 8, m8 = (size_t)Q * 8;
  StagePiece p[] = {{o8, nullptr, out_scores}, {o8, nullptr, out_ids}, {m8, nullptr, out_pos_score}, {m8, nullptr, out_pos_id},
                    {m8 * n_pos, pos_ids}, {(size_t)Q * h->idx_S * sizeof(float), q_host}, {(size_t)Q * 4, nullptr, out_counts}};
  if (stage_in(h, p)) return 1;
  const TopkIo io{p[5].as<float>(), nullptr, nullptr, p[0].as<double>(), p[1].as<int64_t>(), p[6].as<int32_t>()};
  if (score_confusions_dev_locked(h, io, Q, k, p[4].as<int64_t>(), n_pos, margin, p[2].as<double>(), p[3].as<int64_t>(), nullptr)) return 1;
  HIPCHECK(h, sync_stream(nullptr));
  return stage_out(h, p);
}

int sse_merge_topk_strided_dev(sse_handle *h, const double *in_scores_dev, const int64_t *in_ids_dev, int64_t shard_stride,
                               int32_t P, int32_t Q, int32_t k, double *out_scores_dev, int64_t *out_ids_dev, void *stream) {
  SSE_ENTER(h);
  if (P < 1 || Q < 0 || k < 1 || shard_stride < (int64_t)Q * k) return fail(h, "bad arguments to sse_merge_topk_dev");
  if (Q == 0) return 0;
  HIPCHECK(h, launch_merge_topk(in_scores_dev, in_ids_dev, shard_stride, P, Q, k, out_scores_dev, out_ids_dev, (hipStream_t)stream));
  return 0;
}

int sse_merge_topk_dev(sse_handle *h, const double *in_scores_dev, const int64_t *in_ids_dev, int32_t P, int32_t Q,
                       int32_t k, double *out_scores_dev, int64_t *out_ids_dev, void *stream) {
  return sse_merge_topk_strided_dev(h, in_scores_dev, in_ids_dev, (int64_t)Q * k, P, Q, k, out_scores_dev, out_ids_dev, stream);
}

// ---------------------------------------------------------------------------
// Torch-free exchange step of the row-sharded index (BASELINE configs[3]): RCCL straight from the C ABI.
// The library does not LINK librccl: the few entry points it needs are bound at first use, ALL from ONE library instance
// (a per-symbol dlsym(RTLD_DEFAULT) misses an RCCL the host loaded RTLD_LOCAL -- the Python default, torch's
// bundled copy -- and a second instance opened beside it would be handed the first one's ncclComm_t).  Order:
//   1. $SSE_RCCL_LIB, when set: that file (the host names its RCCL explicitly);
//   2. an RCCL already mapped into the process (dl_iterate_phdr, any visibility): dlopen(its path, RTLD_NOLOAD) returns THAT
//      instance, so a communicator the host created with it and this library's ncclAllGather agree;
//   3. librccl.so.1 / librccl.so from the loader path.
// sse_rccl_library_path() reports the choice.  libsse_hip.so still loads on a box without RCCL; every other entry point works.
namespace {
typedef struct { char internal[128]; } sse_nccl_uid;  // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value
struct RcclApi {
  int (*get_unique_id)(sse_nccl_uid *) = nullptr;
  int (*comm_init_rank)(void **, int, sse_nccl_uid, int) = nullptr;
  int (*comm_destroy)(void *) = nullptr;
  int (*all_gather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
  const char *(*error_string)(int) = nullptr;
  const char *why = nullptr;
  std::string path;  // the library instance everything above came from
};
int find_mapped_rccl(struct dl_phdr_info *info, size_t, void *data) {
  const char *name = info->dlpi_name;
  if (!name || !*name) return 0;
  const char *base = strrchr(name, '/');
  base = base ? base + 1 : name;
  if (strncmp(base, "librccl.so", 10) != 0) return 0;
  *static_cast<std::string *>(data) = name;
  return 1;  // first match: stop
}
const RcclApi *rccl_api_ptr() {
  static const RcclApi api = [] {
    RcclApi a;
    void *lib = nullptr;
    if (const char *env = getenv("SSE_RCCL_LIB")) {
      if (*env) {
        lib = dlopen(env, RTLD_NOW | RTLD_LOCAL);
        if (!lib) {
          a.why = "SSE_RCCL_LIB is set but that file does not load as a library";
          return a;
        }
        a.path = env;
      }
    }
    if (!lib) {
      std::string mapped;
      dl_iterate_phdr(find_mapped_rccl, &mapped);
      if (!mapped.empty() && (lib = dlopen(mapped.c_str(), RTLD_NOW | RTLD_NOLOAD)) != nullptr) a.path = mapped;
    }
    for (const char *cand : {"librccl.so.1", "librccl.so"}) {
      if (lib) break;
      if ((lib = dlopen(cand, RTLD_NOW | RTLD_LOCAL)) != nullptr) a.path = cand;
    }
    if (!lib) {
      a.why = "RCCL (librccl.so.1) is not loadable in this process";
      return a;
    }
    a.get_unique_id = reinterpret_cast<int (*)(sse_nccl_uid *)>(dlsym(lib, "ncclGetUniqueId"));
    a.comm_init_rank = reinterpret_cast<int (*)(void **, int, sse_nccl_uid, int)>(dlsym(lib, "ncclCommInitRank"));
    a.comm_destroy = reinterpret_cast<int (*)(void *)>(dlsym(lib, "ncclCommDestroy"));
    a.all_gather = reinterpret_cast<int (*)(const void *, void *, size_t, int, void *, hipStream_t)>(dlsym(lib, "ncclAllGather"));
    a.group_start = reinterpret_cast<int (*)()>(dlsym(lib, "ncclGroupStart"));
    a.group_end = reinterpret_cast<int (*)()>(dlsym(lib, "ncclGroupEnd"));
    a.error_string = reinterpret_cast<const char *(*)(int)>(dlsym(lib, "ncclGetErrorString"));
    if (!a.get_unique_id || !a.comm_init_rank || !a.comm_destroy || !a.all_gather || !a.group_start || !a.group_end)
      a.why = "the RCCL library found in this process lacks an entry point this library binds";
    return a;
  }();
  return &api;
}
constexpr int SSE_NCCL_INT64 = 4;  // ncclInt64 (rccl.h: ncclDataType_t)
int rccl_fail(sse_handle *h, const char *what, int rc) {
  const RcclApi &r = *rccl_api_ptr();
  return fail(h, "%s: RCCL error %d (%s)", what, rc, r.error_string ? r.error_string(rc) : "?");
}
}  // namespace

const char *sse_rccl_library_path(void) {
  const RcclApi &r = *rccl_api_ptr();
  return r.why ? nullptr : r.path.c_str();
}

/* ncclGroupStart / ncclGroupEnd of the bound RCCL: ONE thread that drives several handles (one per GPU) must bracket its
 * sse_rccl_comm_init_rank calls with these, or the first (blocking) call waits for ranks that the thread has not reached yet. */
int sse_rccl_group_start(void) {
  const RcclApi &r = *rccl_api_ptr();
  return r.why ? 1 : (r.group_start() != 0);
}
int sse_rccl_group_end(void) {
  const RcclApi &r = *rccl_api_ptr();
  return r.why ? 1 : (r.group_end() != 0);
}

int sse_rccl_get_unique_id(char *id128) {
  const RcclApi &r = *rccl_api_ptr();
  if (!id128 || r.why) return 1;
  sse_nccl_uid u;
  if (r.get_unique_id(&u) != 0) return 1;
  memcpy(id128, u.internal, sizeof u.internal);
  return 0;
}

int sse_rccl_comm_init_rank(sse_handle *h, void **comm, int32_t world, int32_t rank, const char *id128) {
  if (!h) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  const RcclApi &r = *rccl_api_ptr();
  if (r.why) return fail(h, "%s", r.why);
  if (!comm || !id128 || world < 1 || rank < 0 || rank >= world) return fail(h, "bad arguments to sse_rccl_comm_init_rank");
  HIPCHECK(h, hipSetDevice(h->cfg.device));  // the communicator binds the calling thread's current device
  sse_nccl_uid u;
  memcpy(u.internal, id128, sizeof u.internal);
  const int rc = r.comm_init_rank(comm, world, u, rank);
  return rc == 0 ? 0 : rccl_fail(h, "ncclCommInitRank", rc);
}

int sse_rccl_comm_destroy(sse_handle *h, void *comm) {
  if (!h) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  const RcclApi &r = *rccl_api_ptr();
  if (r.why) return fail(h, "%s", r.why);
  if (!comm) return 0;
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  const int rc = r.comm_destroy(comm);
  return rc == 0 ? 0 : rccl_fail(h, "ncclCommDestroy", rc);
}

// gather + merge of lists that are already on the device; the handle mutex is held by the caller
static int allgather_merge_locked(sse_handle *h, void *comm, int world, const double *loc_s, const int64_t *loc_i, int Q, int k,
                                  double *out_s, int64_t *out_i, hipStream_t st) {
  const RcclApi &r = *rccl_api_ptr();
  if (r.why) return fail(h, "%s", r.why);
  const size_t n = (size_t)Q * k;  // 64-bit words per list
  // exchange buffer: [ this rank's (scores | ids) : 2n words ][ gathered, rank-major: world x 2n words ]
  if (reserve(h, h->s_xchg, (size_t)(world + 1) * 2 * n * 8)) return 1;
  int64_t *loc = (int64_t *)h->s_xchg.p, *all = loc + 2 * n;
  HIPCHECK(h, hipMemcpyAsync(loc, loc_s, n * 8, hipMemcpyDeviceToDevice, st));  // (float64 scores travel as their bit patterns)
  HIPCHECK(h, hipMemcpyAsync(loc + n, loc_i, n * 8, hipMemcpyDeviceToDevice, st));
  const int rc = r.all_gather(loc, all, 2 * n, SSE_NCCL_INT64, comm, st);  // ONE collective for scores and ids
  if (rc != 0) return rccl_fail(h, "ncclAllGather", rc);
  HIPCHECK(h, launch_merge_topk((const double *)all, all + n, (int64_t)(2 * n), world, Q, k, out_s, out_i, st));
  return 0;
}

int sse_allgather_merge_topk_dev(sse_handle *h, void *nccl_comm, int32_t world, const double *local_scores_dev,
                                 const int64_t *local_ids_dev, int32_t Q, int32_t k, double *out_scores_dev, int64_t *out_ids_dev,
                                 void *stream) {
  SSE_ENTER(h);
  if (!nccl_comm || world < 1 || Q < 0 || k < 1 || !local_scores_dev || !local_ids_dev || !out_scores_dev || !out_ids_dev)
    return fail(h, "bad arguments to sse_allgather_merge_topk_dev");
  if (Q == 0) return 0;
  return allgather_merge_locked(h, nccl_comm, world, local_scores_dev, local_ids_dev, Q, k, out_scores_dev, out_ids_dev, (hipStream_t)stream);
}

int sse_score_topk_sharded_dev(sse_handle *h, void *nccl_comm, int32_t world, const float *q_dev, int32_t Q, int32_t k,
                               double *out_scores_dev, int64_t *out_ids_dev, void *stream) {
  SSE_ENTER(h);
  if (!nccl_comm || world < 1 || Q < 0 || k < 1 || !q_dev || !out_scores_dev || !out_ids_dev)
    return fail(h, "bad arguments to sse_score_topk_sharded_dev");
  if (Q == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  // this shard's lists go to the out buffers first (global row ids: id_base of sse_index_set_dev), the merged lists overwrite them
  if (score_dev_locked(h, q_dev, Q, k, out_scores_dev, out_ids_dev, st)) return 1;
  return allgather_merge_locked(h, nccl_comm, world, out_scores_dev, out_ids_dev, Q, k, out_scores_dev, out_ids_dev, st);
}

static int64_t grad_arena_count(sse_handle *h) {
  int64_t n = 4;
  for (auto &v : h->vars) n += v.count;
  return n;
}

static void bind_arena(sse_handle *h, float *p, bool external) {
  TrainState &ts = *h->train;
  ts.arena = p;
  ts.arena_external = external;
  ts.grads_ready = false;
  int64_t off = 0;
  for (auto &v : h->vars) {
    v.grad = p + off;
    off += v.count;
  }
}

int sse_train_grad_count(sse_handle *h, int64_t *count) {
  if (!h || !count) return 1;
  *count = grad_arena_count(h);
  return 0;
}

int sse_train_set_grad_arena(sse_handle *h, float *arena_dev, int64_t count) {
  SSE_ENTER(h);
  if (!h->train) h->train = new TrainState();
  TrainState &ts = *h->train;
  if (arena_dev && count != grad_arena_count(h))
    return fail(h, "gradient arena holds %lld floats, the model needs %lld", (long long)count, (long long)grad_arena_count(h));
  HIPCHECK(h, hipDeviceSynchronize());
  if (ts.arena && !ts.arena_external) HIPCHECK(h, hipFree(ts.arena));
  ts.arena = nullptr;
  if (arena_dev) {
    bind_arena(h, arena_dev, true);
  } else {
    for (auto &v : h->vars) v.grad = nullptr;
    ts.arena_external = false;
    ts.grads_ready = false;
  }
  return 0;
}

static int ensure_arena(sse_handle *h) {
  TrainState &ts = *h->train;
  if (!ts.arena) {
    float *p = nullptr;
    HIPCHECK(h, hipMalloc((void **)&p, grad_arena_count(h) * sizeof(float)));
    bind_arena(h, p, false);
  }
  ts.grads_ready = false;
  return 0;
}

// token ids of one side of the batch into ts.ids[side] ([B][T] on the device): copied from the host, or -- by_rows --
// gathered on the device from the resident corpus by B row numbers (B ints cross PCIe instead of B*T)
// perm (host, [B], or nullptr): internal row r holds the caller's row perm[r].
static int stage_ids(sse_handle *h, TrainState &ts, int side, const int32_t *host, int B, int T, bool by_rows, const int32_t *perm,
                     hipStream_t st) {
  if (reserve(h, ts.ids[side], (size_t)B * T * sizeof(int32_t))) return 1;
  if (!by_rows) {
    if (!perm) {
      HIPCHECK(h, hipMemcpyAsync(ts.ids[side].p, host, (size_t)B * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
      return 0;
    }
    // the batch as handed over is the "corpus", the permutation the row numbers (ts.perm is uploaded by the caller)
    if (reserve(h, ts.ids_raw[side], (size_t)B * T * sizeof(int32_t))) return 1;
    HIPCHECK(h, hipMemcpyAsync(ts.ids_raw[side].p, host, (size_t)B * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHECK(h, launch_gather_id_rows((const int32_t *)ts.ids_raw[side].p, (const int32_t *)ts.perm.p, B, T, B,
                                      (int32_t *)ts.ids[side].p, h->err_flag, st));
    return 0;
  }
  if (!ts.corpus[side].p || ts.corpus_T[side] != T)
    return fail(h, "train step by rows: no %s corpus with T = %d on the device (sse_corpus_upload)", side ? "target" : "source", T);
  if (reserve(h, ts.rows[side], (size_t)B * sizeof(int32_t))) return 1;
  if (perm) {
    ts.h_rows[side].resize(B);
    for (int r = 0; r < B; ++r) ts.h_rows[side][r] = host[perm[r]];
    host = ts.h_rows[side].data();
  }
  HIPCHECK(h, hipMemcpyAsync(ts.rows[side].p, host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHECK(h, launch_gather_id_rows((const int32_t *)ts.corpus[side].p, (const int32_t *)ts.rows[side].p, B, T,
                                    ts.corpus_N[side], (int32_t *)ts.ids[side].p, h->err_flag, st));
  return 0;
}

// ---- the step frame.  Every path reads: begin -> stage inputs -> its forward -> loss -> its backward -> finish, with the
// free target matrix's gather / scatter where the path has always queued them.

// arena, tail, shapes.  row_tile: 64 (text-CNN, fused LSTM) or 32 (any-shape LSTM).  The caller has checked the arguments.
static int step_begin(sse_handle *h, const TrainCall &call, int row_tile, StepFrame &f) {
  if (ensure_arena(h)) return 1;
  f.h = h;  f.call = &call;  f.ts = h->train;  f.st = h->stream;
  f.B = call.B;  f.T = call.T;  f.S = h->cfg.encoding_size;  f.Bp = round_up(call.B, row_tile);
  // source-encoder-only (BUILDER-DEFINED like the CNN mode: the reference's loss is ill-shaped there,
  // sse_model.py:233,290): LSTM source encoder, target side = embedding_lookup(tgt_seq_embedding, rows);
  // call.tgt is int32 [B] rows of the free target matrix.
  f.table_tgt = h->cfg.network_mode == SSE_MODE_SOURCE_ENCODER_ONLY || h->cfg.network_mode == SSE_MODE_SOURCE_ONLY_CNN;
  f.nside = f.table_tgt ? 1 : 2;
  f.emb = &h->vars[0];
  f.table = f.table_tgt ? &h->vars[h->tgt_table] : nullptr;
  f.tail = f.ts->arena + grad_arena_count(h) - 4;
  f.inv_rows = 1.0f / (float)call.rows_global;
  f.n_sq = 0;
  f.class_loss = h->train_class_loss != 0 && call.phase == STEP_WHOLE;  // (an open step takes its objective from the closing call)
  return 0;
}

// both id sides and the labels onto the device, in the internal row order (perm: see pair_permutation; nullptr = the
// caller's), and the buffers every path fills: raw[] / draw[] encodings, per-row loss / accuracy, the n_sq partial sums
static int step_stage_inputs(StepFrame &f, const int32_t *perm, int n_sq) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  const TrainCall &call = *f.call;
  const int B = f.B;
  f.n_sq = n_sq;
  if (stage_ids(h, ts, 0, call.src, B, f.T, call.by_rows, perm, f.st)) return 1;
  if (f.table_tgt) {  // rows of the free target matrix
    if (reserve(h, ts.ids[1], (size_t)B * sizeof(int32_t))) return 1;
    const int32_t *rows = call.tgt;
    if (perm) {
      ts.h_tgt.resize(B);
      for (int r = 0; r < B; ++r) ts.h_tgt[r] = rows[perm[r]];
      rows = ts.h_tgt.data();
    }
    HIPCHECK(h, hipMemcpyAsync(ts.ids[1].p, rows, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, f.st));
  } else if (stage_ids(h, ts, 1, call.tgt, B, f.T, call.by_rows, perm, f.st)) {
    return 1;
  }
  const float *labels = call.labels;
  if (perm) {
    ts.h_labels.resize(B);
    for (int r = 0; r < B; ++r) ts.h_labels[r] = labels[perm[r]];
    labels = ts.h_labels.data();
  }
  if (reserve(h, ts.labels, (size_t)B * sizeof(float))) return 1;
  HIPCHECK(h, hipMemcpyAsync(ts.labels.p, labels, (size_t)B * sizeof(float), hipMemcpyHostToDevice, f.st));
  for (int s = 0; s < 2; ++s) {
    if (reserve(h, ts.raw[s], (size_t)f.Bp * f.S * sizeof(float))) return 1;
    if (reserve(h, ts.draw[s], (size_t)f.Bp * f.S * sizeof(float))) return 1;
  }
  if (reserve(h, ts.row_loss, (size_t)B * sizeof(float))) return 1;
  if (reserve(h, ts.row_acc, (size_t)B * sizeof(float))) return 1;
  return reserve(h, ts.sq_part, (size_t)n_sq * sizeof(float));
}

// table target: raw[1] = the batch's rows of the free matrix (the class loss reads the whole matrix instead)
static int step_table_forward(StepFrame &f) {
  if (!f.table_tgt || f.class_loss) return 0;
  HIPCHECK(f.h, launch_rows_gather(f.table->dev, f.ids(1), f.B, f.Bp, f.table->rows, f.S, f.raw(1), f.h->err_flag, f.st));
  return 0;
}

// option train_loss = 1: the in-batch softmax head over this step's rows.  The keys come from what the step staged, in its
// internal row order: a row's source key is the first row with the same source tokens; its target key the first row with
// the same target tokens, or -- table target -- the row of the free target matrix itself.
static int step_loss_inbatch(StepFrame &f) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  if (reserve_inbatch(h, f.B, f.S)) return 1;
  int32_t *ks = (int32_t *)h->s_inbatch_keys.p, *kt = ks + f.B;
  uint32_t *hash = (uint32_t *)(kt + f.B);
  HIPCHECK(h, launch_inbatch_token_keys(f.ids(0), f.B, f.T, hash, ks, f.st));
  if (f.table_tgt)
    HIPCHECK(h, launch_inbatch_value_keys(f.ids(1), 32, f.B, kt, f.st));
  else
    HIPCHECK(h, launch_inbatch_token_keys(f.ids(1), f.B, f.T, hash, kt, f.st));
  HIPCHECK(h, launch_inbatch_loss(f.raw(0), f.raw(1), (const float *)ts.labels.p, ks, kt, f.B, f.Bp, f.S, (float)h->train_loss_scale,
                                  f.inv_rows, h->s_inbatch.p, f.draw(0), f.draw(1), (float *)ts.row_loss.p, (float *)ts.row_acc.p, f.st));
  HIPCHECK(h, launch_loss_reduce((const float *)ts.row_loss.p, (const float *)ts.row_acc.p, f.B, f.inv_rows, f.tail + 1, f.st));
  h->train_inbatch_steps += 1;
  return 0;
}

// option train_class_loss = 1: the class softmax head over raw[0] and the WHOLE free target matrix.  A row's source key is the
// first row with the same source tokens (as step_loss_inbatch forms it); d(table) goes straight into the matrix's arena block,
// every row of it, so nothing is zeroed or scattered there.  A target row out of range raises the error flag in the head.
static int step_loss_class(StepFrame &f) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  if (reserve_class(h, f.B, f.table->rows, f.S)) return 1;
  int32_t *ks = (int32_t *)h->s_class_keys.p;
  uint32_t *hash = (uint32_t *)(ks + f.B);
  HIPCHECK(h, launch_inbatch_token_keys(f.ids(0), f.B, f.T, hash, ks, f.st));
  HIPCHECK(h, launch_class_loss(f.raw(0), f.table->dev, f.ids(1), (const float *)ts.labels.p, ks, f.B, f.Bp, f.table->rows, f.S,
                                (float)h->train_loss_scale, f.inv_rows, h->s_class.p, h->err_flag, f.draw(0), f.table->grad,
                                (float *)ts.row_loss.p, (float *)ts.row_acc.p, f.st));
  HIPCHECK(h, launch_loss_reduce((const float *)ts.row_loss.p, (const float *)ts.row_acc.p, f.B, f.inv_rows, f.tail + 1, f.st));
  h->train_class_steps += 1;
  return 0;
}

// loss, train accuracy, d(raw encodings); then the two lookup tables' gradients zeroed for the scatters of the backward
static int step_loss(StepFrame &f) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  // token ids / corpus rows / target rows out of range: every backward kernel validates the ids it scatters by itself
  // (the sequence-encoder BPTT kernels, gen_dx_scatter_kernel, cnn_dx_kernel; rows_scatter_kernel validates the target
  // rows itself since round 5), so the fused step (sse_train_step) reads the flag once at its end -- train_apply_locked; a
  // flagged step cancels its own update on the device -- instead of stalling the queue here.  sse_train_grads reads it now,
  // on every path, so that a rank with a bad id fails here instead of only in its own sse_train_apply.
  // (the class head validates the target rows itself -- no gather ran -- so its step reads the flag after the head)
  if (!f.call->defer_err && !f.class_loss && check_err_flag(h, f.st)) return 1;
  if (f.class_loss) {
    if (step_loss_class(f)) return 1;
    if (!f.call->defer_err && check_err_flag(h, f.st)) return 1;
    HIPCHECK(h, hipMemsetAsync(f.emb->grad, 0, f.emb->count * sizeof(float), f.st));
    return 0;
  }
  if (h->train_loss == 1) {
    if (step_loss_inbatch(f)) return 1;
  } else {
    HIPCHECK(h, launch_loss(f.raw(0), f.raw(1), (const float *)ts.labels.p, f.draw(0), f.draw(1), (float *)ts.row_loss.p,
                            (float *)ts.row_acc.p, f.tail + 1, f.B, f.Bp, f.S, f.inv_rows, f.st));
  }
  HIPCHECK(h, hipMemsetAsync(f.emb->grad, 0, f.emb->count * sizeof(float), f.st));
  if (f.table_tgt) HIPCHECK(h, hipMemsetAsync(f.table->grad, 0, f.table->count * sizeof(float), f.st));
  return 0;
}

// the loss stage of a closing call (STEP_CLOSE): draw[] and tail[1..2] are written already; what step_loss does around its head
static int step_loss_closing(StepFrame &f) {
  sse_handle *h = f.h;
  if (check_err_flag(h, f.st)) return 1;
  HIPCHECK(h, hipMemsetAsync(f.emb->grad, 0, f.emb->count * sizeof(float), f.st));
  if (f.table_tgt) HIPCHECK(h, hipMemsetAsync(f.table->grad, 0, f.table->count * sizeof(float), f.st));
  return 0;
}
static int step_loss_of(StepFrame &f) { return f.call->phase == STEP_CLOSE ? step_loss_closing(f) : step_loss(f); }

// table target: d(raw[1]) scattered onto the free matrix's gradient, its slice norms into the last B partial sums
static int step_table_backward(StepFrame &f) {
  if (!f.table_tgt) return 0;
  if (f.class_loss) {  // the matrix's gradient is dense and enters the global norm whole (train_apply_locked): no slice norms
    HIPCHECK(f.h, hipMemsetAsync(f.sq() + (f.n_sq - f.B), 0, (size_t)f.B * sizeof(float), f.st));
    return 0;
  }
  HIPCHECK(f.h, launch_rows_scatter(f.draw(1), f.ids(1), f.B, f.S, f.table->rows, f.table->grad, f.sq() + (f.n_sq - f.B), f.st));
  return 0;
}

// tail[0] = sum of squares of the raw (un-deduplicated) embedding-gradient slices (both lookups are IndexedSlices),
// tail[3] = rows
static int step_finish(StepFrame &f) {
  HIPCHECK(f.h, launch_sum(f.sq(), f.n_sq, (float)f.B, f.tail, f.st));
  f.ts->grads_ready = true;
  f.ts->grads_dense_table = f.class_loss;
  return 0;
}

// ---- source_only_cnn (BUILDER-DEFINED, see cnn_bwd.hip): row b pairs source sequence b with row tgt_rows[b]
// of the free target matrix; same loss kernel, CNN forward with arg-max tape, gather/scatter backward.

// forward with the arg-max tape
static int cnn_forward(StepFrame &f) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  const int B = f.B, T = f.T, V = h->cfg.vocab_size;
  HIPCHECK(h, hipMemsetAsync(ts.feat_rm.p, 0, (size_t)f.Bp * 576 * sizeof(float), f.st));  // padding rows feed the dM GEMM
  if (h->cnn_bf16) {
    // option cnn_bf16 (BASELINE configs[4]): convolution on the bf16 matrix pipe over bf16-rounded embeddings and
    // filters (fp32 masters, copies refreshed by ensure_packed after every update), fp32 accumulation; bias, ReLU,
    // pooling, projection, loss and the optimizer in fp32
    HIPCHECK(h, launch_cnn_fwd_bf16(f.ids(0), h->emb_bf16, h->cnn_Wc16, h->cnn_bias, (float *)h->s_feat.p, h->err_flag, B, T, V,
                                    round_up(h->cfg.embedding_size, 8), (float *)ts.feat_rm.p, (int32_t *)ts.pos.p, f.st));
    HIPCHECK(h, launch_cnn_proj_x3((const float *)h->s_feat.p, h->cnn_Mx3, f.raw(0), B, f.S, 0, f.st));
  } else {
    HIPCHECK(h, launch_cnn_fwd(f.ids(0), h->emb_pad, h->cnn_Wc, h->cnn_bias, h->cnn_Mp, (float *)h->s_feat.p, f.raw(0), h->err_flag,
                               B, T, V, emb_cols(h->cfg), f.S, 0, (float *)ts.feat_rm.p, (int32_t *)ts.pos.p, f.st));
  }
  return 0;
}

static int cnn_backward(StepFrame &f) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  Variable &M = h->vars[h->cnn_M];
  HIPCHECK(h, launch_proj_bwd((const float *)ts.feat_rm.p, f.draw(0), M.dev, f.Bp, 576, 576, f.S, M.grad, (float *)ts.dfeat.p,
                              (float *)ts.dm_part[0].p, f.st));
  const float *W[4];
  float *dW[4], *db[4];
  for (int i = 0; i < 4; ++i) {
    W[i] = h->vars[h->cnn_W[i]].dev;
    dW[i] = h->vars[h->cnn_W[i]].grad;
    db[i] = h->vars[h->cnn_b[i]].grad;
  }
  HIPCHECK(h, launch_cnn_bwd(f.ids(0), f.emb->dev, (const float *)ts.dfeat.p, (const float *)ts.feat_rm.p, (const int32_t *)ts.pos.p,
                             W, dW, db, (float *)ts.dw_part.p, (float *)ts.dbias_part.p, (float *)ts.wt.p, (unsigned short *)ts.wct.p,
                             f.emb->grad, f.sq(), (float *)ts.hot_part[0].p, f.B, f.T, h->cfg.embedding_size, h->cfg.vocab_size,
                             h->cnn_bf16 ? 1 : 0, f.st));
  return 0;
}

static int cnn_train_grads_locked(sse_handle *h, const TrainCall &call) {
  const sse_config &c = h->cfg;
  const int B = call.B, T = call.T, E = c.embedding_size, S = c.encoding_size;
  const bool closing = call.phase == STEP_CLOSE;  // the checks passed and the buffers were reserved when the step was opened
  if (closing) {
    StepFrame f;
    if (step_begin(h, call, 64, f)) return 1;
    f.n_sq = 2 * B;
    return step_loss_of(f) || cnn_backward(f) || step_table_backward(f) || step_finish(f);
  }
  if (T < 5) return fail(h, "source_only_cnn needs max_seq_length >= 5 (widest filter)");
  if (E > 64) return fail(h, "train step: embedding_size %d > 64 not supported yet", E);
  if ((h->cnn_bf16 ? cnn_bf16_lds_bytes(T, round_up(E, 8), 1) : cnn_lds_bytes(T, emb_cols(c), 1)) > 160 * 1024)
    return fail(h, "source_only_cnn training: T*E = %d*%d does not fit the LDS tile of the gfx950 kernel", T, E);
  // the weight-gradient kernel stages two [T][E] fp32 tiles + 384 floats (cnn_bwd.hip): its own limit, named here
  if (((size_t)2 * T * E + 384) * sizeof(float) > (size_t)160 * 1024)
    return fail(h, "source_only_cnn training: T*E = %d*%d needs %zu bytes of LDS in the weight-gradient kernel (limit 160 KiB: T*E <= 20288)",
                T, E, ((size_t)2 * T * E + 384) * sizeof(float));
  StepFrame f;
  h->train_path_cnn += 1;
  if (step_begin(h, call, 64, f)) return 1;
  if (ensure_packed(h, f.st)) return 1;
  if (step_stage_inputs(f, nullptr, 2 * B)) return 1;  // sq_part: one partial sum per source row, one per target row
  TrainState &ts = *f.ts;
  const int Bp = f.Bp;
  if (reserve(h, h->s_feat, (size_t)((B + 31) / 32) * 72 * 256 * sizeof(float)) || reserve(h, ts.feat_rm, (size_t)Bp * 576 * sizeof(float)) ||
      reserve(h, ts.pos, (size_t)Bp * 576 * sizeof(int32_t)) || reserve(h, ts.dfeat, (size_t)Bp * 576 * sizeof(float)) ||
      reserve(h, ts.dw_part, cnn_dw_part_floats(E, B) * sizeof(float)) || reserve(h, ts.dbias_part, (size_t)cnn_bwd_chunks(B) * 576 * sizeof(float)) ||
      reserve(h, ts.wt, (size_t)E * 1728 * sizeof(float)) || reserve(h, ts.wct, cnn_wct_elems(E) * sizeof(unsigned short)) ||
      reserve(h, ts.hot_part[0], (size_t)std::max(B, cnn_dx_mfma_blocks(B)) * 2 * 64 * sizeof(float)) ||
      reserve(h, ts.dm_part[0], (size_t)proj_bwd_chunks(Bp) * 576 * S * sizeof(float)))
    return 1;
  if (cnn_forward(f) || step_table_forward(f)) return 1;
  if (call.phase == STEP_OPEN) return 0;
  return step_loss(f) || cnn_backward(f) || step_table_backward(f) || step_finish(f);
}

// ---- The LSTM modes at shapes the fused training kernels are not laid out for (cell size > 256, embedding_size > 64): the same
// step through lstm_generic.hip -- per-step GEMM + gate kernels, latency-bound but exact fp32 -- so that no reference flag
// combination (sse_train.py:60-74) is rejected.  Same arena layout, same loss / projection-backward / optimizer kernels.

// forward of one encoder with tapes (un-normalised encodings; the loss kernel normalises)
static int generic_forward_side(StepFrame &f, const GenLstmDims &d, int s) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  Encoder &e = h->enc[s];
  const int S = f.S, V = h->cfg.vocab_size;
  if (reserve(h, ts.gen_A[s], gen_lstm_a_floats(d) * sizeof(float)) || reserve(h, ts.gen_tape[s], gen_lstm_tape_floats(d) * sizeof(float)) ||
      reserve(h, ts.gen_dG[s], gen_lstm_dg_floats(d) * sizeof(float)) || reserve(h, ts.gen_hl[s], (size_t)d.Bp * d.Hq * sizeof(float)) ||
      reserve(h, ts.gen_KT[s], gen_lstm_kt_floats(d) * sizeof(float)) || reserve(h, ts.gen_Kq[s], gen_lstm_kt_floats(d) * sizeof(float)) ||
      reserve(h, ts.gen_MT[s], (size_t)S * d.Hq * sizeof(float)))
    return 1;
  if (ts.gen_ver[s] != h->weights_version) {  // (every step changes the weights; repeated sse_train_grads calls on one set do not)
    HIPCHECK(h, launch_gen_pack(h->vars[e.kernel].dev, h->vars[e.proj].dev, d, S, (float *)ts.gen_KT[s].p, (float *)ts.gen_Kq[s].p,
                                (float *)ts.gen_MT[s].p, f.st));
    ts.gen_ver[s] = h->weights_version;
    h->train_generic_repacks += 1;
  }
  HIPCHECK(h, launch_gen_forward(f.ids(s), f.emb->dev, V, (const float *)ts.gen_KT[s].p, h->vars[e.bias].dev, d, (float *)ts.gen_A[s].p,
                                 (float *)ts.gen_G.p, (float *)ts.gen_c.p, (float *)ts.gen_tape[s].p, (float *)ts.gen_hl[s].p,
                                 h->err_flag, f.st));
  HIPCHECK(h, launch_gen_project((const float *)ts.gen_hl[s].p, (const float *)ts.gen_MT[s].p, d, S, f.raw(s), f.st));
  return 0;
}

static int generic_backward_side(StepFrame &f, const GenLstmDims &d, int s) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  Encoder &e = h->enc[s];
  const bool shared = h->cfg.network_mode == SSE_MODE_SHARED_ENCODER;
  if (reserve(h, ts.dh_last[s], (size_t)d.Bp * d.Hq * sizeof(float))) return 1;
  if (reserve(h, ts.dm_part[s], (size_t)proj_bwd_chunks(d.Bp) * e.H * f.S * sizeof(float))) return 1;
  HIPCHECK(h, launch_proj_bwd((const float *)ts.gen_hl[s].p, f.draw(s), h->vars[e.proj].dev, d.Bp, e.H, d.Hq, f.S, h->vars[e.proj].grad,
                              (float *)ts.dh_last[s].p, (float *)ts.dm_part[s].p, f.st));
  HIPCHECK(h, launch_gen_backward(f.ids(s), (const float *)ts.gen_Kq[s].p, d, (const float *)ts.gen_A[s].p,
                                  (const float *)ts.gen_tape[s].p, (const float *)ts.dh_last[s].p, d.Hq, (float *)ts.gen_dG[s].p,
                                  (float *)ts.gen_dA.p, (float *)ts.gen_dc.p, (float *)ts.gen_dkp.p, (shared && s == 1) ? 1 : 0,
                                  h->vars[e.kernel].grad, h->vars[e.bias].grad, f.emb->grad, f.sq() + (size_t)s * f.T * f.B,
                                  h->cfg.vocab_size, f.st));
  return 0;
}

static int train_grads_generic_locked(sse_handle *h, const TrainCall &call) {
  StepFrame f;
  const bool closing = call.phase == STEP_CLOSE;  // the inputs are staged, the forward has run
  if (!closing) h->train_path_generic += 1;
  if (step_begin(h, call, 32, f)) return 1;
  const int B = f.B, T = f.T, nside = f.nside;
  // sq_part: one partial sum per (side, step, row), one per target row in source-encoder-only mode
  f.n_sq = nside * T * B + (f.table_tgt ? B : 0);
  if (!closing && step_stage_inputs(f, nullptr, f.n_sq)) return 1;
  TrainState &ts = *f.ts;
  GenLstmDims dims[2];
  size_t g_max = 0, c_max = 0, da_max = 0, dkp_max = 0;
  for (int s = 0; s < nside; ++s) {
    dims[s] = gen_lstm_dims(B, T, h->cfg.embedding_size, h->enc[s].H);
    const GenLstmDims &d = dims[s];
    g_max = std::max(g_max, (size_t)d.Bp * 4 * d.Hq);
    c_max = std::max(c_max, (size_t)d.Bp * d.Hq);
    da_max = std::max(da_max, (size_t)d.Bp * d.Kp);
    dkp_max = std::max(dkp_max, gen_lstm_dk_part_floats(d));
  }
  if (reserve(h, ts.gen_G, g_max * sizeof(float)) || reserve(h, ts.gen_c, c_max * sizeof(float)) ||
      reserve(h, ts.gen_dA, da_max * sizeof(float)) || reserve(h, ts.gen_dc, c_max * sizeof(float)) ||
      reserve(h, ts.gen_dkp, dkp_max * sizeof(float)))
    return 1;
  if (!closing) {
    if (step_table_forward(f)) return 1;
    for (int s = 0; s < nside; ++s)
      if (generic_forward_side(f, dims[s], s)) return 1;
    if (call.phase == STEP_OPEN) return 0;
  }
  if (step_loss_of(f) || step_table_backward(f)) return 1;
  for (int s = 0; s < nside; ++s)
    if (generic_backward_side(f, dims[s], s)) return 1;
  return step_finish(f);
}

// ---- the fused LSTM path

// do the rows 2i and 2i + 1 of the source side carry the same sequence (by_rows: the same corpus row) for every i?  B even.
static bool batch_is_paired(const int32_t *src, int B, int T, bool by_rows) {
  for (int i = 0; i < B; i += 2) {
    if (by_rows ? src[i] != src[i + 1]
                : memcmp(src + (size_t)i * T, src + (size_t)(i + 1) * T, (size_t)T * sizeof(int32_t)) != 0)
      return false;
  }
  return true;
}

static FusedPlan fused_plan(const StepFrame &f) {
  sse_handle *h = f.h;
  const int E = h->cfg.embedding_size, V = h->cfg.vocab_size;
  FusedPlan p = {};
  p.all_x3 = true;
  for (int s = 0; s < f.nside; ++s) {
    const Encoder &e = h->enc[s];
    p.fwd_x3[s] = h->train_fwd_x3 && h->train_dk_x3 && e.Hp <= 256 && e.H >= 64 && E < 64;
    // (the in-kernel dX scatter addresses the dense embedding gradient through a 32-bit buffer descriptor: tables of
    // 2 GiB and more keep the fp32 dx kernel with its 64-bit pointers)
    p.bwd_x3[s] = h->train_bwd_x3 && h->train_dk_x3 && e.H >= 64 && e.Hp <= 256 && (int64_t)V * E * 4 < ((int64_t)1 << 31);
    p.all_x3 = p.all_x3 && p.fwd_x3[s] && p.bwd_x3[s];
    p.any_bwd_x3 = p.any_bwd_x3 || p.bwd_x3[s];
  }
  // Pure fp32 step (the default): second-generation kernels -- the forward in the inference orientation with register-built
  // tapes (lstm_fwd_kernel<.., TSW>), lstm_bwd2_kernel (dX inside, dG for the weight gradient straight from registers, no
  // A-operand dG copy in HBM), d(bias) as row E of the weight-gradient GEMM.  Any split-operand option, an embedding of 64
  // columns (no room for the constant-1 column in the 64-column x part of the A-tape) or a >= 2 GiB embedding table (32-bit
  // scatter offsets) keeps the first-generation kernels.
  p.bwd2 = !h->train_fwd_x3 && !h->train_bwd_x3 && !h->train_dk_x3 && !h->train_gen1 && E < 64 &&
           (int64_t)V * E * 4 < ((int64_t)1 << 31);
  // Paired batch (data.py:95-115 builds every batch this way: source row 2i and 2i+1 are the same sequence, once with
  // its positive and once with a sampled negative target): the rows are taken in the order [0,2,4,.. | 1,3,5,..], the
  // source encoder runs on the first half only, and its tapes serve both halves of the backward pass.  The backward
  // itself stays per row: clip_by_global_norm sees the two rows' embedding slices separately (sse_model.py:359-362).
  // (an open step runs without the de-duplication: its closing call hands over gradients in the caller's row order)
  p.paired = f.call->phase == STEP_WHOLE && h->train_pair_dedup && f.B % 128 == 0 &&  // both halves whole 64-row tiles
             batch_is_paired(f.call->src, f.B, f.T, f.call->by_rows);
  p.NT32 = f.Bp / 32;
  p.NT_half = p.NT32 / 2;
  // partial sums of dx^2 per side: one per (tile, wave) when dX comes out of the split-operand BPTT kernel, one per
  // (step, tile) from dx_kernel (+ one per target row in source-encoder-only mode)
  for (int s = 0; s < f.nside; ++s)
    p.sq_off[s + 1] = p.sq_off[s] + (p.bwd2 ? dx_scatter_blocks(f.T, p.NT32 * 32) : p.bwd_x3[s] ? p.NT32 * (h->enc[s].Hp / 32) : f.T * p.NT32);
  p.n_sq = p.sq_off[f.nside] + (f.table_tgt ? f.B : 0);
  return p;
}

static int ensure_side_streams(sse_handle *h, TrainState &ts) {
  if (ts.side[0]) return 0;
  // The two encoders of a step run side by side on these two streams.  Streams of ONE priority share the runtime's small pool
  // of hardware queues, and in a process that has created and destroyed many streams both can land on the same queue: the
  // encoders then run one after the other (the qna recipe, T = 1000: 26 ms / step alone, 52 inside the whole test suite, equal
  // to option train_serial; profiles/r06_notes.txt).  Different priorities come from different queue pools.
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  for (int s = 0; s < 2; ++s) {
    HIPCHECK(h, hipStreamCreateWithPriority(&ts.side[s], hipStreamNonBlocking, s == 0 ? prio_least : prio_greatest));
    HIPCHECK(h, hipEventCreateWithFlags(&ts.ev_join[s], hipEventDisableTiming));
  }
  HIPCHECK(h, hipEventCreateWithFlags(&ts.ev_fork, hipEventDisableTiming));
  return 0;
}

// layouts derived from the variables, rebuilt after every update: only the ones this step's kernels read (an all-split
// step needs the projections, Kh^T / Kx^T in split form and -- fused_pack_split_inputs -- the split kernel matrix and embedding
// table; the fp32 fragment copies wait for the next encode or fp32 step: 7 fewer launches on the critical path of a step)
static int fused_refresh_layouts(StepFrame &f, const FusedPlan &p) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  hipStream_t st = f.st;
  const int E = h->cfg.embedding_size;
  if (p.bwd2 ? pack_train_fp32(h, ts, f.nside, st) : p.all_x3 ? ensure_proj_packed(h, st) : ensure_packed(h, st)) return 1;
  // (the split Kh^T / Kx^T copies are only rebuilt by steps that run the split-operand BPTT: a pure fp32 step leaves them stale)
  if (!((p.any_bwd_x3 && ts.packed_dirty) || (!p.all_x3 && ts.fp32_dirty))) return 0;
  if (p.any_bwd_x3 && ts.packed_dirty) h->train_split_repacks += 1;
  const bool fp32_stale = !p.all_x3 && ts.fp32_dirty;  // (a split-copy rebuild alone leaves current fp32 copies as they are)
  if (fp32_stale) h->train_fp32_repacks += 1;
  for (int s = 0; s < f.nside; ++s) {
    Encoder &e = h->enc[s];
    if (e.shares_lstm_with >= 0) {
      ts.KhT[s] = ts.KhT[e.shares_lstm_with];
      ts.KxT[s] = ts.KxT[e.shares_lstm_with];
      ts.KhT16[s] = ts.KhT16[e.shares_lstm_with];
      ts.KxT16[s] = ts.KxT16[e.shares_lstm_with];
      continue;
    }
    if (p.any_bwd_x3 && ts.packed_dirty) {
      if (!ts.KhT16[s]) HIPCHECK(h, hipMalloc((void **)&ts.KhT16[s], kT16_elems(e.Hp) * sizeof(unsigned short)));
      HIPCHECK(h, launch_pack_kT16(h->vars[e.kernel].dev, E, e.H, e.Hp, ts.KhT16[s], st));
      if (!ts.KxT16[s]) HIPCHECK(h, hipMalloc((void **)&ts.KxT16[s], kxT16_elems(e.Hp) * sizeof(unsigned short)));
      HIPCHECK(h, launch_pack_kxT16(h->vars[e.kernel].dev, E, e.H, e.Hp, ts.KxT16[s], st));
    }
    if (fp32_stale) {
      if (!ts.KhT[s]) HIPCHECK(h, hipMalloc((void **)&ts.KhT[s], (size_t)(e.Hp / 32) * (e.Hp / 2) * 256 * sizeof(float)));
      if (!ts.KxT[s]) HIPCHECK(h, hipMalloc((void **)&ts.KxT[s], (size_t)2 * (e.Hp / 2) * 256 * sizeof(float)));
      HIPCHECK(h, launch_pack_kT(h->vars[e.kernel].dev, E, e.H, e.Hp / 32, e.H, e.Hp, ts.KhT[s], st));
      HIPCHECK(h, launch_pack_kT(h->vars[e.kernel].dev, 0, E, 2, e.H, e.Hp, ts.KxT[s], st));
    }
  }
  if (!p.all_x3) ts.fp32_dirty = false;
  if (p.any_bwd_x3) ts.packed_dirty = false;
  return 0;
}

// the BPTT kernels address the gate tape [T][rows/32][Hp/32][5][1024] floats through 32-bit offsets (both generations)
static int fused_check_tape(StepFrame &f, const FusedPlan &p) {
  sse_handle *h = f.h;
  const int B = f.B, T = f.T;
  for (int s = 0; s < f.nside; ++s) {
    const size_t tape_bytes = (size_t)T * p.NT32 * (h->enc[s].Hp / 32) * 5 * 1024 * sizeof(float);
    if (tape_bytes >= ((size_t)1 << 31))
      return fail(h, "train step: batch x T x H too large -- %d rows x %d steps x cell size %d need a %.2f GiB gate tape per encoder, "
                     "the limit is 2 GiB (<= %lld rows at this T and cell size): use a smaller batch, or sse_train_grads per micro-batch with "
                     "rows_global = the whole batch and the gradient arenas summed before sse_train_apply (the data-parallel recipe)",
                  B, T, h->enc[s].H, (double)tape_bytes / (double)((size_t)1 << 30),
                  (long long)(((((size_t)1 << 31) - 1) / ((size_t)T * (h->enc[s].Hp / 32) * 5 * 1024 * sizeof(float))) * 32 / 64 * 64));
  }
  return 0;
}

// the internal row order of a paired batch, [rows 0,2,4,.. | rows 1,3,5,..], on the host (the result) and on the device (ts.perm)
static int pair_permutation(StepFrame &f, const int32_t **perm) {
  TrainState &ts = *f.ts;
  const int B = f.B;
  if ((int)ts.h_perm.size() != B) {
    ts.h_perm.resize(B);
    for (int r = 0; r < B / 2; ++r) {
      ts.h_perm[r] = 2 * r;
      ts.h_perm[B / 2 + r] = 2 * r + 1;
    }
    ts.perm_B = 0;
  }
  *perm = ts.h_perm.data();
  if (ts.perm_B != B) {
    if (reserve(f.h, ts.perm, (size_t)B * sizeof(int32_t))) return 1;
    HIPCHECK(f.h, hipMemcpyAsync(ts.perm.p, *perm, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, f.st));
    ts.perm_B = B;
  }
  return 0;
}

// options train_fwd_x3 + train_dk_x3: the split embedding table of this step's weights (both encoders read it) and the
// source encoder's split kernel matrix, on the main stream ahead of the fork
static int fused_pack_split_inputs(StepFrame &f) {
  sse_handle *h = f.h;
  const int E = h->cfg.embedding_size, V = h->cfg.vocab_size;
  if (!(h->train_fwd_x3 && h->train_dk_x3 && E < 64)) return 0;
  if (!h->emb16) HIPCHECK(h, hipMalloc((void **)&h->emb16, lstm_x3_emb_elems(V, E) * sizeof(unsigned short)));
  Encoder &e0 = h->enc[0];
  if (!e0.Wx3t) HIPCHECK(h, hipMalloc((void **)&e0.Wx3t, lstm_x3_weight_elems(E, e0.Hp) * sizeof(unsigned short)));
  HIPCHECK(h, launch_pack_lstm_x3(h->vars[e0.kernel].dev, h->vars[e0.bias].dev, h->vars[0].dev, V, E, e0.H, e0.Hp, e0.Wx3t,
                                  h->emb16, 1, f.st));
  h->emb16_valid = true;  // (ensure_packed, in fused_refresh_layouts, cleared it: the table matches the current weights again)
  return 0;
}

// the matrix kernel's arguments for the training forward of encoder s over NTf 32-row tiles (Bf rows).  Not fill_fwd_args:
// that also sets H, gate_split and cu_count, which the training forward leaves at their defaults.
static void fill_train_fwd_args(const StepFrame &f, const FusedPlan &p, int s, int Bf, int NTf, LstmFwdArgs &a) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  const Encoder &e = h->enc[s];
  // inputs and output
  a.ids = f.ids(s);  a.emb = h->emb_pad;  a.Wp = e.Wp;  a.Mp = e.Mp;  a.out = f.raw(s);  a.err = h->err_flag;
  // shapes
  a.B = Bf;  a.T = f.T;  a.V = h->cfg.vocab_size;  a.S = f.S;  a.NTS = (f.S + 31) / 32;  a.NT32 = NTf;
  a.Ep = e.Ep;  a.KGx = e.KGx;  a.KGh = e.KGh;  a.KGhe = (e.H + 7) / 8;
  a.normalize = 0;
  a.tiles_elsewhere = (f.nside == 2 && !h->train_serial) ? ((p.paired && s == 1) ? p.NT_half : p.NT32) : 0;  // the other encoder's forward runs beside this one
  a.force_rows = h->lstm_train_rows;
  // tapes
  a.tape_g = (float *)ts.tape_g[s].p;  a.tape_a = (float *)ts.tape_a[s].p;  a.h_last = (float *)ts.h_last[s].p;
  a.tape_a_split = h->train_dk_x3 ? 1 : 0;  a.tape_swap = p.bwd2 ? 1 : 0;
}

// the same call for the split-operand forward (lstm_fwd_x3.hip, TRAIN): same tapes, same outputs
static void fill_train_x3_args(sse_handle *h, const Encoder &e, const Encoder &own, const LstmFwdArgs &a, LstmX3Args &xa) {
  xa.ids = a.ids;  xa.emb16 = h->emb16;  xa.Wx3 = own.Wx3t;  xa.Mp = e.Mp;  xa.out = a.out;  xa.err = h->err_flag;
  xa.B = a.B;  xa.T = a.T;  xa.V = a.V;  xa.S = a.S;  xa.NTS = a.NTS;  xa.NT32 = a.NT32;
  xa.KGX = lstm_x3_kgx(h->cfg.embedding_size);  xa.H = e.H;
  xa.normalize = 0;
  xa.tiles_elsewhere = a.tiles_elsewhere;
  xa.tape_g = a.tape_g;  xa.tape_a = a.tape_a;  xa.h_last = a.h_last;
}

// forward of encoder s with tapes (un-normalised encodings; the loss kernel normalises) on its side stream, between the
// fork event of the main stream and the join back into it
static int fused_forward_side(StepFrame &f, const FusedPlan &p, int s) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  Encoder &e = h->enc[s];
  const int E = h->cfg.embedding_size, V = h->cfg.vocab_size, T = f.T;
  hipStream_t fs = h->train_serial ? ts.side[0] : ts.side[s];
  HIPCHECK(h, hipStreamWaitEvent(fs, ts.ev_fork, 0));
  const int KT = 2 + e.Hp / 32;
  const bool half = p.paired && s == 0;  // the source encoder of a paired batch: first half of the rows only
  const int NTf = half ? p.NT_half : p.NT32, Bf = half ? f.B / 2 : f.B;
  if (reserve(h, ts.tape_g[s], (size_t)T * NTf * 4 * e.UB * 5 * 1024 * sizeof(float))) return 1;
  if (reserve(h, ts.tape_a[s], (size_t)T * NTf * 4 * KT * 256 * sizeof(float))) return 1;
  if (reserve(h, ts.h_last[s], (size_t)f.Bp * e.Hp * sizeof(float))) return 1;
  LstmFwdArgs a;
  fill_train_fwd_args(f, p, s, Bf, NTf, a);
  if (p.fwd_x3[s]) {
    // the gate GEMMs as three bf16 MFMAs on hi + lo split operands
    Encoder &own = lstm_owner(h, e);
    if (e.shares_lstm_with < 0 && s != 0) {  // (side 0 was packed ahead of the fork together with the embedding table)
      if (!own.Wx3t) HIPCHECK(h, hipMalloc((void **)&own.Wx3t, lstm_x3_weight_elems(E, own.Hp) * sizeof(unsigned short)));
      if (!h->emb16) HIPCHECK(h, hipMalloc((void **)&h->emb16, lstm_x3_emb_elems(V, E) * sizeof(unsigned short)));
      // both depend on the weights of this step: repacked on the launch stream (the other side's stream waits for
      // ev_fork, recorded before; the split embedding table is shared, so it is made on `st` ahead of the fork)
      HIPCHECK(h, launch_pack_lstm_x3(h->vars[own.kernel].dev, h->vars[own.bias].dev, h->vars[0].dev, V, E, own.H, own.Hp,
                                      own.Wx3t, nullptr, 1, fs));
    }
    LstmX3Args xa;
    fill_train_x3_args(h, e, own, a, xa);
    HIPCHECK(h, launch_lstm_fwd_x3(xa, fs));
  } else {
    HIPCHECK(h, launch_lstm_fwd(a, e.Hp, fs));
  }
  if (half) {  // rows B/2 .. B-1 are the same sequences: the loss and the projection backward read them per row
    HIPCHECK(h, hipMemcpyAsync(f.raw(s) + (size_t)Bf * f.S, f.raw(s), (size_t)Bf * f.S * sizeof(float), hipMemcpyDeviceToDevice, fs));
    HIPCHECK(h, hipMemcpyAsync((float *)ts.h_last[s].p + (size_t)Bf * e.Hp, ts.h_last[s].p, (size_t)Bf * e.Hp * sizeof(float),
                               hipMemcpyDeviceToDevice, fs));
  }
  HIPCHECK(h, hipEventRecord(ts.ev_join[s], fs));
  HIPCHECK(h, hipStreamWaitEvent(f.st, ts.ev_join[s], 0));
  return 0;
}

// second generation, pure fp32: dX inside the BPTT kernel, d(bias) as row E of the weight-gradient GEMM
static int fused_bwd_gen2(StepFrame &f, const FusedPlan &p, const FusedBwdSide &b) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  const Encoder &e = h->enc[b.s];
  const int s = b.s, T = f.T, E = h->cfg.embedding_size, V = h->cfg.vocab_size;
  HIPCHECK(h, launch_lstm_bwd2((const float *)ts.tape_g[s].p, (const float *)ts.dh_last[s].p, ts.KhT[s], ts.KxT[s],
                               (float *)ts.dg_b[s].p, (float *)ts.dg_a[s].p, f.ids(s), f.emb->grad, b.sq, (float *)ts.hot_part[s].p, T,
                               p.NT32, b.NTa, b.Hp, e.H, f.B, E, V, b.bs));
  HIPCHECK(h, launch_dk((const float *)ts.tape_a[s].p, (const float *)ts.dg_b[s].p, (float *)ts.dk_part[s].p, b.RGa, b.KT, b.NTn, b.SL,
                        E, e.H, b.Hp, b.accumulate, h->vars[e.kernel].grad, b.half ? p.NT_half * 4 : 0, b.bs, h->vars[e.bias].grad));
  HIPCHECK(h, launch_dx_hot_reduce((const float *)ts.hot_part[s].p, dx_scatter_blocks(T, p.NT32 * 32), E, V, f.emb->grad, b.bs));
  return 0;
}

// first generation, pure fp32 (option train_gen1, E = 64, a >= 2 GiB embedding table): lstm_bwd_kernel, d(bias) from its
// partials, dX by dx_kernel from the A-operand dG copy
static int fused_bwd_gen1(StepFrame &f, const FusedPlan &p, const FusedBwdSide &b) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  const Encoder &e = h->enc[b.s];
  const int s = b.s, T = f.T, E = h->cfg.embedding_size, V = h->cfg.vocab_size;
  BwdDxArgs bdx{ts.KxT16[s], f.ids(s), f.emb->grad, b.sq, (float *)ts.hot_part[s].p, f.B, E, V};
  HIPCHECK(h, launch_lstm_bwd((const float *)ts.tape_g[s].p, (const float *)ts.dh_last[s].p, ts.KhT[s], (float *)ts.dg_a[s].p,
                              (float *)ts.dg_b[s].p, (float *)ts.db_part[s].p, T, p.NT32, b.NTa, b.Hp, e.H, 0, nullptr, &bdx, b.bs));
  HIPCHECK(h, launch_dk((const float *)ts.tape_a[s].p, (const float *)ts.dg_b[s].p, (float *)ts.dk_part[s].p, b.RGa, b.KT, b.NTn, b.SL,
                        E, e.H, b.Hp, b.accumulate, h->vars[e.kernel].grad, b.half ? p.NT_half * 4 : 0, b.bs));
  HIPCHECK(h, launch_db_reduce((const float *)ts.db_part[s].p, p.NT32, e.H, b.Hp, b.accumulate, h->vars[e.bias].grad, b.bs));
  HIPCHECK(h, launch_dx((const float *)ts.dg_a[s].p, ts.KxT[s], f.ids(s), f.emb->grad, b.sq, (float *)ts.hot_part[s].p, T, p.NT32, b.KGn,
                        f.B, E, V, e.H, b.bs));
  return 0;
}

// split operands (option train_dk_x3, with or without train_bwd_x3 for this encoder): the weight-gradient GEMM on the bf16
// matrix pipe; with bwd_x3 the recurrent GEMM too, and dX leaves the BPTT kernel
static int fused_bwd_split(StepFrame &f, const FusedPlan &p, const FusedBwdSide &b) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  const Encoder &e = h->enc[b.s];
  const int s = b.s, T = f.T, E = h->cfg.embedding_size, V = h->cfg.vocab_size;
  BwdDxArgs bdx{ts.KxT16[s], f.ids(s), f.emb->grad, b.sq, (float *)ts.hot_part[s].p, f.B, E, V};
  HIPCHECK(h, launch_lstm_bwd((const float *)ts.tape_g[s].p, (const float *)ts.dh_last[s].p, ts.KhT[s], (float *)ts.dg_a[s].p,
                              (float *)ts.dg_b[s].p, (float *)ts.db_part[s].p, T, p.NT32, b.NTa, b.Hp, e.H, 1,
                              p.bwd_x3[s] ? ts.KhT16[s] : nullptr, &bdx, b.bs));
  // the 8-row r-groups of the fp32 layout pair up into 16-row groups: the same bytes
  HIPCHECK(h, launch_dk_x3(ts.tape_a[s].p, ts.dg_b[s].p, (float *)ts.dk_part[s].p, b.RGa / 2, b.KT, b.NTn, b.SL, E, e.H, b.Hp, b.accumulate,
                           h->vars[e.kernel].grad, b.half ? p.NT_half * 2 : 0, b.bs));
  HIPCHECK(h, launch_db_reduce((const float *)ts.db_part[s].p, p.NT32, e.H, b.Hp, b.accumulate, h->vars[e.bias].grad, b.bs));
  if (p.bwd_x3[s])  // dX left the BPTT kernel already; only the PAD / EOS rows are still to be added
    HIPCHECK(h, launch_dx_hot_reduce((const float *)ts.hot_part[s].p, T * p.NT32 * 2, E, V, f.emb->grad, b.bs));
  else
    HIPCHECK(h, launch_dx((const float *)ts.dg_a[s].p, ts.KxT[s], f.ids(s), f.emb->grad, b.sq, (float *)ts.hot_part[s].p, T, p.NT32, b.KGn,
                          f.B, E, V, e.H, b.bs));
  return 0;
}

// backward of encoder s: the projection, one of the three BPTT bodies, the join into the main stream
static int fused_backward_side(StepFrame &f, const FusedPlan &p, int s) {
  sse_handle *h = f.h;
  TrainState &ts = *f.ts;
  Encoder &e = h->enc[s];
  const bool shared = h->cfg.network_mode == SSE_MODE_SHARED_ENCODER;
  const int T = f.T, Hp = e.Hp, RG = T * p.NT32 * 4;
  FusedBwdSide b;
  b.s = s;
  // dual-encoder: the two backward chains are independent -> side streams; shared-encoder: the
  // target side accumulates onto the source side's kernel/bias gradient -> one stream, in order
  b.bs = (shared || h->train_serial) ? ts.side[0] : ts.side[s];
  b.Hp = Hp;  b.KGn = Hp / 2;  b.NTn = Hp / 8;  b.KT = 2 + Hp / 32;
  b.half = p.paired && s == 0;
  b.NTa = b.half ? p.NT_half : p.NT32;  b.RGa = b.half ? RG / 2 : RG;  b.SL = dk_slices(b.RGa);
  b.accumulate = (shared && s == 1) ? 1 : 0;
  b.sq = f.sq() + p.sq_off[s];
  if (!shared || s == 0) HIPCHECK(h, hipStreamWaitEvent(b.bs, ts.ev_fork, 0));
  if (reserve(h, ts.dh_last[s], (size_t)f.Bp * Hp * sizeof(float))) return 1;
  // dg_a: the A-operand dG copy of the first generation (not written when dX leaves the BPTT kernel); second generation: the dX rows
  if (p.bwd2 ? reserve(h, ts.dg_a[s], (size_t)T * p.NT32 * 32 * 64 * sizeof(float))
             : !p.bwd_x3[s] && reserve(h, ts.dg_a[s], (size_t)T * p.NT32 * b.KGn * 256 * sizeof(float)))
    return 1;
  if (reserve(h, ts.hot_part[s], (size_t)std::max(T * p.NT32 * 2, dx_scatter_blocks(T, p.NT32 * 32)) * 2 * 64 * sizeof(float)) ||
      reserve(h, ts.dg_b[s], (size_t)RG * b.NTn * 256 * sizeof(float)) || reserve(h, ts.db_part[s], (size_t)p.NT32 * 4 * Hp * sizeof(float)) ||
      reserve(h, ts.dk_part[s], (size_t)b.SL * b.KT * 32 * b.NTn * 32 * sizeof(float)) ||
      reserve(h, ts.dm_part[s], (size_t)proj_bwd_chunks(f.Bp) * e.H * f.S * sizeof(float)))
    return 1;
  HIPCHECK(h, launch_proj_bwd((const float *)ts.h_last[s].p, f.draw(s), h->vars[e.proj].dev, f.Bp, e.H, Hp, f.S, h->vars[e.proj].grad,
                              (float *)ts.dh_last[s].p, (float *)ts.dm_part[s].p, b.bs));
  if (p.bwd2 ? fused_bwd_gen2(f, p, b) : h->train_dk_x3 ? fused_bwd_split(f, p, b) : fused_bwd_gen1(f, p, b)) return 1;
  if (!shared || s == 1) {
    HIPCHECK(h, hipEventRecord(ts.ev_join[s], b.bs));
    HIPCHECK(h, hipStreamWaitEvent(f.st, ts.ev_join[s], 0));
  }
  return 0;
}

// Cell sizes up to 256 and embeddings up to 64 columns: MFMA forward with tapes and BPTT, the two encoders side by side
static int train_grads_fused_locked(sse_handle *h, const TrainCall &call) {
  if (ensure_side_streams(h, *h->train)) return 1;
  StepFrame f;
  if (step_begin(h, call, 64, f)) return 1;
  TrainState &ts = *f.ts;
  const FusedPlan p = call.phase == STEP_CLOSE ? ts.open.plan : fused_plan(f);
  if (call.phase == STEP_OPEN) ts.open.plan = p;
  if (call.phase != STEP_CLOSE) {
    h->train_path_fused += 1;
    if (p.paired) h->train_paired_steps += 1;
    if (fused_refresh_layouts(f, p) || fused_check_tape(f, p)) return 1;
    const int32_t *perm = nullptr;
    if (p.paired && pair_permutation(f, &perm)) return 1;
    if (step_stage_inputs(f, perm, p.n_sq) || fused_pack_split_inputs(f)) return 1;
    // the two encoders are independent: fork onto two side streams, join before the loss
    HIPCHECK(h, hipEventRecord(ts.ev_fork, f.st));
    if (step_table_forward(f)) return 1;
    for (int s = 0; s < f.nside; ++s)
      if (fused_forward_side(f, p, s)) return 1;
    if (call.phase == STEP_OPEN) return 0;
  } else {
    f.n_sq = p.n_sq;
  }
  if (step_loss_of(f) || step_table_backward(f)) return 1;
  HIPCHECK(h, hipEventRecord(ts.ev_fork, f.st));  // loss + zeroed embedding gradient are ready
  for (int s = 0; s < f.nside; ++s)
    if (fused_backward_side(f, p, s)) return 1;
  return step_finish(f);
}

// Forward, loss and backward of one batch of pair rows; gradients are scaled by 1/rows_global and left in
// the arena (with the tail sums), nothing is updated.
static int train_grads_locked(sse_handle *h, const TrainCall &call) {
  const sse_config &c = h->cfg;
  if (h->train) h->train->open.valid = false;  // whatever step was left open is discarded
  if (call.B < 1 || call.T < 1 || !call.src || !call.tgt || !call.labels || call.rows_global < call.B)
    return fail(h, "bad arguments to the train step");
  if (call.phase == STEP_WHOLE && h->train_class_loss) {
    if (h->tgt_table < 0)
      return fail(h, "train step: train_class_loss = 1 needs a network mode with a free target matrix (source-encoder-only or source_only_cnn)");
    if (h->train_loss == 1)
      return fail(h, "train step: train_class_loss = 1 and train_loss = 1 ask for two objectives; set one of them to 0");
  }
  if (!h->train) h->train = new TrainState();
  int &path = h->train->open.path;  // (read by the closing call of an open step)
  if (c.network_mode == SSE_MODE_SOURCE_ONLY_CNN) return path = OPEN_CNN, cnn_train_grads_locked(h, call);
  // shapes outside the fused training kernels (cell size > 256, embedding_size > 64; option train_generic forces it: tests)
  bool generic = h->train_generic || c.embedding_size > 64;
  for (int s = 0; s < (c.network_mode == SSE_MODE_SOURCE_ENCODER_ONLY ? 1 : 2); ++s)
    generic = generic || h->enc[s].Hp > 256 || h->enc[s].generic;
  path = generic ? OPEN_GENERIC : OPEN_FUSED;
  return generic ? train_grads_generic_locked(h, call) : train_grads_fused_locked(h, call);
}

// ---- the open step: sse_train_forward* stops behind the forward (STEP_OPEN), one closing call supplies d(raw encodings) and
// the loss tail and runs the rest (STEP_CLOSE).  An open step keeps the caller's row order (no pair de-duplication).

static int train_forward_locked(sse_handle *h, TrainCall call) {
  call.phase = STEP_OPEN;
  if (train_grads_locked(h, call)) return 1;
  TrainState::Open &o = h->train->open;
  o.B = call.B;  o.T = call.T;  o.rows_global = call.rows_global;  o.by_rows = call.by_rows;
  o.weights_version = h->weights_version;
  o.valid = true;
  h->train_open_steps += 1;
  return 0;
}

// the open step a closing or reading call refers to, or nullptr with the refusal's text set
static TrainState::Open *open_step(sse_handle *h, const char *who) {
  if (!h->train || !h->train->open.valid) {
    fail(h, "%s: no step is open (sse_train_forward opens one; a closing call or any other train step ends it)", who);
    return nullptr;
  }
  if (h->train->open.weights_version != h->weights_version) {
    fail(h, "%s: the variables changed since sse_train_forward (sse_set_variable or an update): run the forward again", who);
    return nullptr;
  }
  return &h->train->open;
}

static int open_row_tile(const TrainState::Open &o) { return o.path == OPEN_GENERIC ? 32 : 64; }

// the rest of the open step; draw[] (pad rows zeroed) and tail[1..2] have been queued by the caller
static int train_close_locked(sse_handle *h) {
  TrainState::Open &o = h->train->open;
  o.valid = false;
  const TrainCall call{nullptr, nullptr, nullptr, o.B, o.T, o.rows_global, o.by_rows, false, STEP_CLOSE};
  return o.path == OPEN_CNN ? cnn_train_grads_locked(h, call)
         : o.path == OPEN_GENERIC ? train_grads_generic_locked(h, call) : train_grads_fused_locked(h, call);
}

// clip_by_global_norm over the (possibly all-reduced) arena + Adagrad + global_step (sse_model.py:355-364)
static int train_apply_locked(sse_handle *h, float *loss, float *train_acc) {
  if (!h->train || !h->train->grads_ready) return fail(h, "train apply: no gradients pending (call sse_train_grads first)");
  TrainState &ts = *h->train;
  hipStream_t st = h->stream;
  const int NORM_BLOCKS = 64;
  float *tail = ts.arena + grad_arena_count(h) - 4;
  if (reserve(h, ts.scal, 4 * sizeof(float))) return 1;
  float *scal = (float *)ts.scal.p;  // [0] global norm [1] clip scale [2] update cancelled
  if (reserve(h, ts.norm_part, (size_t)(h->vars.size() * NORM_BLOCKS + 1) * sizeof(float))) return 1;
  float *np_ = (float *)ts.norm_part.p;
  if (h->vars.size() > SSE_MAX_TENSORS) return fail(h, "too many variables");
  // dense tensors enter the global norm whole; the lookup tables (word_embedding, tgt_seq_embedding) through the raw
  // slice norm in tail[0] (tf.clip_by_global_norm over IndexedSlices.values, sse_model.py:359-362).  Gradients left by a
  // class-loss step (ts.grads_dense_table, whatever the option says by now) carry a dense tgt_seq_embedding gradient: it
  // enters whole, from the arena as it is now, i.e. after any all-reduce, and tail[0] covers word_embedding alone.
  MultiTensor dense, all;
  dense.n = all.n = 0;
  for (size_t i = 0; i < h->vars.size(); ++i) {
    Variable &v = h->vars[i];
    all.w[all.n] = v.dev;
    all.slot[all.n] = v.slot;
    all.grad[all.n] = v.grad;
    all.count[all.n++] = v.count;
    if (i == 0 || ((int)i == h->tgt_table && !ts.grads_dense_table)) continue;
    dense.w[dense.n] = v.dev;
    dense.slot[dense.n] = v.slot;
    dense.grad[dense.n] = v.grad;
    dense.count[dense.n++] = v.count;
  }
  HIPCHECK(h, launch_sumsq_multi(dense, np_, NORM_BLOCKS, st));
  // a token id out of range seen by this step's kernels (deferred check of the fused step) cancels the update on the device
  HIPCHECK(h, launch_clip_scale_multi(np_, dense.n * NORM_BLOCKS, tail, 5.0f /* max_gradient_norm, sse_model.py:117 */, h->err_flag,
                                      scal, st));
  // ---- Adagrad (dense for every tensor; rows of word_embedding with zero gradient are unchanged)
  HIPCHECK(h, launch_adagrad_multi(all, scal, h->lr, st));
  h->packed_dirty = true;
  h->weights_version += 1;
  h->mp_fresh = false;
  ts.packed_dirty = ts.fp32_dirty = true;
  ts.grads_ready = false;

  float *out = reinterpret_cast<float *>(h->pin_small + 4);
  HIPCHECK(h, hipMemcpyAsync(out, tail, 4 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHECK(h, hipMemcpyAsync(h->pin_small, h->err_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHECK(h, sync_stream(st));
  // bits 1 | 2 | 8 (token id / corpus row out of range, sparse gradient exchange overflow) belong to this step: the update was cancelled on the device, variables
  // unchanged.  Bit 4 (a cluster-kernel give-up of an asynchronous sse_encode_dev issued earlier) is not this step's: it
  // stays in the flag for sse_synchronize / the next encode to report.
  if (h->pin_small[0] & 11) return check_err_flag(h, st);  // (resets the flag)
  h->global_step += 1;
  if (loss) *loss = out[1];
  if (train_acc) *train_acc = out[2];
  return 0;
}

int sse_train_grads(sse_handle *h, const int32_t *src_ids_host, const int32_t *tgt_ids_host, const float *labels_host,
                    int32_t B, int32_t T, int64_t rows_global) {
  SSE_ENTER(h);
  return train_grads_locked(h, TrainCall{src_ids_host, tgt_ids_host, labels_host, B, T, rows_global, false, false});
}

int sse_train_forward(sse_handle *h, const int32_t *src_ids_host, const int32_t *tgt_ids_host, const float *labels_host, int32_t B,
                      int32_t T, int64_t rows_global) {
  SSE_ENTER(h);
  return train_forward_locked(h, TrainCall{src_ids_host, tgt_ids_host, labels_host, B, T, rows_global, false, false});
}

int sse_train_forward_rows(sse_handle *h, const int32_t *src_rows_host, const int32_t *tgt_rows_host, const float *labels_host,
                           int32_t B, int64_t rows_global) {
  SSE_ENTER(h);
  if (!h->train || !h->train->corpus[0].p) return fail(h, "train step by rows: no source corpus on the device (sse_corpus_upload)");
  return train_forward_locked(h, TrainCall{src_rows_host, tgt_rows_host, labels_host, B, h->train->corpus_T[0], rows_global, true, false});
}

int sse_train_open_encodings_dev(sse_handle *h, int side, float *out_dev, void *stream) {
  SSE_ENTER(h);
  if ((side != 0 && side != 1) || !out_dev) return fail(h, "bad arguments to sse_train_open_encodings_dev");
  const TrainState::Open *o = open_step(h, "sse_train_open_encodings_dev");
  if (!o) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (st != h->stream) {  // the forward was queued on the stream of sse_set_stream: the copy waits for it
    hipEvent_t ev;
    HIPCHECK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHECK(h, hipEventRecord(ev, h->stream));
    HIPCHECK(h, hipStreamWaitEvent(st, ev, 0));
    HIPCHECK(h, hipEventDestroy(ev));
  }
  HIPCHECK(h, hipMemcpyAsync(out_dev, h->train->raw[side].p, (size_t)o->B * h->cfg.encoding_size * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}

int sse_train_backward_dev(sse_handle *h, const float *d_src_dev, const float *d_tgt_dev, float loss_part, float acc_part) {
  SSE_ENTER(h);
  if (!d_src_dev || !d_tgt_dev) return fail(h, "sse_train_backward_dev: d_src and d_tgt must not be NULL");
  const TrainState::Open *o = open_step(h, "sse_train_backward_dev");
  if (!o) return 1;
  TrainState &ts = *h->train;
  if (ensure_arena(h)) return 1;
  const int B = o->B, S = h->cfg.encoding_size, Bp = round_up(B, open_row_tile(*o));
  const float *d[2] = {d_src_dev, d_tgt_dev};
  for (int s = 0; s < 2; ++s) {
    HIPCHECK(h, hipMemcpyAsync(ts.draw[s].p, d[s], (size_t)B * S * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (Bp > B) HIPCHECK(h, hipMemsetAsync((float *)ts.draw[s].p + (size_t)B * S, 0, (size_t)(Bp - B) * S * sizeof(float), h->stream));
  }
  HIPCHECK(h, launch_set_pair(ts.arena + grad_arena_count(h) - 4 + 1, loss_part, acc_part, h->stream));
  return train_close_locked(h);
}

static int exchange_target_words(sse_handle *h, int T) { return h->tgt_table >= 0 ? 1 : T; }

int64_t sse_train_exchange_floats(sse_handle *h, int32_t cap, int32_t T) {
  if (!h || cap < 1 || T < 1) return 0;
  return (int64_t)train_exchange_floats(cap, h->cfg.encoding_size, T, exchange_target_words(h, T));
}

int sse_train_pack_exchange(sse_handle *h, int32_t cap, float *block_dev) {
  SSE_ENTER(h);
  if (!block_dev) return fail(h, "sse_train_pack_exchange: block must not be NULL");
  const TrainState::Open *o = open_step(h, "sse_train_pack_exchange");
  if (!o) return 1;
  if (cap < o->B) return fail(h, "sse_train_pack_exchange: cap = %d row slots, the open step holds %d rows", cap, o->B);
  TrainState &ts = *h->train;
  HIPCHECK(h, launch_train_exchange_pack((const float *)ts.raw[0].p, (const float *)ts.raw[1].p, (const float *)ts.labels.p,
                                         (const int32_t *)ts.ids[0].p, (const int32_t *)ts.ids[1].p, o->B, cap, h->cfg.encoding_size, o->T,
                                         exchange_target_words(h, o->T), block_dev, h->stream));
  return 0;
}

int sse_train_backward_inbatch_global(sse_handle *h, const float *gathered_dev, int32_t world, int32_t cap, int32_t rank,
                                      const int32_t *rank_rows_host) {
  SSE_ENTER(h);
  const char *who = "sse_train_backward_inbatch_global";
  if (!gathered_dev || !rank_rows_host) return fail(h, "%s: the gathered blocks and rank_rows must not be NULL", who);
  if (world < 1) return fail(h, "%s: world = %d, must be >= 1", who, world);
  if (rank < 0 || rank >= world) return fail(h, "%s: rank %d outside [0, %d)", who, rank, world);
  const TrainState::Open *o = open_step(h, who);
  if (!o) return 1;
  int64_t sum = 0;
  int32_t most = 0;
  for (int r = 0; r < world; ++r) {
    if (rank_rows_host[r] < 0) return fail(h, "%s: rank_rows[%d] = %d is negative", who, r, rank_rows_host[r]);
    sum += rank_rows_host[r];
    most = std::max(most, rank_rows_host[r]);
  }
  if (rank_rows_host[rank] != o->B)
    return fail(h, "%s: rank_rows[%d] = %d, the open step of this rank holds %d rows", who, rank, rank_rows_host[rank], o->B);
  if (most > cap) return fail(h, "%s: a rank holds %d rows, more than the cap = %d row slots of a block", who, most, cap);
  if (sum != o->rows_global)
    return fail(h, "%s: rank_rows add up to %lld rows, the step was opened with rows_global = %lld", who, (long long)sum, (long long)o->rows_global);
  TrainState &ts = *h->train;
  hipStream_t st = h->stream;
  const int B = o->B, G = (int)sum, S = h->cfg.encoding_size, T = o->T, Tt = exchange_target_words(h, T);
  const int Bp = round_up(B, open_row_tile(*o));
  if (ensure_arena(h) || reserve_inbatch(h, G, S)) return 1;
  for (int s = 0; s < 2; ++s)
    if (reserve(h, ts.xg_raw[s], (size_t)G * S * sizeof(float))) return 1;
  if (reserve(h, ts.xg_labels, (size_t)G * sizeof(float)) || reserve(h, ts.xg_ids[0], (size_t)G * T * sizeof(int32_t)) ||
      reserve(h, ts.xg_ids[1], (size_t)G * Tt * sizeof(int32_t)) || reserve(h, ts.xg_off, (size_t)(world + 1) * sizeof(int32_t)))
    return 1;
  // global row = rows of the lower ranks + local row
  ts.h_off.assign(world + 1, 0);
  for (int r = 0; r < world; ++r) ts.h_off[r + 1] = ts.h_off[r] + rank_rows_host[r];
  const int row_lo = ts.h_off[rank];
  HIPCHECK(h, hipMemcpyAsync(ts.xg_off.p, ts.h_off.data(), (size_t)(world + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  float *gsrc = (float *)ts.xg_raw[0].p, *gtgt = (float *)ts.xg_raw[1].p, *glab = (float *)ts.xg_labels.p;
  int32_t *gid0 = (int32_t *)ts.xg_ids[0].p, *gid1 = (int32_t *)ts.xg_ids[1].p;
  HIPCHECK(h, launch_train_exchange_compact(gathered_dev, (const int32_t *)ts.xg_off.p, world, G, cap, S, T, Tt, gsrc, gtgt, glab, gid0, gid1, st));
  // the keys over the GLOBAL id rows, as step_loss_inbatch forms them over a rank's own: a source or a target repeated on
  // another rank is admitted or excluded as the single-rank step of the concatenated batch decides
  int32_t *ks = (int32_t *)h->s_inbatch_keys.p, *kt = ks + G;
  uint32_t *hash = (uint32_t *)(kt + G);
  HIPCHECK(h, launch_inbatch_token_keys(gid0, G, T, hash, ks, st));
  if (Tt == 1 && h->tgt_table >= 0)
    HIPCHECK(h, launch_inbatch_value_keys(gid1, 32, G, kt, st));
  else
    HIPCHECK(h, launch_inbatch_token_keys(gid1, G, T, hash, kt, st));
  const float inv_rows = 1.0f / (float)o->rows_global;
  HIPCHECK(h, launch_inbatch_loss_window(gsrc, gtgt, glab, ks, kt, G, row_lo, row_lo + B, Bp, S, (float)h->train_loss_scale, inv_rows,
                                         h->s_inbatch.p, (float *)ts.draw[0].p, (float *)ts.draw[1].p, (float *)ts.row_loss.p,
                                         (float *)ts.row_acc.p, st));
  HIPCHECK(h, launch_loss_reduce((const float *)ts.row_loss.p, (const float *)ts.row_acc.p, B, inv_rows,
                                 ts.arena + grad_arena_count(h) - 4 + 1, st));
  h->train_global_inbatch_steps += 1;
  return train_close_locked(h);
}

int sse_corpus_upload(sse_handle *h, int side, const int32_t *ids_host, int64_t N, int32_t T) {
  SSE_ENTER(h);
  if ((side != 0 && side != 1) || !ids_host || N < 1 || T < 1 || N > 2147483000) return fail(h, "bad arguments to sse_corpus_upload");
  if (!h->train) h->train = new TrainState();
  TrainState &ts = *h->train;
  HIPCHECK(h, hipDeviceSynchronize());
  if (reserve(h, ts.corpus[side], (size_t)N * T * sizeof(int32_t))) return 1;
  HIPCHECK(h, hipMemcpy(ts.corpus[side].p, ids_host, (size_t)N * T * sizeof(int32_t), hipMemcpyHostToDevice));
  ts.corpus_N[side] = N;
  ts.corpus_T[side] = T;
  return 0;
}

int sse_train_grads_rows(sse_handle *h, const int32_t *src_rows_host, const int32_t *tgt_rows_host, const float *labels_host,
                         int32_t B, int64_t rows_global) {
  SSE_ENTER(h);
  if (!h->train || !h->train->corpus[0].p) return fail(h, "train step by rows: no source corpus on the device (sse_corpus_upload)");
  return train_grads_locked(h, TrainCall{src_rows_host, tgt_rows_host, labels_host, B, h->train->corpus_T[0], rows_global, true, false});
}

int sse_train_step_rows(sse_handle *h, const int32_t *src_rows_host, const int32_t *tgt_rows_host, const float *labels_host,
                        int32_t B, float *loss, float *train_acc) {
  SSE_ENTER(h);
  if (!h->train || !h->train->corpus[0].p) return fail(h, "train step by rows: no source corpus on the device (sse_corpus_upload)");
  if (train_grads_locked(h, TrainCall{src_rows_host, tgt_rows_host, labels_host, B, h->train->corpus_T[0], B, true, true})) return 1;
  return train_apply_locked(h, loss, train_acc);
}

int64_t sse_train_packed_embedding_floats(sse_handle *h, int32_t cap) {
  if (!h || cap < 1) return 0;
  return emb_grad_packed_floats(h->cfg.embedding_size, cap);
}

int sse_train_pack_embedding_grad(sse_handle *h, int32_t cap, float *packed_dev) {
  SSE_ENTER(h);
  if (!h->train || !h->train->grads_ready) return fail(h, "pack embedding gradient: no gradients pending (call sse_train_grads first)");
  if (cap < 1 || !packed_dev) return fail(h, "bad arguments to sse_train_pack_embedding_grad");
  HIPCHECK(h, launch_emb_grad_pack(h->vars[0].grad, h->cfg.vocab_size, h->cfg.embedding_size, cap, packed_dev, h->err_flag, h->stream));
  return 0;
}

int sse_train_unpack_embedding_grad(sse_handle *h, const float *gathered_dev, int32_t world, int32_t cap) {
  SSE_ENTER(h);
  if (!h->train || !h->train->grads_ready) return fail(h, "unpack embedding gradient: no gradients pending (call sse_train_grads first)");
  if (cap < 1 || world < 1 || !gathered_dev) return fail(h, "bad arguments to sse_train_unpack_embedding_grad");
  HIPCHECK(h, launch_emb_grad_unpack(gathered_dev, world, h->cfg.vocab_size, h->cfg.embedding_size, cap, h->vars[0].grad, h->err_flag,
                                     h->stream));
  return 0;
}

int sse_train_apply(sse_handle *h, float *loss, float *train_acc) {
  SSE_ENTER(h);
  return train_apply_locked(h, loss, train_acc);
}

int sse_train_step(sse_handle *h, const int32_t *src_ids_host, const int32_t *tgt_ids_host, const float *labels_host,
                   int32_t B, int32_t T, float *loss, float *train_acc) {
  // (not SSE_ENTER: a null loss / train_acc is refused here, ahead of the lock, without a step and without an error text;
  // sse_train_step_rows and sse_train_apply accept either as "not wanted")
  if (!h || !loss || !train_acc) return 1;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  // defer_err: one host sync per step, the error flag is read with the loss
  if (train_grads_locked(h, TrainCall{src_ids_host, tgt_ids_host, labels_host, B, T, B, false, true})) return 1;
  return train_apply_locked(h, loss, train_acc);
}

// session.run([model.loss, model.train_acc]) WITHOUT model.train (sse_model.py:290,298,302): both encoders through the
// inference dispatch (encode_dev_locked, un-normalised: every option, path and shape an encode takes), then eval_loss.hip.
// by_rows: src / tgt are row numbers into the corpora of sse_corpus_upload.  Chunks of at most eval_chunk_rows pair rows bound
// the scratch; the per-row values land at the row's position in the call and ONE reduce follows the last chunk, so the result
// does not depend on the chunk size.  Runs on the stream of sse_set_stream, behind whatever a train step queued there.
static int eval_loss_locked(sse_handle *h, const int32_t *src_host, const int32_t *tgt_host, const float *labels_host, int32_t B,
                            int32_t T, bool by_rows, double *sums, float *row_cos_host) {
  const sse_config &c = h->cfg;
  if (!sums || B < 0) return fail(h, "bad arguments to the loss evaluation");
  if (B == 0) {
    sums[0] = sums[1] = sums[2] = 0.0;
    return 0;
  }
  if (T < 1 || !src_host || !tgt_host || !labels_host) return fail(h, "bad arguments to the loss evaluation");
  const bool table_tgt = h->tgt_table >= 0;  // source-encoder-only / source_only_cnn: tgt = rows of the free target matrix
  TrainState *ts = h->train;
  if (by_rows && !table_tgt && (!ts->corpus[1].p || ts->corpus_T[1] != T))
    return fail(h, "loss evaluation by rows: no target corpus with T = %d on the device (sse_corpus_upload)", T);
  const int S = c.encoding_size;
  hipStream_t st = h->stream;

  // paired batch (data.py:95-115): rows 2i, 2i + 1 carry the same source -> one source-encoder row per pair
  const bool paired = h->train_pair_dedup && B % 2 == 0 && batch_is_paired(src_host, B, T, by_rows);
  if (paired) h->eval_paired_calls += 1;

  const int chunk = std::min<int>(B, h->eval_chunk_rows);  // (even, or the whole batch)
  const int chunk_src = paired ? chunk / 2 : chunk;
  if (reserve(h, h->ev_ids[0], (size_t)chunk_src * T * sizeof(int32_t)) || reserve(h, h->ev_raw[0], (size_t)chunk_src * S * sizeof(float)) ||
      reserve(h, h->ev_labels, (size_t)chunk * sizeof(float)) || reserve(h, h->ev_row, (size_t)3 * B * sizeof(float)) ||
      reserve(h, h->ev_sums, 3 * sizeof(double)))
    return 1;
  if (by_rows && reserve(h, h->ev_rows[0], (size_t)chunk * sizeof(int32_t))) return 1;
  if (!by_rows && paired && reserve(h, h->ev_stage, (size_t)chunk * T * sizeof(int32_t))) return 1;
  if ((by_rows || table_tgt) && reserve(h, h->ev_rows[1], (size_t)chunk * sizeof(int32_t))) return 1;
  if (!table_tgt && (reserve(h, h->ev_ids[1], (size_t)chunk * T * sizeof(int32_t)) || reserve(h, h->ev_raw[1], (size_t)chunk * S * sizeof(float))))
    return 1;
  int32_t *ids[2] = {(int32_t *)h->ev_ids[0].p, (int32_t *)h->ev_ids[1].p}, *rows[2] = {(int32_t *)h->ev_rows[0].p, (int32_t *)h->ev_rows[1].p};
  float *raw[2] = {(float *)h->ev_raw[0].p, (float *)h->ev_raw[1].p};
  float *row_loss = (float *)h->ev_row.p, *row_acc = row_loss + B, *row_cos = row_acc + B;
  double *sums_pin = reinterpret_cast<double *>(h->pin_small + 8);

  // the whole call, queued on st (host buffers are the caller's: they outlive the synchronisation below)
  auto queue = [&](bool allow_cluster) -> int {
    EncodeRequest rq;
    rq.allow_cluster = allow_cluster;
    for (int b0 = 0; b0 < B; b0 += chunk) {
      const int nb = std::min(chunk, B - b0), ns = paired ? nb / 2 : nb, stride = paired ? 2 : 1;
      if (by_rows) {
        HIPCHECK(h, hipMemcpyAsync(rows[0], src_host + b0, (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHECK(h, launch_eval_stage_ids((const int32_t *)ts->corpus[0].p, rows[0], stride, ns, T, ts->corpus_N[0], ids[0], h->err_flag, st));
      } else if (paired) {
        HIPCHECK(h, hipMemcpyAsync(h->ev_stage.p, src_host + (size_t)b0 * T, (size_t)nb * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHECK(h, launch_eval_stage_ids((const int32_t *)h->ev_stage.p, nullptr, stride, ns, T, 0, ids[0], h->err_flag, st));
      } else {
        HIPCHECK(h, hipMemcpyAsync(ids[0], src_host + (size_t)b0 * T, (size_t)nb * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
      }
      if (encode_dev_locked(h, SSE_SIDE_SOURCE, ids[0], ns, T, 0, raw[0], st, rq)) return 1;
      if (table_tgt) {
        HIPCHECK(h, hipMemcpyAsync(rows[1], tgt_host + b0, (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice, st));
      } else {
        if (by_rows) {
          HIPCHECK(h, hipMemcpyAsync(rows[1], tgt_host + b0, (size_t)nb * sizeof(int32_t), hipMemcpyHostToDevice, st));
          HIPCHECK(h, launch_eval_stage_ids((const int32_t *)ts->corpus[1].p, rows[1], 1, nb, T, ts->corpus_N[1], ids[1], h->err_flag, st));
        } else {
          HIPCHECK(h, hipMemcpyAsync(ids[1], tgt_host + (size_t)b0 * T, (size_t)nb * T * sizeof(int32_t), hipMemcpyHostToDevice, st));
        }
        if (encode_dev_locked(h, SSE_SIDE_TARGET, ids[1], nb, T, 0, raw[1], st, rq)) return 1;
      }
      HIPCHECK(h, hipMemcpyAsync(h->ev_labels.p, labels_host + b0, (size_t)nb * sizeof(float), hipMemcpyHostToDevice, st));
      const Variable *table = table_tgt ? &h->vars[h->tgt_table] : nullptr;
      HIPCHECK(h, launch_pair_eval(raw[0], table ? table->dev : raw[1], table ? rows[1] : nullptr, table ? table->rows : 0,
                                   (const float *)h->ev_labels.p, row_loss + b0, row_acc + b0, row_cos + b0, h->err_flag, nb, S,
                                   paired ? 1 : 0, st));
    }
    HIPCHECK(h, launch_eval_reduce(row_loss, row_acc, B, (double *)h->ev_sums.p, st));
    HIPCHECK(h, hipMemcpyAsync(sums_pin, h->ev_sums.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    return 0;
  };
  if (queue(true)) return 1;
  int32_t bits = 0;
  if (check_err_flag(h, st, &bits)) return 1;  // (synchronises; an id or a row out of range: reported, flag reset, no outputs)
  if (bits == 4) {
    // a cluster-kernel launch gave up (a workgroup did not arrive): the call once more on the kernels that need no co-residency
    h->persist_fallbacks += 1;
    h->cluster_skip[0] = h->cluster_skip[1] = h->cluster_backoff >= 0 ? h->cluster_backoff : 16;
    if (queue(false)) return 1;
    if (check_err_flag(h, st)) return 1;
  }
  if (row_cos_host) {
    HIPCHECK(h, hipMemcpyAsync(row_cos_host, row_cos, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHECK(h, sync_stream(st));
  }
  for (int i = 0; i < 3; ++i) sums[i] = sums_pin[i];
  return 0;
}

int sse_eval_loss(sse_handle *h, const int32_t *src_ids_host, const int32_t *tgt_ids_host, const float *labels_host, int32_t B,
                  int32_t T, double *sums, float *row_cos_host) {
  SSE_ENTER(h);
  return eval_loss_locked(h, src_ids_host, tgt_ids_host, labels_host, B, T, false, sums, row_cos_host);
}

int sse_eval_loss_rows(sse_handle *h, const int32_t *src_rows_host, const int32_t *tgt_rows_host, const float *labels_host,
                       int32_t B, double *sums, float *row_cos_host) {
  SSE_ENTER(h);
  if (!h->train || !h->train->corpus[0].p) return fail(h, "loss evaluation by rows: no source corpus on the device (sse_corpus_upload)");
  return eval_loss_locked(h, src_rows_host, tgt_rows_host, labels_host, B, h->train->corpus_T[0], true, sums, row_cos_host);
}

int sse_get_learning_rate(sse_handle *h, float *lr) {
  if (!h || !lr) return 1;
  *lr = h->lr;
  return 0;
}
int sse_set_learning_rate(sse_handle *h, float lr) {
  if (!h) return 1;
  h->lr = lr;
  return 0;
}
int sse_decay_learning_rate(sse_handle *h) {
  if (!h) return 1;
  // learning_rate.assign(max(lr * decay, 1e-3)), float32 (sse_model.py:123-124)
  h->lr = fmaxf(h->lr * h->cfg.learning_rate_decay_factor, 1e-3f);
  return 0;
}
int sse_get_global_step(sse_handle *h, int64_t *step) {
  if (!h || !step) return 1;
  *step = h->global_step;
  return 0;
}
int sse_set_global_step(sse_handle *h, int64_t step) {
  if (!h) return 1;
  h->global_step = step;
  return 0;
}

int sse_set_stream(sse_handle *h, void *stream) {
  SSE_ENTER(h);
  HIPCHECK(h, hipStreamSynchronize(h->stream));  // nothing of an earlier step may still be in flight on the old stream
  h->stream = (hipStream_t)stream;
  return 0;
}

int sse_timer_record(sse_handle *h, int32_t slot, void *stream) {
  if (!h) return 1;
  if (slot < 0 || slot >= 256) return fail(h, "timer slot %d out of range [0,256)", slot);
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  if ((int)h->events.size() <= slot) h->events.resize(slot + 1, nullptr);
  if (!h->events[slot]) HIPCHECK(h, hipEventCreate(&h->events[slot]));
  HIPCHECK(h, hipEventRecord(h->events[slot], (hipStream_t)stream));
  return 0;
}
int sse_timer_elapsed_ms(sse_handle *h, int32_t a, int32_t b, float *ms) {
  if (!h || !ms) return 1;
  if (a < 0 || b < 0 || a >= (int)h->events.size() || b >= (int)h->events.size() || !h->events[a] || !h->events[b])
    return fail(h, "timer slots %d/%d were not recorded", a, b);
  HIPCHECK(h, hipSetDevice(h->cfg.device));
  HIPCHECK(h, hipEventSynchronize(h->events[b]));
  HIPCHECK(h, hipEventElapsedTime(ms, h->events[a], h->events[b]));
  return 0;
}
int sse_synchronize(sse_handle *h) {
  SSE_ENTER(h);
  HIPCHECK(h, hipDeviceSynchronize());
  return check_err_flag(h, nullptr);
}

}  // extern "C"
