/*
 * sse_hip.h -- C ABI of libsse_hip.so, the MI355X (gfx950) implementation of
 * the Sequence-Semantic-Embedding hot path.
 *
 * The reference (eBay/Sequence-Semantic-Embedding, pure Python on TensorFlow
 * 1.x) has no FFI; its de-facto boundary for this path is the `SSEModel`
 * object plus `tf.Session.run(fetches, feed_dict)`.  Each entry point below
 * names the reference call it replaces (file:line in the reference tree).
 * The ctypes binding a maintainer adds on the reference side is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error;
 *     sse_last_error(h) (or sse_last_error(NULL) for sse_create failures)
 *     returns a NUL-terminated message owned by the library;
 *   - "host" pointers are caller-owned numpy-style buffers, read/written only
 *     during the call; "dev" pointers are HIP device pointers on the handle's
 *     device, `stream` is a hipStream_t passed as void* (NULL = null stream);
 *   - token ids are row-major int32 [B,T] (sse_model.py:408-409,419-421,430,439),
 *     encodings row-major float32 [B,S];
 *   - alignment: the natural alignment of the element type (4 bytes for float / int32, 8 for double / int64 / uint64) is all
 *     any pointer needs, host or device -- a row of a larger tensor, an offset into an all-gather buffer and the arena of
 *     sse_train_set_grad_arena included.  A 16-byte aligned device pointer lets some launchers take a 16-byte body where they
 *     would take a scalar one; results are identical, except that sse_l2_normalize_dev then sums a row in another order;
 *   - bounds: a call reads and writes only the elements its arguments name ([B,T], [Q,k], `cap` entries, `count` floats):
 *     nothing before a pointer, nothing behind the last element, no input is written, and no memory outside the named
 *     elements can reach a result (tests/guard_bands.py places every device pointer between guards to hold this);
 *   - a handle may be used from several threads for encode/score (calls are
 *     serialised internally, like tf.Session.run in webserver.py:108);
 *     sse_train_step is exclusive;
 *   - the internal mutex serialises the HOST side only: the *_dev entry points enqueue on the stream they are given
 *     and share the handle's packed-weight and scratch buffers, so ONE handle must be driven from ONE stream (or the
 *     caller orders its streams with events); create one handle per stream for concurrent device-side use.  The
 *     host-buffer entry points use the null stream and synchronise before returning; the train step runs on the
 *     stream set with sse_set_stream (default: the null stream).
 */
#ifndef SSE_HIP_H
#define SSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sse_handle sse_handle;

/* network_mode values (sse_model.py:167-177) */
enum {
  SSE_MODE_DUAL_ENCODER = 0,        /* 'dual-encoder'        sse_model.py:236 */
  SSE_MODE_SHARED_ENCODER = 1,      /* 'shared-encoder'      sse_model.py:258 */
  SSE_MODE_SOURCE_ENCODER_ONLY = 2, /* 'source-encoder-only' sse_model.py:217 */
  SSE_MODE_SOURCE_ONLY_CNN = 3      /* 'source_only_cnn'     sse_model.py:179 */
};
enum { SSE_SIDE_SOURCE = 0, SSE_SIDE_TARGET = 1 };

/* modelParams of SSEModel.__init__ (sse_model.py:94-126) */
typedef struct sse_config {
  int32_t network_mode;
  int32_t vocab_size;        /* V */
  int32_t embedding_size;    /* E */
  int32_t encoding_size;     /* S */
  int32_t src_cell_size;     /* H source */
  int32_t tgt_cell_size;     /* H target (ignored in shared-encoder, sse_model.py:269) */
  int32_t max_seq_length;    /* T */
  int32_t target_space_size; /* N targets (source-encoder-only / cnn modes) */
  int32_t device;            /* HIP device ordinal */
  float learning_rate;               /* sse_model.py:122 */
  float learning_rate_decay_factor;  /* sse_model.py:124 */
} sse_config;

/* SSEModel(modelParams) -- sse_model.py:94; sse_train.py:109 */
int sse_create(const sse_config *cfg, sse_handle **out);
void sse_destroy(sse_handle *h);
const char *sse_last_error(sse_handle *h);

/* Variables, addressed by their TF names ('word_embedding',
 * 'source_encoder/rnn/basic_lstm_cell/kernel', '.../bias', 'source_encoder/src_M',
 * ..., and '<name>/Adagrad' for the optimizer slots).  Replaces
 * saver.restore / saver.save (sse_model.py:138,379-386; sse_train.py:110-113). */
int sse_num_variables(sse_handle *h);
int sse_variable_info(sse_handle *h, int index, const char **name, int64_t *count, int32_t *rows, int32_t *cols);
int sse_set_variable(sse_handle *h, const char *name, const float *host, int64_t count);
int sse_get_variable(sse_handle *h, const char *name, float *host, int64_t count);

/* session.run([model.norm_src_seq_embedding | model.src_seq_embedding |
 * model.norm_tgt_seq_embedding], feed) -- sse_evaluator.py:107-109,
 * sse_index.py:90-92, sse_demo.py:121-125.  side: SSE_SIDE_*.  normalize=1
 * gives the l2-normalised encoding (sse_model.py:282-283). */
int sse_encode(sse_handle *h, int side, const int32_t *ids_host, int32_t B, int32_t T,
               int32_t normalize, float *out_host);
int sse_encode_dev(sse_handle *h, int side, const int32_t *ids_dev, int32_t B, int32_t T,
                   int32_t normalize, float *out_dev, void *stream);

/* Library options.  "pad_skip" (default 1): inference encodes skip the left-PAD prefix of
 * every 64-row tile exactly -- the LSTM state after p leading PAD (id 0) steps is
 * sequence-independent (sse_index.py:79-85 left-pads; sse_model.py:240-242 runs all T steps),
 * so it is precomputed per p with the same kernel; results are bit-identical to pad_skip = 0.
 * "pad_sort_dev" (default 1): with pad_skip, sse_encode_dev buckets the rows of a device-resident id matrix by their
 * leading-PAD count on the device (two small launches on the caller's stream, no host round trip) so that every row tile
 * skips its whole common prefix -- what sse_encode does with a host counting sort; outputs keep the caller's row order and
 * are bit-identical.  1 = adaptive (each eligible call measures its batch; rows are bucketed while the latest completed call
 * of that side saw padding, 32-row tiles while its mean prefix was >= T / 4), 2 = always, 0 = off.  Counter "pad_sorted_calls".
 * "lstm_gate_split" (default 1): inference encodes of cell sizes <= 128 at 64-row tiles (batches above 8192 rows) run the
 * gate-split kernel (one gate per wave, two phase-shifted 32-row groups per workgroup); bit-identical to 0.
 * "lstm_x_table" (default 1): LSTM encodes on the matrix kernel with 129 .. 512 hidden units start every step's gate
 * accumulators from a per-token table of x projections (the embedding row and bias through the kernel matrix, built once per
 * weight change by the recurrence's own MFMA chain) instead of recomputing them; bit-identical to 0.  1 = (re)build the
 * table when a batch holds at least as many tokens as the vocabulary (B * T >= vocab_size), use it while it is valid;
 * 2 = always build; 0 = off.  "lstm_x_table_mb" (default 256): largest table built, in MiB (vocab_size * 16 * cell size
 * bytes, rounded up to 32 units); above it the embedding-gather path runs.  Counter "lstm_x_table_builds".
 * "score_two_pass_min_rows" / "score_two_pass_rows" (defaults 49152 / 524288): sse_score_topk* on an index of that many rows
 * with >= 1024 queries, k <= 16 and bf16 candidates ranks by a max-only sweep -> per-query threshold -> collect sweep -> float64
 * select instead of the list sweep: the same exact ids and score bits; max 0 = off.  Counter "score_two_pass_calls".
 * "lstm_small_rows" (default 1024): LSTM encodes of at most this many rows (a demo / web query, an evaluator batch of
 * 600, the tail batch of an index build) run on the few-sequences kernel -- one workgroup per 4 rows, gate GEMV on the
 * vector ALUs streaming the kernel matrix from L2 instead of ~38 us per step for a 32-row matrix tile; the same fp32
 * fma chains in the same order as the matrix kernel: results are bit-identical (tests/test_gpu_encode.py).  0 disables.
 * "score_bf16" (default 1): the candidate pass of sse_score_topk* reads bf16 copies of the index and the queries on
 * the bf16 matrix pipe; the float64 re-scoring pass, its error bound widened to the bf16 rounding, still returns
 * exactly the reference's ids and scores (bit-identical to score_bf16 = 0), ~5x faster; +50 % index memory.  Queries
 * whose result misses the certificate (top scores packed closer than the bf16 bound) are swept again with fp32
 * candidates on the device before anything reaches the float64 brute force.  0 = fp32 candidates only.
 * "lstm_persist_rows" (default 32): encodes of at most this many rows (<= 32) run on a cluster of workgroups that keeps
 * the LSTM kernel matrix in LDS and exchanges h_t every step (single query 0.13 ms at H = 256, T = 32); bit-identical
 * to the other kernels; used only when the device has at least 2 x 8 x 16 CUs.  0 disables.  The cluster's workgroups
 * must be resident together: when one does not arrive within a bounded spin (device busy with other work) the
 * host-buffer entry points re-run the batch on the few-sequences kernel (counter "lstm_persist_fallbacks");
 * sse_encode_dev reports the condition through sse_synchronize.
 * "lstm_x3" (default 0): inference encodes of more than lstm_small_rows rows (cell sizes 64 .. 256, embedding < 64) run
 * their gate GEMMs as three bf16 MFMAs per product on hi + lo split fp32 operands (x = bf16(x) + bf16(x - bf16(x))):
 * NOT bit-identical to the fp32 path, ~2e-6 from it on normalised encodings, 2.2 - 2.9x faster.
 * "train_fwd_x3", "train_bwd_x3", "train_dk_x3" (default 0: sse_train_step* computes in fp32 MFMA throughout, the
 * reference's tf.float32 arithmetic; LSTM modes, cell sizes 64 .. 256): opt in to the forward, the BPTT recurrence (+ dX)
 * and the weight-gradient GEMM on split operands in the same way (~4e-6 relative per product; loss within ~1e-5 .. 1e-4
 * relative of the fp32 kernels; the forward and BPTT variants need train_dk_x3).
 * "train_pair_dedup" (default 1): a train batch whose rows 2i, 2i+1 carry the same source sequence (data.py:95-115 builds
 * every batch that way) runs the source encoder once per pair.  "lstm_train_rows" (0 | 32 | 64): fp32 training forward
 * tile rows (measurement aid).
 * "cnn_bf16" (default 0; source_only_cnn only): the convolution of inference encodes AND of the train step reads
 * embeddings and filters rounded to bf16 (fp32 masters, fp32 accumulation, fp32 bias/ReLU/pool/projection) on the bf16
 * matrix pipe -- the reference has no reduced-precision behaviour; BASELINE configs[4] names bf16.
 * "train_generic" (default 0): run the LSTM train step on the any-shape path whatever the shape (tests, A/B).
 * "train_serial" (default 0): run both encoders of a train step on one stream (profiling aid:
 * isolated kernel durations; same results).
 * "score_small_index" (default 1): >= 1024 queries against <= 1024 index rows (index dimensions 249 .. 256, 57 .. 64,
 * 49 .. 56: the evaluator's shape, sse_evaluator.py:104-112) are scored by one launch that forms all N scores per query and
 * selects the 16 best exactly, instead of the list sweep; identical results.  "score_small_x3" (default 1): that launch
 * forms its candidate scores from split-bf16 operands (hi = bf16(x), lo = bf16(x - hi); q.t ~ qh.th + qh.tl + ql.th on the bf16
 * matrix pipe, a sixth of the fp32 matrix cycles; the split image of the index is built once when the index is set).  The
 * scores only pick 16 candidates and bound the rows left out: every score returned is the float64 re-scoring and every id
 * follows the float64 order, certified with the bound (2^-15 (1 + 2^-6) + 2 (3 S + 2) 2^-24 (1 + 2^-5)) |q| max|t| (1.26e-4
 * at S = 256; fp32 candidates: 3.1e-5), so results are identical; a query whose 10th .. 16th scores sit closer than that
 * takes the collect path (counter "score_collect_queries").  Rows or queries of norm below 2^-100 are outside the bound's
 * claim.  0 = fp32 candidates (v_mfma_f32_32x32x2_f32).  "lstm_cluster_coop" (default 1): the cluster
 * encoder kernels are launched cooperatively (co-residency guaranteed by the runtime; ~20 us per call on ROCm 7.2; 0 =
 * plain launch, the give-up / fall-back path alone).  "lstm_cluster_backoff" (default -1 = automatic): eligible calls that go
 * straight to the kernels needing no co-residency after a cluster launch gave up (a give-up costs 10 ms); automatic arms 16
 * calls once a give-up was observed (another process on the device, or a refused cooperative launch).  "train_gen1" (default 0): the first-generation fp32 training
 * kernels instead of the round-4 ones (A/B and test aid; same results to fp32 summation order).
 * "eval_chunk_rows" (default 65536; >= 2, rounded down to even): sse_eval_loss* stages and encodes its pair rows in chunks of
 * at most this many, so that its scratch is bounded for any batch; the result does not depend on the value.
 * "train_loss" (default 0): the objective of sse_train_step* / sse_train_grads*, every network mode and every path.  0 = the
 * reference's pair loss (sigmoid cross-entropy on 64 cos(src_b, tgt_b), sse_model.py:298); 1 = the in-batch softmax loss of
 * sse_inbatch_loss_dev below over this call's rows, with keys the step forms itself: two rows carry the same source when
 * their source token rows are equal, the same target when their target token rows are equal (dual- and shared-encoder, by
 * ids or by corpus rows) or when they name the same row of the free target matrix (source-encoder-only, source_only_cnn).
 * In a data-parallel job that calls sse_train_grads* the negatives are the rank's own rows (the mean still runs over
 * rows_global); the open step below (sse_train_forward + sse_train_backward_inbatch_global) takes them from the global
 * batch of all ranks instead, and then equals the single-rank step of the concatenated batch.  Any other value is refused.  "train_loss_scale" (default 64, accepted 1 .. 256): the logit scale c of the in-batch loss; the pair loss keeps
 * the reference's 64.  Counter "train_inbatch_steps".  sse_eval_loss* evaluates the pair loss whatever train_loss says: its
 * result is independent of how the rows are chunked, which a softmax over the whole batch cannot be; the held-out measure of
 * the in-batch objective is sse_score_rank (MRR, recall@k), and sse_score_lse for the softmax over the whole INDEX, which
 * is chunk-independent: the full-softmax cross-entropy that the in-batch loss estimates.
 * "train_class_loss" (default 0, accepted 0 | 1): 1 = the loss stage of sse_train_step* / sse_train_grads* runs the class
 * softmax loss of sse_class_loss_dev below: a softmax over EVERY row of the free target matrix
 * target_embedding/tgt_seq_embedding, on every path, by ids and by corpus rows, with the logit scale of "train_loss_scale".
 * Two rows carry the same source when their source token rows are equal.  The gradient of the matrix is dense (every class
 * is a negative of every row) and enters clip_by_global_norm whole, like a projection matrix, instead of through the
 * IndexedSlices slice norm; sse_train_apply takes that from the kind of step that left the pending gradients, not from the
 * option's value at the time.  The objective decomposes over the rows of a batch, so a data-parallel step equals the
 * single-rank step of the concatenated batch up to summation order, at any world size.  A step under this option is refused
 * when the network mode has no free target matrix (dual-encoder, shared-encoder), or when "train_loss" = 1 is set as well
 * (two objectives).  Counter "train_class_steps". */
int sse_set_option(sse_handle *h, const char *name, int32_t value);
/* Diagnostic counters (cumulative).  "score_bf16_second_chance_queries": queries whose bf16-candidate result missed
 * its certificate and were re-run with fp32 candidates.  "score_collect_queries": queries served by the collect path
 * (k > 16, or a k-th score tied with rows outside the candidate lists: one more grid-wide sweep gathers every row that
 * can be in the exact top-k).  "score_bruteforce_queries": queries that fell through to the one-workgroup-per-query
 * float64 sweep (k > 1024, or more than 4096 rows within the fp32 bound of the k-th score).
 * "lstm_persist_fallbacks": host-buffer encodes re-run on the few-sequences kernel (see option lstm_persist_rows).
 * "lstm_coop_refused" (process-wide): cooperative launches the runtime refused -- the plain launch was taken instead.
 * Which kernel an LSTM inference encode was sent to, one count per encode (a host-buffer encode that falls back after a
 * cluster give-up counts twice: the kernel that gave up and the one that re-ran it): "lstm_path_persist" (single-query
 * cluster kernel), "lstm_path_cluster" (MFMA cluster kernel), "lstm_path_small" (few-sequences kernel), "lstm_path_x3"
 * (split-bf16 matrix kernel), "lstm_path_generic" (any-shape path), "lstm_path_fwd" (fp32 matrix kernel).  Of the matrix
 * kernel's encodes: "lstm_fwd_rows32" / "lstm_fwd_rows64" (rows per workgroup; they add up to lstm_path_fwd),
 * "lstm_fwd_gate_split" (the gate-split kernel for small cells; the others ran the unit-block kernel), "lstm_fwd_x_table"
 * (gate accumulators from the x-projection table; the others gathered embedding rows).  The pad-prefix table builds a
 * kernel does for itself are not counted.
 * "eval_paired_calls": sse_eval_loss* calls that ran the source encoder once per pair of rows (option train_pair_dedup).
 * "train_path_fused" / "train_path_generic" / "train_path_cnn": train steps (sse_train_grads*, sse_train_step*) by path.
 * "train_paired_steps": fused steps that ran the source encoder on one row of every pair (option train_pair_dedup).
 * "train_fp32_repacks": steps that rebuilt the fp32 Kh^T / Kx^T fragment copies of the BPTT kernels.
 * "train_split_repacks": steps that rebuilt their split-operand forms (options train_bwd_x3 + train_dk_x3).
 * "train_generic_repacks": packs of the any-shape path built, one per encoder side.
 * "train_inbatch_steps": train steps whose loss stage ran the in-batch softmax head (option train_loss = 1).
 * "train_class_steps": train steps whose loss stage ran the class softmax head (option train_class_loss = 1).
 * "train_open_steps": sse_train_forward* calls that left a step open.
 * "train_global_inbatch_steps": open steps closed by sse_train_backward_inbatch_global.
 * "score_rank_band_rows" / "score_rank_bruteforce_pairs": see sse_score_rank.
 * "score_above_band_rows" / "score_above_bruteforce_pairs" / "score_above_long_segments": see sse_score_above.
 * "score_filtered_collected_rows" / "score_filtered_bruteforce_queries" / "score_filtered_tiles_skipped": see
 * sse_score_topk_filtered.
 * "score_grouped_collected_rows" / "score_grouped_bruteforce_queries": see sse_score_topk_grouped.
 * "score_lse_calls" / "score_lse_tiles_skipped": see sse_score_lse.
 * "index_update_calls" / "index_update_rows" / "index_append_rows" / "index_grow_copies": see sse_index_update. */
int sse_get_counter(sse_handle *h, const char *name, int64_t *value);

/* tf.nn.l2_normalize(x, dim=-1) on device rows (sse_model.py:282-283). */
int sse_l2_normalize_dev(sse_handle *h, const float *x_dev, float *out_dev, int64_t rows, int32_t cols,
                         void *stream);

/* In-batch softmax loss (multiple-negatives ranking loss) over B pair rows of un-normalised encodings [B][S], with its
 * gradient; the loss stage of the train step under option train_loss = 1, and usable with a caller's own encoders.
 *   ns_i = s_i / sqrt(max(|s_i|^2, 1e-12)), nt_j likewise;  L_ij = scale * ns_i . nt_j
 *   column j is admitted for row i when j == i, or when tgt_key_j != tgt_key_i and not (src_key_j == src_key_i and
 *       labels_j != 0): a row with the same target, or another verified target of the same source, is no negative; a row
 *       with label 0 still lends its target as a negative column
 *   lse_i = log sum_{j admitted} exp(L_ij)  (row maximum subtracted);  row_loss_i = labels_i * (lse_i - L_ii)
 *   row_acc_i = 1 when labels_i != 0 and no admitted j != i has L_ij > L_ii, else 0
 *   G_ij = labels_i * scale * inv_rows * (p_ij - [i == j]), p_ij = exp(L_ij - lse_i) on admitted columns, else 0
 *   d(ns_i) = sum_j G_ij nt_j, d(nt_j) = sum_i G_ij ns_i; d_src / d_tgt follow by the l2_normalize backward (below 1e-12
 *       the clamp passes no gradient to the norm)
 * The loss of the batch is inv_rows * sum_i row_loss_i, its accuracy inv_rows * sum_i row_acc_i; the caller adds them up.
 * src_key_dev / tgt_key_dev: [B] int64 on the device, equal values = the same source / target; NULL = every row distinct.
 * d_src_dev / d_tgt_dev: [B][S], or both NULL for loss and accuracy alone.  scale in (0, 256].
 * All arithmetic is fp32 (logits and both gradient products on v_mfma_f32_32x32x2_f32); no B x B buffer exists, the logit
 * tiles are recomputed by each of the three passes; every sum is taken in an order fixed by (B, S), no atomics: the same
 * inputs give the same bits.  Queued on `stream`, no host synchronisation; the scratch (O(B * S + B)) belongs to the handle
 * and only grows.  Bad arguments are refused before anything is queued. */
int sse_inbatch_loss_dev(sse_handle *h, const float *src_raw_dev, const float *tgt_raw_dev, const float *labels_dev,
                         const int64_t *src_key_dev, const int64_t *tgt_key_dev, int32_t B, int32_t S, float scale,
                         float inv_rows, float *d_src_dev, float *d_tgt_dev, float *row_loss_dev, float *row_acc_dev,
                         void *stream);

/* The same head over the B rows of a batch with its OUTPUTS cut to the window of rows [row_lo, row_hi): what one rank of a
 * data-parallel step runs over the gathered global batch (B = rows of all ranks, the window = the rank's own rows).
 *   d_src_dev / d_tgt_dev: [row_hi - row_lo][S] (or both NULL), row_loss_dev / row_acc_dev: [row_hi - row_lo]; output row r
 *   is row row_lo + r of the batch.  Everything else is an argument of sse_inbatch_loss_dev and means the same.
 * Semantics are those of the full head restricted to the window: d(ns_i) of a window row sums over all B columns, d(nt_j) of
 * a window column over all B rows.  So lse_i is formed for every row of the batch; only the two gradient passes, the
 * l2_normalize backward and the loss outputs shrink, to the 32-row tiles of the batch's numbering that meet the window.  Every
 * order of summation still depends on (B, S) alone: each output row is bit-identical to the same row of sse_inbatch_loss_dev on
 * the same inputs, for windows not aligned to 32 and windows inside one tile alike, and the window [0, B) queues exactly the
 * launches of sse_inbatch_loss_dev.
 * Cost per call (per rank): one rows pass of B^2 * 2S flop, plus two gradient passes of (row_hi - row_lo) * B * 2S flop each
 * (rounded up to whole 32-row tiles).  Only the gradient passes shrink with the world size; the rows pass is repeated on
 * every rank.
 * Refused before anything is queued, each with its own text: row_lo < 0, row_hi > B, an empty or inverted window
 * (row_lo >= row_hi), and everything sse_inbatch_loss_dev refuses. */
int sse_inbatch_loss_window_dev(sse_handle *h, const float *src_raw_dev, const float *tgt_raw_dev, const float *labels_dev,
                                const int64_t *src_key_dev, const int64_t *tgt_key_dev, int32_t B, int32_t S,
                                int32_t row_lo, int32_t row_hi, float scale, float inv_rows, float *d_src_dev,
                                float *d_tgt_dev, float *row_loss_dev, float *row_acc_dev, void *stream);

/* Class softmax loss: the full-softmax cross-entropy of B source encodings [B][S] against ALL N rows of a class table
 * [N][S] (both un-normalised), with its gradient; the loss stage of the train step under option train_class_loss = 1, and
 * usable with a caller's own encoder and table.  Row i names its class y_i = tgt_row_i in [0, N).
 *   ns_i = s_i / sqrt(max(|s_i|^2, 1e-12)), nt_j likewise;  L_ij = scale * ns_i . nt_j, j over all N rows of the table
 *   column j is excluded for row i when j != y_i and some row r has src_key_r == src_key_i, labels_r != 0, y_r == j: another
 *       verified class of the same source is no negative, for any number of verified classes per source; a row with label 0
 *       excludes nothing and its own class stays a negative column; y_i itself is always admitted
 *   lse_i = log sum_{j admitted} exp(L_ij)  (running maximum subtracted; the excluded terms are never formed and subtracted)
 *   row_loss_i = labels_i * (lse_i - L_{i,y_i})
 *   row_acc_i = 1 when labels_i != 0 and no admitted j != y_i has L_ij > L_{i,y_i}, else 0
 *   G_ij = labels_i * scale * inv_rows * (p_ij - [j == y_i]), p_ij = exp(L_ij - lse_i) on admitted columns, else 0
 *   d(ns_i) = sum_j G_ij nt_j, d(nt_j) = sum_i G_ij ns_i for EVERY j, also classes no row names; d_src / d_table follow by
 *       the l2_normalize backward (below 1e-12 the clamp passes no gradient to the norm)
 * The loss of the batch is inv_rows * sum_i row_loss_i, its accuracy inv_rows * sum_i row_acc_i; the caller adds them up.
 * tgt_row_dev: [B] int32 on the device.  A row outside [0, N) is found on the device: it raises the handle's error flag as a
 * bad target row of a train step does (reported by sse_synchronize), its loss, accuracy and gradient share are 0.
 * src_key_dev: [B] int64 on the device, equal values = the same source; NULL = every row a source of its own.
 * d_src_dev [B][S] and d_table_dev [N][S] (every row written), or both NULL for loss and accuracy alone.  scale in (0, 256].
 * All arithmetic is fp32 (logits and both gradient products on v_mfma_f32_32x32x2_f32); no B x N buffer exists, the logit
 * tiles are recomputed by each of the three passes; where B or N alone leaves too few workgroups the other dimension is
 * split over workgroups and the partial results are combined in index order; every sum is taken in an order fixed by
 * (B, N, S), no atomics: the same inputs give the same bits.  Queued on `stream`, no host synchronisation; the scratch
 * (O((B + N) * S + B), plus the partial gradients of a split walk: at most 512 * 32 * Sp floats per gradient, Sp = S rounded
 * up to 32, i.e. 16 MiB each at S = 256) belongs to the handle and only grows.  Refused before anything is queued, each with
 * its own text: B, N or S below 1; a NULL among the required pointers; one gradient pointer without the other; scale outside
 * (0, 256]. */
int sse_class_loss_dev(sse_handle *h, const float *src_raw_dev, const float *table_dev, const int32_t *tgt_row_dev,
                       const float *labels_dev, const int64_t *src_key_dev, int32_t B, int32_t N, int32_t S, float scale,
                       float inv_rows, float *d_src_dev, float *d_table_dev, float *row_loss_dev, float *row_acc_dev,
                       void *stream);

/* The target index (Evaluator.__init__ builds it from targetEncodingIndex.tsv,
 * sse_evaluator.py:80-92; sse_demo.py:79-90).  Rows are uploaded once and stay
 * resident.  *_f64 keeps the float64 values the reference parses from text for
 * the exact re-scoring pass; id_base is added to row numbers in results (row
 * shards of one index).  sse_index_set_dev adopts rows already on
 * the device (copied).  A shape the scorer cannot hold (N <= 0, S <= 0,
 * S > 1024, N > 2147483000) is refused with a message before anything is
 * touched: the resident index, its float64 rows, tags and group keys stay. */
int sse_index_upload(sse_handle *h, const float *rows_host, int64_t N, int32_t S, int64_t id_base);
int sse_index_upload_f64(sse_handle *h, const double *rows_host, int64_t N, int32_t S, int64_t id_base);
int sse_index_set_dev(sse_handle *h, const float *rows_dev, int64_t N, int32_t S, int64_t id_base,
                      void *stream);

/* Rows, dimension and id_base of the resident index, and norm_max, the largest row norm as the library formed it in fp32 (the
 * bound every certificate of the scorer scales with); zeros when no index is resident; any pointer may be NULL.  The id an
 * append will give its first row is id_base + N. */
int sse_index_shape(sse_handle *h, int64_t *N, int32_t *S, int64_t *id_base, float *norm_max);

/* Update and append rows of the resident index in place (DESIGN K6n).  The contract: after any sequence of these calls the
 * handle answers every scoring entry point, bit for bit and counter for counter, as a fresh handle that was given the final
 * rows through the same upload entry and then the final tags, group keys and bias.  The cost is O(M S) plus one pass over N
 * floats (the norm bound and max |bias| can fall as well as rise), never O(N S) -- except the copy of an append that
 * outgrows its allocation (storage grows geometrically on that path only; counter "index_grow_copies").
 *
 * update: ids [M] are global ids in [id_base, id_base + N), strictly increasing; rows [M][S] replace those rows.  rows may
 * be NULL when at least one column is given: then only the rows' tag words, group keys or bias values change.  A non-NULL
 * column must be set on the resident index (sse_index_set_tags / _groups / _bias); a NULL column keeps every row's value.
 * append: the M new rows take the ids id_base + N .. id_base + N + M - 1 (N grows by M; id_base and S never change); each
 * column must be given exactly when it is set on the resident index (no default key or tag is invented).
 * The _f64 forms serve an index uploaded with sse_index_upload_f64: they patch its float64 rows and form the fp32 images
 * from (float) of them as that upload does.  A float form with rows on such an index, and an _f64 form on any other, is
 * refused: there is one source of truth.
 * Refused with a message before anything is touched: no resident index, a wrong column combination, an id out of range or
 * ids not strictly increasing (host forms), N + M > 2147483000, a non-finite host bias.  M == 0 succeeds and changes
 * nothing.  The _dev forms take every operand from device memory and run on `stream`; sse_index_update_dev checks the ids
 * on the device: a bad list raises the handle's error word, every later kernel of the call that takes the list reads it and
 * writes nothing, and the call fails having changed nothing (the tile sums and max |bias| are formed again from the unchanged
 * columns).  Both _dev forms synchronise `stream` once (the norm bound lives on the host), and an append that
 * reallocates frees the old storage: work queued on OTHER streams must have finished with the index before it.
 *
 * There is no removal and no compaction: a row's id is id_base + its position, and compaction would renumber other rows
 * behind the caller's back.  To hide a row, reserve one tag bit for "hidden", set it on that row with a columns-only update
 * (rows == NULL, tags = the row's word with the bit), and pass the bit as none_of to sse_score_topk_filtered / _grouped /
 * _after; clearing the bit brings the row back.
 * Counters: "index_update_calls", "index_update_rows", "index_append_rows", "index_grow_copies". */
int sse_index_update(sse_handle *h, const int64_t *ids, const float *rows, int64_t M, const uint64_t *tags,
                     const int64_t *groups, const float *bias);
int sse_index_update_f64(sse_handle *h, const int64_t *ids, const double *rows, int64_t M, const uint64_t *tags,
                         const int64_t *groups, const float *bias);
int sse_index_update_dev(sse_handle *h, const int64_t *ids_dev, const float *rows_dev, int64_t M, const uint64_t *tags_dev,
                         const int64_t *groups_dev, const float *bias_dev, void *stream);
int sse_index_append(sse_handle *h, const float *rows, int64_t M, const uint64_t *tags, const int64_t *groups,
                     const float *bias);
int sse_index_append_f64(sse_handle *h, const double *rows, int64_t M, const uint64_t *tags, const int64_t *groups,
                         const float *bias);
int sse_index_append_dev(sse_handle *h, const float *rows_dev, int64_t M, const uint64_t *tags_dev,
                         const int64_t *groups_dev, const float *bias_dev, void *stream);

/* np.dot(srcEnc, tgtEnc.T) + data_utils.getSortedResults, first k columns only
 * (sse_evaluator.py:110-112, data_utils.py:263-267, sse_demo.py:126-129).
 * Scores are float64 like the reference's; ties rank the lower row id first.
 * out_scores [Q,k] float64, out_ids [Q,k] int64. */
int sse_score_topk(sse_handle *h, const float *q_host, int32_t Q, int32_t k, double *out_scores,
                   int64_t *out_ids);
int sse_score_topk_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, double *out_scores_dev,
                       int64_t *out_ids_dev, void *stream);

/* Exact rank of labelled targets over the WHOLE index: where row g lands in sse_score_topk(..., k = N) without forming that
 * list.  Replaces a full getSortedResults row searched for the label (data_utils.py:263-267: np.argsort of all N scores
 * per query, of which sse_evaluator.py:95,112 then reads 10 columns): what mean reciprocal rank, mean / median rank and
 * recall at any k need.  Pairs are the unit of work: pair p is query row pair_q[p] (in [0, Q)) and a threshold (score,
 * pair_id[p]); out_before[p] = the number of rows r of the resident index with score64(q, r) > score, or == score and
 * id_base + r < pair_id[p] -- the order sse_score_topk ranks by, score64 being the float64 dot product it returns.
 *   pair_score_in == NULL: every pair_id[p] must be a row of this index (id_base <= id < id_base + N); the score is
 *     score64(q, that row), bit-identical to what sse_score_topk returns for it, and out_before[p] is the row's 0-based
 *     rank.  out_score (may be NULL) receives the scores.
 *   pair_score_in != NULL: the thresholds are (pair_score_in[p], pair_id[p]), the id any int64 -- what a row shard counts
 *     for a label that lives in another shard.  Counts of shards add: the global rank is their sum.
 * The counts come from one fp32 MFMA sweep per 4096 pairs (compare-and-count, no lists); only rows whose fp32 score lies
 * within the certified bound of the threshold are re-scored in float64 (counter "score_rank_band_rows"); a pair with more
 * than 4096 such rows is counted by a float64 sweep (counter "score_rank_bruteforce_pairs").  Results are exact either way.
 * Rows or queries of norm below 2^-100 and non-finite input are outside the claim (no fault).
 * A pair_q out of [0, Q), an id out of range in the first form, or no index: error with a message, no output written, the
 * handle stays usable.  L == 0 succeeds.  The host form runs on the null stream and synchronises; the _dev form takes
 * device pointers, enqueues on `stream`, and reports a bad pair through sse_synchronize (like sse_encode_dev). */
int sse_score_rank(sse_handle *h, const float *q_host, int32_t Q, const int32_t *pair_q, const int64_t *pair_id, int64_t L,
                   const double *pair_score_in, int64_t *out_before, double *out_score);
int sse_score_rank_dev(sse_handle *h, const float *q_dev, int32_t Q, const int32_t *pair_q_dev, const int64_t *pair_id_dev,
                       int64_t L, const double *pair_score_in_dev, int64_t *out_before_dev, double *out_score_dev,
                       void *stream);

/* All rows of the resident index that score at least a threshold: per-query result lengths instead of one global k.
 * Replaces a full getSortedResults row cut at a confidence (sse_evaluator.py:110-112 ranks every target and keeps nbest,
 * data_utils.py:263-267 sorts all N float64 scores per query): an answer set with a cut-off instead of nbest, all positives
 * of a query, a near-duplicate self-join, the predicted-positive set behind precision and recall at a threshold.
 * Pairs are the unit of work, as in sse_score_rank: pair p is query row pair_q[p] (in [0, Q)) and threshold pair_thr[p]; one
 * query may carry several thresholds.  Row r matches pair p iff score64(q, r) >= pair_thr[p], score64 being the float64 dot
 * product sse_score_topk returns for that row, bit for bit; the comparison is IEEE (+inf and NaN match nothing, -inf every row).
 *   out_offsets [L + 1] is always written: out_offsets[0] = 0, out_offsets[p + 1] - out_offsets[p] = the exact match count
 *     of pair p (= sse_score_rank with pair_score_in = pair_thr and pair_id = INT64_MAX).
 *   out_ids / out_scores (both or neither, `cap` entries each) are written iff they are given and out_offsets[L] <= cap:
 *     segment [out_offsets[p], out_offsets[p + 1]) holds id_base + r and score64 of pair p's rows, score descending, equal
 *     scores by ascending id -- exactly the first count[p] columns of sse_score_topk(..., k = N) for that query.  When the
 *     total exceeds cap, or the lists are NULL (count-only, cap ignored), the lists are left untouched and the call still
 *     succeeds: read out_offsets[L] and come back with enough room.
 * Counts of row shards add; their lists concatenate and merge in the same order (ids are global through id_base).
 * One fp32 MFMA sweep per 4096 pairs counts (rows within the certified bound of the threshold are decided in float64: counter
 * "score_above_band_rows"; a pair with more than 4096 such rows is counted and listed by a float64 sweep: counter
 * "score_above_bruteforce_pairs"; both counters rise once per call, in its counting pass), a scan of the counts gives the offsets, the same sweep again appends the rows, and the
 * segments are scored in float64 and sorted (more than 8192 entries: merged through global memory, counter
 * "score_above_long_segments").  Scratch is O(L + cap), never Q x N.  Results are exact and deterministic.
 * Rows or queries of norm below 2^-100 and non-finite input are outside the claim (no fault).
 * A pair_q out of [0, Q) or no index: error with a message, no output written, the handle stays usable.  L == 0 succeeds
 * and writes out_offsets[0] = 0.  The host form runs on the null stream and synchronises; the _dev form takes device
 * pointers, enqueues on `stream`, never waits for the device (whether the total fits cap is decided there), and reports a
 * bad pair through sse_synchronize (like sse_score_rank_dev). */
int sse_score_above(sse_handle *h, const float *q_host, int32_t Q, const int32_t *pair_q, const double *pair_thr, int64_t L,
                    int64_t cap, int64_t *out_offsets, int64_t *out_ids, double *out_scores);
int sse_score_above_dev(sse_handle *h, const float *q_dev, int32_t Q, const int32_t *pair_q_dev, const double *pair_thr_dev,
                        int64_t L, int64_t cap, int64_t *out_offsets_dev, int64_t *out_ids_dev, double *out_scores_dev,
                        void *stream);

/* Tags of the resident index: one 64-bit word per row, copied and kept on the device (with the OR of every 32-row tile's
 * words beside them).  N must equal the index's row count, otherwise the call errors with a message and the tags stay as
 * they were.  tags == NULL clears them; setting, uploading or adopting a new index (sse_index_upload*, sse_index_set_dev)
 * clears them too.  The _dev form takes a device pointer and enqueues the copy on `stream`. */
int sse_index_set_tags(sse_handle *h, const uint64_t *tags_host, int64_t N);
int sse_index_set_tags_dev(sse_handle *h, const uint64_t *tags_dev, int64_t N, void *stream);

/* Exact top-k among the rows a query may return: the best leaves under a known meta-category (sse_model.py:36-41 maps a
 * title to one of 20,000+ leaf categories, webserver.py:158-159 returns targetCategoryId), the hardest negatives of a
 * labelled source (data.py:95-115 samples them at random), neighbours other than the row itself.  Row r of the index is
 * ELIGIBLE for query q iff (q_any[q] == 0 || (tags[r] & q_any[q]) != 0) && (tags[r] & q_none[q]) == 0 and id_base + r is not
 * among excl_ids[q * n_excl .. (q + 1) * n_excl).  q_any / q_none == NULL mean all-zero words (no requirement); giving either
 * while no tags are set is an error.  excl_ids may be NULL with n_excl == 0; 0 <= n_excl <= 64; entries outside
 * [id_base, id_base + N) (a padding value such as -1, ids of another shard) are ignored, duplicates are allowed.
 *   out_counts [Q]: c = min(k, eligible rows of q).
 *   out_scores / out_ids [Q][k]: columns 0 .. c of row q are exactly the columns of sse_score_topk(..., k = N) for that query
 *     with the ineligible rows removed -- the same float64 score bits, score descending, equal scores by ascending id, ids
 *     including id_base; columns c .. k hold (-inf, INT64_MAX).  1 <= k <= 1024; k may exceed N.
 * With no masks and n_excl == 0 the columns are sse_score_topk's.  The filter is inside the sweep: an fp32 MFMA sweep keeps
 * maxima of tag-eligible rows over disjoint row sets, their (k + n_excl)-th largest less twice the certified bound is a
 * threshold no row of the answer scores below, the same sweep again collects every tag-eligible row at or above it, and
 * those are re-scored in float64 without the excluded ids and sorted (counter "score_filtered_collected_rows"); a query
 * with more than 4096 such rows is served by a float64 sweep of the whole index ("score_filtered_bruteforce_queries").
 * Index tiles none of whose rows carries a bit any query of a workgroup's query block asks for are skipped
 * ("score_filtered_tiles_skipped", counted in the first sweep; option "score_filtered_skip", default 1, 0 = never skip:
 * the results are identical).  Scratch is bounded by the chunk of 4096 queries.  Rows or queries of norm below 2^-100 and
 * non-finite input are outside the claim (no fault).
 * Q == 0 succeeds.  No index, k or n_excl out of range, masks without tags: error with a message, no output written, the
 * handle stays usable.  The host form runs on the null stream and synchronises; the _dev form takes device pointers,
 * enqueues on `stream` and never waits for the device. */
int sse_score_topk_filtered(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const uint64_t *q_any,
                            const uint64_t *q_none, const int64_t *excl_ids, int32_t n_excl, double *out_scores,
                            int64_t *out_ids, int32_t *out_counts);
int sse_score_topk_filtered_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const uint64_t *q_any_dev,
                                const uint64_t *q_none_dev, const int64_t *excl_ids_dev, int32_t n_excl,
                                double *out_scores_dev, int64_t *out_ids_dev, int32_t *out_counts_dev, void *stream);

/* Group keys of the resident index: one int64 key per row, copied and kept on the device.  Any value is a key (negative
 * ones, keys above 2^32, INT64_MAX); rows with equal keys form a group.  N must equal the index's row count, otherwise the
 * call errors with a message and the keys stay as they were.  groups == NULL clears them; setting, uploading or adopting a
 * new index (sse_index_upload*, sse_index_set_dev) clears them too.  Tags and group keys are independent of each other.  The
 * _dev form takes a device pointer and enqueues the copy on `stream`. */
int sse_index_set_groups(sse_handle *h, const int64_t *groups_host, int64_t N);
int sse_index_set_groups_dev(sse_handle *h, const int64_t *groups_dev, int64_t N, void *stream);

/* Exact top-k DISTINCT groups, when several index rows stand for the same thing: the leaf categories of a title, each
 * represented by many labelled example titles rather than by its one name (README: "one or multiples of the 20,000+ leaf
 * categories"), result pages that collapse the listings of one product or near-duplicate cluster.  Row eligibility is the
 * tag rule of sse_score_topk_filtered (q_any / q_none may be NULL; giving either while no tags are set is an error); there
 * are no exclusion lists.  For query q take the columns of sse_score_topk(..., k = N) -- the float64 score bits, score
 * descending, equal scores by ascending id -- remove the ineligible rows, then every row whose group already appeared to its
 * left.  Of what remains:
 *   out_counts [Q]: c = min(k, groups with an eligible row).
 *   out_scores / out_ids / out_groups [Q][k]: columns 0 .. c are the first c entries: each group once, represented by its
 *     best row (the lowest id among equal bests), ids including id_base, out_groups that row's key; columns c .. k hold
 *     (-inf, INT64_MAX, INT64_MAX) -- out_counts is authoritative, a real group may carry that key.
 * 1 <= k <= 1024; k may exceed the number of groups or N.  With every row in a group of its own and no masks the score and id
 * columns are sse_score_topk's.  The stages are sse_score_topk_filtered's with a threshold from distinct groups: an fp32
 * MFMA sweep keeps the maxima of tag-eligible rows over disjoint row sets together with their rows, the k-th largest of
 * the per-group bests among them less twice the certified bound is a threshold the representative of no answer group
 * scores below, the collect sweep takes every tag-eligible row at or above it, those are re-scored in float64, reduced to
 * one entry per group and sorted (counter "score_grouped_collected_rows"); a query with more than 4096 such rows -- one
 * that sits deep inside a large group whose rows all outscore the k-th group -- is served by a float64 sweep of the whole
 * index with the same reduction ("score_grouped_bruteforce_queries"); the result is exact either way.  Option
 * "score_filtered_skip" governs the tile skip here too and changes no result.  Scratch is bounded by the chunk of 4096
 * queries.  Rows or queries of norm below 2^-100 and non-finite input are outside the claim (no fault).
 * Q == 0 succeeds.  No index, no group keys, k out of range, masks without tags: error with a message, decided on the host
 * before anything is queued, no output written, the handle stays usable.  The host form runs on the null stream and
 * synchronises; the _dev form takes device pointers, enqueues on `stream` and never waits for the device. */
int sse_score_topk_grouped(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const uint64_t *q_any,
                           const uint64_t *q_none, double *out_scores, int64_t *out_ids, int64_t *out_groups,
                           int32_t *out_counts);
int sse_score_topk_grouped_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const uint64_t *q_any_dev,
                               const uint64_t *q_none_dev, double *out_scores_dev, int64_t *out_ids_dev,
                               int64_t *out_groups_dev, int32_t *out_counts_dev, void *stream);

/* Exact next page of the ranked list: the k best rows AFTER a (score, id) cursor, in the order sse_score_topk ranks by.  The
 * reference cuts the sorted row of every target at nbest (webserver.py:144-151); what follows the rows a caller already holds
 * is asked for here by handing back the last (score, id) it saw.  The cursor is stateless, and the same cursor is valid on
 * every row shard because ids are global through id_base.
 *   Row r is AFTER the cursor of query q iff score64(q, r) < after_score[q], or score64(q, r) == after_score[q] and
 *   id_base + r > after_id[q], where score64 is the float64 dot product sse_score_topk returns for that row, bit for bit,
 *   and the comparisons are IEEE: a cursor score of +inf puts every row after it (the first page), NaN and -inf none.  The
 *   cursor need not be a row of this index: any (double, int64) is valid -- what a shard gets for a cursor row that lives
 *   elsewhere.
 * after_score and after_id are both given or both NULL; both NULL means no cursor (every row is after it).  Row eligibility is
 * the tag rule of sse_score_topk_filtered (q_any / q_none may be NULL; giving either while no tags are set is an error); there
 * are no exclusion lists.
 *   out_counts [Q]: c = min(k, eligible rows after the cursor).
 *   out_scores / out_ids [Q][k]: columns 0 .. c of row q are exactly the columns of sse_score_topk(..., k = N) for that query
 *     with the ineligible rows and the rows not after the cursor removed -- the same float64 score bits, score descending,
 *     equal scores by ascending id, ids including id_base; columns c .. k hold (-inf, INT64_MAX).  1 <= k <= 1024; k may
 *     exceed N.
 * Feeding the last (score, id) of a page back as the cursor yields the following rows: pages concatenated are
 * sse_score_topk(k = N).  With e the certified fp32 bound of the query, a first kernel brackets the cursor score by
 * lo = (after_score - e) rounded down and hi = (after_score + e) rounded up to fp32; the fp32 MFMA sweep keeps maxima over
 * disjoint row sets of the tag-eligible rows below lo (certainly after the cursor), their k-th largest less 2 e is a threshold
 * no row of the answer scores below, the same sweep again collects every tag-eligible row from there up to hi, and those are
 * re-scored in float64, the rows not after the cursor dropped on (score64, id), the rest sorted (counter
 * "score_after_collected_rows": rows re-scored); a query with more than 4096 such rows is served by a float64 sweep of the
 * whole index with the same predicate ("score_after_bruteforce_queries").  Option "score_filtered_skip" governs the tile skip
 * here too and changes no result.  Scratch is bounded by the chunk of 4096 queries.  Rows or queries of norm below 2^-100 and
 * non-finite rows or queries are outside the claim (no fault); non-finite cursors are inside it, as stated above.
 * Q == 0 succeeds.  No index, k out of range, one cursor array without the other, masks without tags: error with a message,
 * decided on the host before anything is queued, no output written, the handle stays usable.  The host form runs on the null
 * stream and synchronises; the _dev form takes device pointers, enqueues on `stream` and never waits for the device. */
int sse_score_topk_after(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const double *after_score,
                         const int64_t *after_id, const uint64_t *q_any, const uint64_t *q_none, double *out_scores,
                         int64_t *out_ids, int32_t *out_counts);
int sse_score_topk_after_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const double *after_score_dev,
                             const int64_t *after_id_dev, const uint64_t *q_any_dev, const uint64_t *q_none_dev,
                             double *out_scores_dev, int64_t *out_ids_dev, int32_t *out_counts_dev, void *stream);

/* The confusions of a training source: the best k index rows that are NOT among its verified targets and score at or above a
 * floor derived from them.  The reference declares get_hard_learning_train_batch and compute_training_confusion_sampes and
 * leaves both empty (data.py:124-129: "Not implemented yet."); the only negatives it trains on are uniform draws
 * (data.py:108-114).  A hard negative matters when it scores near or above the source's best verified target; that score
 * differs per query and is formed here on the device, so mining is one call with no host round trip.
 *   Positives: pos_ids is [Q][n_pos], 1 <= n_pos <= 64, the layout and cap of excl_ids.  Entries outside
 *     [id_base, id_base + N) (a padding value such as -1, ids of another shard) are ignored, duplicates are allowed.  P(q) is
 *     the set of in-range entries of row q.
 *   Best positive: (m, b) is the first of {(score64(q, p), p) : p in P(q)} by score descending, then ascending id, where
 *     score64 is the float64 dot product sse_score_topk returns for that row, bit for bit.  P(q) empty: (-inf, INT64_MAX).
 *     out_pos_score / out_pos_id [Q] receive (m, b); either may be NULL.
 *   Floor: f = m - margin, formed once in IEEE double on the device.  margin is finite or +inf; margin = +inf or an empty P(q)
 *     give f = -inf, no cut.
 *   Row r is a CONFUSION of q iff id_base + r is not in P(q) and score64(q, r) >= f.
 *   out_counts [Q]: c = min(k, confusions of q).
 *   out_scores / out_ids [Q][k]: columns 0 .. c of row q are exactly the columns of sse_score_topk(..., k = N) for that query
 *     with the positives and the rows below f removed -- the same float64 score bits, score descending, equal scores by
 *     ascending id, ids including id_base; columns c .. k hold (-inf, INT64_MAX).  1 <= k <= 1024; k may exceed N.
 * The call takes no tag masks: every row is tag-eligible whatever tags the index carries, and no tile is skipped.  With
 * margin = +inf the columns are those of sse_score_topk_filtered(excl_ids = pos_ids) without masks.  With e the certified fp32
 * bound of the query, a first kernel scores the positives in float64 and forms f and flo = (f - e) rounded down to fp32; the
 * filtered call's fp32 MFMA sweep keeps maxima over disjoint row sets; the collect threshold is the larger of the filtered
 * call's (the (k + n_pos)-th largest maximum less 2 e) and flo: a row of the answer has score64 >= f, hence an fp32 score
 * >= f - e >= flo, and it is among the best k non-positives, which the filtered call's argument puts at or above the other
 * term.  The same sweep again collects every row at or above the threshold (counter "score_confusions_collected_rows": rows
 * collected, the positives among them included); those are re-scored in float64 without the positives, the rows below f
 * dropped, the rest sorted.  A query with more than 4096 collected rows is served by a float64 sweep of the whole index with
 * the same tests ("score_confusions_bruteforce_queries"); "score_confusions_floor_queries" counts the queries whose
 * threshold is flo.  Only the float64 comparison decides membership.  Scratch is bounded by the chunk of 4096 queries.  Rows
 * or queries of norm below 2^-100 and non-finite input are outside the claim (no fault).
 * Q == 0 succeeds.  No index, k or n_pos out of range, a margin that is NaN or -inf, pos_ids == NULL: error with a message,
 * decided on the host before anything is queued, no output written, the handle stays usable.  The host form runs on the null
 * stream and synchronises; the _dev form takes device pointers, enqueues on `stream` and never waits for the device. */
int sse_score_confusions(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const int64_t *pos_ids, int32_t n_pos,
                         double margin, double *out_scores, int64_t *out_ids, int32_t *out_counts, double *out_pos_score,
                         int64_t *out_pos_id);
int sse_score_confusions_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const int64_t *pos_ids_dev,
                             int32_t n_pos, double margin, double *out_scores_dev, int64_t *out_ids_dev,
                             int32_t *out_counts_dev, double *out_pos_score_dev, int64_t *out_pos_id_dev, void *stream);

/* Bias of the resident index: one float per row, copied and kept on the device -- an item prior (quality, recency, stock), the
 * log-prior of a leaf category, the hubness correction of cross-lingual retrieval (CSLS ranks by 2 cos(x,t) - r_T(x) - r_S(t);
 * r_T(x) is constant per query and r_S(t) is known at index time, so bias[t] = -0.5 r_S(t) with weight 1 gives the CSLS
 * ranking).  N must equal the index's row count, otherwise the call errors with a message and the bias stays as it was.
 * bias == NULL clears it; uploading or adopting a new index (sse_index_upload*, sse_index_set_dev) clears it too, exactly as
 * tags and group keys are cleared.  The bias is independent of tags and group keys.  The host form reads the array once and
 * refuses a non-finite value with a message (the bias stays as it was); in the _dev form, which takes a device pointer and
 * enqueues the copy on `stream`, a non-finite value is outside the claim (no fault).  Beside the array the handle keeps
 * bias_absmax = max |bias|, as it keeps the largest row norm of the index; it is formed on the device behind the copy and
 * stays there, so neither form waits for anything the setters of tags and group keys do not wait for. */
int sse_index_set_bias(sse_handle *h, const float *bias_host, int64_t N);
int sse_index_set_bias_dev(sse_handle *h, const float *bias_dev, int64_t N, void *stream);

/* Exact top-k by cosine + per-row prior.  The biased score of row r for query q is
 *     sb(q, r) = score64(q, r) + (double)w[q] * (double)bias[r]
 * where score64 is the float64 dot product sse_score_topk returns for that row, bit for bit, bias is the array of
 * sse_index_set_bias* and w[q] = q_weight[q], or 1.0f for every query when q_weight == NULL.  Both factors are floats, so
 * their product is exact in double and sb is rounded ONCE; contracting the expression into a fused multiply-add cannot
 * change it.  That is why the weight is a float and not a double.  Row eligibility is the tag rule of
 * sse_score_topk_filtered (q_any / q_none may be NULL; giving either while no tags are set is an error).
 *   out_counts [Q]: c = min(k, eligible rows).
 *   out_scores / out_ids [Q][k]: columns 0 .. c of row q are the eligible rows by sb descending, equal sb by ascending id, ids
 *     including id_base, out_scores holding sb; columns c .. k hold (-inf, INT64_MAX).  1 <= k <= 1024; k may exceed N.
 * With w[q] == 0, or an all-zero bias, row q is sse_score_topk_filtered's row (no exclusion list), bit for bit.  A re-ranking
 * of sse_score_topk's columns on the host is NOT this call: a row outside the unbiased top-k may belong in the biased one.
 * The route is the filtered call's, carried out on the biased fp32 value y = fmaf(w, bias[r], fp32 score): a first kernel forms
 * per query e_b = e + u (|q| idx_norm_max + e + |w| bias_absmax), rounded outward, with e the certified fp32 bound of the
 * query and u = 2^-23 over the one rounding of the fused add (and of sb); the fp32 MFMA sweep keeps maxima of y over disjoint
 * row sets of the tag-eligible rows, their k-th largest less 2 e_b is a threshold no row of the answer has y below, the same
 * sweep again collects every tag-eligible row at or above it, and those are re-scored in float64, the bias added, and sorted
 * (counter "score_biased_collected_rows": rows re-scored); a query with more than 4096 such rows is served by a float64 sweep
 * of the whole index that adds the bias likewise ("score_biased_bruteforce_queries").  Cost note: a large |w| bias_absmax
 * widens the band 2 e_b and sends more rows to float64; the result stays exact.  Option "score_filtered_skip" governs the tile
 * skip here too and changes no result.  Scratch is bounded by the chunk of 4096 queries.  Rows or queries of norm below
 * 2^-100, non-finite rows or queries and a non-finite weight are outside the claim (no fault).
 * Out of scope here: exclusion lists, the (score, id) cursor of sse_score_topk_after, the group reduction of
 * sse_score_topk_grouped, and the web routes (they page, so they wait for a cursor form).
 * Q == 0 succeeds.  No index, no bias set, k out of range, masks without tags: error with a message, decided on the host before
 * anything is queued, no output written, the handle stays usable.  The host form runs on the null stream and synchronises;
 * the _dev form takes device pointers, enqueues on `stream` and never waits for the device. */
int sse_score_topk_biased(sse_handle *h, const float *q_host, int32_t Q, int32_t k, const float *q_weight,
                          const uint64_t *q_any, const uint64_t *q_none, double *out_scores, int64_t *out_ids,
                          int32_t *out_counts);
int sse_score_topk_biased_dev(sse_handle *h, const float *q_dev, int32_t Q, int32_t k, const float *q_weight_dev,
                              const uint64_t *q_any_dev, const uint64_t *q_none_dev, double *out_scores_dev,
                              int64_t *out_ids_dev, int32_t *out_counts_dev, void *stream);

/* Softmax log-partition over the whole index: the denominator that turns a returned score into P(row | query), and the
 * first term of the full-softmax cross-entropy that the in-batch loss (option train_loss = 1) estimates.  Row r is eligible
 * for query q by the tag rule of sse_score_topk_filtered (no exclusion list; q_any / q_none may be NULL), and
 *     z_r = (double)scale * (score64(q, r) + (double)q_weight[q] * (double)bias[r])
 * where score64 is the float64 dot product sse_score_topk returns and the parenthesis is the value sse_score_topk_biased
 * returns; q_weight == NULL means no bias term.  So for any row the biased, the filtered or the plain top-k call returns,
 *     P(row | q) = exp(scale * returned_score - out_lse[q]).
 *   out_lse [Q]:   log of the sum of exp(z_r) over the eligible rows; -inf when no row is eligible; never NaN inside the claim.
 *   out_count [Q]: the exact number of eligible rows.
 *   out_bound [Q] (may be NULL): a certified bound on |out_lse[q] - LSE64(q)|, LSE64 the same sum taken in float64 from
 *     score64: scale * e_b + 2^-16, with e_b the bound of sse_score_topk_biased on |fp32 biased score - its float64 value|
 *     (e = eps32 |q| (1 + 2^-20) without a bias term).  Moving every logit by at most d moves the log of the sum by at most d;
 *     the 2^-16 covers everything behind the dot product for every N (DESIGN K6m).
 * Route: one fp32 MFMA sweep of the index (the bf16 images are not used: their score error times the scale is a fraction of
 * a nat).  A lane keeps (m, sum of 2^(x - m), count) per query with x = z log2(e) and m an INTEGER reference, so a rising
 * maximum rescales by an exact power of two and an index sorted by ascending score loses nothing; sums run in fp32 over the
 * 16 rows of a tile and in float64 across tiles; the per (split, wave, lane half) partials are merged per query in a fixed
 * order by a second kernel.  No floating-point atomics: the same inputs give the same bits.  Option "score_filtered_skip"
 * governs the tile skip here too and changes no result.  Counters "score_lse_calls" (calls that passed their checks) and
 * "score_lse_tiles_skipped".  Scratch is bounded by the chunk of 4096 queries.
 * Rows or queries of norm below 2^-100, non-finite input and scale * |q| * (largest row norm + |w| bias_absmax) above 2^16
 * are outside the claim (no fault).  This is the held-out measure of the softmax objective that sse_eval_loss* cannot be:
 * nll(q, g) = out_lse[q] - scale * score64(q, g), the second term from sse_score_rank's out_score.
 * Q == 0 succeeds.  No index, scale outside (0, 256], q_weight with no bias set, masks without tags: error with a message,
 * decided on the host before anything is queued, no output written, the handle stays usable.  The host form runs on the null
 * stream and synchronises; the _dev form takes device pointers, enqueues on `stream` and never waits for the device. */
int sse_score_lse(sse_handle *h, const float *q_host, int32_t Q, float scale, const float *q_weight, const uint64_t *q_any,
                  const uint64_t *q_none, double *out_lse, int64_t *out_count, double *out_bound);
int sse_score_lse_dev(sse_handle *h, const float *q_dev, int32_t Q, float scale, const float *q_weight_dev,
                      const uint64_t *q_any_dev, const uint64_t *q_none_dev, double *out_lse_dev, int64_t *out_count_dev,
                      double *out_bound_dev, void *stream);

/* encode + score in one call, the encodings never leaving the device: session.run([src_seq_embedding | norm_...])
 * followed by np.dot + getSortedResults[:k] as sse_demo.py:121-129, webserver.py:144-151 (and the three other routes)
 * and sse_evaluator.py:107-111 do per query / batch.  enc_out_host (may be NULL) also receives the [B,S] encodings. */
int sse_encode_score_topk(sse_handle *h, int side, const int32_t *ids_host, int32_t B, int32_t T, int32_t normalize,
                          int32_t k, double *out_scores, int64_t *out_ids, float *enc_out_host);

/* k-way merge of P per-shard top-k lists per query (after the RCCL all-gather
 * of SURVEY 8e): in_* are [P,Q,k] (shard-major), out_* [Q,k]; same order rule. */
int sse_merge_topk_dev(sse_handle *h, const double *in_scores_dev, const int64_t *in_ids_dev, int32_t P,
                       int32_t Q, int32_t k, double *out_scores_dev, int64_t *out_ids_dev, void *stream);
/* The same merge on lists that sit `shard_stride` elements apart per shard (list (p, q, j) at p * shard_stride + q * k
 * + j): lets ONE all-gather carry scores and ids together ([P][2][Q][k] 64-bit words, shard_stride = 2*Q*k). */
int sse_merge_topk_strided_dev(sse_handle *h, const double *in_scores_dev, const int64_t *in_ids_dev,
                               int64_t shard_stride, int32_t P, int32_t Q, int32_t k, double *out_scores_dev,
                               int64_t *out_ids_dev, void *stream);

/* The exchange step WITHOUT torch: RCCL from the C ABI, so that the reference-side binding of
 * INTEGRATION.md can shard an index with ctypes alone.  `nccl_comm` is an ncclComm_t (one rank per GPU, created on the handle's
 * device) OF THE RCCL INSTANCE THIS LIBRARY BOUND: libsse_hip.so does not link RCCL, it binds every entry point it needs from
 * ONE library at first use -- $SSE_RCCL_LIB when set; else an RCCL already mapped into the process, whatever its visibility
 * (a host that imported torch: torch's copy); else librccl.so.1.  sse_rccl_library_path() names it (NULL: none loadable).
 * A communicator from sse_rccl_comm_init_rank is always of that instance; one the host made itself is valid here only if the
 * host's RCCL is the file sse_rccl_library_path() reports (two RCCL instances in one process do not share communicators).
 * Threads: one thread or process per rank.  ncclCommInitRank blocks until every rank has called it, so ONE thread driving
 * several handles must bracket its sse_rccl_comm_init_rank calls with sse_rccl_group_start / sse_rccl_group_end
 * (ncclGroupStart / ncclGroupEnd); the handle's mutex is held for the duration of the call.
 *   sse_allgather_merge_topk_dev  this rank's [Q][k] lists (global row ids) -> ONE ncclAllGather of the packed
 *       (float64 score bits | int64 ids) words on `stream` -> k-way merge: the unsharded result on every rank;
 *   sse_score_topk_sharded_dev    sse_score_topk_dev on this rank's shard (rows set with id_base = shard offset) + the above;
 *       LIMIT: k is handed to the shard sweep as it is, so k <= the rows of EVERY rank's shard (and no rank without rows):
 *       a 571-row index over 8 ranks takes k <= 71.  A host that needs more ranks min(k, rows) per shard, pads the lists to k
 *       with (-inf, INT64_MAX) and calls sse_allgather_merge_topk_dev -- the merge never emits a padding slot while the shards
 *       together hold >= k rows (sharded.py::ShardedIndex does this over torch.distributed);
 *   sse_rccl_get_unique_id / sse_rccl_comm_init_rank / sse_rccl_comm_destroy: thin conveniences over ncclGetUniqueId /
 *       ncclCommInitRank / ncclCommDestroy for hosts without an RCCL binding of their own (id128: the 128-byte ncclUniqueId;
 *       rank 0 creates it and hands it to the other ranks by whatever channel the host has -- file, socket, MPI).
 * Replaces nothing in the reference (it has no distributed code); consumes what sse_evaluator.py:110-111 / data_utils.py:263-267
 * compute per shard. */
const char *sse_rccl_library_path(void);
int sse_rccl_group_start(void);
int sse_rccl_group_end(void);
int sse_rccl_get_unique_id(char *id128);
int sse_rccl_comm_init_rank(sse_handle *h, void **comm, int32_t world, int32_t rank, const char *id128);
int sse_rccl_comm_destroy(sse_handle *h, void *comm);
int sse_allgather_merge_topk_dev(sse_handle *h, void *nccl_comm, int32_t world, const double *local_scores_dev,
                                 const int64_t *local_ids_dev, int32_t Q, int32_t k, double *out_scores_dev,
                                 int64_t *out_ids_dev, void *stream);
int sse_score_topk_sharded_dev(sse_handle *h, void *nccl_comm, int32_t world, const float *q_dev, int32_t Q, int32_t k,
                               double *out_scores_dev, int64_t *out_ids_dev, void *stream);

/* session.run([model.train, model.loss, model.train_acc], feed) --
 * sse_train.py:170-172; loss/acc are evaluated before the update.  labels
 * float32 [B] (sse_model.py:420).  tgt_ids_host is int32 [B,T] token ids in the
 * dual- and shared-encoder modes; in source-encoder-only and source_only_cnn
 * (builder-defined training: the reference's loss is ill-shaped for the free
 * target matrix and its CNN graph does not build) it is int32 [B] rows of the
 * free target matrix.  LSTM modes accept ANY cell size / embedding_size / encoding_size (round 5): the fused kernels cover
 * cell sizes <= 512 (training <= 256), embeddings that fit their LDS tile (training <= 64 columns) and encodings <= 512;
 * every other shape runs the per-step any-shape path (csrc/lstm_generic.hip: same arithmetic, exact fp32, latency-bound).
 * Remaining limits (rejected with an error, never silently): source_only_cnn embedding_size <= 64 for training and
 * T x E within the LDS tile; index dimension <= 1024 for scoring. */
int sse_train_step(sse_handle *h, const int32_t *src_ids_host, const int32_t *tgt_ids_host,
                   const float *labels_host, int32_t B, int32_t T, float *loss, float *train_acc);

/* Data-parallel training (SURVEY 8e "Training"): sse_train_step split at the
 * gradient exchange.  sse_train_grads runs forward + loss + backward on this
 * rank's B pair rows with the loss defined as the mean over rows_global rows
 * (the sum of B over all ranks) and leaves everything that has to be summed
 * across ranks in ONE flat float32 device buffer, the gradient arena:
 *   [ d word_embedding (dense [V,E]) | d <variable 1> | ... | tail[4] ]
 * in sse_variable_info order, tail = { sum of squares of the un-deduplicated
 * embedding-gradient slices (what tf.clip_by_global_norm sees for the
 * IndexedSlices of sse_model.py:355-359), loss, train_acc, rows }.
 * The caller all-reduces (sum) the arena over RCCL, then sse_train_apply
 * clips by the global norm of the reduced gradients and applies Adagrad --
 * bit-identical on every rank.  sse_train_set_grad_arena lets the caller own
 * the buffer (e.g. a torch tensor handed to torch.distributed.all_reduce);
 * NULL returns to a library-owned one.  sse_train_step == grads(rows_global =
 * B) + apply.  sse_train_grads[_rows] fails (no gradients pending, so a
 * following sse_train_apply changes nothing) on a token id, corpus row or
 * free-target-matrix row out of range, whatever the shape, path or network mode. */
/* The stream the train-step entry points (sse_train_step[_rows], sse_train_grads[_rows], sse_train_apply) enqueue on;
 * NULL (the default) is the null stream.  The two encoders of a step run on internal side streams forked from and joined
 * to this stream, so a caller that orders other work against it (torch.distributed orders a collective against torch's
 * current stream: data_parallel.py hands that stream over) needs no further synchronisation.  The call waits for the
 * previously set stream to drain.  The other entry points take their stream per call (*_dev) or use the null stream and
 * synchronise before returning (host buffers). */
int sse_set_stream(sse_handle *h, void *stream);
int sse_train_grad_count(sse_handle *h, int64_t *count);
int sse_train_set_grad_arena(sse_handle *h, float *arena_dev, int64_t count);
int sse_train_grads(sse_handle *h, const int32_t *src_ids_host, const int32_t *tgt_ids_host,
                    const float *labels_host, int32_t B, int32_t T, int64_t rows_global);
int sse_train_apply(sse_handle *h, float *loss, float *train_acc);
/* The word-embedding gradient of a data-parallel step as (row id, gradient row) pairs (SURVEY 8e "Training": "all-gather
 * of (row-id, grad-row) for the sparse embedding grads") -- for vocabularies where the dense [V,E] block dwarfs the rows a
 * step touches.  Between sse_train_grads and sse_train_apply, on the stream of sse_set_stream, no host synchronisation:
 *   sse_train_pack_embedding_grad   compacts the rows of the arena's dense block that carry any non-zero gradient into
 *       packed_dev = [ count (int32), 0, 0, 0 | ids (int32 x cap, padded to a multiple of 4) | rows (cap x E floats) ],
 *       sse_train_packed_embedding_floats(cap) floats in all; cap = an upper bound of the rows one rank can touch that is
 *       IDENTICAL on all ranks (min(V, 2 * max rows per rank * T)): the caller all-gathers the fixed-size buffers;
 *   sse_train_unpack_embedding_grad zeroes the dense block and adds the `world` gathered buffers in rank order -- the same
 *       sums in the same order on every rank; the rest of the arena is all-reduced as before.
 * A slot overflow or a row id out of range raises device error bit 8: sse_train_apply cancels the update and reports it. */
int64_t sse_train_packed_embedding_floats(sse_handle *h, int32_t cap);
int sse_train_pack_embedding_grad(sse_handle *h, int32_t cap, float *packed_dev);
int sse_train_unpack_embedding_grad(sse_handle *h, const float *gathered_dev, int32_t world, int32_t cap);
/* The open train step: sse_train_grads* cut at its loss stage, so that the objective can see more than this rank's rows, or
 * be the caller's own.  All calls take the handle's lock and run on the stream of sse_set_stream.
 *   sse_train_forward[_rows]   the arguments, checks and forward of sse_train_grads[_rows] -- input staging, both encoders
 *       with their tapes, the gather of the free target matrix's rows in the table modes -- on every path (fused LSTM,
 *       any-shape LSTM, text-CNN) and in every network mode.  The step is then left OPEN: its encodings, tapes and staged
 *       inputs stay in the handle, no pointer of the caller's is kept.  The options "train_loss" and "train_class_loss" are
 *       NOT consulted: the closing call supplies the objective.  An open step does not apply the pair de-duplication: it
 *       runs as with "train_pair_dedup" = 0 (its rows stay in the caller's order) and "train_paired_steps" does not rise.
 *   sse_train_open_encodings_dev   copies the un-normalised encodings [B][S] of the open step, in the caller's row order, to
 *       out_dev on `stream` (ordered behind the forward).  side 0 = source, 1 = target; in the table modes side 1 is the
 *       gathered rows of the free target matrix.
 *   sse_train_backward_dev   closes the step with the caller's gradients d_src_dev / d_tgt_dev [B][S]: the gradient of the
 *       GLOBAL mean objective with respect to this rank's un-normalised encodings, already scaled by 1 / rows_global as the
 *       loss heads produce them (read on the stream of sse_set_stream: the caller orders their production against it).
 *       loss_part / acc_part go to tail[1] / tail[2] of the gradient arena, so that the arena's all-reduce adds the ranks'
 *       shares up.  Then everything sse_train_grads does behind its loss head: the error-flag read, the zeroing of the
 *       lookup-table gradients, the scatter onto the free target matrix, the path's backward, the tail.  The pending
 *       gradients are IndexedSlices on both lookup tables (never the dense table of a class-loss step).
 *       sse_train_apply (and the packed embedding exchange) follow as after sse_train_grads.
 *   sse_train_pack_exchange   writes the open step's rows into ONE fixed-size block of 32-bit words for one all-gather,
 *       sse_train_exchange_floats(cap, T) words for cap >= B row slots in the caller's row order (Tt = T words of a target
 *       token row, or 1 in the table modes: the row number of the free target matrix; ids travel as their bit patterns):
 *         [ rows (int32), S, T, Tt | src raw (cap x S) | tgt raw (cap x S) | labels (cap) | src ids (cap x T) | tgt ids (cap x Tt) ]
 *       Slots B .. cap-1 are zeroed.  cap is IDENTICAL on all ranks (the largest row count of a rank).
 *   sse_train_backward_inbatch_global   closes the step with the in-batch softmax loss over the GLOBAL batch.  gathered_dev:
 *       the `world` blocks back to back in rank order; rank_rows (host, [world]): the ranks' row counts.  It compacts the
 *       blocks into contiguous global arrays (global row = rows of the lower ranks + local row), forms the source and target
 *       keys over the GLOBAL id rows exactly as a train_loss = 1 step forms them over its own (a source or a target repeated
 *       on another rank is admitted or excluded as the single-rank step of the concatenated batch decides), runs
 *       sse_inbatch_loss_window_dev's head on this rank's window with scale "train_loss_scale" and inv_rows = 1 / rows_global,
 *       reduces the window's row losses and accuracies into the tail, and closes as sse_train_backward_dev does.  No host
 *       synchronisation beyond that of sse_train_grads.  On the wire: 2S + 1 + T + Tt words per row slot, once, beside the
 *       gradient exchange; on the device: the cost stated at sse_inbatch_loss_window_dev with B = rows_global.
 * Lifetime: any sse_train_grads*, sse_train_step* or sse_train_forward* discards an open step.  A closing call (or
 * sse_train_open_encodings_dev, sse_train_pack_exchange) without an open step is refused; so is one after the variables
 * changed (sse_set_variable, an update), and a second closing call.  sse_train_backward_inbatch_global refuses, each with
 * its own text and before anything is queued: world < 1, rank outside [0, world), rank_rows[rank] != B, a rank with more than
 * cap rows, rank_rows not adding up to rows_global, NULL pointers.  After any refusal the handle stays usable.
 * Counters "train_open_steps", "train_global_inbatch_steps". */
int sse_train_forward(sse_handle *h, const int32_t *src_ids_host, const int32_t *tgt_ids_host, const float *labels_host,
                      int32_t B, int32_t T, int64_t rows_global);
int sse_train_forward_rows(sse_handle *h, const int32_t *src_rows_host, const int32_t *tgt_rows_host,
                           const float *labels_host, int32_t B, int64_t rows_global);
int sse_train_open_encodings_dev(sse_handle *h, int side, float *out_dev, void *stream);
int sse_train_backward_dev(sse_handle *h, const float *d_src_dev, const float *d_tgt_dev, float loss_part, float acc_part);
int64_t sse_train_exchange_floats(sse_handle *h, int32_t cap, int32_t T);
int sse_train_pack_exchange(sse_handle *h, int32_t cap, float *block_dev);
int sse_train_backward_inbatch_global(sse_handle *h, const float *gathered_dev, int32_t world, int32_t cap, int32_t rank,
                                      const int32_t *rank_rows_host);
/* Batches by row number: the padded source / target corpora (the token-id matrices Data builds
 * from TrainPairs / targetIDs, data.py:95-115) are uploaded once with sse_corpus_upload (side 0 = source corpus
 * [N,T], side 1 = target corpus) and a step ships 2*B row numbers instead of 2*B*T token ids; the batch's id matrix
 * is gathered on the device and the step is otherwise sse_train_step / sse_train_grads.  In the modes whose target
 * side is already a row of the free target matrix, tgt_rows keeps that meaning and no target corpus is needed. */
int sse_corpus_upload(sse_handle *h, int side, const int32_t *ids_host, int64_t N, int32_t T);
int sse_train_step_rows(sse_handle *h, const int32_t *src_rows_host, const int32_t *tgt_rows_host,
                        const float *labels_host, int32_t B, float *loss, float *train_acc);
int sse_train_grads_rows(sse_handle *h, const int32_t *src_rows_host, const int32_t *tgt_rows_host,
                         const float *labels_host, int32_t B, int64_t rows_global);
/* session.run([model.loss, model.train_acc], feed) WITHOUT model.train, and the per-row `binarylogit` cosines
 * (sse_model.py:290,298,302): loss and accuracy of held-out pairs -- a validation curve, early stopping, a threshold chosen
 * on labelled pairs, a restored checkpoint checked against the run that wrote it.  Forward only: the arguments mean what
 * they mean for sse_train_step / sse_train_step_rows (tgt: [B,T] token ids in the dual- and shared-encoder modes, [B] rows
 * of the free target matrix in source-encoder-only and source_only_cnn; the rows form reads the corpora of
 * sse_corpus_upload), but both encoders run on the INFERENCE kernels, un-normalised -- every network mode, every shape
 * an encode accepts, the inference options (lstm_x3, cnn_bf16, pad_skip, lstm_x_table, ...; the train_*_x3 options do not
 * apply), the lstm_path_* counters counting once per encode -- and there are no BPTT tapes, hence no 2 GiB tape limit.
 *   sums[3] = { sum of the row losses, sum of the row accuracies, B } in double, rows added in an order that depends on B
 *       alone: loss = sums[0] / sums[2], train_acc = sums[1] / sums[2]; sums of ranks or slices of a held-out set add up.
 *   row_cos_host (NULL or [B]) receives cos(src_b, tgt_b), float32; the logit is 64 cos.
 * Pair rows are staged and encoded in chunks of option eval_chunk_rows; any chunk size gives the same bits.  With option
 * train_pair_dedup (default 1), an even B and rows 2i, 2i + 1 carrying the same source (data.py:95-115), the source encoder
 * runs once per pair (counter eval_paired_calls): the same bits again.  The call runs on the stream of sse_set_stream and
 * synchronises before it returns.  It changes no variable, Adagrad slot, global_step or learning rate, and nothing of a
 * gradient result pending between sse_train_grads and sse_train_apply (arena, grads_ready): its scratch is its own.
 * A token id, corpus row or target-matrix row out of range fails with a message, writes no output and leaves the error
 * flag clear for the next call.  B == 0 returns sums of 0. */
int sse_eval_loss(sse_handle *h, const int32_t *src_ids_host, const int32_t *tgt_ids_host, const float *labels_host,
                  int32_t B, int32_t T, double *sums, float *row_cos_host);
int sse_eval_loss_rows(sse_handle *h, const int32_t *src_rows_host, const int32_t *tgt_rows_host, const float *labels_host,
                       int32_t B, double *sums, float *row_cos_host);
/* model.learning_rate.eval(), model.global_step.eval(), learning_rate_decay_op
 * (sse_train.py:181,200; sse_model.py:122-125) */
int sse_get_learning_rate(sse_handle *h, float *lr);
int sse_set_learning_rate(sse_handle *h, float lr);
int sse_decay_learning_rate(sse_handle *h);
int sse_get_global_step(sse_handle *h, int64_t *step);
int sse_set_global_step(sse_handle *h, int64_t step);

/* Timing helper for bench.py: HIP events recorded on the stream the kernels are
 * launched on.  sse_timer_record stamps event `slot` (0..255); sse_timer_elapsed_ms
 * waits for event `b` and returns the time from event `a` to event `b`. */
int sse_timer_record(sse_handle *h, int32_t slot, void *stream);
int sse_timer_elapsed_ms(sse_handle *h, int32_t a, int32_t b, float *ms);
/* hipDeviceSynchronize + report deferred device-side errors (e.g. an id out of
 * range seen by an asynchronous sse_encode_dev). */
int sse_synchronize(sse_handle *h);


/* ---- targetEncodingIndex.tsv text I/O, host only (no handle, no GPU) --------
 * sse_format_rows_f32: the vector field of sse_index.py:93-95,
 *   ",".join([str(n) for n in row]) with n a numpy.float32, byte-identical
 *   (shortest round-trip digits; positional for 1e-4 <= |x| < 1e16, else
 *   scientific).  Row r is written at out + r * sse_format_rows_stride(S)
 *   (no terminator) and its length stored in lengths[r].  Multi-threaded.
 * sse_parse_rows_f64: the inverse as sse_evaluator.py:87 / sse_demo.py:87 do it,
 *   [float(f) for f in field.split(",")] -> float64; row r is
 *   text[offsets[r] .. offsets[r+1]) (trailing newline / blanks ignored) and
 *   must hold exactly S numbers, else the call returns 2 and *bad_row is the
 *   first offending row. */
int64_t sse_format_rows_stride(int32_t S);
int sse_format_rows_f32(const float *rows, int64_t n_rows, int32_t S, char *out, int64_t *lengths);
int sse_parse_rows_f64(const char *text, const int64_t *offsets, int64_t n_rows, int32_t S, double *out,
                       int64_t *bad_row);
/* CRC-32C (Castagnoli) of n bytes, host only: the checksum TensorFlow V2 checkpoints carry per table block and per
 * tensor (saver.restore of a reference-trained model directory, sse_train.py:110-113: tf_checkpoint.py verifies them).
 * seed = 0 for a fresh sum, or the value returned for the preceding bytes. */
uint32_t sse_crc32c(const void *data, int64_t n, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* SSE_HIP_H */
