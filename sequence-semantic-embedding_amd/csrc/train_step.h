// The structs of the train-step host driver in sse_api.hip (its only includer): the state a handle keeps between steps,
// the description of one call, the frame the three paths share and the plan of the fused path.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

struct sse_handle;

namespace {

struct Variable;

struct DevBuf {  // grow-only device scratch; freed with its owner (handle / TrainState)
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// Which kernels one fused LSTM step runs and what follows from it; decided once per call (fused_plan), const afterwards.
struct FusedPlan {
  // which kernel families run on split bf16 operands (options train_fwd_x3 / train_bwd_x3 / train_dk_x3), per encoder
  bool fwd_x3[2], bwd_x3[2], all_x3, any_bwd_x3;
  bool bwd2;    // second-generation fp32 kernels
  bool paired;  // paired batch: the source encoder runs on the first half of the rows
  int NT32, NT_half;  // 32-row tiles of the batch; paired: of one half (B % 128 == 0: Bp = B, NT_half even)
  int sq_off[3];      // where each encoder's partial sums of dx^2 start in sq_part
  int n_sq;
};

// device buffers of the training path, grown on demand
struct TrainState {
  DevBuf ids[2], labels, raw[2], draw[2], tape_g[2], tape_a[2], h_last[2], dh_last[2], dg_a[2], dg_b[2], db_part[2],
      dk_part[2], dm_part[2], sq_part, norm_part, row_loss, row_acc, scal;
  DevBuf feat_rm, pos, dfeat, dw_part, dbias_part, wt, wct;  // text-CNN training
  uint64_t gen_ver[2] = {0, 0};  // weights_version the any-shape packs gen_KT / gen_Kq / gen_MT were built from
  DevBuf gen_A[2], gen_tape[2], gen_dG[2], gen_hl[2], gen_KT[2], gen_Kq[2], gen_MT[2], gen_G, gen_c, gen_dA, gen_dc, gen_dkp;  // any-shape LSTM path
  hipStream_t side[2] = {nullptr, nullptr};  // the two encoders run concurrently (forward and backward)
  hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  float *KhT[2] = {nullptr, nullptr}, *KxT[2] = {nullptr, nullptr};
  unsigned short *KhT16[2] = {nullptr, nullptr};  // option train_bwd_x3: Kh^T as split frag16 blocks
  unsigned short *KxT16[2] = {nullptr, nullptr};  // ... and Kx^T as 16x16x32 B fragments (dX inside the BPTT kernel)
  bool packed_dirty = true;
  bool fp32_dirty = true;  // the fp32 Kh^T / Kx^T fragment copies are stale (rebuilt only by steps that run fp32 BPTT kernels)
  // gradient arena: [grad of variable 0 | ... | grad of variable n-1 | tail[4]]; tail = {sum of squares of the
  // un-deduplicated embedding-gradient slices, loss, train_acc, rows}, every entry a plain sum over the
  // ranks of a data-parallel job (one flat all-reduce)
  float *arena = nullptr;
  bool arena_external = false, grads_ready = false;
  bool grads_dense_table = false;  // the pending gradients come from a class-loss step: tgt_seq_embedding's block is dense
  // corpus resident on the device (sse_corpus_upload): the *_rows train entry points ship row numbers, not token ids
  DevBuf corpus[2], rows[2];
  int64_t corpus_N[2] = {0, 0};
  int32_t corpus_T[2] = {0, 0};
  // paired batches (data.py:95-115: every source row appears twice, once with its positive and once with a negative
  // target): internal row order = [rows 0,2,4,.. | rows 1,3,5,..], the source encoder runs on the first half only
  DevBuf ids_raw[2], perm, hot_part[2];
  int perm_B = 0;
  std::vector<int32_t> h_perm, h_rows[2], h_tgt;
  std::vector<float> h_labels;
  // the open step (sse_train_forward*): what its closing call needs to rebuild the frame -- no pointer of the caller's
  struct Open {
    bool valid = false;
    int path = 0;                  // OPEN_CNN | OPEN_GENERIC | OPEN_FUSED
    int32_t B = 0, T = 0;
    int64_t rows_global = 0;
    bool by_rows = false;
    uint64_t weights_version = 0;  // the variables the forward ran on; a closing call after they changed is refused
    FusedPlan plan = {};           // OPEN_FUSED: the plan the forward ran under (the options may have changed since)
  } open;
  DevBuf xg_raw[2], xg_labels, xg_ids[2], xg_off;  // the global batch of sse_train_backward_inbatch_global, compacted
  std::vector<int32_t> h_off;
};
enum { OPEN_CNN, OPEN_GENERIC, OPEN_FUSED };
// a train step whole, or cut at its loss stage: STEP_OPEN stops behind the forward, STEP_CLOSE resumes there with d(raw
// encodings) and the loss tail already written by the closing call
enum { STEP_WHOLE, STEP_OPEN, STEP_CLOSE };

// One call of the train step as its entry point received it.  src / tgt: id matrices [B][T], or -- by_rows -- row numbers
// into the corpora of sse_corpus_upload; tgt is rows of the free target matrix in the table modes either way.
struct TrainCall {
  const int32_t *src, *tgt;
  const float *labels;
  int32_t B, T;
  int64_t rows_global;
  bool by_rows;
  bool defer_err;  // the fused step entry points: the device error flag is read once, with the loss, after the whole step
                   // has been queued (a flagged step cancels its own update on the device)
  int phase;       // STEP_WHOLE (the default of the brace initialisers), STEP_OPEN, STEP_CLOSE (src / tgt / labels are null)
};

// What the three paths of a step (text-CNN, any-shape LSTM, fused LSTM) share: filled by step_begin, n_sq by step_stage_inputs
struct StepFrame {
  sse_handle *h;
  const TrainCall *call;
  TrainState *ts;
  hipStream_t st;
  int B, T, S;
  int Bp;          // rows of raw[] / draw[]: B rounded up to the path's row tile
  bool table_tgt;  // target side = rows of the free target matrix
  bool class_loss; // option train_class_loss: the loss stage runs the class softmax head over the whole matrix
  int nside;       // sequence encoders in the step
  Variable *emb, *table;
  float *tail, inv_rows;
  int n_sq;        // partial sums in sq_part; the table target's B come last
  float *raw(int s) const { return (float *)ts->raw[s].p; }
  float *draw(int s) const { return (float *)ts->draw[s].p; }
  const int32_t *ids(int s) const { return (const int32_t *)ts->ids[s].p; }
  float *sq() const { return (float *)ts->sq_part.p; }
};

// one encoder's backward of the fused path as its three bodies see it
struct FusedBwdSide {
  int s;
  hipStream_t bs;
  int Hp, KGn, NTn, KT;
  bool half;       // the source encoder of a paired batch: tape_a holds half the rows, the dK GEMM adds the two halves' dG fragments
  int NTa, RGa;    // 32-row tiles / 8-row r-groups of tape_a
  int SL;
  int accumulate;  // shared-encoder, target side: onto the source side's kernel / bias gradient
  float *sq;       // this side's partial sums of dx^2
};

}  // namespace
