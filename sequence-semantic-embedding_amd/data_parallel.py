"""Data-parallel train step over the GPUs of one node (SURVEY 8e "Training"; BASELINE configs[4]).

Every rank holds the full model, runs forward + loss + backward on ITS pair rows with the loss defined as the mean
over the rows of all ranks, sums one flat float32 buffer over RCCL (dense gradients of every variable, the squared
norm of the raw embedding-gradient slices that `tf.clip_by_global_norm` sees, loss, train_acc, rows -- the "gradient
arena" of include/sse_hip.h), then clips by the global norm of the REDUCED gradients and applies Adagrad: the update is
bit-identical on every rank and equals the single-process step on the concatenated batch up to fp32 summation order.

With global_negatives=True the in-batch softmax loss sees the rows of ALL ranks as negatives: one more all-gather, of the ranks'
encodings, ahead of the loss (DataParallelTrainer.__init__).

The reference trains in one process (sse_train.py:170-172); this is the exchange step a multi-GPU job adds.
The engine is anything with train_grad_count / train_bind_arena / train_grads / train_apply (and, for eval_loss,
eval_loss_sums / eval_loss_rows_sums): the HIP handle
(sequence-semantic-embedding_amd/_lib.py) in the product, the numpy oracle in the CPU `gloo` tests.
torch / torch.distributed are plumbing only.  The collectives go through collectives.py: RCCL as is under `nccl`, staged
through the host under any other backend (ranks as processes on one GPU).

Known property: every rank must reach every collective of a step.  A rank whose train_grads raises (a bad token id, say)
leaves the step before the all-reduce while its peers wait in it until the process group's timeout; the caller ends the job.
"""


class DataParallelTrainer(object):
    def __init__(self, engine, device=None, group=None, always_reduce=False, sparse_embedding=None, options=None,
                 global_negatives=False):
        """always_reduce: issue the collective even in a 1-rank group (exercises the RCCL path on one GPU).
        options: {name: value} set on this rank's engine (engine.set_option) before the first step, e.g.
        {"train_loss": 1, "train_loss_scale": 64} for the in-batch softmax loss: every rank passes the same dict, so every
        rank's handle computes the same objective.  By default its negatives are the rank's own rows (the mean runs over
        rows_global), so the objective depends on the world size: 8 ranks of 128 rows see 127 negatives per row, not 1023.
        global_negatives=True: the in-batch softmax loss over the GLOBAL batch instead, whatever "train_loss" says (the scale
        is "train_loss_scale").  Every rank runs the forward alone (engine.train_forward), the ranks' encodings, labels and
        id rows cross the wire in ONE all-gather of fixed-size blocks (engine.train_pack_exchange: 2S + 1 + 2T words per row
        slot, T + 1 in the free-target-matrix modes), and every rank closes its step with the head over the gathered batch
        cut to its own rows (engine.train_backward_inbatch_global: one rows pass over rows_global^2 logits on every rank,
        two gradient passes over its rows x rows_global).  The step then equals the single-rank train_loss = 1 step of the
        concatenated batch up to summation order, at any world size and for any split of the rows.  The gradient exchange
        and the update follow as without it.
        {"train_class_loss": 1} selects the class softmax loss of the free-target-matrix modes instead.  That objective,
        unlike the in-batch one, is identical at any world size: a softmax over the whole class table decomposes over the
        rows of a batch, so the step equals the single-rank step of the concatenated batch up to summation order (the rows
        of one source kept on one rank: the exclusion of its other verified classes is formed from the rank's own rows).
        sparse_embedding: exchange the word-embedding gradient as (row id, gradient row) pairs -- SURVEY 8e's shape for
        large vocabularies (the 1M-title ranking vocabulary, reference README.md:116) -- instead of all-reducing the
        dense [V,E] block; None = automatic (sparse when the GLOBAL batch touches fewer than V/4 rows: 2 * rows_global * T < V / 4)."""
        import torch
        self.engine, self.group, self.always_reduce = engine, group, bool(always_reduce)
        self.sparse_embedding = sparse_embedding
        self.global_negatives = bool(global_negatives)
        if self.global_negatives and not all(hasattr(engine, n) for n in ("train_forward", "train_exchange_floats", "train_pack_exchange",
                                                                          "train_backward_inbatch_global")):
            raise ValueError("global_negatives=True needs an engine with the open train step (train_forward, train_exchange_floats, "
                             "train_pack_exchange, train_backward_inbatch_global)")
        self._block = self._blocks = None      # this rank's exchange block and the gathered ones
        for name, value in (options or {}).items():
            engine.set_option(name, value)
        self.arena =torch.zeros(engine.train_grad_count(), dtype=torch.float32, device=device or "cpu")
        engine.train_bind_arena(self.arena)
        self._stream = None
        # where the dense word_embedding gradient sits in the arena: (offset, V, E); the HIP handle keeps it first
        sl = getattr(engine, "embedding_slice", None)
        self.emb_slice = tuple(sl()) if sl is not None else None
        self.last_exchange = None          # "dense" | "sparse": what the last step put on the wire (tests, bench)
        self._packed = self._gathered = None   # the packed (row id, gradient row) buffers of the sparse exchange

    @property
    def world(self):
        import torch.distributed as dist
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def global_rows(self, local_rows):
        """Sum of the ranks' row counts (ranks may hold different numbers of rows: the reference's batches are
        truncated at the end of the corpus, data.py:98)."""
        return self._rows_sum_max(local_rows)[0]

    def _rows_sum_max(self, local_rows):
        """(sum, max) of the ranks' row counts: one tiny all-gather (both are needed: the loss is a mean over the sum,
        the packed embedding exchange is sized by the max)."""
        rows = self._rank_rows(local_rows)
        return sum(rows), max(rows)

    def _rank_rows(self, local_rows):
        """The ranks' row counts, in rank order: one tiny all-gather."""
        import torch
        from .collectives import all_gather_into
        if self.world == 1:
            return [int(local_rows)]
        t = torch.tensor([int(local_rows)], dtype=torch.int64, device=self.arena.device)
        out = torch.empty(self.world, dtype=torch.int64, device=self.arena.device)
        all_gather_into(out, t, group=self.group)
        return [int(v) for v in out.cpu()]

    @property
    def rank(self):
        import torch.distributed as dist
        return dist.get_rank(self.group) if dist.is_available() and dist.is_initialized() else 0

    def train_step(self, src_ids, tgt_ids, labels, rows_global=None, by_rows=False):
        """One step on this rank's rows; returns the GLOBAL (loss, train_acc), evaluated before the update.
        Pass rows_global when it is known and the batch is split evenly (split_batch: every rank holds at most
        ceil(rows_global / world) rows) to save the tiny extra all-gather of the row counts; ranks with arbitrary row counts
        (the reference's truncated batches, data.py:98) leave it None.
        by_rows: src_ids / tgt_ids are row numbers into the corpora uploaded with engine.corpus_upload."""
        import torch
        from .collectives import all_reduce_
        if self.arena.is_cuda and hasattr(self.engine, "set_stream"):
            # the train step runs on the library's own streams forked from / joined to ONE stream, and torch.distributed
            # orders the collective against torch's CURRENT stream: hand that stream to the library (sse_set_stream)
            cur = torch.cuda.current_stream(self.arena.device).cuda_stream
            if cur != self._stream:
                self.engine.set_stream(cur)
                self._stream = cur
        rank_rows = None
        if rows_global is None:
            rank_rows = self._rank_rows(len(labels))
            rows_global, rows_cap = sum(rank_rows), max(rank_rows)
        else:
            rows_cap = -(-int(rows_global) // self.world)
            if len(labels) > rows_cap:
                raise ValueError("rank holds %d rows, more than ceil(rows_global / world) = %d: leave rows_global=None for "
                                 "unevenly split batches" % (len(labels), rows_cap))
        if self.global_negatives:
            if rank_rows is None:                      # the even split of split_batch
                from .sharded import shard_bounds
                rank_rows = [e - s for s, e in shard_bounds(int(rows_global), self.world)]
                if rank_rows[self.rank] != len(labels):
                    raise ValueError("rank %d holds %d rows, split_batch gives it %d of %d: leave rows_global=None for other splits"
                                     % (self.rank, len(labels), rank_rows[self.rank], rows_global))
            self._global_inbatch_grads(src_ids, tgt_ids, labels, rows_global, rows_cap, rank_rows, by_rows)
        elif by_rows:
            self.engine.train_grads_rows(src_ids, tgt_ids, labels, rows_global)
        else:
            self.engine.train_grads(src_ids, tgt_ids, labels, rows_global)
        if self.world > 1 or self.always_reduce:
            if self._use_sparse(rows_global, src_ids, by_rows):
                self._exchange_sparse(rows_cap, self._seq_len(src_ids, by_rows))
            else:
                all_reduce_(self.arena, group=self.group)          # ONE collective per step (sum)
                self.last_exchange = "dense"
        return self.engine.train_apply()

    def _global_inbatch_grads(self, src_ids, tgt_ids, labels, rows_global, rows_cap, rank_rows, by_rows):
        """forward -> pack -> ONE all-gather of the ranks' blocks -> the in-batch head over the global batch, cut to this rank's
        rows, and the backward.  Leaves the arena as train_grads does."""
        import torch
        from .collectives import all_gather_into
        if by_rows:
            self.engine.train_forward_rows(src_ids, tgt_ids, labels, rows_global)
        else:
            self.engine.train_forward(src_ids, tgt_ids, labels, rows_global)
        n = self.engine.train_exchange_floats(rows_cap, self._seq_len(src_ids, by_rows))
        if self._block is None or self._block.numel() != n or self._blocks.numel() != n * self.world:
            self._block = torch.zeros(n, dtype=torch.float32, device=self.arena.device)
            self._blocks = torch.zeros(n * self.world, dtype=torch.float32, device=self.arena.device)
        self.engine.train_pack_exchange(rows_cap, self._block)
        if self.world == 1 and not self.always_reduce:
            self._blocks.copy_(self._block)
        else:
            all_gather_into(self._blocks, self._block, group=self.group)
        self.engine.train_backward_inbatch_global(self._blocks, self.world, rows_cap, self.rank, rank_rows)

    def eval_loss(self, src_ids, tgt_ids, labels, by_rows=False):
        """Forward-only GLOBAL (loss, train_acc) of held-out pairs split over the ranks (any row counts, a rank may hold none):
        the engine's three float64 sums {row losses, row accuracies, rows} of this rank's rows, ONE all-reduce (sum), the
        two quotients.  No update, no gradient arena.  The engine needs eval_loss_sums / eval_loss_rows_sums."""
        import torch
        from .collectives import all_reduce_
        if self.arena.is_cuda and hasattr(self.engine, "set_stream"):
            cur = torch.cuda.current_stream(self.arena.device).cuda_stream
            if cur != self._stream:
                self.engine.set_stream(cur)
                self._stream = cur
        fn = self.engine.eval_loss_rows_sums if by_rows else self.engine.eval_loss_sums
        sums = torch.tensor([float(v) for v in fn(src_ids, tgt_ids, labels)], dtype=torch.float64, device=self.arena.device)
        if self.world > 1 or self.always_reduce:
            all_reduce_(sums, group=self.group)
        tot_loss, tot_acc, rows = (float(v) for v in sums.cpu())
        if rows == 0:
            return 0.0, 0.0
        return tot_loss / rows, tot_acc / rows

    # ---- (row id, gradient row) exchange of the embedding gradient (SURVEY 8e "Training") ----------------------------
    def _seq_len(self, src_ids, by_rows):
        T = getattr(self.engine, "max_seq_length", None)
        if T is None:
            import numpy as np
            if by_rows:
                raise ValueError("engine without max_seq_length: cannot size the packed exchange of a step by rows")
            T = int(np.asarray(src_ids).shape[-1])
        return int(T)

    def _use_sparse(self, rows_global, src_ids, by_rows):
        """Decided from values that are IDENTICAL on every rank (rows_global, T, V): ranks whose local row counts differ
        by one (split_batch) must not disagree about which collectives the step issues."""
        if self.emb_slice is None or self.sparse_embedding is False:
            return False
        if self.sparse_embedding:
            return True
        V = self.emb_slice[1]
        return 2 * int(rows_global) * self._seq_len(src_ids, by_rows) < V // 4

    def _exchange_sparse(self, rows_cap, T):
        """Same sums as the dense all-reduce.  The dense variables and the tail go through one all-reduce of the arena
        BEHIND the embedding block (two when the block is not at the start); the embedding block travels as the rows this
        rank touched: compacted on the device into a FIXED-size packed buffer (cap = min(V, 2 * rows_cap * T) slots, the
        same on every rank: no count has to cross the host), ONE all-gather, then added into the zeroed block in rank
        order by the engine (HIP kernels behind the C ABI: sse_train_pack / unpack_embedding_grad) -- no torch kernels, no
        host synchronisation."""
        import torch
        from .collectives import all_gather_into, all_reduce_
        off, V, E = self.emb_slice
        cap = max(1, min(V, 2 * int(rows_cap) * int(T)))
        n = self.engine.dp_packed_floats(cap)
        if self._packed is None or self._packed.numel() != n or self._gathered.numel() != n * self.world:
            self._packed = torch.zeros(n, dtype=torch.float32, device=self.arena.device)
            self._gathered = torch.zeros(n * self.world, dtype=torch.float32, device=self.arena.device)
        works = [all_reduce_(part, group=self.group, async_op=True)              # everything but the embedding block
                 for part in (self.arena[:off], self.arena[off + V * E:]) if part.numel()]
        self.engine.dp_pack_embedding(cap, self._packed)
        if self.world == 1 and not self.always_reduce:
            self._gathered.copy_(self._packed)
        else:
            all_gather_into(self._gathered, self._packed, group=self.group)
        self.engine.dp_unpack_embedding(self._gathered, self.world, cap)
        for w in works:
            w.wait()
        self.last_exchange = "sparse"
        self.last_cap = cap


def split_batch(src_ids, tgt_ids, labels, rank, world):
    """Contiguous, balanced slice of a global batch for one rank (same rule as the index shards)."""
    from .sharded import shard_bounds
    s, e = shard_bounds(len(labels), world)[rank]
    return src_ids[s:e], tgt_ids[s:e], labels[s:e]
