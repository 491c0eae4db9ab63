"""Row-sharded target index over the GPUs of one node (BASELINE
configs[3]): rank g holds rows [g*N/P, (g+1)*N/P), queries are replicated, every
rank computes its shard's top-k with GLOBAL row ids, ONE all-gather per query
block (RCCL over xGMI when the process group is `nccl`) exchanges the [Q,k]
(float64 score, int64 id) lists packed in one buffer -- 16*Q*k bytes per rank; the
exact float64 scores must travel: a rank cannot re-score candidates of rows it
does not hold -- and a k-way merge with the same order rule (score desc, row id
asc) yields exactly the unsharded result.  Queries go in blocks: the gather of
block i runs on RCCL's stream while block i+1 sweeps the shard.  Every library
call is enqueued on torch's CURRENT stream (passed explicitly), which is also
the stream torch.distributed orders its collectives against.

Any 1 <= k <= n_total is served: a shard with r < k rows (the 571-row demo index over 8 ranks at k = 100; an EMPTY
shard when n_total < world) scores min(k, r) and pads its list to k with (-inf, INT64_MAX) before the gather.  The
merge ranks such a slot behind every real row and, because the shards together hold >= k real rows, never writes one
into the result.  Under a backend other than `nccl` the gather is staged through the host (collectives.py).

The reference has no distributed code at all; this is the one real exchange
step of the hot path.  torch / torch.distributed are plumbing only.
"""


def shard_bounds(n_rows, world):
    """Contiguous, balanced row ranges: [(start, end)] * world; sizes differ by <= 1."""
    base, extra = divmod(int(n_rows), int(world))
    out, start = [], 0
    for r in range(world):
        size = base + (1 if r < extra else 0)
        out.append((start, start + size))
        start += size
    return out


def all_gather_topk(local_scores, local_ids, group=None, force=False):
    """All-gather the per-shard lists.  local_* are [Q,k] tensors (CUDA with the
    nccl backend, CPU with gloo); returns ([P,Q,k] scores, [P,Q,k] ids), shard-major."""
    import torch
    import torch.distributed as dist
    from .collectives import all_gather_into
    world = dist.get_world_size(group)
    gs = torch.empty((world,) + tuple(local_scores.shape), dtype=local_scores.dtype, device=local_scores.device)
    gi = torch.empty((world,) + tuple(local_ids.shape), dtype=local_ids.dtype, device=local_ids.device)
    if world == 1 and not force:
        gs[0].copy_(local_scores)
        gi[0].copy_(local_ids)
        return gs, gi
    if local_scores.is_cuda:
        all_gather_into(gs, local_scores.contiguous(), group=group)
        all_gather_into(gi, local_ids.contiguous(), group=group)
    else:                                   # gloo: list form
        dist.all_gather(list(gs.unbind(0)), local_scores.contiguous(), group=group)
        dist.all_gather(list(gi.unbind(0)), local_ids.contiguous(), group=group)
    return gs, gi


def merge_above_runs(pair, scores, ids, L):
    """The per-pair merge of ShardedIndex.score_above on torch tensors of any device: the shards' entries concatenated
    (pair int64 [M] = the pair of each entry, scores float64 [M], ids int64 [M], in any order) -> (offsets int64 [L+1],
    ids, scores) with every pair's entries together, score descending, equal scores by ascending id.  Three stable sorts,
    least significant key first."""
    import torch
    o = torch.sort(ids, stable=True).indices
    o = o[torch.sort(scores[o], descending=True, stable=True).indices]
    o = o[torch.sort(pair[o], stable=True).indices]
    offsets = torch.zeros(L + 1, dtype=torch.int64, device=pair.device)
    if L > 0:
        offsets[1:] = torch.cumsum(torch.bincount(pair, minlength=L), 0)
    return offsets, ids[o], scores[o]


def merge_grouped_lists(scores, ids, groups, k):
    """The merge of ShardedIndex.score_topk_grouped on torch tensors of any device: the shards' lists side by side (scores
    float64 [Q,M], ids int64 [Q,M], groups int64 [Q,M]; padding entries carry id INT64_MAX) -> (scores [Q,k], ids [Q,k],
    groups [Q,k], counts int32 [Q]).  A group may live on several shards, so the lists are collapsed again: entries ordered by
    (score descending, id ascending), the first entry of each group kept, cut to k, padded with (-inf, INT64_MAX, INT64_MAX);
    the count is the number of distinct groups kept."""
    import torch
    Q, M = scores.shape
    pad = torch.iinfo(torch.int64).max
    out_s = torch.full((Q, k), float("-inf"), dtype=torch.float64, device=scores.device)
    out_i = torch.full((Q, k), pad, dtype=torch.int64, device=scores.device)
    out_g = torch.full((Q, k), pad, dtype=torch.int64, device=scores.device)
    if Q == 0 or M == 0:
        return out_s, out_i, out_g, torch.zeros(Q, dtype=torch.int32, device=scores.device)
    # rank of every entry in (score descending, id ascending): two stable sorts, least significant key first
    o = torch.sort(ids, dim=1, stable=True).indices
    o = torch.gather(o, 1, torch.sort(torch.gather(scores, 1, o), dim=1, descending=True, stable=True).indices)
    s, i, g = torch.gather(scores, 1, o), torch.gather(ids, 1, o), torch.gather(groups, 1, o)
    # an entry is its group's first iff its position is the least of its group: stable sort by group, heads of the runs
    og = torch.sort(g, dim=1, stable=True).indices
    gs = torch.gather(g, 1, og)
    head = torch.ones((Q, M), dtype=torch.bool, device=scores.device)
    head[:, 1:] = gs[:, 1:] != gs[:, :-1]
    keep = torch.zeros((Q, M), dtype=torch.bool, device=scores.device)
    keep.scatter_(1, og, head)
    keep &= i != pad                                            # padding stands for no group
    rank = torch.cumsum(keep.to(torch.int64), 1) - 1           # column of a kept entry
    take = keep & (rank < k)
    rows = torch.arange(Q, device=scores.device).unsqueeze(1).expand(Q, M)[take]
    cols = rank[take]
    out_s[rows, cols], out_i[rows, cols], out_g[rows, cols] = s[take], i[take], g[take]
    return out_s, out_i, out_g, take.sum(1).to(torch.int32)


def merge_confusion_lists(scores, ids, pos_scores, pos_ids, margin, k):
    """The merge of ShardedIndex.score_confusions on torch tensors of any device: the shards' local top-k non-positives side
    by side (scores float64 [Q,M], ids int64 [Q,M]; padding entries carry id INT64_MAX) and every shard's local best
    positive (pos_scores float64 [P,Q], pos_ids int64 [P,Q]; (-inf, INT64_MAX) where a shard holds none) -> (scores [Q,k],
    ids [Q,k], counts int32 [Q], pos_scores [Q], pos_ids [Q]).  The best positive is the first of the shards' in (score
    descending, id ascending); f = it - margin in IEEE double; the entries are ordered the same way, cut at f (>= stays)
    and at k, padded with (-inf, INT64_MAX).  Exact: the global answer is a prefix of the merged non-positives, and every
    shard's share of the best k of those is within its own best k."""
    import torch
    Q, M = scores.shape
    pad = torch.iinfo(torch.int64).max
    dev = scores.device
    m = pos_scores.max(dim=0).values if pos_scores.shape[0] else torch.full((Q,), float("-inf"), dtype=torch.float64, device=dev)
    if pos_ids.shape[0]:
        b = torch.where(pos_scores == m.unsqueeze(0), pos_ids, torch.full_like(pos_ids, pad)).min(dim=0).values
    else:
        b = torch.full((Q,), pad, dtype=torch.int64, device=dev)
    out_s = torch.full((Q, k), float("-inf"), dtype=torch.float64, device=dev)
    out_i = torch.full((Q, k), pad, dtype=torch.int64, device=dev)
    if Q == 0 or M == 0:
        return out_s, out_i, torch.zeros(Q, dtype=torch.int32, device=dev), m, b
    f = m - float(margin)
    # (score descending, id ascending): two stable sorts, least significant key first
    o = torch.sort(ids, dim=1, stable=True).indices
    o = torch.gather(o, 1, torch.sort(torch.gather(scores, 1, o), dim=1, descending=True, stable=True).indices)
    s, i = torch.gather(scores, 1, o), torch.gather(ids, 1, o)
    keep = (i != pad) & (s >= f.unsqueeze(1))
    rank = torch.cumsum(keep.to(torch.int64), 1) - 1           # column of a kept entry
    take = keep & (rank < k)
    rows = torch.arange(Q, device=dev).unsqueeze(1).expand(Q, M)[take]
    cols = rank[take]
    out_s[rows, cols], out_i[rows, cols] = s[take], i[take]
    return out_s, out_i, take.sum(1).to(torch.int32), m, b


def merge_lse_lists(lse, count, bound):
    """The merge of ShardedIndex.score_lse on torch tensors of any device: the shards' results stacked in rank order (lse
    float64 [W,Q], -inf where a shard has no eligible row; count int64 [W,Q]; bound float64 [W,Q]) -> (lse [Q], count [Q],
    bound [Q]).  The log-partition of a union of disjoint row sets is the logaddexp of the parts: taken over the ranks in
    rank order, so every rank forms the same bits.  Each part lies within its own bound of its float64 value, so their
    logaddexp lies within the largest of them; the W - 1 float64 logaddexp of the merge add at most 2^-50 max(1, |lse|) each."""
    import torch
    W, Q = lse.shape
    out = torch.full((Q,), float("-inf"), dtype=torch.float64, device=lse.device)
    for r in range(W):
        out = torch.logaddexp(out, lse[r])
    total = count.sum(dim=0) if W else torch.zeros(Q, dtype=torch.int64, device=lse.device)
    out = torch.where(total > 0, out, torch.full_like(out, float("-inf")))
    if W:
        b = bound.max(dim=0).values                          # (a rank without rows hands in 0)
    else:
        b = torch.zeros(Q, dtype=torch.float64, device=lse.device)
    mag = torch.where(total > 0, out.abs(), torch.zeros_like(out)).clamp(min=1.0)
    return out, total, b + max(W - 1, 0) * 2.0 ** -50 * mag


class ShardedIndex(object):
    """One rank's view of the sharded index.  `handle` is an sse_amd Handle."""

    def __init__(self, handle, rank, world, n_total, group=None, always_gather=False):
        """always_gather: run the all-gather + merge even with one shard (exercises the RCCL path on one GPU)."""
        self.handle, self.rank, self.world, self.group = handle, int(rank), int(world), group
        self.always_gather = bool(always_gather)
        self.n_total = int(n_total)
        self.start, self.end = shard_bounds(n_total, world)[rank]

    def set_local_rows(self, rows):
        """rows: CUDA float32 tensor [end-start, S] -- this rank's shard, already on its GPU.  A rank without rows
        (n_total < world) passes its [0, S] tensor: nothing is uploaded, score_topk contributes an empty list."""
        if rows.shape[0] != self.end - self.start:
            raise ValueError("shard of rank %d must have %d rows, got %d" % (self.rank, self.end - self.start, rows.shape[0]))
        if rows.shape[0] > 0:
            self.handle.index_set_dev(rows.data_ptr(), rows.shape[0], rows.shape[1], id_base=self.start)

    def update_rows(self, ids, rows=None, tags=None, groups=None, bias=None):
        """Replace rows (and / or their tag words, group keys, bias values) of the sharded index in place: ids int64 [M]
        GLOBAL ids, rows [M,S] and the columns as Handle.index_update takes them (host arrays, identical on every rank).
        Each rank applies the ids that fall in its shard: global ids make this a filter, nothing is exchanged.  Returns
        the number of ids this rank applied.  There is no sharded append: the shard bounds are fixed at construction."""
        import numpy as np
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if ((ids < 0) | (ids >= self.n_total)).any():
            raise ValueError("update_rows: ids must be in [0, %d)" % self.n_total)
        mine = np.flatnonzero((ids >= self.start) & (ids < self.end))
        if mine.size:
            pick = lambda x: None if x is None else np.asarray(x)[mine]
            self.handle.index_update(ids[mine], pick(rows), pick(tags), pick(groups), pick(bias))
        return int(mine.size)

    def score_topk(self, queries, k, block=8192):
        """queries: CUDA float32 [Q,S] (identical on every rank).  Returns the global
        top-k (scores float64 [Q,k], row ids int64 [Q,k]) on every rank, for any 1 <= k <= n_total (ValueError
        otherwise, on every rank alike and before any collective)."""
        import torch
        import torch.distributed as dist
        from .collectives import all_gather_into
        k = int(k)
        if not 1 <= k <= self.n_total:
            raise ValueError("k=%d must be in [1, n_total=%d]" % (k, self.n_total))
        Q = queries.shape[0]
        dev = queries.device
        stream = self._stream(queries)
        out = torch.empty((2, Q, k), dtype=torch.int64, device=dev)        # [0] = float64 score bits, [1] = row ids
        fs, fi = out[0].view(torch.float64), out[1]
        if self._single():
            self.handle.score_topk_dev(queries.data_ptr(), Q, k, fs.data_ptr(), fi.data_ptr(), stream)
            return fs, fi
        world = dist.get_world_size(self.group)
        kl = min(k, self.end - self.start)                                 # what this shard can rank: the library takes k <= rows
        pending = None                                                     # (work, gathered, q0, n) of the previous block
        for q0 in list(range(0, Q, block)) + [None]:
            if q0 is not None:
                n = min(block, Q - q0)
                loc = torch.empty((2, n, k), dtype=torch.int64, device=dev)
                if kl == k:
                    self.handle.score_topk_dev(queries[q0:q0 + n].data_ptr(), n, k, loc[0].data_ptr(), loc[1].data_ptr(), stream)
                else:
                    # short shard: slots kl .. k-1 of every list hold (-inf, INT64_MAX); the library's packed [n, kl]
                    # result is spread into the k-wide rows by a strided device copy on the same stream
                    loc[0].view(torch.float64).fill_(float("-inf"))
                    loc[1].fill_(torch.iinfo(torch.int64).max)
                    if kl > 0:
                        short = torch.empty((2, n, kl), dtype=torch.int64, device=dev)
                        self.handle.score_topk_dev(queries[q0:q0 + n].data_ptr(), n, kl, short[0].data_ptr(), short[1].data_ptr(), stream)
                        loc[:, :, :kl].copy_(short)
                g = torch.empty((world * 2, n, k), dtype=torch.int64, device=dev)   # concatenation along dim 0 (gloo and nccl)
                # one collective for scores and ids; async: RCCL's stream waits for the sweep just enqueued, the host
                # goes on to enqueue the next block's sweep
                work = all_gather_into(g, loc, group=self.group, async_op=True)
                nxt = (work, g, loc, q0, n)
            else:
                nxt = None
            if pending is not None:
                work, g, _loc, p0, pn = pending
                work.wait()                                               # current stream waits for the gather
                self.handle.merge_topk_strided_dev(g.data_ptr(), g[1].data_ptr(), 2 * pn * k, world, pn, k,
                                                   fs[p0:p0 + pn].data_ptr(), fi[p0:p0 + pn].data_ptr(), stream)
            pending = nxt
        return fs, fi

    # -- the eligible-rows family (filtered, after, biased, grouped, lse, confusions): one copy of the checks, of the local
    # lists and of the exchange.  Every check raises before any device call and any collective, on every rank alike.

    def _single(self):
        """One shard and no forced gather: the local call is the result, no collective runs."""
        return self.world == 1 and not self.always_gather

    @staticmethod
    def _stream(t):
        """torch's current stream on t's device as the library takes it (0 for a CPU tensor)."""
        import torch
        return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0

    @staticmethod
    def _opt_ptr(t):
        return t.data_ptr() if t is not None else None

    @staticmethod
    def _check_k(k):
        k = int(k)
        if not 1 <= k <= 1024:
            raise ValueError("k=%d must be in [1, 1024]" % k)
        return k

    @staticmethod
    def _check_masks(any_of, none_of, Q):
        """Both masks checked, then both contiguous (None stays None)."""
        import torch
        for m in (any_of, none_of):
            if m is not None and (m.shape[0] != Q or m.dtype != torch.int64):
                raise ValueError("any_of / none_of must be int64 [Q] tensors of mask bits")
        return [m.contiguous() if m is not None else None for m in (any_of, none_of)]

    @staticmethod
    def _weight_tensor(weight, Q, dev):
        """None, a number or a float32 [Q] tensor -> None or the contiguous float32 [Q] tensor."""
        import torch
        if weight is None:
            return None
        if not torch.is_tensor(weight):
            weight = torch.full((Q,), float(weight), dtype=torch.float32, device=dev)
        if weight.shape[0] != Q or weight.dtype != torch.float32:
            raise ValueError("weight must be a number or a float32 [Q] tensor")
        return weight.contiguous()

    def _set_local_column(self, values, what, dtype, setter):
        """set_local_tags / _groups / _bias: one value per row of this rank goes to `setter`, the handle's index_set_*_dev.
        what = (the values' name in the length error, the whole dtype error); dtype = the torch dtype's name, None: any."""
        if values is not None and values.shape[0] != self.end - self.start:
            raise ValueError("rank %d holds %d rows, got %d %s" % (self.rank, self.end - self.start, values.shape[0], what[0]))
        if self.end == self.start:
            return
        if values is None:
            setter(None, 0)
            return
        import torch
        if dtype is not None and values.dtype != getattr(torch, dtype):
            raise ValueError(what[1])
        values = values.contiguous()
        setter(values.data_ptr(), values.shape[0], self._stream(values))

    def _local_lists(self, planes, queries, k, stream, call):
        """This rank's lists: (loc int64 [planes, Q, k] -- plane 0 float64 score bits, plane 1 row ids, plane 2 group keys --
        and counts int32 [Q]).  With rows and Q > 0, call(one pointer per plane, counts pointer, stream) makes the device
        call; otherwise no handle call is made and the lists are all padding, (-inf, INT64_MAX)."""
        import torch
        Q = int(queries.shape[0])
        loc = torch.empty((planes, Q, k), dtype=torch.int64, device=queries.device)
        cnt = torch.zeros(Q, dtype=torch.int32, device=queries.device)
        if self.end > self.start and Q > 0:
            call(*([loc[p].data_ptr() for p in range(planes)] + [cnt.data_ptr(), stream]))
        else:
            loc[0].view(torch.float64).fill_(float("-inf"))
            loc[1:].fill_(torch.iinfo(torch.int64).max)
        return loc, cnt

    def _gather(self, loc):
        """ONE all-gather of every rank's `loc`: (world, the ranks' tensors concatenated along dim 0)."""
        import torch
        import torch.distributed as dist
        from .collectives import all_gather_into
        world = dist.get_world_size(self.group)
        g = torch.empty((world * loc.shape[0],) + tuple(loc.shape[1:]), dtype=loc.dtype, device=loc.device)
        all_gather_into(g, loc, group=self.group)
        return world, g

    def _merged_topk(self, queries, k, call):
        """What score_topk_filtered, _after and _biased do once their arguments are checked: the local lists (`call` is
        their one differing device call), ONE all-gather, the k-way (score, id) merge, ONE all-reduce of the counts, cut
        at k.  A single shard, or Q == 0, returns the local lists."""
        import torch
        from .collectives import all_reduce_
        Q = int(queries.shape[0])
        stream = self._stream(queries)
        loc, cnt = self._local_lists(2, queries, k, stream, call)
        if Q == 0 or self._single():
            return loc[0].view(torch.float64), loc[1], cnt
        world, g = self._gather(loc)
        out = torch.empty((2, Q, k), dtype=torch.int64, device=queries.device)
        self.handle.merge_topk_strided_dev(g.data_ptr(), g[1].data_ptr(), 2 * Q * k, world, Q, k, out[0].data_ptr(), out[1].data_ptr(), stream)
        total = cnt.to(torch.int64)
        all_reduce_(total, group=self.group)
        return out[0].view(torch.float64), out[1], torch.clamp(total, max=k).to(torch.int32)

    def set_local_tags(self, tags):
        """tags: CUDA uint64 (or int64 holding the same bits) tensor [end-start] -- the tag words of this rank's rows, set
        after set_local_rows.  None clears them; a rank without rows has nothing to tag."""
        self._set_local_column(tags, ("tags", None), None, self.handle.index_set_tags_dev)

    def set_local_groups(self, groups):
        """groups: CUDA int64 tensor [end-start] -- the group keys of this rank's rows, set after set_local_rows.  None
        clears them; a rank without rows has nothing to group."""
        self._set_local_column(groups, ("group keys", "group keys must be an int64 tensor"), "int64", self.handle.index_set_groups_dev)

    def set_local_bias(self, bias):
        """bias: CUDA float32 tensor [end-start] -- the bias of this rank's rows (Handle.index_set_bias), set after
        set_local_rows.  None clears it; a rank without rows has nothing to bias."""
        self._set_local_column(bias, ("bias values", "bias must be a float32 tensor"), "float32", self.handle.index_set_bias_dev)

    def score_topk_filtered(self, queries, k, any_of=None, none_of=None, exclude=None):
        """Handle.score_topk_filtered over the whole sharded index: queries CUDA float32 [Q,S], any_of / none_of int64 [Q]
        tensors holding the uint64 mask bits (or None), exclude int64 [Q, n] GLOBAL row ids (or None), identical on every
        rank.  Returns (scores float64 [Q,k], ids int64 [Q,k], counts int32 [Q]) on every rank: what the unsharded call
        returns.  Every rank makes the local call with the full k (its padding makes short shards uniform; a rank
        without rows contributes all padding), ONE all-gather exchanges the lists, the k-way merge ranks padding behind
        every real entry and fills the slots past the real entries with it, ONE all-reduce adds the counts."""
        import torch
        k = self._check_k(k)
        Q = int(queries.shape[0])
        n_excl = 0
        if exclude is not None:
            if exclude.dim() != 2 or exclude.shape[0] != Q or exclude.dtype != torch.int64 or exclude.shape[1] > 64:
                raise ValueError("exclude must be int64 [Q, n <= 64]")
            n_excl = int(exclude.shape[1])
            exclude = exclude.contiguous() if n_excl else None
        any_of, none_of = self._check_masks(any_of, none_of, Q)
        queries, p = queries.contiguous(), self._opt_ptr
        return self._merged_topk(queries, k, lambda s, i, c, stream: self.handle.score_topk_filtered_dev(
            queries.data_ptr(), Q, k, p(any_of), p(none_of), p(exclude), n_excl, s, i, c, stream))

    def score_topk_after(self, queries, k, after=None, any_of=None, none_of=None):
        """Handle.score_topk_after over the whole sharded index: queries CUDA float32 [Q,S], after = None or (scores float64
        [Q], ids int64 [Q]) tensors -- GLOBAL cursors, the same on every rank, whichever rank holds the cursor's row --
        any_of / none_of int64 [Q] tensors holding the uint64 mask bits (or None).  Returns (scores float64 [Q,k], ids int64
        [Q,k], counts int32 [Q]) on every rank: what the unsharded call returns.  An offset could not be sharded (a shard
        cannot know how many of the rows before it are its own); a cursor can: every rank returns its own k rows after it,
        padded to k, ONE all-gather exchanges the lists, the k-way merge ranks padding behind every real entry, ONE
        all-reduce adds the counts."""
        import torch
        k = self._check_k(k)
        Q = int(queries.shape[0])
        cs = ci = None
        if after is not None:
            cs, ci = after
            if cs.shape[0] != Q or ci.shape[0] != Q or cs.dtype != torch.float64 or ci.dtype != torch.int64:
                raise ValueError("after must be (float64 [Q], int64 [Q]) tensors")
            cs, ci = cs.contiguous(), ci.contiguous()
        any_of, none_of = self._check_masks(any_of, none_of, Q)
        queries, p = queries.contiguous(), self._opt_ptr
        return self._merged_topk(queries, k, lambda s, i, c, stream: self.handle.score_topk_after_dev(
            queries.data_ptr(), Q, k, p(cs), p(ci), p(any_of), p(none_of), s, i, c, stream))

    def score_topk_biased(self, queries, k, weight=None, any_of=None, none_of=None):
        """Handle.score_topk_biased over the whole sharded index: queries CUDA float32 [Q,S], weight None, a number or a
        float32 [Q] tensor, any_of / none_of int64 [Q] tensors holding the uint64 mask bits (or None), identical on every
        rank.  Returns (scores float64 [Q,k], ids int64 [Q,k], counts int32 [Q]) on every rank: what the unsharded call
        returns.  A biased score depends on the query and the row alone, so it is a global quantity: every rank makes the
        local call with the full k, ONE all-gather exchanges the lists, the plain (score, id) merge of score_topk_filtered
        ranks padding behind every real entry, ONE all-reduce adds the counts."""
        k = self._check_k(k)
        Q = int(queries.shape[0])
        weight = self._weight_tensor(weight, Q, queries.device)
        any_of, none_of = self._check_masks(any_of, none_of, Q)
        queries, p = queries.contiguous(), self._opt_ptr
        return self._merged_topk(queries, k, lambda s, i, c, stream: self.handle.score_topk_biased_dev(
            queries.data_ptr(), Q, k, p(weight), p(any_of), p(none_of), s, i, c, stream))

    def score_topk_grouped(self, queries, k, any_of=None, none_of=None):
        """Handle.score_topk_grouped over the whole sharded index: queries CUDA float32 [Q,S], any_of / none_of int64 [Q]
        tensors holding the uint64 mask bits (or None), identical on every rank.  Returns (scores float64 [Q,k], ids int64
        [Q,k], groups int64 [Q,k], counts int32 [Q]) on every rank: what the unsharded call returns.  Every rank makes the
        local call with the full k (a rank without rows contributes all padding), ONE all-gather carries scores, ids and
        groups, merge_grouped_lists collapses the groups again.  Exact: were the representative of an answer group missing
        from its rank's local top-k, k other groups would beat it on that rank alone."""
        import torch
        k = self._check_k(k)
        Q = int(queries.shape[0])
        any_of, none_of = self._check_masks(any_of, none_of, Q)
        queries, p = queries.contiguous(), self._opt_ptr
        loc, cnt = self._local_lists(3, queries, k, self._stream(queries), lambda s, i, g, c, stream: self.handle.score_topk_grouped_dev(
            queries.data_ptr(), Q, k, p(any_of), p(none_of), s, i, g, c, stream))
        if Q == 0 or self._single():
            return loc[0].view(torch.float64), loc[1], loc[2], cnt
        world, g = self._gather(loc)
        g = g.view(world, 3, Q, k).permute(1, 2, 0, 3).reshape(3, Q, world * k)   # the shards' lists side by side
        return merge_grouped_lists(g[0].view(torch.float64), g[1], g[2], k)

    def score_lse(self, queries, scale, weight=None, any_of=None, none_of=None):
        """Handle.score_lse over the whole sharded index: queries CUDA float32 [Q,S], weight None, a number or a float32 [Q]
        tensor, any_of / none_of int64 [Q] tensors holding the uint64 mask bits (or None), identical on every rank.  Returns
        (lse float64 [Q], count int64 [Q], bound float64 [Q]) on every rank.  The reduction is associative across row
        shards: every rank makes the local call, ONE all-gather carries its [Q] results, merge_lse_lists takes the
        logaddexp over the ranks in rank order, adds the counts and takes the largest bound.  A rank without rows, or
        without an eligible row, contributes (-inf, 0)."""
        import torch
        Q = int(queries.shape[0])
        weight = self._weight_tensor(weight, Q, queries.device)
        any_of, none_of = self._check_masks(any_of, none_of, Q)
        queries, p = queries.contiguous(), self._opt_ptr
        loc = torch.zeros((3, Q), dtype=torch.int64, device=queries.device)   # [0] = lse bits, [1] = count, [2] = bound bits
        loc[0].view(torch.float64).fill_(float("-inf"))
        if self.end > self.start and Q > 0:
            self.handle.score_lse_dev(queries.data_ptr(), Q, float(scale), p(weight), p(any_of), p(none_of),
                                      loc[0].data_ptr(), loc[1].data_ptr(), loc[2].data_ptr(), self._stream(queries))
        if Q == 0 or self._single():
            return loc[0].view(torch.float64), loc[1], loc[2].view(torch.float64)
        world, g = self._gather(loc)
        g = g.view(world, 3, Q)
        return merge_lse_lists(g[:, 0].contiguous().view(torch.float64), g[:, 1], g[:, 2].contiguous().view(torch.float64))

    def score_confusions(self, queries, k, positives, margin=float("inf")):
        """Handle.score_confusions over the whole sharded index: queries CUDA float32 [Q,S], positives int64 [Q, n_pos <= 64]
        GLOBAL row ids padded with -1, identical on every rank.  Returns (scores float64 [Q,k], ids int64 [Q,k], counts int32
        [Q], pos_scores float64 [Q], pos_ids int64 [Q]) on every rank: what the unsharded call returns.  The floor hangs on
        the best positive, which one shard holds: every rank calls its handle with margin = +inf (its best k non-positives
        and its own best positive), ONE all-gather carries lists and positives, merge_confusion_lists takes the best
        positive over the ranks, forms the floor and cuts the merged lists at it.  No second device pass."""
        import math
        import torch
        k, margin = self._check_k(k), float(margin)
        if math.isnan(margin) or margin == float("-inf"):
            raise ValueError("margin=%r must be finite or +inf" % margin)
        Q = int(queries.shape[0])
        dev = queries.device
        if positives.dim() != 2 or positives.shape[0] != Q or positives.dtype != torch.int64 or not 1 <= positives.shape[1] <= 64:
            raise ValueError("positives must be int64 [Q, 1 <= n_pos <= 64]")
        queries, positives = queries.contiguous(), positives.contiguous()
        single = self._single()
        pad = torch.iinfo(torch.int64).max
        loc = torch.empty(2 * Q * k + 2 * Q, dtype=torch.int64, device=dev)   # score bits [Q,k] | ids [Q,k] | m bits [Q] | b [Q]
        ls, li = loc[:Q * k].view(Q, k), loc[Q * k:2 * Q * k].view(Q, k)
        lm, lb = loc[2 * Q * k:2 * Q * k + Q], loc[2 * Q * k + Q:]
        cnt = torch.zeros(Q, dtype=torch.int32, device=dev)
        if self.end > self.start and Q > 0:
            self.handle.score_confusions_dev(queries.data_ptr(), Q, k, positives.data_ptr(), positives.shape[1],
                                             margin if single else float("inf"), ls.data_ptr(), li.data_ptr(), cnt.data_ptr(),
                                             lm.data_ptr(), lb.data_ptr(), self._stream(queries))
        else:
            ls.view(torch.float64).fill_(float("-inf"))
            li.fill_(pad)
            lm.view(torch.float64).fill_(float("-inf"))
            lb.fill_(pad)
        if Q == 0 or single:
            return ls.view(torch.float64), li, cnt, lm.view(torch.float64), lb
        world, g = self._gather(loc)
        g = g.view(world, -1)
        gs = g[:, :Q * k].view(torch.float64).view(world, Q, k).permute(1, 0, 2).reshape(Q, world * k)
        gi = g[:, Q * k:2 * Q * k].view(world, Q, k).permute(1, 0, 2).reshape(Q, world * k)
        gm = g[:, 2 * Q * k:2 * Q * k + Q].contiguous().view(torch.float64)
        gb = g[:, 2 * Q * k + Q:]
        return merge_confusion_lists(gs, gi, gm, gb, margin, k)

    def rank_of(self, queries, pair_q, pair_id):
        """Exact global rank of labelled rows: queries CUDA float32 [Q,S], pair_q int32 [L] (query row of pair p), pair_id
        int64 [L] (GLOBAL row id of its label), identical on every rank.  Returns the int64 [L] ranks -- the position of row
        pair_id[p] in score_topk(queries, n_total)[pair_q[p]] -- on every rank.  No lists travel: (1) every rank scores and
        counts the pairs whose row it holds (Handle.score_rank_dev), (2) ONE all-gather hands every rank every pair's
        float64 score (a rank cannot score a row it does not hold), (3) every rank counts, for the pairs it does not own,
        the rows of its shard ranked before the threshold (score, id), (4) ONE all-reduce adds the counts.  An empty shard
        owns no pair and counts nothing.  Bad input raises ValueError on every rank alike, before any collective."""
        import torch
        import torch.distributed as dist
        from .collectives import all_gather_into, all_reduce_
        dev = queries.device
        Q, L = int(queries.shape[0]), int(pair_q.shape[0])
        if pair_id.shape[0] != L or pair_q.dtype != torch.int32 or pair_id.dtype != torch.int64:
            raise ValueError("pair_q int32 [L] and pair_id int64 [L] are required")
        out = torch.zeros(L, dtype=torch.int64, device=dev)
        if L == 0:
            return out
        if bool(((pair_q < 0) | (pair_q >= Q) | (pair_id < 0) | (pair_id >= self.n_total)).any().item()):
            raise ValueError("pair_q must be in [0, Q=%d) and pair_id in [0, n_total=%d)" % (Q, self.n_total))
        stream = self._stream(queries)
        queries, pair_q, pair_id = queries.contiguous(), pair_q.contiguous(), pair_id.contiguous()
        have_rows = self.end > self.start
        if self._single():
            self.handle.score_rank_dev(queries.data_ptr(), Q, pair_q.data_ptr(), pair_id.data_ptr(), L, None, out.data_ptr(), None, stream)
            return out
        world = dist.get_world_size(self.group)
        mine = (pair_id >= self.start) & (pair_id < self.end)
        own, other = torch.nonzero(mine).reshape(-1), torch.nonzero(~mine).reshape(-1)
        score = torch.zeros(L, dtype=torch.float64, device=dev)
        if own.numel() > 0:                                               # (1) owned pairs: scores + local ranks
            pq, pi = pair_q[own].contiguous(), pair_id[own].contiguous()
            b = torch.empty(own.numel(), dtype=torch.int64, device=dev)
            sc = torch.empty(own.numel(), dtype=torch.float64, device=dev)
            self.handle.score_rank_dev(queries.data_ptr(), Q, pq.data_ptr(), pi.data_ptr(), own.numel(), None, b.data_ptr(), sc.data_ptr(), stream)
            out[own] = b
            score[own] = sc
        gathered = torch.empty(world * L, dtype=torch.float64, device=dev)    # (2) concatenation along dim 0, as the lists travel
        all_gather_into(gathered, score, group=self.group)
        bounds = torch.tensor([e for _, e in shard_bounds(self.n_total, world)], dtype=torch.int64, device=dev)
        owner = torch.bucketize(pair_id, bounds, right=True)              # rank whose [start, end) holds the id
        score = gathered.view(world, L).gather(0, owner.view(1, L)).view(L)
        if have_rows and other.numel() > 0:                               # (3) the other ranks' pairs: thresholds
            pq, pi, ps = pair_q[other].contiguous(), pair_id[other].contiguous(), score[other].contiguous()
            b = torch.empty(other.numel(), dtype=torch.int64, device=dev)
            self.handle.score_rank_dev(queries.data_ptr(), Q, pq.data_ptr(), pi.data_ptr(), other.numel(), ps.data_ptr(), b.data_ptr(), None, stream)
            out[other] = b
        all_reduce_(out, group=self.group)                                # (4)
        return out

    def _above_check(self, queries, pair_q, pair_thr):
        import torch
        Q, L = int(queries.shape[0]), int(pair_q.shape[0])
        if pair_thr.shape[0] != L or pair_q.dtype != torch.int32 or pair_thr.dtype != torch.float64:
            raise ValueError("pair_q int32 [L] and pair_thr float64 [L] are required")
        if L > 0 and bool(((pair_q < 0) | (pair_q >= Q)).any().item()):
            raise ValueError("pair_q must be in [0, Q=%d)" % Q)
        return Q, L

    def _above_local(self, queries, pair_q, pair_thr, Q, L, lists):
        """This shard's call: (offsets [L+1], ids, scores) on the device, the lists None when not wanted.  The count-only
        call sizes the lists (one read-back of the total); an empty shard has no index and contributes nothing."""
        import torch
        dev = queries.device
        stream = self._stream(queries)
        off = torch.zeros(L + 1, dtype=torch.int64, device=dev)
        empty = (torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float64, device=dev))
        if self.end == self.start or L == 0:
            return (off,) + (empty if lists else (None, None))
        self.handle.score_above_dev(queries.data_ptr(), Q, pair_q.data_ptr(), pair_thr.data_ptr(), L, 0, off.data_ptr(), None, None, stream)
        if not lists:
            return off, None, None
        total = int(off[-1].item())
        if total == 0:
            return (off,) + empty
        ids = torch.empty(total, dtype=torch.int64, device=dev)
        sc = torch.empty(total, dtype=torch.float64, device=dev)
        self.handle.score_above_dev(queries.data_ptr(), Q, pair_q.data_ptr(), pair_thr.data_ptr(), L, total, off.data_ptr(),
                                    ids.data_ptr(), sc.data_ptr(), stream)
        return off, ids, sc

    def count_above(self, queries, pair_q, pair_thr):
        """Global match counts, int64 [L] on every rank: rows of the whole index with float64 score >= pair_thr[p] for query
        row pair_q[p].  Every shard counts its own rows; ONE all-reduce adds them."""
        import torch
        from .collectives import all_reduce_
        Q, L = self._above_check(queries, pair_q, pair_thr)
        queries, pair_q, pair_thr = queries.contiguous(), pair_q.contiguous(), pair_thr.contiguous()
        off, _, _ = self._above_local(queries, pair_q, pair_thr, Q, L, False)
        cnt = (off[1:] - off[:-1]).contiguous()
        if L > 0 and not self._single():
            all_reduce_(cnt, group=self.group)
        return cnt

    def score_above(self, queries, pair_q, pair_thr):
        """All rows of the whole index at or above a threshold: queries CUDA float32 [Q,S], pair_q int32 [L], pair_thr
        float64 [L], identical on every rank.  Returns (offsets int64 [L+1], ids int64 [total], scores float64 [total]) --
        what the unsharded Handle.score_above returns -- on every rank.  (1) every rank lists its shard's matches with
        global ids, (2) ONE all-gather of the per-pair counts, (3) ONE all-gather of the lists padded to the largest local
        total, (4) every pair's runs merged in the library's order (torch stable sorts: plumbing).  An empty shard
        contributes nothing.  Bad input raises ValueError on every rank alike, before any collective."""
        import torch
        import torch.distributed as dist
        from .collectives import all_gather_into
        Q, L = self._above_check(queries, pair_q, pair_thr)
        dev = queries.device
        queries, pair_q, pair_thr = queries.contiguous(), pair_q.contiguous(), pair_thr.contiguous()
        off, ids, sc = self._above_local(queries, pair_q, pair_thr, Q, L, True)
        if L == 0 or self._single():
            return off, ids, sc
        world = dist.get_world_size(self.group)
        cnt = (off[1:] - off[:-1]).contiguous()
        counts = torch.empty(world * L, dtype=torch.int64, device=dev)
        all_gather_into(counts, cnt, group=self.group)
        counts = counts.view(world, L)
        width = int(counts.sum(1).max().item())
        if width == 0:
            return off, ids, sc
        loc = torch.zeros((2, width), dtype=torch.int64, device=dev)          # [0] = float64 score bits, [1] = ids
        loc[0, :ids.numel()] = sc.view(torch.int64)
        loc[1, :ids.numel()] = ids
        g = torch.empty((world * 2, width), dtype=torch.int64, device=dev)
        all_gather_into(g, loc, group=self.group)
        g = g.view(world, 2, width)
        pair_all, sc_all, id_all = [], [], []
        pairs = torch.arange(L, dtype=torch.int64, device=dev)
        for r in range(world):                                                # a shard's list is pair-major: its counts say whose entry is whose
            n = int(counts[r].sum().item())
            pair_all.append(torch.repeat_interleave(pairs, counts[r]))
            sc_all.append(g[r, 0, :n].view(torch.float64))
            id_all.append(g[r, 1, :n])
        return merge_above_runs(torch.cat(pair_all), torch.cat(sc_all), torch.cat(id_all), L)


class RcclShardedIndex(object):
    """The same sharded index WITHOUT torch.distributed: the exchange is the library's own entry point
    (sse_score_topk_sharded_dev: shard sweep -> ONE ncclAllGather of the packed lists -> k-way merge, all on one stream)
    over an RCCL communicator created through the C ABI.  What a reference-side integration that must not import torch
    uses; the host moves the 128-byte unique id from rank 0 to the other ranks itself.
    Limit: k <= the rows of EVERY shard (sse_score_topk_sharded_dev passes k to the shard sweep unchanged), and no shard
    may be empty; ShardedIndex pads short shards instead."""

    def __init__(self, handle, rank, world, n_total, unique_id):
        self.handle, self.rank, self.world = handle, int(rank), int(world)
        self.n_total = int(n_total)
        self.start, self.end = shard_bounds(n_total, world)[rank]
        self.comm = handle.rccl_comm_init_rank(world, rank, unique_id)

    def close(self):
        if self.comm:
            self.handle.rccl_comm_destroy(self.comm)
            self.comm = None

    def set_local_rows_ptr(self, rows_ptr, n_rows, S, stream=0):
        """rows_ptr: device pointer of this rank's [end-start, S] float32 shard."""
        if n_rows != self.end - self.start:
            raise ValueError("shard of rank %d must have %d rows, got %d" % (self.rank, self.end - self.start, n_rows))
        self.handle.index_set_dev(rows_ptr, n_rows, S, id_base=self.start, stream=stream)

    def score_topk_ptr(self, q_ptr, Q, k, out_scores_ptr, out_ids_ptr, stream=0):
        """q_ptr: device float32 [Q,S] (identical on every rank); out_*: device float64 / int64 [Q,k]: the global top-k."""
        self.handle.score_topk_sharded_dev(self.comm, self.world, q_ptr, Q, k, out_scores_ptr, out_ids_ptr, stream)


def split_rows(n_rows, rank, world):
    """Independent units (sequences to encode): the slice of [0, n_rows) rank handles; no collective."""
    return shard_bounds(n_rows, world)[rank]
