"""Top-n evaluation against the target index (reference `sse_evaluator.py:61-114`,
`data_utils.py:263-304`).  The index is uploaded to the GPU once; per batch of
600 sources the encoder output is scored with the fused cosine top-k kernel
instead of np.dot + a full argsort.  The reported numbers keep the reference's
definition: "tight" accuracy per batch, batch accuracies averaged UNWEIGHTED,
for n in (1, 3, 10).  Unlike the reference, sources are encoded and ranked
once, not once per n -- the numbers are identical."""
import codecs

import numpy as np

from . import index_io


def load_index_file(path):
    """Parse targetEncodingIndex.tsv as Evaluator.__init__ does (sse_evaluator.py:80-92):
    lines without exactly 3 fields are skipped; float() per component -> float64."""
    ids, names, fields, id_map = [], [], [], {}
    for line in codecs.open(path, "r", "utf-8").readlines():
        info = line.strip().split("\t")
        if len(info) != 3:
            print("Error in targetIndexFile! %s" % line)
            continue
        id_map[info[0]] = len(ids)
        ids.append(info[0])
        names.append(info[1])
        fields.append(info[2].strip())
    # [float(f) for f in field.split(",")] per row, in C (csrc/index_io.cpp): same float64 values
    return ids, names, index_io.parse_rows(fields), id_map


def topk_tight_accuracy(topk, labels, ranked_idx):
    """computeTopK_TightVersion_accuracy (data_utils.py:270-286)."""
    assert len(labels) == len(ranked_idx)
    k = min(topk, ranked_idx.shape[1])
    total = 0.0
    for i in range(ranked_idx.shape[0]):
        head = ranked_idx[i][:k]
        total += sum(1.0 for lab in labels[i] if lab in head) / len(labels[i])
    return total / float(ranked_idx.shape[0])


def topk_accuracy(topk, labels, ranked_idx):
    """computeTopK_accuracy (data_utils.py:289-304)."""
    assert len(labels) == len(ranked_idx)
    k = min(topk, ranked_idx.shape[1])
    hit = sum(1.0 for i in range(ranked_idx.shape[0]) if any(lab in ranked_idx[i][:k] for lab in labels[i]))
    return hit / float(ranked_idx.shape[0])


def rank_metrics_from_ranks(ranks, top_n=(1, 3, 10), batch=600):
    """Ranking metrics from the exact 0-based ranks of every source's labels (a list of int arrays, label order):
    mrr = mean over sources of 1 / (1 + best rank among its labels); mean_rank / median_rank of 1 + best rank;
    tight_acc[i] = share of a source's labels with rank < top_n[i], averaged per batch of `batch` sources, the batch means
    averaged UNWEIGHTED -- the arithmetic of topk_tight_accuracy + Evaluator.eval, so the values are equal to eval()'s."""
    best = np.array([int(min(r)) for r in ranks], dtype=np.int64)
    tight = []
    for n in top_n:
        accs = []
        for b0 in range(0, len(ranks), batch):
            rows = ranks[b0:b0 + batch]
            total = 0.0
            for r in rows:
                total += sum(1.0 for v in r if v < n) / len(r)
            accs.append(total / float(len(rows)))
        tight.append(np.mean(accs))
    return {"mrr": float(np.mean(1.0 / (1.0 + best))), "mean_rank": float(np.mean(1.0 + best)),
            "median_rank": float(np.median(1.0 + best)), "tight_acc": tight}


def softmax_nll_from(lse, label_scores, scale):
    """Full-softmax negative log-likelihood per source from the log-partition over the whole index (lse float64 [Q],
    Handle.score_lse) and the float64 scores of each source's labels (a list of Q arrays, Handle.score_rank's out_score):
    nll = lse - log sum over its DISTINCT labels of exp(scale * score): the mass the softmax puts on the source's label set.
    `label_scores` holds one score per distinct label.  Returns float64 [Q]; 0 when the labels are all the eligible rows."""
    lse = np.asarray(lse, np.float64)
    out = np.empty(len(label_scores), np.float64)
    for i, s in enumerate(label_scores):
        out[i] = lse[i] - np.logaddexp.reduce(float(scale) * np.asarray(s, np.float64))
    return out


class Evaluator(object):
    def __init__(self, model, eval_corpus, tgtIndexFile, session):
        self.model = model
        self.session = session
        self.srcSeq_batch = [entry[0] for entry in eval_corpus]
        self.targetIDs, _, self.targetEncodings, self.idLabelMap = load_index_file(tgtIndexFile)
        self.eval_Labels = [[self.idLabelMap[t] for t in entry[1]] for entry in eval_corpus]
        model.handle.index_upload(self.targetEncodings)         # float64 rows, resident on the GPU
        self._index_gen = model.handle.index_gen

    def ranked(self, k=10, batch=600):
        """Top-k row indices per eval source, in batches of 600 (sse_evaluator.py:104-111)."""
        k = min(k, len(self.targetIDs))
        h = self.model.handle
        if h.index_gen != self._index_gen:      # predict()/similarity or another Evaluator replaced the handle's index
            h.index_upload(self.targetEncodings)
            self._index_gen = h.index_gen
        # The reference feeds 600 sources per session.run (sse_evaluator.py:104-109).  Rows are independent and every
        # encoder kernel returns the same bits for a row whatever batch it arrives in (tests/test_gpu_encode.py), so the
        # sources go to the device in chunks of up to 32768 rows -- the 64-row-tile matrix kernel at full occupancy
        # instead of 28 launches of the few-sequences kernel on crosslingual's 16,491 queries -- and the ranked lists are
        # cut back into the reference's batches of 600 for its per-batch accuracy means.
        chunk = max(batch, 32768 // batch * batch)
        out = []
        for c0 in range(0, len(self.srcSeq_batch), chunk):
            ids = np.array(self.srcSeq_batch[c0:c0 + chunk], dtype=np.int32)               # the feed dict's array
            # session.run([norm_src_seq_embedding]) + np.dot + getSortedResults in one call: the encodings go from
            # the encoder to the scorer on the device
            _, idx = h.encode_score_topk(0, ids, True, k)
            out.extend(idx[b0:b0 + batch] for b0 in range(0, len(ids), batch))
        return out

    def ranks(self, batch=600):
        """Exact 0-based rank of every eval source's labels over the WHOLE index (label order; int64 arrays): the position
        each label has in the full getSortedResults row (data_utils.py:263-267) that the reference never looks past column
        10 of.  Sources are encoded as ranked() encodes them (same chunks, same bits); the count runs on the device
        (Handle.score_rank), nothing of size Q x N is formed."""
        h = self.model.handle
        if h.index_gen != self._index_gen:      # as in ranked()
            h.index_upload(self.targetEncodings)
            self._index_gen = h.index_gen
        chunk = max(batch, 32768 // batch * batch)
        out = []
        for c0 in range(0, len(self.srcSeq_batch), chunk):
            ids = np.array(self.srcSeq_batch[c0:c0 + chunk], dtype=np.int32)
            labels = self.eval_Labels[c0:c0 + chunk]
            counts = np.array([len(l) for l in labels], dtype=np.int64)
            pair_q = np.repeat(np.arange(len(ids), dtype=np.int32), counts)
            pair_id = np.array([t for l in labels for t in l], dtype=np.int64)
            before, _ = h.score_rank(h.encode(0, ids, True), pair_q, pair_id)
            out.extend(np.split(before, np.cumsum(counts)[:-1]))
        return out

    def softmax_terms(self, scale=64.0, batch=600):
        """(lse float64 [Q], bound float64 [Q], label_scores: Q float64 arrays, one score per DISTINCT label in order of first
        appearance) of the evaluation corpus: the two terms of softmax_nll.  Sources are encoded as ranks() encodes them
        (same chunks, same bits); the log-partition is Handle.score_lse over the whole index, the label scores are
        Handle.score_rank's out_score."""
        h = self.model.handle
        if h.index_gen != self._index_gen:      # as in ranked()
            h.index_upload(self.targetEncodings)
            self._index_gen = h.index_gen
        chunk = max(batch, 32768 // batch * batch)
        lses, bounds, scores = [], [], []
        for c0 in range(0, len(self.srcSeq_batch), chunk):
            ids = np.array(self.srcSeq_batch[c0:c0 + chunk], dtype=np.int32)
            labels = [list(dict.fromkeys(l)) for l in self.eval_Labels[c0:c0 + chunk]]
            counts = np.array([len(l) for l in labels], dtype=np.int64)
            pair_q = np.repeat(np.arange(len(ids), dtype=np.int32), counts)
            pair_id = np.array([t for l in labels for t in l], dtype=np.int64)
            enc = h.encode(0, ids, True)
            _, sc = h.score_rank(enc, pair_q, pair_id)
            lse, _, bound = h.score_lse(enc, scale)
            lses.append(lse)
            bounds.append(bound)
            scores.extend(np.split(sc, np.cumsum(counts)[:-1]))
        return np.concatenate(lses), np.concatenate(bounds), scores

    def softmax_nll(self, scale=64.0, batch=600):
        """Held-out full-softmax cross-entropy over the WHOLE index at logit scale `scale`: per source nll = lse - log sum
        over its distinct labels of exp(scale * score64(label)) -- the objective the in-batch loss (option train_loss = 1)
        estimates, independent of how the sources are chunked.  Returns {"nll": mean nll, "label_prob": mean of exp(-nll)}."""
        self.model.set_forward_only(True)
        lse, _, scores = self.softmax_terms(scale, batch)
        nll = softmax_nll_from(lse, scores, scale)
        return {"nll": float(np.mean(nll)), "label_prob": float(np.mean(np.exp(-nll)))}

    def rank_metrics(self, top_n=(1, 3, 10), batch=600):
        """{mrr, mean_rank, median_rank, tight_acc} over the evaluation corpus (rank_metrics_from_ranks); tight_acc equals
        eval(top_n) exactly, the other three do not saturate when the label falls out of the top 10."""
        self.model.set_forward_only(True)
        return rank_metrics_from_ranks(self.ranks(batch), top_n, batch)

    def eval(self, top_n=(1, 3, 10), batch=600):
        self.model.set_forward_only(True)
        per_batch = self.ranked(max(top_n), batch)
        acc = []
        for n in top_n:
            accs = [topk_tight_accuracy(n, self.eval_Labels[b * batch:(b + 1) * batch], idx)
                    for b, idx in enumerate(per_batch)]
            acc.append(np.mean(accs))
        return acc
