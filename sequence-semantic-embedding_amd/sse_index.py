"""`sse_index` command: encode every target with the target encoder and write
targetEncodingIndex.tsv (reference `sse_index.py:55-126`; same flags, same file
format `id \\t original-case sentence \\t str(np.float32),...`)."""
import codecs
import math
import os
import sys

import numpy as np

from . import flags, index_io, sse_data, sse_text
from .sse_model import Session, SSEModel, get_checkpoint_state

FLAGS = flags.FlagSet("sse_index", [
    ("idx_model_dir", str, "models-classification", "Trained model directory."),
    ("idx_rawfilename", str, "targetIDs", "raw target sequence file to be indexed"),
    ("idx_encodedIndexFile", str, "targetEncodingIndex.tsv", "target sequece encoding index file."),
    ("device", str, "0", "GPU ordinal"),
    ("near_dup_threshold", float, 0.0, "when > 0: also write nearDuplicates.tsv, every pair of targets whose encodings score at least this"),
])


def createIndexFile(model, encoder, rawfile, max_seq_len, encodeIndexFile, session, batchsize=10000, row_of=None):
    if not os.path.exists(rawfile):
        raise FileNotFoundError("Error!! Could not find raw target file to be indexed!! :%s" % rawfile)
    lines = codecs.open(rawfile, "r", "utf-8").readlines()
    cnt = 0
    print("Start indexing whole target space entries with current model ...")
    if model.network_mode in ("source_only_cnn", "source-encoder-only"):
        # no target sequence encoder: norm_tgt_seq_embedding IS the [N,S] variable (sse_model.py:214,233,283);
        # a target id owns the row of its FIRST occurrence among the well-formed lines -- the order in which
        # training numbers the ids (Data.target_row: de-duplicated dict order of fullSetTargetIds); a duplicate id
        # in the file must not shift every later row by one.  row_of(id) overrides when the caller knows better.
        n_rows = int(model.targetSpaceSize)
        first_row = {}
        table = np.vstack(session.run([model.norm_tgt_seq_embedding],
                                      feed_dict=model.get_target_encoding_feed_dict(np.zeros((n_rows, max_seq_len), np.int32))))
        with codecs.open(encodeIndexFile, "w", "utf-8") as out:
            r = 0
            for line in lines:
                cnt += 1
                info = line.strip().split("\t")
                if len(info) != 2:
                    print("Missing field with error line in raw target file: %s " % line)
                    continue
                if info[1] not in first_row:
                    first_row[info[1]] = r
                    r += 1
                row = row_of(info[1]) if row_of else first_row[info[1]]
                if row >= n_rows:
                    raise ValueError("target file has more entries than the model's target matrix (%d rows)" % n_rows)
                out.write(info[1] + "\t" + info[0] + "\t" + index_io.format_rows(table[row:row + 1])[0] + "\n")
        print("Done of all indexing total count:%d" % cnt)
        return
    with codecs.open(encodeIndexFile, "w", "utf-8") as out:
        for b in range(int(math.ceil(len(lines) / float(batchsize)))):
            ids, tids, sents = [], [], []
            for line in lines[b * batchsize:(b + 1) * batchsize]:
                cnt += 1
                info = line.strip().split("\t")
                if len(info) != 2:                                    # sse_index.py:72-74
                    print("Missing field with error line in raw target file: %s " % line)
                    continue
                ids.append(sse_text.pad_tokens(encoder.encode(info[0].lower()), max_seq_len))
                tids.append(info[1])
                sents.append(info[0])
            if not ids:
                continue
            enc = np.vstack(session.run([model.norm_tgt_seq_embedding],
                                        feed_dict=model.get_target_encoding_feed_dict(ids)))
            vecs = index_io.format_rows(enc)          # == ",".join([str(n) for n in enc[i]]), sse_index.py:95
            for i in range(len(sents)):
                out.write(tids[i] + "\t" + sents[i] + "\t" + vecs[i] + "\n")
    print("Done of all indexing total count:%d" % cnt)


def near_duplicate_pairs(handle, rows, threshold, block=4096):
    """Near-duplicate self-join of a target space: `rows` float32 [N,S] are the rows of the handle's resident index (uploaded
    with id_base 0), queried with themselves in blocks of `block` through Handle.score_above.  Returns the list of
    (i, j, score) with i < j and float64 score >= threshold, each pair once, sorted by (i, j)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    ii, jj, ss = [], [], []
    for b0 in range(0, rows.shape[0], int(block)):
        q = rows[b0:b0 + int(block)]
        off, ids, sc = handle.score_above(q, np.full(q.shape[0], float(threshold)))
        qi = np.repeat(np.arange(b0, b0 + q.shape[0], dtype=np.int64), np.diff(off))
        keep = ids > qi                                   # (i, j) and (j, i) both match, (i, i) matches itself: i < j once
        ii.append(qi[keep])
        jj.append(ids[keep])
        ss.append(sc[keep])
    if not ii:
        return []
    ii, jj, ss = np.concatenate(ii), np.concatenate(jj), np.concatenate(ss)
    order = np.lexsort((jj, ii))
    return [(int(ii[o]), int(jj[o]), float(ss[o])) for o in order]


def tag_words(groups):
    """Tag words for Handle.index_set_tags from one group label per row (a meta-category, a language, a shop): `groups` is a
    sequence of N labels with at most 64 distinct ones.  Returns (uint64 [N] one-hot words, {label: bit}); bits are handed out
    in order of first appearance, so `1 << bits[label]` is the `any_of` / `none_of` mask that asks for / rules out a group."""
    bits = {}
    words = np.zeros(len(groups), np.uint64)
    for r, g in enumerate(groups):
        if g not in bits:
            if len(bits) == 64:
                raise ValueError("more than 64 distinct group labels: a tag word has 64 bits")
            bits[g] = len(bits)
        words[r] = np.uint64(1) << np.uint64(bits[g])
    return words, bits


def group_keys(labels):
    """Group keys for Handle.index_set_groups from one label per row (a leaf category, a product, a cluster number): `labels`
    is a sequence of N hashable labels.  Returns (int64 [N] keys, {label: key}).  An integer that fits int64 is its own key;
    every other label gets, in order of first appearance, the smallest key >= 0 that no integer label uses."""
    lo, hi = -(1 << 63), (1 << 63) - 1

    def own(g):
        return isinstance(g, (int, np.integer)) and lo <= int(g) <= hi

    table = {}
    taken = {int(g) for g in labels if own(g)}
    nxt = 0
    keys = np.zeros(len(labels), np.int64)
    for r, g in enumerate(labels):
        if g not in table:
            if own(g):
                table[g] = int(g)
            else:
                while nxt in taken:
                    nxt += 1
                table[g] = nxt
                nxt += 1
        keys[r] = table[g]
    return keys, table


def hard_negatives(handle, queries, positives, n):
    """The n best rows of the handle's resident index per query that are NOT among its labelled positives (the reference
    samples negatives at random, data.py:95-115): `positives` is a sequence of Q sequences of row ids (at most 64 each).
    Returns (ids int64 [Q,n], scores float64 [Q,n]); a query with fewer than n other rows is padded with (INT64_MAX, -inf)."""
    width = max([len(p) for p in positives] + [1])
    if width > 64:
        raise ValueError("at most 64 positives per query can be excluded, got %d" % width)
    ex = np.full((len(positives), width), -1, np.int64)      # -1: no row has this id
    for i, p in enumerate(positives):
        ex[i, :len(p)] = np.asarray(p, np.int64)
    scores, ids, _ = handle.score_topk_filtered(queries, n, exclude=ex)
    return ids, scores


def refresh_rows(model, handle, ids, token_rows, tags=None, groups=None, bias=None, normalize=True):
    """Re-encode changed targets and patch them into the resident index in place: ids int64 [M] global ids (any order, the
    last of a repeated id wins), token_rows int32 [M,T] their padded token rows.  The rows are encoded on the device
    (Handle.encode_dev, target side of `model`) and handed to Handle.index_update_dev as they lie there: the encodings never
    leave the device.  tags / groups / bias: optional new column values per id.  What hard-learning mining and a serving
    process call when targets change; `handle` is the handle holding the index (model.handle unless sharded)."""
    import torch
    ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    toks = np.ascontiguousarray(token_rows, dtype=np.int32)
    if toks.ndim != 2 or toks.shape[0] != ids.shape[0]:
        raise ValueError("token_rows must be [M,T], one row per id")
    order = (ids.shape[0] - 1 - np.argsort(ids[::-1], kind="stable")).astype(np.int64)   # sorted; of equal ids the last first
    order = order[np.concatenate([[True], ids[order][1:] != ids[order][:-1]])] if ids.shape[0] else order
    M = int(order.shape[0])
    if M == 0:
        return 0
    dev = torch.device("cuda:%d" % model.handle.cfg.device)
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt).reshape(-1)[order])).to(dev)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids[order])).to(dev)
    d_tok = torch.from_numpy(np.ascontiguousarray(toks[order])).to(dev)
    enc = torch.empty((M, model.handle.cfg.encoding_size), dtype=torch.float32, device=dev)
    d_tags = up(None if tags is None else np.asarray(tags, np.uint64).view(np.int64), np.int64)
    d_groups, d_bias = up(groups, np.int64), up(bias, np.float32)
    torch.cuda.synchronize(dev)
    model.handle.encode_dev(1, d_tok.data_ptr(), M, toks.shape[1], normalize, enc.data_ptr())
    if handle is not model.handle:
        model.handle.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()
    handle.index_update_dev(d_ids.data_ptr(), enc.data_ptr(), M, ptr(d_tags), ptr(d_groups), ptr(d_bias))
    return M


def csls_bias(handle, target_rows, source_rows, k=10, block=4096):
    """The per-row bias that turns Handle.score_topk_biased (weight 1.0) into the CSLS ranking of cross-lingual retrieval.
    CSLS ranks a source x against targets t by 2 cos(x,t) - r_T(x) - r_S(t), r_S(t) the mean score of t's k nearest SOURCE
    rows; r_T(x) is the same for every target of a query, so the order is that of cos(x,t) - 0.5 r_S(t).  `source_rows`
    float32 [M,S] are uploaded as the handle's index (id_base 0), `target_rows` float32 [N,S] are scored against them with
    Handle.score_topk(..., min(k, M)) in blocks of `block`; returns float32 [N], -0.5 * (mean of those scores) per target row.
    The handle is left holding the SOURCE rows: upload the target index afterwards, then Handle.index_set_bias the result."""
    src = np.ascontiguousarray(source_rows, dtype=np.float32)
    tgt = np.ascontiguousarray(target_rows, dtype=np.float32)
    kk = min(int(k), src.shape[0])
    handle.index_upload(src)
    out = np.empty(tgt.shape[0], np.float32)
    for b0 in range(0, tgt.shape[0], int(block)):
        scores, _ = handle.score_topk(tgt[b0:b0 + int(block)], kk)
        out[b0:b0 + scores.shape[0]] = (-0.5 * np.asarray(scores, np.float64).mean(axis=1)).astype(np.float32)
    return out


def softmax_probs(scores, lse, scale):
    """P(row | query) of returned scores: exp(scale * scores - lse[:, None]) in float64, with `scores` float64 [Q,k] as
    Handle.score_topk / score_topk_filtered / score_topk_biased return them and `lse` float64 [Q] from Handle.score_lse made
    with the same scale, weight and masks.  Padding columns (-inf) give 0, and so does every column of a query whose
    eligible set is empty (lse = -inf)."""
    s = np.asarray(scores, np.float64)
    l = np.asarray(lse, np.float64).reshape(-1, 1)
    live = np.isfinite(s) & np.isfinite(l)
    z = np.where(live, float(scale) * np.where(live, s, 0.0) - np.where(np.isfinite(l), l, 0.0), -np.inf)
    return np.exp(z)


def ranked_pages(handle, queries, page, any_of=None, none_of=None):
    """The whole ranked list of every query, page after page (the reference sorts all targets and cuts once, webserver.py:
    144-151): a generator of (scores float64 [Q,page], ids int64 [Q,page], counts int32 [Q]) from Handle.score_topk_after, each
    call fed with every query's last real entry of the call before.  The pages of a query concatenated over their counts are
    Handle.score_topk(k = N) with the ineligible rows removed; a query that has run out keeps returning count 0.  Stops
    when every count is 0 (that page is not yielded) -- known without a call once every count fell short of `page`."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    Q, page = q.shape[0], int(page)
    cs = np.full(Q, np.inf)                                  # +inf: every row is after it
    ci = np.zeros(Q, np.int64)
    while Q > 0:
        scores, ids, counts = handle.score_topk_after(q, page, after=(cs, ci), any_of=any_of, none_of=none_of)
        if not counts.any():
            return
        yield scores, ids, counts
        if (counts < page).all():
            return
        rows = np.flatnonzero(counts > 0)
        cs[rows], ci[rows] = scores[rows, counts[rows] - 1], ids[rows, counts[rows] - 1]
        # (a query whose count is 0 keeps the cursor that already has nothing after it)


def ranked_rows(handle, queries, k_total, page=1024):
    """The first k_total rows of every query's ranked list for ANY k_total, built from ranked_pages in pages of at most 1024:
    (scores, ids), two lists of Q float64 / int64 arrays of min(k_total, N) entries each, score_topk's columns bit for bit."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    Q, k_total = q.shape[0], int(k_total)
    out_s, out_i = [[] for _ in range(Q)], [[] for _ in range(Q)]
    have = 0
    if k_total > 0:
        for scores, ids, counts in ranked_pages(handle, q, min(int(page), 1024)):
            for r in range(Q):
                out_s[r].append(scores[r, :counts[r]])
                out_i[r].append(ids[r, :counts[r]])
            have += scores.shape[1]
            if have >= k_total:
                break
    return ([np.concatenate(s)[:k_total] if s else np.zeros(0, np.float64) for s in out_s],
            [np.concatenate(i)[:k_total] if i else np.zeros(0, np.int64) for i in out_i])


def write_near_duplicates(path, tgt_ids, pairs):
    """nearDuplicates.tsv: tgtid_a \\t tgtid_b \\t repr(float64 score), one pair per line."""
    with codecs.open(path, "w", "utf-8") as out:
        for i, j, s in pairs:
            out.write("%s\t%s\t%r\n" % (tgt_ids[i], tgt_ids[j], s))


def read_near_duplicates(path):
    out = []
    for line in codecs.open(path, "r", "utf-8"):
        a, b, s = line.rstrip("\n").split("\t")
        out.append((a, b, float(s)))
    return out


def near_duplicates_of_index_file(model, encodeIndexFile, threshold, out_path):
    """reads the index file just written, makes it the model handle's resident index and writes its near-duplicate pairs"""
    tgt_ids, vecs = [], []
    for line in codecs.open(encodeIndexFile, "r", "utf-8"):
        info = line.rstrip("\n").split("\t")
        if len(info) != 3:
            continue
        tgt_ids.append(info[0])
        vecs.append(info[2])
    rows = index_io.parse_rows(vecs).astype(np.float32)
    if rows.shape[0] == 0:
        write_near_duplicates(out_path, tgt_ids, [])
        return 0
    model.handle.index_upload(rows)
    pairs = near_duplicate_pairs(model.handle, rows, threshold)
    write_near_duplicates(out_path, tgt_ids, pairs)
    print("Wrote %d near-duplicate pairs (score >= %r) to %s" % (len(pairs), threshold, out_path))
    return len(pairs)


def index(model_dir, rawfile, encodeIndexFile, batchsize=10000, device=0, near_dup_threshold=0.0):
    if not os.path.exists(model_dir):
        raise FileNotFoundError("Error! Model folder does not exist!! : %s" % model_dir)
    vocab_file = os.path.join(model_dir, "vocabulary.txt")
    if not os.path.exists(vocab_file):
        raise FileNotFoundError("Error!! Could not find vocabulary file for encoder in folder :%s" % model_dir)
    encoder = sse_text.SubwordVocab(vocab_file)
    print("Loaded  vocab size is: %d" % encoder.vocab_size)
    cfg = sse_data.load_model_configs(model_dir)
    model = SSEModel(cfg, device=device)
    ckpt = get_checkpoint_state(model_dir)
    if not ckpt:
        raise FileNotFoundError("Error!!!Could not load any model from specified folder: %s" % model_dir)
    print("Reading model parameters from %s" % ckpt)
    model.saver.restore(None, ckpt)
    createIndexFile(model, encoder, rawfile, int(cfg["max_seq_length"]), encodeIndexFile, Session(model), batchsize)
    if near_dup_threshold > 0:
        near_duplicates_of_index_file(model, encodeIndexFile, near_dup_threshold,
                                      os.path.join(os.path.dirname(encodeIndexFile), "nearDuplicates.tsv"))


def main(argv=None):
    f = FLAGS.parse(sys.argv[1:] if argv is None else argv)
    index(f.idx_model_dir, os.path.join(f.idx_model_dir, f.idx_rawfilename),
          os.path.join(f.idx_model_dir, f.idx_encodedIndexFile), device=int(f.device), near_dup_threshold=float(f.near_dup_threshold))


if __name__ == "__main__":
    main()
