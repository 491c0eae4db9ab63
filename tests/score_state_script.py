"""Scripts for the scoring state a long-lived handle keeps from call to call (DESIGN K6, "per-index state"): the steps, the
indexes, one runner and StateOracle, a numpy model of the handle's scoring interface.  Shared by tests/test_gpu_score_state.py
(GPU: the runner drives sse_amd's Handle and compares every call with a fresh handle, bit for bit and counter for counter) and
tests/test_score_state_host.py (CPU: the runner drives StateOracle, clean and with planted defects).

A step is one of set_index(name) | set_tags(words or None, dev) | set_groups(keys or None, dev) | set_option(name, value) |
call(entry, forms, **args) | refused(step, regex).  The runner hands the steps to a DRIVER (set_index / set_tags / set_groups /
set_option / call / close; GpuDriver in the GPU test, StateOracle here) and keeps a clean StateOracle of its own, the TRUTH,
that sees the same steps: every result is held to the truth's -- ids, counts, offsets and padding exact, scores within
topk_cases.score_bar's formula max(1e-12, two float64 summation orders) |q| |t| -- and preconditions() proves (on the CPU) that the
truth is one a device summing in its own order must reproduce id for id.

Where the references come from.  The case modules' inputs() / expected() / preconditions() / check() are keyed by their own
Case objects (a seed builds queries and index together; no id_base, tags or keys from outside), so they cannot be handed the
script's indexes.  What the script takes from them directly: O.scores_f64 and O.topk (topk_cases), topk_cases.unit and the rows
of its f64_rows / f64_rows_rounded cases (D64 / D32), rank_cases.ranks_from_scores (ranks of index rows),
above_cases.expected_above, grouped_cases.collapse, after_cases.after_on_host, and the formula of topk_cases.score_bar as
the only score tolerance.  What it restates, in float64 numpy: the eligibility rule of filtered_cases.eligible
(StateOracle._eligible), the count of rows before a (score, id) threshold that is no row of the index (StateOracle._rank with
pair_score), and, in place of the modules' preconditions() / check(), preconditions() and against_truth() below -- the same
claims (neighbours further apart than two summation orders; ids, counts and padding exact; scores within the bar) on the
truth's arrays.  tests/test_score_state_host.py proves them on the CPU for every call of every script.

No GPU import here."""
import functools
import re

import numpy as np

from oracle import sse_oracle as O
from tests import above_cases as ABC
from tests import after_cases as AC
from tests import filtered_cases as FC
from tests import grouped_cases as GC
from tests import rank_cases as RC
from tests import topk_cases as TC

BASE = TC.BASE
PAD = FC.PAD_ID
bit = FC.bit
FORMS = ("host", "dev", "queued")     # host buffers | device pointers on the null stream, synchronised | on a stream of its own


# ---------------------------------------------------------------------------------------------------------------- indexes

class Index:
    def __init__(self, name, rows, how, id_base, why):
        self.name, self.rows, self.how, self.id_base, self.why = name, rows, how, id_base, why
        self.N, self.S = rows.shape
        rows.setflags(write=False)

    def __repr__(self):
        return "%s[%dx%d %s base %d]" % (self.name, self.N, self.S, self.how, self.id_base)


def _unit(seed, n, s):
    return TC.unit(np.random.RandomState(seed), n, s)


# score_eps32 of csrc/sse_api.hip (`static float score_eps32(const sse_handle *h)`: 2 (idx_S + 2) 5.97e-8 idx_norm_max), per unit |q|
def score_eps32(S, norm_max):
    return 2.0 * (S + 2) * 5.97e-8 * norm_max


PLANT = 64          # rows per planted group of transition 3
PLANT_Q = 2         # its two queries: 0 the wide group (3 .. 10 eps32(norm 1) |q| from the label), 1 the narrow one (a 16th of that)


@functools.lru_cache(maxsize=None)
def planted():
    """Transition 3 on A2's draw: (q float32 [2,S], rows float32 [9000,S], group rows [2][64], label rows [2]).
    Group g holds 64 rows label_g + d q_g / |q_g|^2, 32 above and 32 below the label's score, |d| from 3.6 to 9 units of
    e_g = eps32(norm 1) |q_g| (g = 0) or e_0 / 16 (g = 1).  With the true norm of A2 the band [s - e, s + e] of the label holds
    none of group 0 and all of group 1; with A16 = 16 x rows (norm 16, band 16 e on scores 16 times as large) the same; a handle
    that scored A2 with the bound of A16 would put group 0 in the band (+64), one that scored A16 with the bound of A2 would
    leave group 1 out (-64).  host test: test_band_preconditions."""
    rng = np.random.RandomState(303)
    t = _unit(102, 9000, 64).astype(np.float64)
    q = TC.unit(rng, PLANT_Q, 64)
    # the labels: the rows at rank 50 of the two queries (about 80 rows at or above them: short lists)
    labels = tuple(int(np.argsort(-(t @ q[g].astype(np.float64)), kind="stable")[50]) for g in range(PLANT_Q))
    groups = []
    free = np.setdiff1d(np.arange(40, 8990), labels)
    spots = rng.choice(free, size=2 * PLANT, replace=False)
    for g in range(PLANT_Q):
        q64 = q[g].astype(np.float64)
        e = score_eps32(64, 1.0) * np.linalg.norm(q64) / (1.0 if g == 0 else 16.0)
        d = np.linspace(3.6, 9.0, PLANT // 2) * e
        d = np.concatenate([d, -d])
        rows = np.sort(spots[g * PLANT:(g + 1) * PLANT])
        t[rows] = t[labels[g]][None, :] + d[:, None] * q64[None, :] / q64.dot(q64)
        groups.append(rows)
    t = t.astype(np.float32)
    for a in (q, t):
        a.setflags(write=False)
    return q, t, tuple(groups), labels


@functools.lru_cache(maxsize=None)
def index(name):
    f64 = TC.inputs(TC.BY_NAME["f64_rows"])[1]
    table = {
        "A": lambda: (_unit(101, 9000, 64), "f32", 0, "N >= 8192: bf16 candidates and idxp16; idx_rm; eight rows in the tail tile"),
        "A2": lambda: (planted()[1].copy(), "f32", 0, "another draw of the same shape (with the planted rows of transition 3)"),
        "A16": lambda: (planted()[1] * np.float32(16.0), "f32", 0, "A2 x 16: idx_norm_max = 16"),
        "B": lambda: (_unit(103, 1001, 40), "dev", BASE, "KG 5 inside the allocation A left, tail tile of 9, a shard base"),
        "Bu": lambda: (_unit(103, 1001, 40), "dev_unaligned", BASE, "B's rows 4 bytes past a 16-byte boundary: scalar pack, no idx_rm"),
        "Bx": lambda: (_unit(108, 1001, 64), "f32", 7, "<= 1024 rows at KG 8: the small-index scorer and idx_x3 (Q >= 1024)"),
        "C": lambda: (_unit(104, 1001, 41), "f32", 0, "S % 4 != 0: no idx_rm, KG 6, scalar pack"),
        "D64": lambda: (np.array(f64), "f64", 0, "float64 rows that are not float32 numbers: idx64 set"),
        "D32": lambda: (np.array(TC.inputs(TC.BY_NAME["f64_rows_rounded"])[1]), "f32", 0, "the same rows rounded: idx64 freed"),
        "E": lambda: (_unit(105, 700, 620), "f32", 0, "NQ 1"),
        "F": lambda: (_unit(106, 700, 300), "f32", 3, "NQ 2"),
        "G": lambda: (_unit(107, 33, 5), "f32", 0, "one row in the tail tile, S < 8"),
        # shapes the library refuses (SSE_MAX_INDEX_DIM = 1024).  W64 holds more float64 values than D64 (1500 x 48): a handle
        # that had taken its rows for D64's would read inside the allocation
        "W32": lambda: (_unit(110, 4, 1025), "f32", 0, "refused: S > 1024, float32"),
        "W64": lambda: (_unit(111, 71, 1025).astype(np.float64) * (1.0 + 1e-9), "f64", 0, "refused: S > 1024, float64"),
        "Wd": lambda: (_unit(112, 4, 1025), "dev", 0, "refused: S > 1024, device rows"),
        "H8": lambda: (_unit(109, 300, 8), "f32", 0, "S = the scorer model's encoding size (encode_score_topk)"),
    }
    return Index(name, *table[name]())


def queries(name, Q=10, seed=0):
    """Q unit queries of the index's dimension: the second half are the first half negated (the whole ranking reversed: a
    left-over row scoring 0 sits above every row the negated query scores below zero)."""
    idx = index(name)
    key = {"Bu": "B", "A16": "A2", "D32": "D64"}.get(name, name)
    h = (Q + 1) // 2
    q = _unit(7000 + sum(map(ord, key)) + 13 * seed + Q, h, idx.S)
    q = np.concatenate([q, -q[:Q - h]])
    q.setflags(write=False)
    return q


# ------------------------------------------------------------------------------------------------------------------ steps

class Step:
    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)

    def __repr__(self):
        if self.kind == "set_index":
            return "set_index(%r)" % index(self.name)
        if self.kind in ("set_tags", "set_groups"):
            return "%s(%s%s)" % (self.kind, "None" if self.words is None else "%s[%d]" % (self.label, len(self.words)), ", dev" if self.dev else "")
        if self.kind == "set_option":
            return "set_option(%s=%d)" % (self.name, self.value)
        if self.kind == "refused":
            return "refused(%r)" % self.step
        return "%s%s %s" % (self.entry, list(self.forms), shape_of(self.entry, self.args))


def set_index(name):
    return Step("set_index", name=name)


def set_tags(words, dev=False, label="tags"):
    return Step("set_tags", words=None if words is None else np.ascontiguousarray(words, np.uint64), dev=dev, label=label)


def set_groups(keys, dev=False, label="groups"):
    return Step("set_groups", words=None if keys is None else np.ascontiguousarray(keys, np.int64), dev=dev, label=label)


def set_option(name, value):
    return Step("set_option", name=name, value=int(value))


def call(entry, forms=("host",), **args):
    forms = (forms,) if isinstance(forms, str) else tuple(forms)
    assert all(f in FORMS for f in forms)
    return Step("call", entry=entry, forms=forms, args=args)


def refused(step, regex):
    return Step("refused", step=step, regex=regex)


def shape_of(entry, a):
    out = []
    for key in ("q", "ids"):
        if a.get(key) is not None:
            out.append("%s %s" % (key, "x".join(map(str, np.shape(a[key])))))
    if "k" in a:
        out.append("k %d" % a["k"])
    for key in ("pair_q", "thr"):
        if a.get(key) is not None:
            out.append("L %d" % len(a[key]))
            break
    if a.get("cap") is not None:
        out.append("cap %d" % a["cap"])
    for key in ("after", "any_of", "none_of", "exclude", "pair_score"):
        if a.get(key) is not None:
            out.append(key)
    return " ".join(out)


# ------------------------------------------------------------------------------------------------------------ StateOracle

class Refused(Exception):
    """what the library answers with rc != 0; the text holds the library's wording where a script quotes it"""


MAX_INDEX_DIM = 1024      # SSE_MAX_INDEX_DIM

DEFECTS = ("refused_upload_drops_f64", "tags_kept", "groups_kept", "id_base_kept", "f64_kept", "rows_behind_n", "tag_words_behind_n", "tile_sums_stale",
           "refused_set_tags_changes", "refused_rank_writes")


class StateOracle:
    """The handle's scoring interface on the float64 oracle, with the per-index state of the header (include/sse_hip.h): a new
    index replaces rows and id_base and clears tags and group keys; float32 rows are scored as float32 numbers, float64 rows
    as they came; tags and keys live until the next index or set_*(None); a refused call changes nothing.  `defect`: one of
    DEFECTS, a model of one stale piece (what the GPU test would meet if an invalidation were missing)."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect
        self.t = None
        self.id_base = 0
        self.tags = self.groups = None
        self.opts = {"score_filtered_skip": 1}
        self.prev_t = None            # defects: the index before this one,
        self.ghost_tags = None        # tag words of earlier indexes by row number (zero where none was ever set),
        self.tile_sum = None          # per-tile OR as first computed

    # -- state
    N = property(lambda self: 0 if self.t is None else self.t.shape[0])
    S = property(lambda self: 0 if self.t is None else self.t.shape[1])

    def set_index(self, rows, how, id_base):
        rows = np.asarray(rows)
        d = self.defect
        if rows.shape[1] > MAX_INDEX_DIM:
            if d == "refused_upload_drops_f64" and self.t is not None:
                self.t = self.t.astype(np.float32).astype(np.float64)     # the float64 rows are gone: the float32 image answers
            raise Refused("index dimension %d > %d not supported by the scoring kernel" % (rows.shape[1], MAX_INDEX_DIM))
        new = rows.astype(np.float64) if how == "f64" else rows.astype(np.float32).astype(np.float64)
        if d == "f64_kept" and self.t is not None and how != "f64" and self.t.shape == new.shape and getattr(self, "_was_f64", False):
            new = self.t                                        # the float64 image outlives the float32 upload
        self._was_f64 = how == "f64" or (d == "f64_kept" and new is self.t)
        self.prev_t, self.t = self.t, new
        if not (d == "id_base_kept" and self.prev_t is not None):
            self.id_base = int(id_base)
        if self.tags is not None:
            g = np.zeros(max(len(self.tags), 0 if self.ghost_tags is None else len(self.ghost_tags)), np.uint64)
            if self.ghost_tags is not None:
                g[:len(self.ghost_tags)] = self.ghost_tags
            g[:len(self.tags)] = self.tags
            self.ghost_tags = g
        self.tags = self._carry(self.tags) if d == "tags_kept" else None
        self.groups = self._carry(self.groups) if d == "groups_kept" else None

    def _carry(self, words):
        if words is None:
            return None
        out = np.zeros(self.N, words.dtype)
        n = min(self.N, len(words))
        out[:n] = words[:n]
        return out

    def set_tags(self, words, dev=False):
        if words is None:
            self.tags = None
            return
        words = np.ascontiguousarray(words, np.uint64)
        if self.t is None:
            raise Refused("sse_index_set_tags: no index uploaded")
        if len(words) != self.N:
            if self.defect == "refused_set_tags_changes":
                self.tags = self._carry(words)
            raise Refused("sse_index_set_tags: %d tags for an index of %d rows; the tags are unchanged" % (len(words), self.N))
        self.tags = words.copy()
        if self.tile_sum is None or self.defect != "tile_sums_stale":
            self.tile_sum = self._sums(self.tags)

    @staticmethod
    def _sums(tags):
        pad = np.zeros((len(tags) + 31) // 32 * 32, np.uint64)
        pad[:len(tags)] = tags
        return np.bitwise_or.reduce(pad.reshape(-1, 32), axis=1)

    def set_groups(self, keys, dev=False):
        if keys is None:
            self.groups = None
            return
        keys = np.ascontiguousarray(keys, np.int64)
        if self.t is None:
            raise Refused("sse_index_set_groups: no index uploaded")
        if len(keys) != self.N:
            raise Refused("sse_index_set_groups: %d keys for an index of %d rows; the keys are unchanged" % (len(keys), self.N))
        self.groups = keys.copy()

    def set_option(self, name, value):
        self.opts[name] = int(value)

    def close(self):
        pass

    # -- the table a call ranks: rows, ids, tag words, keys (a defect adds rows behind N)
    def _table(self, masked):
        t, N = self.t, self.N
        ids = np.arange(N, dtype=np.int64)
        tags = self.tags
        ghost = None
        if self.defect == "rows_behind_n" and self.prev_t is not None and self.prev_t.shape[0] > N:
            ghost = np.zeros((self.prev_t.shape[0] - N, self.S))
            c = min(self.S, self.prev_t.shape[1])
            ghost[:, :c] = self.prev_t[N:, :c]
            gt = np.zeros(len(ghost), np.uint64)
        elif self.defect == "tag_words_behind_n" and masked and self.ghost_tags is not None and N % 32:
            M = (N + 31) // 32 * 32
            ghost = np.zeros((M - N, self.S))                    # the padding rows of the tail tile score 0 ...
            gt = np.zeros(M - N, np.uint64)
            n = max(0, min(M, len(self.ghost_tags)) - N)
            gt[:n] = self.ghost_tags[N:N + n]                   # ... and carry the words an earlier index left there
            keep = gt != 0
            ghost, gt = ghost[keep], gt[keep]
            ids = np.concatenate([ids, N + np.flatnonzero(keep)])
            t = np.concatenate([t, ghost])
            tags = None if tags is None else np.concatenate([tags, gt])
            return t, ids + self.id_base, tags, self.groups
        if ghost is not None:
            t = np.concatenate([t, ghost])
            ids = np.arange(len(t), dtype=np.int64)
            tags = None if tags is None else np.concatenate([tags, gt])
        return t, ids + self.id_base, tags, self.groups

    def _scores(self, q, masked=False):
        t, ids, tags, groups = self._table(masked)
        return np.ascontiguousarray(O.scores_f64(np.asarray(q, np.float32), t)), ids, tags

    def _eligible(self, entry, Q, tags, any_of, none_of, M):
        """filtered_cases.eligible's rule on the table"""
        if (any_of is not None or none_of is not None) and self.tags is None:
            raise Refused("%s: tag masks given but the index has no tags (sse_index_set_tags)" % entry)
        e = np.ones((Q, M), bool)
        if any_of is not None:
            a = np.asarray(any_of, np.uint64)[:, None]
            e &= (a == 0) | ((tags[None, :] & a) != 0)
        if none_of is not None:
            e &= (tags[None, :] & np.asarray(none_of, np.uint64)[:, None]) == 0
        if self.defect == "tile_sums_stale" and self.opts.get("score_filtered_skip", 1) and any_of is not None and self.tile_sum is not None \
                and (np.asarray(any_of, np.uint64) != 0).all():
            want = np.bitwise_or.reduce(np.asarray(any_of, np.uint64))
            sums = np.zeros((M + 31) // 32, np.uint64)
            n = min(len(sums), len(self.tile_sum))
            sums[:n] = self.tile_sum[:n]
            e &= ((sums & want) != 0)[np.arange(M) // 32][None, :]     # a tile no query of the call can use is skipped
        return e

    # -- entries: every one returns a tuple of arrays
    def call(self, entry, a, form="host"):
        if self.t is None:
            raise Refused("no index uploaded")
        return getattr(self, "_" + entry)(**a)

    def _topk(self, q, k):
        s, ids, _ = self._scores(q)
        if not 1 <= k <= self.N:
            raise Refused("k=%d must be in [1, N=%d]" % (k, self.N))
        ws, wi = O.topk(s, k)
        return np.ascontiguousarray(ws), np.ascontiguousarray(ids[wi])

    def _rank(self, q, pair_q, pair_id, pair_score=None):
        Q = len(q)
        pair_q, pair_id = np.asarray(pair_q, np.int32), np.asarray(pair_id, np.int64)
        bad = [p for p in range(len(pair_q)) if not 0 <= pair_q[p] < Q or (pair_score is None and not self.id_base <= pair_id[p] < self.id_base + self.N)]
        s, ids, _ = self._scores(q)
        before = np.zeros(len(pair_q), np.int64)
        score = np.zeros(len(pair_q), np.float64)
        ranks = RC.ranks_from_scores(s) if pair_score is None else None
        for p in range(len(pair_q)):
            if p in bad:
                continue
            row = s[pair_q[p]]
            if pair_score is None:
                before[p], score[p] = ranks[pair_q[p], pair_id[p] - self.id_base], row[pair_id[p] - self.id_base]
            else:                                              # any (score, id): the rows before it in ranks_from_scores' order
                thr = float(pair_score[p])
                before[p], score[p] = int((row > thr).sum() + ((row == thr) & (ids < pair_id[p])).sum()), thr
        if bad:
            e = Refused("sse_score_rank: pair_q[%d] = %d is not in [0, Q = %d) or a pair_id that is not a row of this index; the call wrote no output"
                        % (bad[0], pair_q[bad[0]], Q))
            e.wrote = (before, score) if self.defect == "refused_rank_writes" else None
            raise e
        return before, score

    def _above(self, q, thr, pair_q, cap):
        pair_q = np.asarray(pair_q, np.int32)
        if ((pair_q < 0) | (pair_q >= len(q))).any():
            raise Refused("sse_score_above: pair_q is not in [0, Q); the call wrote no output")
        s, ids, _ = self._scores(q)
        off, wi, ws = ABC.expected_above(s, pair_q, thr, 0)
        if off[-1] > cap:                                       # the lists do not fit: offsets only
            return off, np.zeros(0, np.int64), np.zeros(0, np.float64)
        return off, np.ascontiguousarray(ids[wi]), ws

    def _count_above(self, q, thr, pair_q):
        return (np.diff(self._above(q, thr, pair_q, 1 << 62)[0]),)

    def _lists(self, entry, q, k, any_of, none_of, max_k=1024):
        if not 1 <= k <= max_k:
            raise Refused("%s: k = %d is not in [1, %d]" % (entry, k, max_k))
        masked = any_of is not None or none_of is not None
        s, ids, tags = self._scores(q, masked)
        e = self._eligible(entry, len(q), tags, any_of, none_of, s.shape[1])
        o = np.argsort(-s, axis=1, kind="stable")               # O.topk's order over the whole table
        return s, ids, e, o

    def _filtered(self, q, k, any_of=None, none_of=None, exclude=None):
        if exclude is not None and np.shape(exclude)[1] > 64:
            raise Refused("sse_score_topk_filtered: n_excl = %d is not in [0, 64]" % np.shape(exclude)[1])
        s, ids, e, o = self._lists("sse_score_topk_filtered", q, k, any_of, none_of)
        if exclude is not None:
            for qi in range(len(q)):
                e[qi] &= ~np.isin(ids, np.asarray(exclude[qi], np.int64))
        return AC.after_on_host(np.take_along_axis(s, o, 1), ids[o], k, None, np.take_along_axis(e, o, 1))

    def _after(self, q, k, after=None, any_of=None, none_of=None):
        if after is not None and (after[0] is None) != (after[1] is None):
            raise Refused("sse_score_topk_after: after_score and after_id are both given or both NULL (%s is missing)"
                          % ("after_score" if after[0] is None else "after_id"))
        s, ids, e, o = self._lists("sse_score_topk_after", q, k, any_of, none_of)
        return AC.after_on_host(np.take_along_axis(s, o, 1), ids[o], k, after, np.take_along_axis(e, o, 1))

    def _grouped(self, q, k, any_of=None, none_of=None):
        if self.groups is None:
            raise Refused("sse_score_topk_grouped: the index has no group keys (sse_index_set_groups)")
        s, ids, e, o = self._lists("sse_score_topk_grouped", q, k, any_of, none_of)
        Q = len(q)
        ws, wi, wg = np.full((Q, k), -np.inf), np.full((Q, k), PAD, np.int64), np.full((Q, k), PAD, np.int64)
        wc = np.zeros(Q, np.int32)
        keys = self.groups
        if len(keys) < s.shape[1]:                              # (rows a defect added: keys of their own)
            keys = np.concatenate([keys, -(10 ** 15) - np.arange(s.shape[1] - len(keys))])
        for qi in range(Q):
            rows = o[qi][e[qi, o[qi]]]
            reps = GC.collapse(rows, keys)[:k] if rows.size else rows
            c = reps.size
            ws[qi, :c], wi[qi, :c], wg[qi, :c], wc[qi] = s[qi, reps], ids[reps], keys[reps], c
        return ws, wi, wg, wc


# --------------------------------------------------------------------------------------- what the truth must satisfy (CPU)

def score_tol(truth, q):
    """(tol, bar) of topk_cases.scales / score_bar on the current index and these queries"""
    qn = float(np.linalg.norm(np.asarray(q, np.float64), axis=1).max())
    tn = float(np.linalg.norm(truth.t, axis=1).max())
    tol = 2.0 * truth.S * 2.0 ** -53 * qn * tn
    return tol, max(1e-12 * qn * tn, tol)


def preconditions(truth, entry, a, want):
    """AssertionError unless the truth's answer to this call is one a device summing in its own order must reproduce id for id:
    every decision of the call (two neighbours of a returned list and the first row left out, a row against a threshold, a
    row against a label) is further apart than two float64 summation orders can move it.  Returns the smallest margin / tol."""
    q = a["q"]
    tol, _ = score_tol(truth, q)
    s = O.scores_f64(np.asarray(q, np.float32), truth.t)
    worst = np.inf
    if entry in ("topk", "filtered", "after", "grouped"):
        # any two rows from the top of the query's ranking down to the first row below its last returned one (every row a
        # mask, a cursor or a group removes on the way included: stricter than needed)
        srt = -np.sort(-s, axis=1)
        for qi in range(len(srt)):
            fin = want[0][qi][np.isfinite(want[0][qi])]
            m = min(int((srt[qi] >= fin.min()).sum()) + 1, srt.shape[1]) if fin.size else 0
            if m > 1:
                worst = min(worst, float((srt[qi, :m - 1] - srt[qi, 1:m]).min()))
    elif entry == "rank":
        for p in range(len(a["pair_q"])):
            row = s[a["pair_q"][p]]
            thr = row[a["pair_id"][p] - truth.id_base] if a.get("pair_score") is None else a["pair_score"][p]
            d = np.abs(row - thr)
            if a.get("pair_score") is None:
                d[a["pair_id"][p] - truth.id_base] = np.inf
            worst = min(worst, float(d.min()))
    elif entry in ("above", "count_above"):
        for p in range(len(a["pair_q"])):
            worst = min(worst, float(np.abs(s[a["pair_q"][p]] - a["thr"][p]).min()))
        srt = -np.sort(-s, axis=1)
        worst = min(worst, float((srt[:, :-1] - srt[:, 1:]).min()))
    assert worst > 2 * tol, "%s %s: a decision %.3e apart, 2 tol = %.3e" % (entry, shape_of(entry, a), worst, 2 * tol)
    return worst / tol


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_outputs(a, b):
    return len(a) == len(b) and all(bits_equal(x, y) for x, y in zip(a, b))


def first_difference(a, b):
    for j, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape:
            return "output %d: shapes %s, %s" % (j, x.shape, y.shape)
        if not bits_equal(x, y):
            w = np.argwhere(x.view(np.int64 if x.itemsize == 8 else np.int32) != y.view(np.int64 if y.itemsize == 8 else np.int32))
            at = tuple(w[0])
            return "output %d: %d entries differ, first at %s: %r, %r" % (j, len(w), at, x[at], y[at])
    return "outputs %d, %d" % (len(a), len(b))


def against_truth(entry, got, want, bar):
    """ids, counts, offsets, keys and padding exact; scores within bar.  Returns the worst |score - truth|."""
    assert len(got) == len(want), (len(got), len(want))
    worst = 0.0
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, "output %d: %s %s, truth %s %s" % (j, g.shape, g.dtype, w.shape, w.dtype)
        if g.dtype == np.float64:
            assert not np.isnan(g).any(), "output %d: NaN" % j
            fin = np.isfinite(w)
            assert np.array_equal(g[~fin], w[~fin]), "output %d: a padding score that is not the truth's" % j
            if fin.any():
                worst = max(worst, float(np.abs(g[fin] - w[fin]).max()))
        else:
            bad = np.argwhere(g != w)
            assert bad.size == 0, "output %d: %d entries differ from the oracle, first at %s: got %d, want %d" % (
                j, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
    assert worst <= bar, "score off by %.3e, bar %.3e" % (worst, bar)
    return worst


# ----------------------------------------------------------------------------------------------------------------- runner

class StepFailed(AssertionError):
    def __init__(self, number, step, message):
        AssertionError.__init__(self, message)
        self.number, self.step = number, step


class Runner:
    """Drives one driver through steps.  fresh: a factory of drivers for comparison (a) of the GPU test (None: no comparison);
    counters: names whose deltas are recorded per call (the driver answers counters(names))."""

    def __init__(self, driver, fresh=None, counters=(), exempt=(), name="", check_preconditions=False, out=None):
        self.d, self.fresh, self.names, self.exempt, self.name = driver, fresh, tuple(counters), tuple(exempt), name
        self.truth = StateOracle()
        self.check_preconditions = check_preconditions
        self.state = dict(index=None, tags=None, groups=None, opts={})
        self.done, self.results, self.lines = [], [], []
        self.out = out

    # -- one step
    def _tag(self, st):
        return "%s step %d %s on %s opts %s after [%s]" % (self.name, len(self.done) + 1, st, self.state["index"], self.state["opts"],
                                                          " -> ".join(map(repr, self.done)) or "-")

    def _fail(self, st, msg):
        raise StepFailed(len(self.done) + 1, st, "%s: %s" % (self._tag(st), msg))

    def _apply(self, d, st):
        if st.kind == "set_index":
            idx = index(st.name)
            d.set_index(idx.rows, idx.how, idx.id_base)
        elif st.kind == "set_tags":
            d.set_tags(st.words, st.dev)
        elif st.kind == "set_groups":
            d.set_groups(st.words, st.dev)
        elif st.kind == "set_option":
            d.set_option(st.name, st.value)

    def _record(self, st):
        s = self.state
        if st.kind == "set_index":
            s.update(index=st.name, tags=None, groups=None)
        elif st.kind == "set_tags":
            s["tags"] = None if st.words is None else st
        elif st.kind == "set_groups":
            s["groups"] = None if st.words is None else st
        elif st.kind == "set_option":
            s["opts"][st.name] = st.value

    def resolve(self, a):
        """("page_after", n): the cursor is the last entry of every list step n returned (the device's own score and id)"""
        a = dict(a)
        if isinstance(a.get("after"), tuple) and isinstance(a["after"][0], str):
            sc, ids = self.results[a["after"][1] - 1][:2]
            a["after"] = (np.ascontiguousarray(sc[:, -1]), np.ascontiguousarray(ids[:, -1]))
        return a

    def _truth_call(self, entry, a):
        if entry == "after" and a.get("after") is not None and a["after"][0] is not None and a["after"][1] is not None:
            # a device score stands for the truth's score of the same row (after_cases: a cursor is written in rank space)
            cs, ci = np.array(a["after"][0], np.float64), np.asarray(a["after"][1], np.int64)
            s = O.scores_f64(np.asarray(a["q"], np.float32), self.truth.t)
            _, bar = score_tol(self.truth, a["q"])
            for qi in range(len(cs)):
                r = ci[qi] - self.truth.id_base
                if 0 <= r < self.truth.N and abs(s[qi, r] - cs[qi]) <= bar:
                    cs[qi] = s[qi, r]
            a = dict(a, after=(cs, ci))
        return self.truth.call(entry, a)

    def step(self, st):
        if st.kind == "call":
            self._call(st)
        elif st.kind == "refused":
            self._refused(st)
        else:
            try:
                self._apply(self.d, st)
            except Refused as e:
                self._fail(st, "refused: %s" % e)
            self._apply(self.truth, st)
            self._record(st)
            self.results.append(None)
        self.done.append(st)

    def run(self, steps):
        for st in steps:
            self.step(st)
        return self

    def _counted(self, d, entry, a, form):
        c0 = d.counters(self.names) if self.names else ()
        out = d.call(entry, a, form)
        c1 = d.counters(self.names) if self.names else ()
        return out, tuple(y - x for x, y in zip(c0, c1))

    def _build_fresh(self):
        f = self.fresh()
        s = self.state
        for k, v in s["opts"].items():
            f.set_option(k, v)
        self._apply(f, set_index(s["index"]))
        for key in ("tags", "groups"):
            if s[key] is not None:
                self._apply(f, s[key])
        return f

    def _call(self, st):
        a = self.resolve(st.args)
        want = self._truth_call(st.entry, a) if st.entry != "encode_topk" else None
        if self.check_preconditions and want is not None:
            preconditions(self.truth, st.entry, a, want)
        outs, deltas = [], []
        for form in st.forms:
            try:
                o, d = self._counted(self.d, st.entry, a, form)
            except Refused as e:
                self._fail(st, "%s form refused: %s" % (form, e))
            outs.append(o)
            deltas.append(d)
        self._judge(st, a, want, outs, deltas)

    def _judge(self, st, a, want, outs, deltas):
        """forms equal, (a) fresh handle, (b) oracle, the SCORESTATE line; deltas[0] None: the caller compares a block's total.
        Returns the fresh handle's deltas (or None)."""
        for form, o in zip(st.forms[1:], outs[1:]):
            if not same_outputs(outs[0], o):
                self._fail(st, "the %s form differs from the %s form (%s)" % (form, st.forms[0], first_difference(outs[0], o)))
        fd = None
        if self.fresh is not None:
            f = self._build_fresh()
            try:
                fo, fd = self._counted(f, st.entry, a, st.forms[0])
            finally:
                f.close()
            if not same_outputs(outs[0], fo):
                self._fail(st, "differs from a fresh handle holding the same index, tags, keys and options (%s)" % first_difference(outs[0], fo))
            if deltas[0] is not None:
                moved = {n: (x, y) for n, x, y in zip(self.names, deltas[0], fd) if x != y and n not in self.exempt}
                if moved:
                    self._fail(st, "counter deltas (long-lived, fresh) differ: %s" % moved)
        worst = 0.0
        if want is not None:
            _, bar = score_tol(self.truth, a["q"])
            try:
                worst = against_truth(st.entry, outs[0], want, bar)
            except AssertionError as e:
                self._fail(st, "against the float64 oracle: %s" % e)

        def show(d):
            return ",".join("%s=%d" % (n.replace("score_", ""), v) for n, v in zip(self.names, d) if v) or "-"
        line = "SCORESTATE %s step %d %s index %s: worst |score - oracle| %.3e, deltas %s%s" % (
            self.name, len(self.done) + 1, st, self.state["index"], worst,
            " ".join("%s:%s" % (f, show(d)) for f, d in zip(st.forms, deltas) if d is not None),
            "" if fd is None else " fresh:%s" % show(fd))
        self.lines.append(line)
        if self.out is not None:
            self.out(line)
        self.results.append(outs[0])
        return fd

    def block(self, steps):
        """Calls of one form queued back to back on the driver's stream, ONE synchronisation at the end; the counters are read
        around the block and must move by the sum of what the fresh handles' single calls move them by."""
        args = [self.resolve(st.args) for st in steps]
        c0 = self.d.counters(self.names)
        try:
            outs = self.d.queue_block([(st.entry, a) for st, a in zip(steps, args)])
        except Refused as e:
            self._fail(steps[0], "a queued block of %d calls refused: %s" % (len(steps), e))
        total = tuple(y - x for x, y in zip(c0, self.d.counters(self.names)))
        summed = [0] * len(self.names)
        for st, a, o in zip(steps, args, outs):
            want = self._truth_call(st.entry, a)
            fd = self._judge(st, a, want, [o], [None])
            self.done.append(st)
            if fd is not None:
                summed = [x + y for x, y in zip(summed, fd)]
        if self.fresh is not None:
            moved = {n: (x, y) for n, x, y in zip(self.names, total, summed) if x != y and n not in self.exempt}
            assert not moved, "%s: counter deltas of the queued block (long-lived, sum of fresh) differ: %s" % (self._tag(steps[-1]), moved)
        return total

    def _refused(self, st):
        inner = st.step
        try:
            if inner.kind == "call":
                a = self.resolve(inner.args)
                wrote = self.d.call_refused(inner.entry, a, inner.forms[0]) if hasattr(self.d, "call_refused") else self.d.call(inner.entry, a, inner.forms[0])
                if isinstance(wrote, tuple) and len(wrote) == 2 and isinstance(wrote[0], str):
                    msg, touched = wrote                      # (message, None | outputs that no longer hold their pre-fill)
                else:
                    self._fail(st, "was served")
            else:
                self._apply(self.d, inner)
                self._fail(st, "was accepted")
        except Refused as e:
            msg, touched = str(e), getattr(e, "wrote", None)
        if not re.search(st.regex, msg):
            self._fail(st, "refused with %r, want /%s/" % (msg, st.regex))
        if touched is not None:
            self._fail(st, "the refused call wrote output")
        self.results.append(None)


# ---------------------------------------------------------------------------------------------------------------- scripts

def battery(name, page_k=10):
    """The calls of transition 1 after set_index(name): top-k on its three routes, rank, count / rows above, page 2."""
    idx = index(name)
    q = queries(name)
    Q, N = len(q), idx.N
    s = O.scores_f64(q, np.asarray(idx.rows, np.float64))
    srt = -np.sort(-s, axis=1)
    rng = np.random.RandomState(N + idx.S)
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), 3)
    rows = np.stack([np.zeros(Q, np.int64), np.full(Q, N - 1, np.int64), rng.randint(0, N, size=Q)], axis=1).reshape(-1)
    n_above = min(20, N - 1)
    thr = np.concatenate([(srt[:, n_above - 1] + srt[:, n_above]) / 2, [srt[0, 0] + 1.0]])      # 20 rows each; nothing for the last pair
    apq = np.concatenate([np.arange(Q, dtype=np.int32), [0]]).astype(np.int32)
    big = 1030 if N >= 1030 else N
    steps = [call("topk", FORMS, q=q, k=10)]
    at_topk = len(steps)
    steps += [call("topk", q=q, k=min(40, N)),
              call("rank", FORMS, q=q, pair_q=pair_q, pair_id=rows + idx.id_base),
              call("count_above", q=q, thr=thr, pair_q=apq),
              call("above", FORMS, q=q, thr=thr, pair_q=apq, cap=n_above * Q + 3),
              ("page2", at_topk),
              call("topk", q=q[[0, 1, Q - 2, Q - 1]], k=big)]
    return steps, q


def with_pages(steps, offset):
    """("page2", j): score_topk_after with the cursor of the j-th step of this battery, at position offset + j of the script"""
    out = []
    for st in steps:
        if isinstance(st, tuple):
            src = steps[st[1] - 1]
            st = call("after", FORMS, q=src.args["q"], k=src.args["k"], after=("page_after", offset + st[1]))
        out.append(st)
    return out


CHAIN = ("A", "B", "A2", "G", "Bx", "C", "Bu", "D64", "D32", "E", "F", "A")


def chain_script(names=CHAIN):
    """Transition 1.  Returns (steps, {position in names: (first, last) step numbers of its battery})."""
    steps, where = [], {}
    for pos, name in enumerate(names):
        steps.append(set_index(name))
        b, q = battery(name)
        first = len(steps) + 1
        steps += with_pages(b, len(steps))
        if name == "Bx":                                        # the small-index scorer needs Q >= 1024
            steps.append(call("topk", ("host", "dev"), q=queries("Bx", 1024, seed=1), k=10))
        where[pos] = (first, len(steps))
    return steps, where


def sorted_tags(N, nbits=8, reverse=False):
    g = (np.arange(N) * nbits // N).astype(np.uint64)
    if reverse:
        g = np.uint64(nbits - 1) - g
    return (FC.U1 << g).astype(np.uint64)


def tags_script():
    """Transition 4."""
    A, B = index("A"), index("B")
    qa, qb = queries("A"), queries("B")
    Q = len(qa)
    rng = np.random.RandomState(44)
    tags_a = sorted_tags(A.N)
    any_a = (FC.U1 << rng.randint(0, 8, size=Q).astype(np.uint64)).astype(np.uint64)
    none_a = np.full(Q, bit(3), np.uint64)
    keys_a = (rng.permutation(A.N) // 3).astype(np.int64) - 1000
    s = [set_index("A"), set_tags(tags_a, label="sorted"), set_groups(keys_a, label="of3"),
         call("filtered", ("host", "dev"), q=qa, k=10, any_of=any_a, none_of=none_a),
         call("filtered", q=qa, k=40, any_of=any_a)]
    s += [call("after", ("host", "dev"), q=qa, k=40, after=("page_after", len(s)), any_of=any_a),
          call("grouped", ("host", "dev"), q=qa, k=10, any_of=any_a, none_of=none_a),
          # the same N, another draw: tags and keys are gone
          set_index("A2")]
    q2 = queries("A2")
    s += [refused(call("filtered", q=q2, k=10, any_of=any_a), r"tag masks given but the index has no tags"),
          refused(call("after", q=q2, k=10, any_of=any_a), r"tag masks given but the index has no tags"),
          refused(call("grouped", q=q2, k=10), r"no group keys"),
          call("topk", q=q2, k=10)]
    at = len(s)
    s += [call("filtered", q=q2, k=10), call("after", q=q2, k=10), call("topk", q=q2, k=40), call("filtered", q=q2, k=40)]
    # a refused set_tags leaves the old tags in use
    tags_2 = sorted_tags(A.N, reverse=True)
    s += [set_tags(tags_2, label="sorted_reversed"),
          refused(set_tags(tags_a[:-1], label="one_short"), r"the tags are unchanged"),
          refused(set_tags(np.concatenate([tags_a, tags_a[:1]]), label="one_long"), r"the tags are unchanged"),
          call("filtered", q=q2, k=10, any_of=any_a),
          set_tags(None),
          refused(call("filtered", q=q2, k=10, any_of=any_a), r"tag masks given but the index has no tags"),
          # a smaller index, N % 32 != 0, new sorted tags, tile skip on
          set_index("B"), set_option("score_filtered_skip", 1), set_tags(sorted_tags(B.N, reverse=True), label="sorted_reversed")]
    any_b = (FC.U1 << (np.arange(Q) % 8).astype(np.uint64)).astype(np.uint64)
    s += [call("filtered", ("host", "dev"), q=qb, k=100, any_of=any_b),
          call("filtered", q=qb, k=10, any_of=np.full(Q, bit(7), np.uint64)),
          call("after", q=qb, k=100, any_of=any_b),
          set_option("score_filtered_skip", 0),
          call("filtered", q=qb, k=100, any_of=any_b),
          set_option("score_filtered_skip", 1)]
    # tags and keys from device pointers, then replaced on the live index
    keys_b = (rng.permutation(B.N) // 4).astype(np.int64) * 7 - 2 ** 40
    tags_b2 = (FC.U1 << rng.randint(0, 8, size=B.N).astype(np.uint64)).astype(np.uint64)
    s += [set_tags(tags_b2, dev=True, label="random_dev"), set_groups(keys_b, dev=True, label="of4_dev"),
          call("filtered", ("host", "dev"), q=qb, k=40, any_of=any_b),
          call("grouped", ("host", "dev"), q=qb, k=40, any_of=any_b),
          set_tags(sorted_tags(B.N), dev=True, label="sorted_dev"), set_groups(keys_b[::-1].copy(), dev=True, label="of4_reversed_dev"),
          call("filtered", q=qb, k=40, any_of=any_b),
          call("grouped", q=qb, k=40, any_of=any_b),
          call("grouped", q=qb, k=10)]
    return s, dict(same_as_topk=((at, at + 1, at + 2), (at + 3, at + 4)))


def refused_script():
    """Transition 6: every refused call is followed at once by a good one."""
    A = index("A")
    q = queries("A")
    Q = len(q)
    b, _ = battery("A")
    rank, above = b[2], b[4]
    total = 20 * Q
    bad_pq = rank.args["pair_q"].copy()
    bad_pq[7] = Q
    good = call("topk", ("host", "dev"), q=q, k=10)
    s = [set_index("A"), set_tags(sorted_tags(A.N), label="sorted"), good]
    s += [refused(call("topk", q=q, k=0), r"k=0 must be in \[1, N=9000\]"), good,
          refused(call("topk", "dev", q=q, k=A.N + 1), r"k=9001 must be in \[1, N=9000\]"), call("topk", q=q, k=40),
          refused(call("rank", q=q, pair_q=bad_pq, pair_id=rank.args["pair_id"]), r"pair_q\[7\] = 10 is not in \[0, Q = 10\)"), rank,
          refused(call("rank", "dev", q=q, pair_q=bad_pq, pair_id=rank.args["pair_id"]), r"the call wrote no output"), rank,
          # a cap one below the total: offsets only, no error; the lists of the next call are whole
          call("above", ("host", "dev"), q=q, thr=above.args["thr"], pair_q=above.args["pair_q"], cap=total - 1), above,
          refused(call("after", "dev", q=q, k=10, after=(np.zeros(Q), None)), r"both given or both NULL \(after_id is missing\)"),
          call("after", ("host", "dev"), q=q, k=10, after=("page_after", 3)),
          refused(call("filtered", q=q, k=10, exclude=np.zeros((Q, 65), np.int64)), r"n_excl = 65 is not in \[0, 64\]"),
          call("filtered", ("host", "dev"), q=q, k=10, any_of=np.full(Q, bit(2), np.uint64), exclude=np.full((Q, 64), -1, np.int64)),
          refused(call("filtered", q=q, k=0), r"k = 0 is not in \[1, 1024\]"),
          refused(call("grouped", q=q, k=10), r"no group keys"), good]
    return s


def refused_upload_script():
    """Transition 6, uploads: an index the library refuses leaves the resident one -- float64 rows, id_base, tags, keys -- as
    it was, whichever entry point refused it."""
    D = index("D64")
    q = queries("D64")
    Q = len(q)
    rng = np.random.RandomState(66)
    tags = (FC.U1 << rng.randint(0, 4, size=D.N).astype(np.uint64)).astype(np.uint64)
    keys = (rng.permutation(D.N) // 2).astype(np.int64)
    any_ = (FC.U1 << (np.arange(Q) % 4).astype(np.uint64)).astype(np.uint64)
    good = [call("topk", ("host", "dev"), q=q, k=10), call("topk", q=q, k=40), call("filtered", q=q, k=10, any_of=any_),
            call("grouped", q=q, k=10, any_of=any_), call("rank", q=q, pair_q=np.arange(Q, dtype=np.int32), pair_id=np.arange(Q, dtype=np.int64) * 149)]
    s = [set_index("D64"), set_tags(tags, label="one_of_4"), set_groups(keys, label="pairs")] + good
    for bad in ("W32", "W64", "Wd"):
        s += [refused(set_index(bad), r"index dimension 1025 > 1024")] + good
    return s


def two_handles_script():
    """Transition 7: (steps of X on E, steps of Y on G), alternated call by call by the tests."""
    out = []
    for name in ("E", "G"):
        idx = index(name)
        b, q = battery(name)
        Q = len(q)
        rng = np.random.RandomState(idx.N)
        tags = (FC.U1 << rng.randint(0, 4, size=idx.N).astype(np.uint64)).astype(np.uint64)
        keys = (rng.permutation(idx.N) // 2).astype(np.int64)
        any_ = (FC.U1 << (np.arange(Q) % 4).astype(np.uint64)).astype(np.uint64)
        k = min(40, idx.N)
        s = [set_index(name), set_tags(tags, label="one_of_4"), set_groups(keys, label="pairs")]
        s += with_pages(b, len(s))
        s += [call("filtered", q=q, k=k, any_of=any_), call("grouped", q=q, k=k, any_of=any_)]
        out.append(s)
    return out


def alternate(x, y):
    """[(0, step), (1, step), ...]: the set-up steps of both first, then call by call"""
    order = []
    n = max(len(x), len(y))
    for i in range(n):
        if i < len(x):
            order.append((0, x[i]))
        if i < len(y):
            order.append((1, y[i]))
    return order


def bf16_script():
    """Transition 2."""
    qa = queries("A", 129, seed=2)
    qm = queries("A", 1024, seed=3)
    same = call("topk", ("host", "dev"), q=qa, k=10)
    narrow = [set_option("score_two_pass_min_rows", 8999), set_option("score_two_pass_rows", 9001)]
    wide = [set_option("score_two_pass_min_rows", 49152), set_option("score_two_pass_rows", 524288)]
    two_pass = narrow + [call("topk", ("host", "dev"), q=qm, k=10)] + wide
    return ([set_option("score_bf16", 1), set_index("A"), same, set_index("A2"), same, set_option("score_bf16", 0), same,
             set_option("score_bf16", 1), same, set_index("A"), same] + two_pass + [set_index("A2")] + two_pass + [same], qa)


def norm_script():
    """Transition 3."""
    q, t, groups, labels = planted()
    ids = np.array(labels, np.int64)
    pq = np.arange(PLANT_Q, dtype=np.int32)
    s64 = O.scores_f64(q, t.astype(np.float64))
    unit = np.array([score_eps32(64, 1.0) * np.linalg.norm(q[g].astype(np.float64)) / (1.0 if g == 0 else 16.0) for g in range(PLANT_Q)])
    thr = np.array([s64[g, labels[g]] for g in range(PLANT_Q)]) - unit / 2

    def calls(scale):
        return [call("rank", ("host", "dev"), q=q, pair_q=pq, pair_id=ids),
                call("count_above", q=q, thr=thr * scale, pair_q=pq),
                call("above", ("host", "dev"), q=q, thr=thr * scale, pair_q=pq, cap=400)]
    return [set_index("A2")] + calls(1.0) + [set_index("A16")] + calls(16.0) + [set_index("A2")] + calls(1.0)


def scratch_script(form):
    """Transition 5: the calls on A in the order of the issue, all in one form."""
    A = index("A")
    q = queries("A", 40, seed=5)
    Q = len(q)
    rng = np.random.RandomState(55)
    L = 4097
    pair_q = rng.randint(0, Q, size=L).astype(np.int32)
    pair_id = rng.randint(0, A.N, size=L).astype(np.int64)
    s = O.scores_f64(q, np.asarray(A.rows, np.float64))
    srt = -np.sort(-s, axis=1)
    thr = (srt[:, 29] + srt[:, 30]) / 2
    tags = sorted_tags(A.N)
    keys = (rng.permutation(A.N) // 3).astype(np.int64)
    any33 = (FC.U1 << (np.arange(33) % 8).astype(np.uint64)).astype(np.uint64)
    first = call("topk", form, q=q, k=10)
    calls = [first,
             call("rank", form, q=q, pair_q=pair_q, pair_id=pair_id),
             call("filtered", form, q=q[:33], k=40, any_of=any33),
             call("above", form, q=q, thr=thr, pair_q=np.arange(Q, dtype=np.int32), cap=30 * Q + 5),
             call("grouped", form, q=q[:33], k=40, any_of=any33),
             None,
             call("topk", form, q=queries("A", 2080, seed=6), k=20),
             first]
    return [set_index("A"), set_tags(tags, label="sorted"), set_groups(keys, label="of3")], calls, q
