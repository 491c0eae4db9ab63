"""Scripts for in-place index updates (sse_index_update* / sse_index_append*, DESIGN K6n), in the style of
tests/score_state_script.py and on its runner: the contract is that after any sequence of updates and appends a handle is
indistinguishable from a fresh handle given the final rows, tags, group keys and bias.

Steps added to the script's vocabulary: start(label, rows, how, id_base) | update(ids, rows, tags, groups, bias, form) |
append(rows, tags, groups, bias, form) | set_bias(values).  UpdateRunner keeps the FINAL arrays of the index as its state: the
truth (StateOracle) and every fresh handle are given those, so Runner's comparisons (a) fresh handle, bit for bit and counter
for counter, (b) float64 oracle, (c) forms equal, apply unchanged to a handle that reached the same state through updates.

IndexModel is a numpy model of the images a handle keeps (shared with tests/test_index_update_host.py): the update and append
algebra of csrc/sse_api.hip (index_apply_delta / index_grow) with one planted defect at a time.

No GPU import here."""
import numpy as np

from oracle import sse_oracle as O
from tests import confusion_cases as CC
from tests import lse_cases as LC
from tests import score_state_script as SS
from tests import topk_cases as TC

Step, call, FORMS = SS.Step, SS.call, SS.FORMS
KINDS = ("start", "update", "append", "set_bias")


def start(label, rows, how="f32", id_base=0):
    return Step("start", label=label, rows=np.ascontiguousarray(rows), how=how, id_base=int(id_base))


def _col(x, dtype):
    return None if x is None else np.ascontiguousarray(x, dtype).reshape(-1)


def update(ids, rows=None, tags=None, groups=None, bias=None, form="host", label="update"):
    return Step("update", ids=np.ascontiguousarray(ids, np.int64).reshape(-1), rows=None if rows is None else np.ascontiguousarray(rows),
                tags=_col(tags, np.uint64), groups=_col(groups, np.int64), bias=_col(bias, np.float32), form=form, label=label)


def append(rows, tags=None, groups=None, bias=None, form="host", label="append"):
    return Step("append", rows=np.ascontiguousarray(rows), tags=_col(tags, np.uint64), groups=_col(groups, np.int64),
                bias=_col(bias, np.float32), form=form, label=label)


def set_bias(values):
    return Step("set_bias", values=_col(values, np.float32))


def _repr(st):
    if st.kind == "start":
        return "start(%s %dx%d %s base %d)" % (st.label, st.rows.shape[0], st.rows.shape[1], st.how, st.id_base)
    if st.kind == "set_bias":
        return "set_bias(%s)" % ("None" if st.values is None else len(st.values))
    cols = "".join(" +" + n for n in ("tags", "groups", "bias") if getattr(st, n) is not None)
    n = len(st.ids) if st.kind == "update" else len(st.rows)
    return "%s[%s](%d%s%s, %s)" % (st.kind, st.label, n, "" if st.rows is not None else " no rows", cols, st.form)


def apply_to_arrays(state, st):
    """the final arrays after step st (update: entries in order, so the last of a repeated id wins)"""
    s = state
    if st.kind == "start":
        s.update(index=st.label, rows=np.array(st.rows), how=st.how, id_base=st.id_base, tags=None, groups=None, bias=None)
    elif st.kind == "set_bias":
        s["bias"] = None if st.values is None else np.array(st.values)
    elif st.kind == "update":
        r = st.ids - s["id_base"]
        for m in range(len(r)):
            if st.rows is not None:
                s["rows"][r[m]] = st.rows[m]
            for n in ("tags", "groups", "bias"):
                if getattr(st, n) is not None:
                    s[n][r[m]] = getattr(st, n)[m]
    elif st.kind == "append":
        s["rows"] = np.concatenate([s["rows"], st.rows.astype(s["rows"].dtype)])
        for n in ("tags", "groups", "bias"):
            if s[n] is not None:
                s[n] = np.concatenate([s[n], getattr(st, n)])


class UpdateRunner(SS.Runner):
    """Runner over the wider vocabulary.  Drivers answer, besides the script's interface: update(st), append(st), set_bias(values)
    and the entries biased / lse / confusions."""

    def __init__(self, *a, **kw):
        SS.Runner.__init__(self, *a, **kw)
        self.state = dict(index=None, rows=None, how="f32", id_base=0, tags=None, groups=None, bias=None, opts={})

    def _tag(self, st):
        def show(x):
            if x.kind == "refused":
                return "refused(%s)" % show(x.step)
            return _repr(x) if x.kind in KINDS else repr(x)
        return "%s step %d %s after [%s]" % (self.name, len(self.done) + 1, show(st), " -> ".join(show(x) for x in self.done[-6:]) or "-")

    def _apply(self, d, st):
        if st.kind == "start":
            d.set_index(st.rows, st.how, st.id_base)
        elif st.kind == "update":
            d.update(st)
        elif st.kind == "append":
            d.append(st)
        elif st.kind == "set_bias":
            d.set_bias(st.values)
        else:
            SS.Runner._apply(self, d, st)

    def _sync_truth(self):
        s = self.state
        self.truth.set_index(s["rows"], s["how"], s["id_base"])
        self.truth.set_tags(s["tags"])
        self.truth.set_groups(s["groups"])

    def step(self, st):
        if st.kind not in KINDS and st.kind not in ("set_tags", "set_groups"):
            return SS.Runner.step(self, st)
        try:
            self._apply(self.d, st)
        except SS.Refused as e:
            self._fail(st, "refused: %s" % e)
        if st.kind in KINDS:
            apply_to_arrays(self.state, st)
        else:
            self.state["tags" if st.kind == "set_tags" else "groups"] = None if st.words is None else np.array(st.words)
        self._sync_truth()
        self.results.append(None)
        self.done.append(st)

    def _build_fresh(self):
        f = self.fresh()
        s = self.state
        for k, v in s["opts"].items():
            f.set_option(k, v)
        f.set_index(s["rows"], s["how"], s["id_base"])
        if s["tags"] is not None:
            f.set_tags(s["tags"])
        if s["groups"] is not None:
            f.set_groups(s["groups"])
        if s["bias"] is not None:
            f.set_bias(s["bias"])
        return f

    def _truth_call(self, entry, a):
        if entry == "biased":
            s = O.scores_f64(np.asarray(a["q"], np.float32), self.truth.t) + self.state["bias"].astype(np.float64)[None, :]
            sc, ids = O.topk(s, a["k"])
            return sc, ids + self.truth.id_base, np.full(len(s), a["k"], np.int32)
        if entry == "lse":
            s = a["scale"] * O.scores_f64(np.asarray(a["q"], np.float32), self.truth.t)
            return (np.logaddexp.reduce(s, axis=1), np.full(len(s), self.truth.N, np.int64))
        if entry == "confusions":            # the float64 reference of tests/confusion_cases.py on the truth's score matrix
            s = O.scores_f64(np.asarray(a["q"], np.float32), self.truth.t)
            return CC.reference_arrays(s, np.asarray(a["positives"], np.int64), np.inf, a["k"], self.truth.id_base)
        return SS.Runner._truth_call(self, entry, a)

    def lse_bar(self, a):
        """The bar of tests/lse_cases.py (no bias term) on the current index: scale * eps32 |q| (1 + 2^-20), eps32 the host
        layer's score_eps32 at the float64 norm of the largest fp32 row, a factor (1 + S 2^-22) (1 + 2^-22) for the fp32 norm
        and the fp32 rounding of eps32, plus lse_cases.REST = 2^-14 for everything behind the dot products."""
        S = self.truth.S
        norm_max = float(np.linalg.norm(self.truth.t.astype(np.float32).astype(np.float64), axis=1).max())
        qn = np.linalg.norm(np.asarray(a["q"], np.float64), axis=1)
        e = SS.score_eps32(S, norm_max * (1.0 + S * 2.0 ** -22)) * qn * (1.0 + 2.0 ** -20)
        return a["scale"] * e * (1.0 + 2.0 ** -22) + LC.REST

    def _judge(self, st, a, want, outs, deltas):
        if st.entry == "lse":
            # (lse, count, bound): count exact, lse within the bar above of float64 logsumexp, and the call's own bound no
            # wider than that bar; the three outputs are still held to the fresh handle and to each other form bit for bit
            lse, count, bound = outs[0]
            bar = self.lse_bar(a)
            if not np.array_equal(count, want[1]):
                self._fail(st, "lse counts %s, oracle %s" % (count[:8], want[1][:8]))
            err = np.abs(lse - want[0])
            if not (err <= bar).all():
                self._fail(st, "lse off the float64 oracle by %.3e, bar %.3e" % (err.max(), bar[np.argmax(err - bar)]))
            if not ((bound > 0) & (bound <= bar)).all():
                self._fail(st, "lse's own bound %.3e outside (0, bar %.3e]" % (bound.max(), bar[np.argmax(bound - bar)]))
            want = None
        return SS.Runner._judge(self, st, a, want, outs, deltas)


def battery(state, q, after_step, positives=None, tokens=None):
    """every entry of the contract on the state's current arrays: topk at k = 5 and 17, rank, above, filtered, grouped, after,
    biased, lse, confusions in the host, device-pointer and queued forms, and encode_topk (host buffers: its only form) on
    `tokens` int32 [B,T].  after_step: the script position of the first call (its cursor pages the after call)."""
    rows, base = state["rows"], state["id_base"]
    N, Q = len(rows), len(q)
    s = O.scores_f64(q, rows.astype(np.float64) if state["how"] == "f64" else rows.astype(np.float32).astype(np.float64))
    srt = -np.sort(-s, axis=1)
    rng = np.random.RandomState(N)
    pair_q = np.repeat(np.arange(Q, dtype=np.int32), 3)
    pid = np.stack([np.zeros(Q, np.int64), np.full(Q, N - 1, np.int64), rng.randint(0, N, size=Q)], axis=1).reshape(-1) + base
    n_above = min(20, N - 1)
    thr = (srt[:, n_above - 1] + srt[:, n_above]) / 2
    apq = np.arange(Q, dtype=np.int32)
    steps = [call("topk", FORMS, q=q, k=5), call("topk", FORMS, q=q, k=min(17, N)),
             call("rank", FORMS, q=q, pair_q=pair_q, pair_id=pid),
             call("above", FORMS, q=q, thr=thr, pair_q=apq, cap=n_above * Q + 3),
             call("after", FORMS, q=q, k=5, after=("page_after", after_step)),
             call("lse", FORMS, q=q, scale=16.0)]
    if state["tags"] is not None:
        any_of = np.full(Q, 0x6, np.uint64)
        none_of = np.full(Q, 0x1, np.uint64)
        steps.append(call("filtered", FORMS, q=q, k=5, any_of=any_of, none_of=none_of))
        if state["groups"] is not None:
            steps.append(call("grouped", FORMS, q=q, k=5, none_of=none_of))
    elif state["groups"] is not None:
        steps.append(call("grouped", FORMS, q=q, k=5))
    if state["bias"] is not None:
        steps.append(call("biased", FORMS, q=q, k=5))
    pos = np.stack([pid[0::3], pid[2::3]], axis=1) if positives is None else positives
    steps.append(call("confusions", FORMS, q=q, k=5, positives=pos))
    if tokens is not None:
        steps.append(call("encode_topk", ids=tokens, k=min(5, N)))
    return steps


def unit(seed, n, s):
    return TC.unit(np.random.RandomState(seed), n, s)


def columns(N, seed):
    """tags with bits 0..3 (bit 0 doubles as the "hidden" bit of the header's recipe), keys in few groups, a small bias"""
    rng = np.random.RandomState(seed)
    tags = (rng.randint(0, 16, size=N).astype(np.uint64) | np.uint64(2)) & ~np.uint64(1) | (rng.rand(N) < 0.1).astype(np.uint64)
    groups = rng.randint(0, max(4, N // 3), size=N).astype(np.int64)
    bias = (rng.randn(N) * 0.05).astype(np.float32)
    return tags, groups, bias


# ---------------------------------------------------------------------------------------------------------------- IndexModel

DEFECTS = ("idx_rm_stale", "idx64_stale", "idxp16_stale", "idx_x3_stale", "norm2_stale", "norm_max_only_rises", "tile_sum_keeps_bit",
           "absmax_only_rises", "tail_padding_not_zeroed", "idx_x3_valid_past_limit", "idx_rm_valid_past_limit", "realloc_loses_contents",
           "first_duplicate_wins", "refused_call_applies")

RM_LIMIT = 64 << 20       # bytes of row-major rows a handle keeps (index_from_dev_rows)
X3_ROWS = 1024            # rows the small-index scorer serves (score_small_index_applies: <= 32 tiles)


def bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def sumsq(rows32):
    """per-row fp32 sum of squares (the model does not restate the device's summation order: only that every image's norm is
    formed from its own row, by one function)"""
    r = np.asarray(rows32, np.float32)
    return (r * r).sum(axis=1, dtype=np.float32)


class IndexModel:
    """The per-index images of a handle (DESIGN K6, "per-index state"): idxp as rows padded to whole 32-row tiles inside a
    capacity, idx_rm / idx64 / idxp16 / idx_x3 with their valid flags, the per-row norms and norm_max, tags with tile sums,
    keys, bias with absmax, N.  upload() is the fresh handle; update() / append() follow index_apply_delta / index_grow."""

    def __init__(self, defect=None, rm_limit=RM_LIMIT):
        assert defect is None or defect in DEFECTS
        self.defect, self.rm_limit = defect, rm_limit
        self.N = 0
        self.grow_copies = 0

    # -- the fresh handle
    def upload(self, rows, id_base=0, f64=False, garbage=None):
        rows = np.asarray(rows)
        N, S = rows.shape
        self.N, self.S, self.id_base = N, S, int(id_base)
        self.idx64 = rows.astype(np.float64).copy() if f64 else None
        r32 = rows.astype(np.float32)
        NT = (N + 31) // 32
        self.cap_tiles = NT
        self.idxp = np.zeros((NT * 32, S), np.float32)
        self.idxp[:N] = r32
        self.idx_rm = r32.copy() if S % 4 == 0 and N * S * 4 <= self.rm_limit else None
        self.idx_x3 = self._split(self.idxp) if N <= X3_ROWS else None
        self.idxp16 = None                       # built by the first bf16 call
        self.norm2 = None                        # built by the first update
        self.norm_max = np.sqrt(sumsq(r32).max())
        self.tags = self.tile_sum = self.groups = self.bias = self.absmax = None
        self.garbage = garbage                   # what an allocation holds behind the index (a smaller upload into a larger one)
        return self

    @staticmethod
    def _split(p):
        hi = bf16(p)
        return np.stack([hi, bf16(p - hi)])

    def set_columns(self, tags=None, groups=None, bias=None):
        NT = (self.N + 31) // 32
        if tags is not None:
            self.tags = np.zeros(NT * 32, np.uint64)
            self.tags[:self.N] = tags
            self.tile_sum = np.bitwise_or.reduce(self.tags.reshape(-1, 32), axis=1)
        if groups is not None:
            self.groups = np.array(groups, np.int64)
        if bias is not None:
            self.bias = np.zeros(NT * 32, np.float32)
            self.bias[:self.N] = bias
            self.absmax = np.abs(self.bias[:self.N]).max()
        return self

    def bf16_call(self):
        if self.idxp16 is None:
            self.idxp16 = bf16(self.idxp[:(self.N + 31) // 32 * 32])

    # -- refusals (index_delta_check and the host forms' id checks): None, or the reason
    def refusal(self, append, ids, rows, tags, groups, bias, f64=False):
        if self.N == 0:
            return "no index uploaded"
        have = (self.tags is not None, self.groups is not None, self.bias is not None)
        given = (tags is not None, groups is not None, bias is not None)
        if rows is not None and f64 != (self.idx64 is not None):
            return "float64"
        if append:
            if rows is None:
                return "rows must not be NULL"
            if given != have:
                return "exactly when"
            if self.N + len(rows) > 2147483000:
                return "too large"
        else:
            if rows is None and not any(given):
                return "nothing to update"
            if any(g and not h for g, h in zip(given, have)):
                return "not set"
            ids = np.asarray(ids, np.int64)
            if ((ids < self.id_base) | (ids >= self.id_base + self.N)).any():
                return "outside the index"
            if (np.diff(ids) <= 0).any():
                return "strictly increasing"
        if bias is not None and not np.isfinite(bias).all():
            return "not finite"
        return None

    # -- the wrapper's sort (Handle.index_update): ids in any order, the last of a repeated id wins
    def sort_ids(self, ids, *cols):
        ids = np.asarray(ids, np.int64)
        if self.defect == "first_duplicate_wins":
            order = np.argsort(ids, kind="stable")
        else:
            order = len(ids) - 1 - np.argsort(ids[::-1], kind="stable")
        keep = np.ones(len(order), bool)
        keep[1:] = ids[order][1:] != ids[order][:-1]
        order = order[keep]
        return (ids[order],) + tuple(None if c is None else np.asarray(c)[order] for c in cols)

    def _touch(self, r, rows, tags, groups, bias):
        d = self.defect
        if rows is not None:
            if self.norm2 is None:
                self.norm2 = np.zeros(len(self.idxp), np.float32)
                self.norm2[:self.N] = sumsq(self.idxp[:self.N])
            r32 = rows.astype(np.float32)
            self.idxp[r] = r32
            if self.idx64 is not None and d != "idx64_stale":
                self.idx64[r] = rows
            if self.idx_rm is not None and d != "idx_rm_stale":
                self.idx_rm[r] = r32
            if d != "norm2_stale":
                self.norm2[r] = sumsq(r32)
            n2 = self.norm2[:self.N].max()
            self.norm_max = max(self.norm_max, np.sqrt(n2)) if d == "norm_max_only_rises" else np.sqrt(n2)
            tiles = np.unique(r // 32)
            span = (tiles[:, None] * 32 + np.arange(32)[None, :]).reshape(-1)
            if self.idx_x3 is not None and d != "idx_x3_stale":
                self.idx_x3[:, span] = self._split(self.idxp[span])
            if self.idxp16 is not None and d != "idxp16_stale":
                self.idxp16[span] = bf16(self.idxp[span])
        if tags is not None:
            self.tags[r] = tags
            new = np.bitwise_or.reduce(self.tags[:(self.N + 31) // 32 * 32].reshape(-1, 32), axis=1)
            self.tile_sum = (self.tile_sum[:len(new)] | new) if d == "tile_sum_keeps_bit" and len(self.tile_sum) >= len(new) else new
        if groups is not None:
            self.groups[r] = groups
        if bias is not None:
            self.bias[r] = bias
            m = np.abs(self.bias[:self.N]).max()
            self.absmax = max(self.absmax, m) if d == "absmax_only_rises" else m

    def update(self, ids, rows=None, tags=None, groups=None, bias=None, f64=False):
        why = self.refusal(False, ids, rows, tags, groups, bias, f64)
        if why is not None and self.defect != "refused_call_applies":
            return why
        ids = np.asarray(ids, np.int64)
        ok = (ids >= self.id_base) & (ids < self.id_base + self.N)
        pick = lambda c: None if c is None else np.asarray(c)[ok]
        if why is None or (ok.any() and (rows is None or f64 == (self.idx64 is not None))
                           and all(c is None or h is not None for c, h in ((tags, self.tags), (groups, self.groups), (bias, self.bias)))):
            self._touch(ids[ok] - self.id_base, pick(rows), pick(tags), pick(groups), pick(bias))
        return why

    def _grow(self, image, rows_needed, used_rows, fill=0):
        """an image of at least rows_needed rows that keeps its first used_rows"""
        if image is None or len(image) >= rows_needed:
            return image
        out = np.full((rows_needed,) + image.shape[1:], fill, image.dtype)
        if self.defect != "realloc_loses_contents":
            out[:used_rows] = image[:used_rows]
        return out

    def append(self, rows, tags=None, groups=None, bias=None, f64=False):
        why = self.refusal(True, None, rows, tags, groups, bias, f64)
        if why is not None:
            return why
        rows = np.asarray(rows)
        N, M = self.N, len(rows)
        newN = N + M
        NT, newNT = (N + 31) // 32, (newN + 31) // 32
        if newNT > self.cap_tiles:                        # geometric, on this path only
            self.cap_tiles = max(newNT, 2 * self.cap_tiles)
            self.grow_copies += 1
            grown = np.zeros((self.cap_tiles * 32, self.S), np.float32)
            if self.garbage is not None:
                grown[:] = self.garbage
            if self.defect != "realloc_loses_contents":
                grown[:NT * 32] = self.idxp[:NT * 32]
            self.idxp = grown
        if self.defect != "tail_padding_not_zeroed":
            self.idxp[NT * 32:newNT * 32] = 0             # new tiles start as zeros whatever the allocation held
        elif self.garbage is not None:
            self.idxp[NT * 32:newNT * 32] = self.garbage
        if self.idx_rm is not None:
            if newN * self.S * 4 > self.rm_limit and self.defect != "idx_rm_valid_past_limit":
                self.idx_rm = None
            else:
                self.idx_rm = self._grow(self.idx_rm, newN, N)
        self.idx64 = self._grow(self.idx64, newN, N)
        if self.idx_x3 is not None:
            if newN > X3_ROWS and self.defect != "idx_x3_valid_past_limit":
                self.idx_x3 = None
            else:
                x = np.zeros((2, newNT * 32, self.S), np.float32)
                if self.defect != "realloc_loses_contents":
                    x[:, :NT * 32] = self.idx_x3[:, :NT * 32]
                self.idx_x3 = x
        self.idxp16 = self._grow(self.idxp16, newNT * 32, NT * 32)
        self.tags = self._grow(self.tags, newNT * 32, NT * 32)
        self.bias = self._grow(self.bias, newNT * 32, NT * 32)
        self.groups = self._grow(self.groups, newN, N)
        self.norm2 = self._grow(self.norm2, len(self.idxp), N)
        self.N = newN
        self._touch(np.arange(N, newN), rows, tags, groups, bias)
        return None

    # -- what the routes read: every image cut to the live index, invalid ones as None
    def observe(self):
        N, NT32 = self.N, (self.N + 31) // 32 * 32
        cut = lambda x, n: None if x is None else np.array(x[..., :n, :] if x.ndim > 1 else x[:n])
        return dict(N=N, id_base=self.id_base, idxp=cut(self.idxp, NT32), idx_rm=cut(self.idx_rm, N), idx64=cut(self.idx64, N),
                    idxp16=cut(self.idxp16, NT32), idx_x3=cut(self.idx_x3, NT32), norm_max=np.float32(self.norm_max),
                    tags=cut(self.tags, NT32), tile_sum=None if self.tile_sum is None else self.tile_sum[:NT32 // 32].copy(),
                    groups=cut(self.groups, N), bias=cut(self.bias, NT32), absmax=None if self.absmax is None else np.float32(self.absmax))


def fresh_like(model, state, had_bf16):
    """the fresh handle of the contract: the final arrays through the same upload entry, then the setters (and the bf16 call
    that built idxp16, if the long-lived model has made one)"""
    f = IndexModel(rm_limit=model.rm_limit).upload(state["rows"], state["id_base"], f64=state["how"] == "f64")
    f.set_columns(state["tags"], state["groups"], state["bias"])
    if had_bf16:
        f.bf16_call()
    return f


def first_mismatch(a, b):
    """the first image of two observations that differs, or None"""
    for k in a:
        x, y = a[k], b[k]
        if (x is None) != (y is None):
            return "%s: %s, fresh %s" % (k, "invalid" if x is None else "valid", "invalid" if y is None else "valid")
        if x is not None and not SS.bits_equal(np.asarray(x), np.asarray(y)):
            return k
    return None
