"""The eligible-rows family of ShardedIndex on the CPU: score_topk_filtered, score_topk_grouped, score_topk_after,
score_topk_biased, score_lse and score_confusions as real `gloo` ranks over a stand-in handle (raw pointers of CPU tensors in,
oracle arithmetic), in the style of tests/test_distributed_gloo.py.  What is under test is everything sharded.py does around the
device calls: the checks (which raise before any device call and any collective), the tensors handed down, the padding of a
rank without rows, the collectives and their order, the merges.  Rows, queries, bias and weights are multiples of 1/4 (the
rank_cases.quarter_set construction): every score is exact in any order, so a sharded result must equal the oracle on the
whole index bit for bit, padding included.

Two launches, the smallest that can still go wrong: two ranks over 5 rows (3 + 2, rows 2 and 3 equal: a tie across the
boundary) and three ranks over 2 rows (rank 2 holds nothing, k exceeds the rows), both with k = 4 and Q = 3; and the
single-shard path in this process.  The workers assert; a failed assertion fails the launch with the worker's traceback."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import sse_oracle as O
from tests import after_cases as AC
from tests import biased_cases as BC
from tests import confusion_cases as CC
from tests import grouped_cases as GC
from tests import lse_cases as LC
from tests import rank_cases as RC
from tests.rank_launch import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = np.iinfo(np.int64).max
S, Q, K, SCALE, MARGIN = 16, 3, 4, 2.0, 0.5
MASKED = ("score_topk_filtered", "score_topk_grouped", "score_topk_after", "score_topk_biased", "score_lse")
MASK_TEXT = "any_of / none_of must be int64 [Q] tensors of mask bits"
WEIGHT_TEXT = "weight must be a number or a float32 [Q] tensor"
K_TEXT = "k=%d must be in [1, 1024]"


class _Rows(object):
    """Some rows of the index with their columns (global ids from `base`) and the six calls on them, numpy in and out: the host
    oracles of the *_cases modules on arbitrary arrays.  The whole index for the expected result, one shard inside the
    stand-in handle."""

    def __init__(self, t, base=0, tags=None, groups=None, bias=None):
        self.t, self.base, self.tags, self.groups, self.bias = np.asarray(t, np.float64), int(base), tags, groups, bias

    def _ok(self, n_q, any_, none_):
        n = self.t.shape[0]
        tg = (self.tags if self.tags is not None else np.zeros(n, np.uint64))[None, :]
        e = np.ones((n_q, n), bool)
        if any_ is not None:
            e &= (any_[:, None] == 0) | ((tg & any_[:, None]) != 0)
        if none_ is not None:
            e &= (tg & none_[:, None]) == 0
        return e

    def _bias(self):
        return self.bias if self.bias is not None else np.zeros(self.t.shape[0], np.float32)

    def _best(self, s, ok, k, after=None):
        """score_topk's order of the score matrix s, the entries ok (and after the cursor) kept, cut to k and padded"""
        o = np.argsort(-s, axis=1, kind="stable")
        return AC.after_on_host(np.take_along_axis(s, o, 1), o.astype(np.int64) + self.base, k, after, np.take_along_axis(ok, o, 1))

    def filtered(self, q, k, any_=None, none_=None, exclude=None):
        ok = self._ok(q.shape[0], any_, none_)
        if exclude is not None:
            for qi in range(q.shape[0]):
                r = exclude[qi] - self.base
                ok[qi, r[(r >= 0) & (r < self.t.shape[0])]] = False
        return self._best(O.scores_f64(q, self.t), ok, k)

    def after(self, q, k, after=None, any_=None, none_=None):
        return self._best(O.scores_f64(q, self.t), self._ok(q.shape[0], any_, none_), k, after)

    def biased(self, q, k, w=None, any_=None, none_=None):
        w = np.ones(q.shape[0], np.float32) if w is None else w
        return self._best(BC.biased(O.scores_f64(q, self.t), w, self._bias()), self._ok(q.shape[0], any_, none_), k)

    def grouped(self, q, k, any_=None, none_=None):
        s, ok = O.scores_f64(q, self.t), self._ok(q.shape[0], any_, none_)
        ws, wi, wg = np.full((q.shape[0], k), -np.inf), np.full((q.shape[0], k), PAD, np.int64), np.full((q.shape[0], k), PAD, np.int64)
        cnt = np.zeros(q.shape[0], np.int32)
        for qi in range(q.shape[0]):
            rows = np.argsort(-s[qi], kind="stable")
            reps = GC.collapse(rows[ok[qi, rows]], self.groups)[:k]
            c = cnt[qi] = reps.size
            ws[qi, :c], wi[qi, :c], wg[qi, :c] = s[qi, reps], reps + self.base, self.groups[reps]
        return ws, wi, wg, cnt

    def lse(self, q, scale, w=None, any_=None, none_=None):
        s = O.scores_f64(q, self.t)
        if w is not None:
            s = BC.biased(s, w, self._bias())
        return LC.lse_of(scale * s, self._ok(q.shape[0], any_, none_))

    def confusions(self, q, k, pos, margin):
        return CC.reference_arrays(O.scores_f64(q, self.t), pos, margin, k, id_base=self.base)


def _view(ptr, shape, dtype):
    n = int(np.prod(shape))
    buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def _opt(ptr, shape, dtype):
    return None if ptr is None else _view(ptr, shape, dtype)


class _CpuFamilyHandle(object):
    """Stands in for the HIP handle on CPU tensors.  Every call is recorded as (method, Q, k, the optional pointers that were
    None, n_excl, margin); a field a method does not have is None.  Like the library it refuses an empty index."""

    def __init__(self, width):
        self.S, self.rows, self.calls = width, None, []

    def _note(self, method, n_q=None, k=None, n_excl=None, margin=None, **optional):
        self.calls.append((method, n_q, k, tuple(sorted(n for n, p in optional.items() if p is None)), n_excl, margin))

    def _q(self, q_ptr, n_q):
        return _view(q_ptr, (n_q, self.S), np.float32)

    def index_set_dev(self, ptr, n, width, id_base=0, stream=0):
        self._note("index_set_dev")
        if n <= 0:
            raise ValueError("empty index")                                     # as sse_index_set_dev
        self.rows = _Rows(_view(ptr, (n, width), np.float32).copy(), id_base)

    def _column(self, name, ptr, n, dtype):
        self._note("index_set_%s_dev" % name, ptr=ptr)
        assert (ptr is None and n == 0) or n == self.rows.t.shape[0]
        setattr(self.rows, name, None if ptr is None else _view(ptr, (n,), dtype).copy())

    def index_set_tags_dev(self, ptr, n, stream=0):
        self._column("tags", ptr, n, np.uint64)

    def index_set_groups_dev(self, ptr, n, stream=0):
        self._column("groups", ptr, n, np.int64)

    def index_set_bias_dev(self, ptr, n, stream=0):
        self._column("bias", ptr, n, np.float32)

    @staticmethod
    def _put(outs, ptrs):
        for a, p in zip(outs, ptrs):
            _view(p, a.shape, a.dtype)[...] = a

    def score_topk_filtered_dev(self, q_ptr, n_q, k, any_ptr, none_ptr, excl_ptr, n_excl, s_ptr, i_ptr, c_ptr, stream=0):
        self._note("score_topk_filtered_dev", n_q, k, n_excl, any=any_ptr, none=none_ptr, exclude=excl_ptr)
        self._put(self.rows.filtered(self._q(q_ptr, n_q), k, _opt(any_ptr, (n_q,), np.uint64), _opt(none_ptr, (n_q,), np.uint64),
                                     _opt(excl_ptr, (n_q, n_excl), np.int64)), (s_ptr, i_ptr, c_ptr))

    def score_topk_after_dev(self, q_ptr, n_q, k, cs_ptr, ci_ptr, any_ptr, none_ptr, s_ptr, i_ptr, c_ptr, stream=0):
        self._note("score_topk_after_dev", n_q, k, after_score=cs_ptr, after_id=ci_ptr, any=any_ptr, none=none_ptr)
        assert (cs_ptr is None) == (ci_ptr is None)
        after = None if cs_ptr is None else (_view(cs_ptr, (n_q,), np.float64), _view(ci_ptr, (n_q,), np.int64))
        self._put(self.rows.after(self._q(q_ptr, n_q), k, after, _opt(any_ptr, (n_q,), np.uint64), _opt(none_ptr, (n_q,), np.uint64)),
                  (s_ptr, i_ptr, c_ptr))

    def score_topk_biased_dev(self, q_ptr, n_q, k, w_ptr, any_ptr, none_ptr, s_ptr, i_ptr, c_ptr, stream=0):
        self._note("score_topk_biased_dev", n_q, k, weight=w_ptr, any=any_ptr, none=none_ptr)
        self._put(self.rows.biased(self._q(q_ptr, n_q), k, _opt(w_ptr, (n_q,), np.float32), _opt(any_ptr, (n_q,), np.uint64),
                                   _opt(none_ptr, (n_q,), np.uint64)), (s_ptr, i_ptr, c_ptr))

    def score_topk_grouped_dev(self, q_ptr, n_q, k, any_ptr, none_ptr, s_ptr, i_ptr, g_ptr, c_ptr, stream=0):
        self._note("score_topk_grouped_dev", n_q, k, any=any_ptr, none=none_ptr)
        self._put(self.rows.grouped(self._q(q_ptr, n_q), k, _opt(any_ptr, (n_q,), np.uint64), _opt(none_ptr, (n_q,), np.uint64)),
                  (s_ptr, i_ptr, g_ptr, c_ptr))

    def local_bound(self, n_q):
        """what this shard claims for |lse - its float64 value|: differs by shard, so that the merge has a largest to take"""
        return np.full(n_q, 2.0 ** -40 * (1 + self.rows.base))

    def score_lse_dev(self, q_ptr, n_q, scale, w_ptr, any_ptr, none_ptr, lse_ptr, count_ptr, bound_ptr=None, stream=0):
        self._note("score_lse_dev", n_q, None, None, scale, weight=w_ptr, any=any_ptr, none=none_ptr, bound=bound_ptr)
        lse, count = self.rows.lse(self._q(q_ptr, n_q), scale, _opt(w_ptr, (n_q,), np.float32), _opt(any_ptr, (n_q,), np.uint64),
                                   _opt(none_ptr, (n_q,), np.uint64))
        self._put((lse, count, self.local_bound(n_q)), (lse_ptr, count_ptr, bound_ptr))

    def score_confusions_dev(self, q_ptr, n_q, k, pos_ptr, n_pos, margin, s_ptr, i_ptr, c_ptr, pm_ptr=None, pb_ptr=None, stream=0):
        self._note("score_confusions_dev", n_q, k, None, margin, pos_score=pm_ptr, pos_id=pb_ptr)
        self._put(self.rows.confusions(self._q(q_ptr, n_q), k, _view(pos_ptr, (n_q, n_pos), np.int64), margin),
                  (s_ptr, i_ptr, c_ptr, pm_ptr, pb_ptr))

    def merge_topk_strided_dev(self, s_ptr, i_ptr, stride, P, n_q, k, os_ptr, oi_ptr, stream=0):
        self._note("merge_topk_strided_dev", n_q, k, stride, P)                 # (stride and P in the last two fields)
        assert i_ptr - s_ptr == 8 * n_q * k
        s, i = _view(s_ptr, (P * stride,), np.float64), _view(s_ptr, (P * stride,), np.int64)
        ms = np.stack([s[p * stride:p * stride + n_q * k].reshape(n_q, k) for p in range(P)], 1).reshape(n_q, -1)
        mi = np.stack([i[p * stride + n_q * k:p * stride + 2 * n_q * k].reshape(n_q, k) for p in range(P)], 1).reshape(n_q, -1)
        order = np.lexsort((mi, -ms), axis=1)[:, :k]
        self._put((np.take_along_axis(ms, order, 1), np.take_along_axis(mi, order, 1)), (os_ptr, oi_ptr))


@functools.lru_cache(maxsize=None)
def _inputs(n_rows):
    """The index, its columns and the arguments of every call: the same for every rank.  Read-only."""
    q, t = RC.quarter_set(60 + n_rows, Q, n_rows, S)
    if n_rows > 3:
        t[3] = t[2]                                                             # a tie across the boundary of 3 + 2 rows
        q[0] = t[2]
    d = dict(q=q, t=t, tags=np.array([1, 2, 3, 4, 1], np.uint64)[:n_rows], groups=np.array([7, 7, 9, 7, 9], np.int64)[:n_rows],
             bias=np.array([0.25, -0.5, 1.0, 0.0, 0.75], np.float32)[:n_rows],
             any=np.array([0, 1, 6], np.uint64), none=np.array([0, 2, 0], np.uint64), w=np.array([1.0, 0.5, -0.25], np.float32),
             exclude=np.array([[0, -1], [4, 1], [n_rows + 3, -1]], np.int64),
             positives=np.array([[2 % n_rows, -1], [0, 4], [1, -1]], np.int64))
    full = _Rows(t).after(q, n_rows)                                            # the cursor: each query's second row; query 2 from the top
    d["after_s"] = np.array([full[0][0, 1], full[0][1, 1], np.inf])
    d["after_i"] = np.array([full[1][0, 1], full[1][1, 1], -1], np.int64)
    for a in d.values():
        a.setflags(write=False)
    return d


def _calls(d):
    """name -> (method, args and keywords as numpy arrays): every method once with all it takes, once with the least"""
    m = dict(any_=d["any"], none_=d["none"])
    return {
        "filtered": ("score_topk_filtered", (K,), dict(m, exclude=d["exclude"])), "filtered_plain": ("score_topk_filtered", (K,), {}),
        "after": ("score_topk_after", (K,), dict(m, after=(d["after_s"], d["after_i"]))), "after_plain": ("score_topk_after", (K,), {}),
        "biased": ("score_topk_biased", (K,), dict(m, w=d["w"])), "biased_plain": ("score_topk_biased", (K,), {}),
        "biased_number": ("score_topk_biased", (K,), dict(w=0.5)),
        "grouped": ("score_topk_grouped", (K,), m), "grouped_plain": ("score_topk_grouped", (K,), {}),
        "lse": ("score_lse", (SCALE,), dict(m, w=d["w"])), "lse_plain": ("score_lse", (SCALE,), {}),
        "confusions": ("score_confusions", (K, d["positives"], MARGIN), {}),
        "confusions_no_cut": ("score_confusions", (K, d["positives"]), {}),
    }


def _oracle(rows, q, method, args, kw):
    kw = dict(kw)
    if isinstance(kw.get("w"), float):
        kw["w"] = np.full(q.shape[0], kw["w"], np.float32)
    if method == "score_confusions" and len(args) == 2:
        args = args + (np.inf,)
    return getattr(rows, method.replace("score_topk_", "").replace("score_", ""))(q, *args, **kw)


@functools.lru_cache(maxsize=None)
def _expected(n_rows, world):
    """name -> the arrays every rank must hold.  Everything but lse: the oracle on the WHOLE index.  lse: the shards' oracle
    results joined as merge_lse_lists documents it -- logaddexp over the ranks in rank order from -inf, counts added, the
    largest local bound plus (world - 1) 2^-50 max(1, |lse|) -- which is checked against the whole index below."""
    from sse_amd.sharded import shard_bounds
    d = _inputs(n_rows)
    whole = _Rows(d["t"], 0, d["tags"], d["groups"], d["bias"])
    out = {}
    for name, (method, args, kw) in _calls(d).items():
        want = _oracle(whole, d["q"], method, args, kw)
        if method == "score_lse" and world > 1:
            lse, count, bound = torch.full((Q,), float("-inf"), dtype=torch.float64), np.zeros(Q, np.int64), np.zeros(Q)
            for lo, hi in shard_bounds(n_rows, world):
                if hi > lo:
                    part = _oracle(_Rows(d["t"][lo:hi], lo, d["tags"][lo:hi], d["groups"][lo:hi], d["bias"][lo:hi]), d["q"], method, args, kw)
                    lse, count = torch.logaddexp(lse, torch.from_numpy(part[0])), count + part[1]
                    bound = np.maximum(bound, 2.0 ** -40 * (1 + lo))
            lse = np.where(count > 0, lse.numpy(), -np.inf)
            bound = bound + (world - 1) * 2.0 ** -50 * np.maximum(np.where(count > 0, np.abs(lse), 0.0), 1.0)
            # a logaddexp is within an ulp or two of exact: the joined value is within its own bound (and numpy's reduce)
            assert np.array_equal(count, want[1]) and np.array_equal(np.isinf(lse), np.isinf(want[0]))
            fin = np.isfinite(lse)
            assert (np.abs(lse - want[0])[fin] <= (bound + 2.0 ** -50 * np.maximum(np.abs(want[0]), 1.0))[fin]).all()
            want = (lse, count, bound)
        elif method == "score_lse":
            want = want + (2.0 ** -40 * np.ones(Q),)
        out[name] = tuple(np.ascontiguousarray(a) for a in want)
    return out


def _tensors(method, args, kw):
    """the numpy arguments of _calls() as ShardedIndex takes them: CPU tensors, masks as int64 bits"""
    def bits(a):
        return torch.from_numpy(a.view(np.int64).copy())
    out = {}
    if "any_" in kw:
        out.update(any_of=bits(kw["any_"]), none_of=bits(kw["none_"]))
    if "exclude" in kw:
        out["exclude"] = torch.from_numpy(kw["exclude"].copy())
    if "after" in kw:
        out["after"] = tuple(torch.from_numpy(a.copy()) for a in kw["after"])
    if "w" in kw:
        out["weight"] = kw["w"] if isinstance(kw["w"], float) else torch.from_numpy(kw["w"].copy())
    return tuple(torch.from_numpy(a.copy()) if isinstance(a, np.ndarray) else a for a in args), out


def _local_call(method, args, kw, single):
    """the record the stand-in must hold of the one local call"""
    nones = {"score_topk_filtered": ("any", "exclude", "none"), "score_topk_after": ("after_id", "after_score", "any", "none"),
             "score_topk_biased": ("any", "none", "weight"), "score_topk_grouped": ("any", "none"),
             "score_lse": ("any", "bound", "none", "weight"), "score_confusions": ("pos_id", "pos_score")}[method]
    given = {"any_": ("any",), "none_": ("none",), "exclude": ("exclude",), "after": ("after_id", "after_score"), "w": ("weight",)}
    have = set(n for key in kw for n in given[key]) | {"bound", "pos_id", "pos_score"}
    k = None if method == "score_lse" else K
    n_excl = (2 if "exclude" in kw else 0) if method == "score_topk_filtered" else None
    margin = SCALE if method == "score_lse" else None
    if method == "score_confusions":
        margin = (args[2] if len(args) == 3 else float("inf")) if single else float("inf")
    return (method + "_dev", Q, k, tuple(n for n in nones if n not in have), n_excl, margin)


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        g = g.numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), "%s: %r != %r" % (what, g, w)


def _raises(text, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == text


def _check_setters(sh, h, d):
    """refuse a wrong length (with or without rows); with rows: set, clear on None, set again; without: no handle call"""
    n = sh.end - sh.start
    cols = (("tags", sh.set_local_tags, torch.from_numpy(d["tags"].view(np.int64).copy()), "rank %d holds %d rows, got %d tags"),
            ("groups", sh.set_local_groups, torch.from_numpy(d["groups"].copy()), "rank %d holds %d rows, got %d group keys"),
            ("bias", sh.set_local_bias, torch.from_numpy(d["bias"].copy()), "rank %d holds %d rows, got %d bias values"))
    for name, setter, values, text in cols:
        del h.calls[:]
        _raises(text % (sh.rank, n, n + 1), setter, torch.zeros(n + 1, dtype=values.dtype))
        assert h.calls == []
        setter(values[sh.start:sh.end])
        setter(None)
        if n == 0:
            assert h.calls == []
            continue
        assert getattr(h.rows, name) is None
        assert h.calls == [("index_set_%s_dev" % name, None, None, (), None, None), ("index_set_%s_dev" % name, None, None, ("ptr",), None, None)]
        setter(values[sh.start:sh.end])
        assert np.array_equal(getattr(h.rows, name).view(np.int64) if name == "tags" else getattr(h.rows, name),
                              values[sh.start:sh.end].numpy())
    if n > 0:
        _raises("group keys must be an int64 tensor", sh.set_local_groups, torch.zeros(n, dtype=torch.int32))
        _raises("bias must be a float32 tensor", sh.set_local_bias, torch.zeros(n, dtype=torch.float64))


def _check_errors(sh, h, coll, q):
    """every ValueError with its text, and neither a handle call nor a collective before it"""
    del h.calls[:], coll[:]
    good, pos = torch.zeros(Q, dtype=torch.int64), torch.zeros((Q, 1), dtype=torch.int64)
    for name in ("score_topk_filtered", "score_topk_grouped", "score_topk_after", "score_topk_biased"):
        for k in (0, 1025):
            _raises(K_TEXT % k, getattr(sh, name), q, k)
    for k in (0, 1025):
        _raises(K_TEXT % k, sh.score_confusions, q, k, pos)
    for name in MASKED:
        first = SCALE if name == "score_lse" else K
        for bad in (torch.zeros(Q + 1, dtype=torch.int64), torch.zeros(Q, dtype=torch.int32)):   # wrong length, wrong dtype
            _raises(MASK_TEXT, getattr(sh, name), q, first, any_of=bad)
            _raises(MASK_TEXT, getattr(sh, name), q, first, any_of=good, none_of=bad)
    for name, first in (("score_topk_biased", K), ("score_lse", SCALE)):
        _raises(WEIGHT_TEXT, getattr(sh, name), q, first, weight=torch.zeros(Q + 1, dtype=torch.float32))
        _raises(WEIGHT_TEXT, getattr(sh, name), q, first, weight=torch.zeros(Q, dtype=torch.float64))
    _raises("exclude must be int64 [Q, n <= 64]", sh.score_topk_filtered, q, K, exclude=torch.zeros((Q, 65), dtype=torch.int64))
    _raises("exclude must be int64 [Q, n <= 64]", sh.score_topk_filtered, q, K, exclude=torch.zeros((Q + 1, 2), dtype=torch.int64))
    _raises("after must be (float64 [Q], int64 [Q]) tensors", sh.score_topk_after, q, K,
            after=(torch.zeros(Q, dtype=torch.float32), torch.zeros(Q, dtype=torch.int64)))
    _raises("positives must be int64 [Q, 1 <= n_pos <= 64]", sh.score_confusions, q, K, torch.zeros((Q, 0), dtype=torch.int64))
    _raises("positives must be int64 [Q, 1 <= n_pos <= 64]", sh.score_confusions, q, K, torch.zeros((Q, 1), dtype=torch.int32))
    _raises("margin=nan must be finite or +inf", sh.score_confusions, q, K, pos, float("nan"))
    _raises("margin=-inf must be finite or +inf", sh.score_confusions, q, K, pos, float("-inf"))
    assert h.calls == [] and coll == []


def _check_family(sh, h, coll, n_rows, world):
    d, want = _inputs(n_rows), _expected(n_rows, world)
    q = torch.from_numpy(d["q"].copy())
    single = world == 1
    have_rows = sh.end > sh.start
    _check_errors(sh, h, coll, q)
    for name, (method, args, kw) in _calls(d).items():
        del h.calls[:], coll[:]
        targs, tkw = _tensors(method, args, kw)
        got = getattr(sh, method)(q, *targs, **tkw)
        _same(got, want[name], "%s on rank %d of %d" % (name, sh.rank, world))
        merged = method in ("score_topk_filtered", "score_topk_after", "score_topk_biased") and not single
        assert coll == ([] if single else ["all_gather_into", "all_reduce_"] if merged else ["all_gather_into"]), (name, coll)
        calls = [_local_call(method, args, kw, single)] if have_rows else []       # a rank without rows makes no local call
        if merged:
            calls.append(("merge_topk_strided_dev", Q, K, (), 2 * Q * K, world))
        assert h.calls == calls, (name, h.calls, calls)
    # no query: the padded (empty) result, no local call, no collective
    del h.calls[:], coll[:]
    q0 = torch.zeros((0, S), dtype=torch.float32)
    for method, first, rest in (("score_topk_filtered", K, ()), ("score_topk_after", K, ()), ("score_topk_biased", K, ()),
                                ("score_topk_grouped", K, ()), ("score_lse", SCALE, ()),
                                ("score_confusions", K, (torch.zeros((0, 1), dtype=torch.int64),))):
        got = getattr(sh, method)(q0, first, *rest)
        assert all(g.shape[0] == 0 for g in got) and (method == "score_lse" or got[0].shape == (0, K)), method
    assert h.calls == [] and coll == []


def _family_worker(rank, world, port, n_rows):
    sys.path.insert(0, ROOT)
    os.environ["SSE_NO_TORCH"] = "1"
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sse_amd
    from sse_amd import collectives
    coll = []
    for name in ("all_gather_into", "all_reduce_"):                               # sharded.py looks them up at every call
        def counted(*a, _fn=getattr(collectives, name), _name=name, **kw):
            coll.append(_name)
            return _fn(*a, **kw)
        setattr(collectives, name, counted)
    d = _inputs(n_rows)
    h = _CpuFamilyHandle(S)
    sh = sse_amd.ShardedIndex(h, rank, world, n_rows)
    sh.set_local_rows(torch.from_numpy(d["t"][sh.start:sh.end].copy()))
    assert len(h.calls) == (1 if sh.end > sh.start else 0)
    _check_setters(sh, h, d)
    _check_family(sh, h, coll, n_rows, world)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_rows", [(2, 5), (3, 2)], ids=["tie_across_two_ranks", "empty_third_rank"])
def test_sharded_family_equals_the_whole_index_on_every_rank(world, n_rows):
    from sse_amd.sharded import shard_bounds
    assert shard_bounds(n_rows, world) == ([(0, 3), (3, 5)] if world == 2 else [(0, 1), (1, 2), (2, 2)])
    want = _expected(n_rows, world)
    if world == 2:
        assert want["filtered_plain"][1][0, :2].tolist() == [2, 3] and want["filtered_plain"][0][0, 0] == want["filtered_plain"][0][0, 1]
    else:
        assert (want["filtered_plain"][2] == 2).all() and (want["filtered_plain"][1][:, 2:] == PAD).all()      # k above the rows
    mp.spawn(_family_worker, args=(world, free_port(), n_rows), nprocs=world, join=True)


def test_single_shard_makes_the_local_call_alone():
    """world == 1 without always_gather: no process group exists, so any collective would raise; the result is the local
    call's, and score_confusions hands the caller's margin to the device."""
    import sse_amd
    from sse_amd import collectives
    coll = []
    saved = collectives.all_gather_into, collectives.all_reduce_
    collectives.all_gather_into = collectives.all_reduce_ = lambda *a, **kw: coll.append("collective")
    try:
        d = _inputs(5)
        h = _CpuFamilyHandle(S)
        sh = sse_amd.ShardedIndex(h, 0, 1, 5)
        sh.set_local_rows(torch.from_numpy(d["t"].copy()))
        _check_setters(sh, h, d)
        _check_family(sh, h, coll, 5, 1)
    finally:
        collectives.all_gather_into, collectives.all_reduce_ = saved
