"""Cases shared by tests/test_gpu_score_lse.py (GPU) and tests/test_lse_cases_host.py (CPU): sse_score_lse, the softmax
log-partition over the tag-eligible rows of the index.  DESIGN K6m.

  lse[q] = log sum_{eligible r} exp(z_r),  z_r = float64(scale) * (score64(q, r) + float64(w[q]) * float64(bias[r]))

One list, CASES.  inputs(case) builds the index, the queries, the tags and masks, the bias and the weights from the case's
seed; reference(case) is the float64 restatement -- score64 = q.astype(f64) @ t.astype(f64).T in the index's stored
precision, the bias added, the masks applied, np.logaddexp.reduce over the eligible columns --; check(case, lse, count, bound)
is what every entry point's result must pass; model(case, defect) is a numpy model of the kernel's arithmetic (fp32 dots,
power-of-two reference, (split, wave, lane half) partials, fixed-order merge) that can carry one planted defect.

The bars.  d_q = scale * e_b bounds the effect of the fp32 dot products: e = eps32 |q| (1 + 2^-20) with eps32 =
float32(2 (S + 2) 5.97e-8 norm_max) (score_eps32 of the host layer), widened to e_b = (e + 2^-23 (|q| norm_max + e + |w| bmax) +
2^-149) (1 + 2^-20) under a bias (score_biased.hip).  The library forms norm_max from an fp32 sum of squares, which may sit
S 2^-24 (relative) either side of the float64 norm this file computes: d_hi / d_lo carry a factor (1 +- S 2^-22) for that and
for the float32 rounding of eps32.  check() asserts
  count exact;  lse == -inf exactly where count == 0;  no NaN;  |lse - reference| <= bound;
  d_lo <= bound <= d_hi + 2^-14   (the issue's budget for everything behind the dot product; the library claims 2^-16).
No GPU import here."""
import functools

import numpy as np

BASE = 5_000_000_000          # an id_base beyond int32
LOG2E = 1.4426950408889634
REST = 2.0 ** -14             # budget of the non-dot part of out_bound


class Case:
    def __init__(self, name, Q, N, S, scale, seed, kind="unit", tags=None, bias=None, upload="f32", id_base=0, qnorm=1.0,
                 nsplit=None, why=""):
        self.name, self.Q, self.N, self.S, self.scale, self.seed, self.kind = name, Q, N, S, float(scale), seed, kind
        self.tags, self.bias, self.upload, self.id_base, self.qnorm = tags, bias, upload, id_base, qnorm
        self.nsplit = nsplit          # what the launcher's rule gives for (Q, N): asserted by the GPU test through nsplit_of
        self.why = why

    def __repr__(self):
        return self.name


def bit(b):
    return np.uint64(1) << np.uint64(b)


def unit(a):
    return a / np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True)


def nsplit_of(Q, N):
    """choose_nsplit of the host layer for a chunk of Q <= 32 queries (one query block of one column tile)"""
    assert Q <= 32
    NT = (N + 31) // 32
    ns = 1
    while ns < 256 and ns < 512 and NT // (ns * 2) >= 16:
        ns *= 2
    if ns <= 8:
        ns = 1
        while ns < 8 and ns < 256 and NT // (ns * 2) >= 8:
            ns *= 2
    return ns


# ---- tag builders: (case, rng) -> dict(tags uint64 [N], any uint64 [Q] or None, none uint64 [Q] or None)

def _t_mixed(case, rng):
    """eight one-hot groups; query 0 asks for a group nobody has (empty set), query 1 is unrestricted (any_of == 0) with one
    group ruled out, query 2 asks for the one row of the tail tile, the rest ask for one group and rule out another"""
    tags = bit(0) << (rng.randint(0, 8, case.N).astype(np.uint64))
    tags[case.N - 1] = bit(20)
    any_ = bit(0) << (rng.randint(0, 8, case.Q).astype(np.uint64))
    none = bit(0) << (rng.randint(0, 8, case.Q).astype(np.uint64))
    none[none == any_] = 0
    any_[0], none[0] = bit(40), 0
    if case.Q > 1:
        any_[1], none[1] = 0, bit(3)
    if case.Q > 2:
        any_[2], none[2] = bit(20), 0
    return dict(tags=tags, any=any_, none=none)


def _t_none_only(case, rng):
    """any_of NULL: only the none_of rule"""
    tags = bit(0) << (rng.randint(0, 4, case.N).astype(np.uint64))
    return dict(tags=tags, any=None, none=bit(0) << (rng.randint(0, 4, case.Q).astype(np.uint64)))


def _t_blocks(case, rng):
    """sixteen contiguous blocks of rows, one tag each, every query asks for two of them: whole tiles can be skipped"""
    tags = bit(0) << ((np.arange(case.N) * 16 // case.N).astype(np.uint64))
    a = rng.randint(0, 16, case.Q)
    return dict(tags=tags, any=(bit(0) << a.astype(np.uint64)) | (bit(0) << ((a + 5) % 16).astype(np.uint64)), none=None)


# ---- bias builders: (case, rng) -> (bias float32 [N], w float32 [Q])

def _b_mixed(case, rng):
    return (0.2 * rng.standard_normal(case.N)).astype(np.float32), np.linspace(-1.0, 2.0, case.Q).astype(np.float32)


def _b_log_prior(case, rng):
    prior = rng.dirichlet(np.full(case.N, 0.5)) + 1e-12
    return (np.log(prior) / case.scale).astype(np.float32), np.ones(case.Q, np.float32)


CASES = [
    Case("n1", 3, 1, 8, 64, 1, why="one row: lse = its logit"),
    Case("n31", 3, 31, 8, 64, 2, why="tail mask: one short tile"),
    Case("n32", 3, 32, 8, 64, 3, why="a whole tile"),
    Case("n33", 3, 33, 8, 64, 4, why="one row in the tail tile"),
    Case("n95", 5, 95, 9, 64, 5, why="three tiles, S = 9: a partial second k-group"),
    Case("two_splits", 5, 600, 16, 64, 6, nsplit=2, why="19 tiles: the launcher takes 2 splits"),
    Case("folded_decode", 5, 16400, 16, 64, 7, nsplit=32, why="513 tiles, 5 queries: 32 splits, the decode of more than 8"),
    Case("s1", 4, 70, 1, 64, 8, why="S = 1"),
    Case("s7", 4, 70, 7, 64, 9, why="S = 7: KG = 1"),
    Case("s50", 4, 70, 50, 64, 10, why="S = 50: KG = 7, remainder 3"),
    Case("s256", 4, 200, 256, 64, 11, why="S = 256: KG = 32"),
    Case("s1024", 40, 70, 1024, 64, 12, why="S = 1024: one column tile per block, two query blocks"),
    Case("q1", 1, 300, 32, 64, 13, why="half-empty column tile"),
    Case("q33", 33, 300, 32, 64, 14, why="a second column tile with one query"),
    Case("q129", 129, 300, 32, 64, 15, why="a second query block"),
    # (S = 32 as the other Q cases: at S = 7 the margin of eps32, 2 (S + 2) against the S + 1 roundings of a dot product, is at
    # its thinnest, and the largest of 4097 x 95 fp32 dot errors reaches 0.12 d_q, past the tenth test_lse_cases_host.py asks for)
    Case("q4097", 4097, 95, 32, 64, 16, why="a second chunk of one query"),
    Case("scale1", 5, 500, 32, 1, 17, why="scale 1: a flat softmax, lse near log N"),
    Case("scale256", 5, 500, 32, 256, 18, why="scale 256 on unit vectors: logits to +-256, exp overflows fp32 without a reference"),
    Case("ascending", 4, 640, 16, 256, 19, kind="ascending", why="rows sorted by ascending score of query 0: the reference rises on every tile"),
    Case("descending", 4, 640, 16, 256, 19, kind="descending", why="the same rows in descending order"),
    Case("short_query", 4, 300, 64, 64, 20, qnorm=0.25, why="|q| = 1/4: the bound carries the query norm"),
    Case("tags_mixed", 9, 289, 24, 64, 21, tags=_t_mixed, why="an empty set, any_of == 0, one eligible row in the tail tile"),
    Case("tags_none_only", 5, 200, 24, 64, 22, tags=_t_none_only, why="any_of NULL"),
    Case("tags_skip", 5, 4000, 16, 64, 23, tags=_t_blocks, why="contiguous tag blocks: tiles are skipped"),
    Case("bias_mixed", 9, 500, 32, 64, 24, bias=_b_mixed, why="weights from -1 to 2, zero included"),
    Case("bias_log_prior", 5, 500, 32, 64, 25, bias=_b_log_prior, why="bias = log(prior) / scale: the class log-prior"),
    Case("bias_and_tags", 9, 289, 24, 64, 26, tags=_t_mixed, bias=_b_mixed, why="masks and bias together"),
    Case("shard_f64", 9, 1200, 40, 64, 27, tags=_t_mixed, bias=_b_mixed, upload="f64", id_base=BASE, why="float64 upload, id_base != 0"),
    Case("shard_dev", 9, 1200, 40, 64, 27, tags=_t_mixed, bias=_b_mixed, upload="dev", id_base=BASE, why="device-adopted index, id_base != 0"),
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def inputs(case):
    """dict(q float32 [Q,S], t [N,S] in the upload's precision, tags, any, none, bias, w: arrays or None), read-only"""
    rng = np.random.RandomState(case.seed)
    t = unit(rng.standard_normal((case.N, case.S)))
    q = unit(rng.standard_normal((case.Q, case.S))) * case.qnorm
    if case.kind in ("ascending", "descending"):
        o = np.argsort(t @ q[0], kind="stable")
        t = t[o if case.kind == "ascending" else o[::-1]]
    t = np.ascontiguousarray(t, np.float64 if case.upload == "f64" else np.float32)
    q = np.ascontiguousarray(q, np.float32)
    d = dict(q=q, t=t, tags=None, any=None, none=None, bias=None, w=None)
    if case.tags is not None:
        d.update(case.tags(case, rng))
    if case.bias is not None:
        d["bias"], d["w"] = case.bias(case, rng)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def eligible(case):
    I = inputs(case)
    e = np.ones((case.Q, case.N), bool)
    if I["tags"] is not None:
        tg = I["tags"][None, :]
        if I["any"] is not None:
            e &= (I["any"][:, None] == 0) | ((tg & I["any"][:, None]) != 0)
        if I["none"] is not None:
            e &= (tg & I["none"][:, None]) == 0
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def logits(case):
    """z float64 [Q,N] of every row, eligible or not"""
    I = inputs(case)
    s = I["q"].astype(np.float64) @ np.asarray(I["t"], np.float64).T
    if I["w"] is not None:
        s = s + I["w"].astype(np.float64)[:, None] * I["bias"].astype(np.float64)[None, :]
    z = case.scale * s
    z.setflags(write=False)
    return z


def lse_of(z, e):
    """(lse float64 [Q], count int64 [Q]) of logits z over the columns e"""
    with np.errstate(divide="ignore"):
        return np.logaddexp.reduce(np.where(e, z, -np.inf), axis=1), e.sum(axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(case):
    out = lse_of(logits(case), eligible(case))
    for a in out:
        a.setflags(write=False)
    return out


def dot_bounds(case, norm_factor=1.0):
    """d_q float64 [Q] = scale * e_b, with norm_max scaled by norm_factor"""
    I = inputs(case)
    norm_max = float(np.linalg.norm(np.asarray(I["t"], np.float64).astype(np.float32).astype(np.float64), axis=1).max()) * norm_factor
    eps32 = 2.0 * (case.S + 2) * 5.97e-8 * norm_max
    qn = np.linalg.norm(I["q"].astype(np.float64), axis=1)
    e = eps32 * qn * (1.0 + 2.0 ** -20)
    if I["w"] is not None:
        B = np.abs(I["w"].astype(np.float64)) * float(np.abs(I["bias"]).max())
        e = (e + 2.0 ** -23 * (qn * norm_max + e + B) + 2.0 ** -149) * (1.0 + 2.0 ** -20)
    return case.scale * e


def check(case, lse, count, bound, ref=None):
    """The whole claim on one result.  Returns (worst |lse - reference| / bound, worst bound - d_q)."""
    wl, wc = reference(case) if ref is None else ref
    lse, count, bound = np.asarray(lse), np.asarray(count), np.asarray(bound)
    assert lse.shape == (case.Q,) and count.shape == (case.Q,) and bound.shape == (case.Q,), (lse.shape, count.shape, bound.shape)
    assert lse.dtype == np.float64 and count.dtype == np.int64 and bound.dtype == np.float64
    assert np.array_equal(count, wc), "%s: counts %s, want %s" % (case.name, count.tolist()[:12], wc.tolist()[:12])
    assert not np.isnan(lse).any(), "%s: a NaN lse" % case.name
    empty = wc == 0
    assert np.array_equal(lse == -np.inf, empty), "%s: lse is -inf at %s, the empty sets are %s" % (
        case.name, np.flatnonzero(lse == -np.inf).tolist()[:8], np.flatnonzero(empty).tolist()[:8])
    assert np.isfinite(bound).all() and (bound > 0).all()
    f = case.S * 2.0 ** -22
    d_lo, d_hi = dot_bounds(case, 1.0 - f) * (1.0 - 2.0 ** -22), dot_bounds(case, 1.0 + f) * (1.0 + 2.0 ** -22)
    assert (bound >= d_lo).all(), "%s: bound %.3e below the dot part %.3e" % (case.name, bound.min(), d_lo[np.argmin(bound - d_lo)])
    over = bound - d_hi
    assert (over <= REST).all(), "%s: bound exceeds d_q by %.3e > 2^-14" % (case.name, over.max())
    live = ~empty
    err = np.abs(lse[live] - wl[live])
    assert (err <= bound[live]).all(), "%s: |lse - reference| = %.3e > bound %.3e at query %d" % (
        case.name, err.max(), bound[live][np.argmax(err - bound[live])], np.flatnonzero(live)[np.argmax(err - bound[live])])
    return (float((err / bound[live]).max()) if live.any() else 0.0), float(over.max())


# ---- the kernel's arithmetic in numpy

DEFECTS = ("pad_counted", "none_ignored", "any0_nothing", "bias_dropped", "bias_outside_scale", "split_dropped", "merge_adds_logs",
           "no_reference", "empty_nan", "bound_without_qnorm")
M_EMPTY = -(1 << 24)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def model(case, defect=None, nsplit=2):
    """(lse, count, bound) as the kernels form them: fp32 dots (numpy's order), y = fma(w, bias, x), the integer reference
    m = ceil(max y c_hi) per (split, wave, lane half) partial and tile, t = fma(y, c_lo, fma(y, c_hi, -m)), 2^t in fp32, a
    sequential fp32 sum over a tile's 16 rows, float64 across tiles with exact ldexp rescaling, partials merged in index order.
    Rows are padded to whole tiles with zero rows, zero tags and zero bias, as the index is.  defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    I = inputs(case)
    Q, N = case.Q, case.N
    NT = (N + 31) // 32
    NP = NT * 32
    t32 = np.zeros((NP, case.S), np.float32)
    t32[:N] = np.asarray(I["t"]).astype(np.float32)
    y = I["q"] @ t32.T                                                  # float32 [Q, NP]
    biased = I["w"] is not None and defect != "bias_dropped"
    bias = np.zeros(NP, np.float32)
    if biased:
        bias[:N] = I["bias"]
        if defect != "bias_outside_scale":
            y = _f32(y.astype(np.float64) + I["w"].astype(np.float64)[:, None] * bias.astype(np.float64)[None, :])
    e = np.zeros((Q, NP), bool)
    if I["tags"] is not None:
        tg = np.zeros(NP, np.uint64)
        tg[:N] = I["tags"]
        e[:] = True
        if I["any"] is not None:
            an = I["any"][:, None]
            e &= ((tg[None, :] & an) != 0) if defect == "any0_nothing" else ((an == 0) | ((tg[None, :] & an) != 0))
        if I["none"] is not None and defect != "none_ignored":
            e &= (tg[None, :] & I["none"][:, None]) == 0
    else:
        e[:] = True
    if defect != "pad_counted":
        e[:, N:] = False
    c = case.scale * LOG2E
    c_hi = np.float32(c)
    c_lo = np.float32(c - float(c_hi))
    tps = (NT + nsplit - 1) // nsplit
    parts = []                                                          # (m int64 [Q], sum float64 [Q], count int64 [Q]) in slot order
    rows_of_half = [np.array([(r & 3) + 8 * (r >> 2) + 4 * h for r in range(16)]) for h in (0, 1)]
    for split in range(nsplit):
        t0, t1 = split * tps, min(NT, split * tps + tps)
        for w in range(8):
            for h in (0, 1):
                m = np.full(Q, M_EMPTY, np.int64)
                s = np.zeros(Q)
                cnt = np.zeros(Q, np.int64)
                for tile in range(t0 + w, t1, 8):
                    cols = tile * 32 + rows_of_half[h]
                    yy, ee = y[:, cols], e[:, cols]
                    if defect == "no_reference":
                        with np.errstate(over="ignore"):
                            term = np.exp(_f32(np.float32(case.scale) * yy)).astype(np.float32)
                        ts = np.zeros(Q, np.float32)
                        for r in range(16):
                            ts = ts + np.where(ee[:, r], term[:, r], np.float32(0))
                        s = s + ts.astype(np.float64)
                        m = np.where(ee.any(1), 0, m)
                        cnt += ee.sum(1)
                        continue
                    x = np.where(ee, yy * c_hi, -np.inf).astype(np.float32)
                    xmax = x.max(1)
                    mt = np.where(xmax > -np.inf, np.ceil(np.where(xmax > -np.inf, xmax, 0)), M_EMPTY).astype(np.int64)
                    mn = np.maximum(m, mt)
                    tt = _f32(yy.astype(np.float64) * float(c_hi) - mn[:, None].astype(np.float64))
                    tt = _f32(yy.astype(np.float64) * float(c_lo) + tt.astype(np.float64))
                    with np.errstate(over="ignore"):
                        term = _f32(np.exp2(tt.astype(np.float64)))
                    ts = np.zeros(Q, np.float32)
                    for r in range(16):
                        ts = ts + np.where(ee[:, r], term[:, r], np.float32(0))
                    s = np.ldexp(s, np.maximum(m - mn, -4000).astype(np.int64)) + ts.astype(np.float64)
                    m = mn
                    cnt += ee.sum(1)
                parts.append((m, s, cnt))
    if defect == "split_dropped":
        parts = parts[:16 * (nsplit - 1)]
    m = np.full(Q, M_EMPTY, np.int64)
    s = np.zeros(Q)
    cnt = np.zeros(Q, np.int64)
    logsum = np.zeros(Q)
    for pm, ps, pc in parts:
        mn = np.maximum(m, pm)
        s = np.ldexp(s, np.maximum(m - mn, -4000)) + np.ldexp(ps, np.maximum(pm - mn, -4000))
        m = mn
        cnt += pc
        with np.errstate(divide="ignore"):
            logsum += np.where(pc > 0, np.log(np.where(pc > 0, ps, 1.0)) + pm * np.log(2.0), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.log(s) + m * np.log(2.0)
        if defect == "no_reference":
            lse = np.log(s)
        if defect == "merge_adds_logs":
            lse = logsum
        if defect == "empty_nan":
            lse = np.where(cnt > 0, lse, np.nan)
        else:
            lse = np.where(cnt > 0, lse, -np.inf)
    if defect == "bias_outside_scale" and biased:
        # exp(scale * score + w * bias): the logit scale misses the bias.  Re-run the reduction on those logits in float64: the
        # defect is in the definition, not in the arithmetic
        z = case.scale * y[:, :N].astype(np.float64) + I["w"].astype(np.float64)[:, None] * I["bias"].astype(np.float64)[None, :]
        lse = lse_of(z, e[:, :N])[0]
    qn = np.linalg.norm(I["q"].astype(np.float64), axis=1)
    d = dot_bounds(case)
    if defect == "bound_without_qnorm":
        d = d / np.where(qn > 0, qn, 1.0)
    return lse, cnt, d * (1.0 + 2.0 ** -20) + 2.0 ** -16
