"""The class softmax loss (sse_class_loss_dev; the train step under option train_class_loss = 1): its definition restated in
numpy, the cases of the head and of the whole step, and the checks.  Shared by tests/test_class_loss_cases_host.py (CPU),
tests/test_gpu_class_loss.py (the head alone), tests/test_gpu_class_train.py (the whole step) and
tests/test_gpu_class_two_ranks.py.

Definition (include/sse_hip.h):  ns_i = s_i / sqrt(max(|s_i|^2, 1e-12)), nt_j likewise over ALL N rows of the table;
L_ij = c ns_i . nt_j;  column j is excluded for row i when j != y_i and some row r has ks_r == ks_i, z_r != 0, y_r == j;
lse_i = log sum_admitted exp(L_ij);  row_loss_i = z_i (lse_i - L_{i,y_i});  row_acc_i = [z_i != 0 and no admitted j != y_i has
L_ij > L_{i,y_i}];  G_ij = z_i c inv_rows (p_ij - [j == y_i]);  d ns_i = sum_j G_ij nt_j, d nt_j = sum_i G_ij ns_i for every j,
then the l2_normalize backward.

Bars, as tests/inbatch_cases.py sets them.  Gradients are held to util.GRAD_BARS_EXACT unless the float32 restatement of this
very definition (head(.., dtype=float32)) is not 10x inside it; such a case carries bars of its own = 10 x the restatement's
error, rounded up, with the measured value beside it (tests/test_class_loss_cases_host.py asserts the 10x margin for every
case).  row_loss_i is a difference of two logit-sized numbers: LOSS_REL_EXACT |want| + z_i * 2 c (S + 2) 2^-24.  row_acc is
compared on every row; that the float64 gap |L_{i,y_i} - best other admitted logit| exceeds 4 c (S + 2) 2^-24 on every active
row is a precondition of the inputs (head_case_seeded), not a tolerance."""
import numpy as np

from oracle import sse_oracle as O
from tests.inbatch_cases import _row_keys, accuracy_gap_bound
from tests.util import GRAD_BARS_EXACT, LOSS_REL_EXACT, check_grads, check_tail, model_params, oracle_float64, oracle_params, random_ids

TABLE = "target_embedding/tgt_seq_embedding"
DEFECTS = ("tail-columns-admitted", "other-verified-unmasked", "own-target-masked", "label0-row-excludes", "label0-row-has-loss",
           "no-delta", "mean-over-active", "no-max-subtraction", "clamp-ignored", "table-gradient-on-batch-rows-only",
           "exclusion-by-subtraction")


def excluded(z, ks, y, N, defect=None):
    """[B][N] bool: column j excluded for row i."""
    z, y = np.asarray(z), np.asarray(y)
    B = len(z)
    ks = np.arange(B) if ks is None else np.asarray(ks)
    _, grp = np.unique(ks, return_inverse=True)
    grp = grp.ravel()
    marks = np.zeros((int(grp.max()) + 1, N), bool)
    ver = np.ones(B, bool) if defect == "label0-row-excludes" else z != 0
    marks[grp[ver], y[ver]] = True
    ex = marks[grp].copy()
    if defect != "own-target-masked":
        ex[np.arange(B), y] = False
    if defect == "other-verified-unmasked":
        ex[:] = False
    return ex


def head(s, table, y, z, ks=None, scale=64.0, inv_rows=None, dtype=np.float64, defect=None):
    """The head in `dtype` arithmetic.  Returns dict(row_loss, row_acc, d_src, d_table, logits, adm, loss, acc).  defect: one
    of DEFECTS (a planted error, for the CPU self-test)."""
    dt = dtype
    s, t, z = np.asarray(s, dt), np.asarray(table, dt), np.asarray(z, dt)
    y = np.asarray(y).astype(np.int64)
    B, S = s.shape
    N = t.shape[0]
    assert ((y >= 0) & (y < N)).all()
    c = dt(scale)
    inv = dt(1.0 / B if inv_rows is None else inv_rows)
    if defect == "mean-over-active":
        inv = dt(1.0 / max(1, int((z != 0).sum())))
    eps = dt(1e-12)
    pad = (-N) % 32 if defect == "tail-columns-admitted" else 0    # zero padding of the last column tile entering as logits of 0
    ss, tt = np.sum(s * s, axis=1, dtype=dt), np.sum(t * t, axis=1, dtype=dt)
    rs, rt = dt(1) / np.sqrt(np.maximum(ss, eps)), dt(1) / np.sqrt(np.maximum(tt, eps))
    ns, nt = (s * rs[:, None]).astype(dt), (t * rt[:, None]).astype(dt)
    L = (c * (ns @ nt.T)).astype(dt)
    ex = excluded(z, ks, y, N, defect)
    adm = ~ex
    own = np.zeros((B, N), bool)
    own[np.arange(B), y] = True
    neg = dt(-np.inf)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if defect == "exclusion-by-subtraction":    # the whole row summed, the excluded terms taken off afterwards
            mx = L.max(axis=1)
            e_all = np.exp(L - mx[:, None]).astype(dt)
            tot = e_all.sum(axis=1, dtype=dt) - np.where(ex, e_all, dt(0)).sum(axis=1, dtype=dt)
            e = np.where(adm, e_all, dt(0)).astype(dt)
        else:
            mx = np.zeros(B, dt) if defect == "no-max-subtraction" else np.where(adm, L, neg).max(axis=1)
            e = np.where(adm, np.exp(L - mx[:, None]), dt(0)).astype(dt)
            tot = e.sum(axis=1, dtype=dt) + dt(pad) * np.exp(-mx)
        lse = mx + np.log(tot)
        p = (e / tot[:, None]).astype(dt)
    d = L[np.arange(B), y]
    zl = np.ones_like(z) if defect == "label0-row-has-loss" else z
    row_loss = (zl * (lse - d)).astype(dt)
    others = np.where(adm & ~own, L, neg).max(axis=1) if N > 1 else np.full(B, neg)
    row_acc = ((z != 0) & ~(others > d)).astype(dt)
    delta = dt(0) if defect == "no-delta" else own.astype(dt)
    G = (zl[:, None] * c * inv * (p - delta)).astype(dt)
    dns, dnt = (G @ nt).astype(dt), (G.T @ ns).astype(dt)
    if defect == "table-gradient-on-batch-rows-only":
        dnt[~np.isin(np.arange(N), y)] = 0

    def l2_bwd(n, dn, r, sq):
        full = r[:, None] * (dn - n * np.sum(n * dn, axis=1, keepdims=True, dtype=dt))
        if defect == "clamp-ignored":
            return full.astype(dt)
        return np.where((sq < eps)[:, None], r[:, None] * dn, full).astype(dt)
    return dict(row_loss=row_loss, row_acc=row_acc, d_src=l2_bwd(ns, dns, rs, ss), d_table=l2_bwd(nt, dnt, rt, tt), logits=L, adm=adm,
                loss=dt(inv * row_loss.sum(dtype=dt)), acc=dt(inv * row_acc.sum(dtype=dt)))


def min_accuracy_gap(r, y, z):
    """Smallest float64 |L_{i,y_i} - best other admitted logit| over the active rows of a float64 head result (inf when no
    active row has another admitted column)."""
    L, adm = r["logits"], r["adm"]
    B, N = L.shape
    own = np.zeros((B, N), bool)
    own[np.arange(B), y] = True
    others = np.where(adm & ~own, L, -np.inf).max(axis=1) if N > 1 else np.full(B, -np.inf)
    gap = np.abs(L[np.arange(B), y] - others)[np.asarray(z) != 0]
    return float(gap.min()) if gap.size else np.inf


# ---- head cases ---------------------------------------------------------------------------------------------------------
def _hc(cid, B, N, S, kind="plain", scale=64.0, rows_factor=1, seed=0, bars=None, f32_err=None):
    return dict(id=cid, B=B, N=N, S=S, kind=kind, scale=scale, rows_factor=rows_factor, seed=seed, bars=bars or GRAD_BARS_EXACT,
                f32_err=f32_err)


# bars = (norm-relative, max-element-relative) over d_src and d_table.  A case whose float32 restatement is not 10x inside
# GRAD_BARS_EXACT carries 10 x its restatement's error, rounded up; f32_err = that measured error (CPU, numpy float32).
HEAD_CASES = [
    _hc("b1-n1-s3", 1, 1, 3),
    _hc("b2-n5-s64", 2, 5, 64),
    _hc("b31-n33-s130", 31, 33, 130, kind="keys"),
    _hc("b33-n31-s64", 33, 31, 64, kind="keys"),
    _hc("b33-n32-s64-last-class", 33, 32, 64, kind="last"),
    _hc("b65-n571-s64", 65, 571, 64, kind="keys"),                       # 17 column tiles + 27 columns; the rows pass splits its walk
    _hc("b100-n300-s130-rows-global", 100, 300, 130, kind="keys", rows_factor=2),
    _hc("b300-n65-s64", 300, 65, 64, kind="keys"),                       # d(table): a wave walks two row tiles, the walk split in two
    _hc("b128-n5000-s64-split-classes", 128, 5000, 64, kind="keys"),     # rows pass and d(src): the class walk in 20 chunks
    _hc("b600-n40-s64-split-rows", 600, 40, 64, kind="keys"),            # d(table): the row walk in 3 chunks
    # S = 1: ns, nt = +-1, so the l2_normalize backward cancels exactly and both gradients are zero up to rounding -- held to
    # 16 * 2^-24 * max(1 / norm) * c * inv_rows as in-batch case b33-s1; scale 1 keeps the softmax off saturation
    _hc("b33-n33-s1", 33, 33, 1, kind="s1", scale=1.0),
    _hc("labels-all-0", 33, 31, 64, kind="labels0"),
    _hc("fractional-labels", 31, 33, 64, kind="fractional"),
    _hc("one-class", 33, 40, 64, kind="one-class"),
    _hc("zero-rows", 33, 40, 64, kind="zeros"),
    _hc("s-equals-t-scale256", 33, 33, 64, kind="equal", scale=256.0, bars=(1.1e-4, 1.3e-4), f32_err=(1.04e-5, 1.29e-5)),
    _hc("three-class-source", 33, 70, 64, kind="three"),
    _hc("forty-class-source", 72, 300, 64, kind="forty"),
    _hc("null-keys", 65, 100, 64, kind="null", bars=(1.1e-5, 2e-5), f32_err=(1.08e-6, 1.36e-6)),
    _hc("all-logits-negative", 33, 33, 64, kind="negative", bars=(1.8e-5, 5.2e-5), f32_err=(1.79e-6, 5.14e-6)),
]
HEAD_CASES_BY_ID = {c["id"]: c for c in HEAD_CASES}


def _own_cosine(N, S):
    """The cosine at which a row's own class is the best column of about half the rows: the typical maximum of N random
    cosines in S dimensions."""
    return float(min(0.9, max(0.05, np.sqrt(2.0 * np.log(max(N, 2)) / max(S, 2)))))


def head_inputs(c, seed=None):
    """dict(s, t, y, z, ks, scale, inv_rows) of a head case (float32 inputs, int32 target rows, int64 keys or None)."""
    B, N, S, kind = c["B"], c["N"], c["S"], c["kind"]
    rng = np.random.RandomState(2000 + (c["seed"] if seed is None else seed))
    cos = _own_cosine(N, S)
    corr = cos / np.sqrt(1.0 - cos * cos)
    t = rng.normal(size=(N, S)).astype(np.float32)
    y = rng.randint(0, N, size=B).astype(np.int32)
    s = (corr * t[y] + rng.normal(size=(B, S))).astype(np.float32)
    z = (rng.uniform(size=B) < 0.6).astype(np.float32)
    z[0] = 1.0
    ks = np.arange(B, dtype=np.int64) * 7 + 3                           # distinct, not the row numbers
    if kind == "keys" and B > 4:                                        # a few sources twice, anywhere in the batch, with another class
        for _ in range(max(2, B // 8)):
            i, j = rng.randint(0, B, size=2)
            ks[j] = ks[i]
            s[j] = s[i]
    elif kind == "last":
        y[0] = N - 1
        y[5] = 0
        z[5] = 1.0
    elif kind == "s1":           # S = 1: every logit is +-c; the active rows name the one class on their side, every other class opposes
        s = (np.abs(s) + 0.5).astype(np.float32)
        t = (-np.abs(t) - 0.5).astype(np.float32)
        t[4] = 1.25
        y[z != 0] = 4
    elif kind == "labels0":
        z[:] = 0.0
    elif kind == "fractional":
        z = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 1.5], np.float32), size=B).astype(np.float32)
        z[0] = 0.5
    elif kind == "one-class":
        y[:] = 7
        z[:] = 1.0
        s = (corr * t[y] + rng.normal(size=(B, S))).astype(np.float32)
    elif kind == "zeros":        # exact zeros: a source row with label 0 (an active all-zero row would tie every logit at 0), a class an
        z[3] = 0.0               # active row names, a class nobody names; and rows below the clamp on both sides, active
        s[3] = 0.0
        y[6], z[6] = 11, 1.0
        t[11] = 0.0
        y[y == 12] = 13
        t[12] = 0.0
        z[8] = z[9] = 1.0
        s[8] = (s[8] * 1e-8).astype(np.float32)
        y[9] = 20
        t[20] = (t[20] * 1e-8).astype(np.float32)
    elif kind == "equal":        # L_{i,y_i} = c exactly; odd classes lie close to their even neighbour, so a row's softmax has a second
        t[1::2] = (t[0:N - 1:2] + 0.02 * t[1::2]).astype(np.float32)    # column within a fraction of a logit of c
        y = np.arange(B, dtype=np.int32) % N
        s = t[y].copy()
        z[:] = 1.0
    elif kind == "three":        # rows 0 .. 3 are one source: verified classes 5, 37, 66 and a label-0 row naming class 40.  The source
        t[40] = (t[5] + 1.0 * rng.normal(size=S)).astype(np.float32)    # lies on class 5: for rows 1 and 2 the excluded column 5 is by
        src = (t[5] + 0.3 * rng.normal(size=S)).astype(np.float32)      # far the largest term of the row, class 40 the next
        s[0:4] = src
        ks[0:4] = ks[0]
        y[0:4] = (5, 37, 66, 40)
        z[0:4] = (1, 1, 1, 0)
    elif kind == "forty":        # rows 0 .. 39 are one source naming classes 3, 10, .., 276 (nine column tiles), beside single-label sources
        s[0:40] = s[0]
        ks[0:40] = ks[0]
        y[0:40] = 3 + 7 * np.arange(40)
        z[0:40] = 1.0
    elif kind == "null":
        ks = None
    elif kind == "negative":     # every logit near -0.9 c: a zero logit let in by mistake (the padding of the last tile) would own the softmax
        u = rng.normal(size=(1, S))
        s = (u + 0.3 * rng.normal(size=(B, S))).astype(np.float32)
        t = (-u + 0.3 * rng.normal(size=(N, S))).astype(np.float32)
    return dict(s=s, t=t, y=y, z=z, ks=ks, scale=c["scale"], inv_rows=1.0 / (c["rows_factor"] * B))


def head_want(x):
    w = head(x["s"], x["t"], x["y"], x["z"], x["ks"], x["scale"], x["inv_rows"])
    w["z"] = x["z"]
    w["x"] = x
    return w


_SEEDED = {}


def head_case_seeded(c):
    """(inputs, float64 head) of a case at the first seed (from the case's own upwards) that meets the accuracy precondition on
    every active row.  Computed once per case and shared: callers must leave both unchanged."""
    if c["id"] not in _SEEDED:
        for k in range(64):
            x = head_inputs(c, c["seed"] + k)
            w = head_want(x)
            if min_accuracy_gap(w, x["y"], x["z"]) > accuracy_gap_bound(x["scale"], c["S"]):
                _SEEDED[c["id"]] = (x, w)
                break
        else:
            raise AssertionError("no seed meets the accuracy precondition for %s" % c["id"])
    return _SEEDED[c["id"]]


def head_errors(got, want):
    """(norm-relative, max-element-relative) error over d_src and d_table together."""
    g = np.concatenate([np.asarray(got["d_src"], np.float64).ravel(), np.asarray(got["d_table"], np.float64).ravel()])
    w = np.concatenate([want["d_src"].ravel(), want["d_table"].ravel()])
    d = np.abs(g - w)
    if not np.isfinite(g).all():
        return np.inf, np.inf
    if not w.any():
        return (0.0, 0.0) if not d.any() else (np.inf, np.inf)
    return float(np.linalg.norm(g - w) / np.linalg.norm(w)), float(d.max() / np.abs(w).max())


def check_head(got, want, c, bars=None, what=""):
    """got: dict(row_loss, row_acc[, d_src, d_table]) against the float64 head `want`; every row and element compared."""
    bars = bars or c["bars"]
    x_scale, S = c["scale"], c["S"]
    z = np.asarray(want["z"], np.float64)
    rl = np.asarray(got["row_loss"], np.float64)
    tol = LOSS_REL_EXACT * np.abs(want["row_loss"]) + np.abs(z) * 2 * x_scale * (S + 2) * 2.0 ** -24
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(rl - want["row_loss"]) <= tol)
    assert not bad.any(), "%s%s row_loss: rows %s got %s want %s" % (
        what, c["id"], np.nonzero(bad)[0][:5], rl[bad][:5], want["row_loss"][bad][:5])
    assert np.array_equal(np.asarray(got["row_acc"], np.float64), want["row_acc"]), "%s%s row_acc differs at rows %s" % (
        what, c["id"], np.nonzero(np.asarray(got["row_acc"]) != want["row_acc"])[0][:8])
    if "d_src" not in got:
        return None
    for k in ("d_src", "d_table"):
        assert np.isfinite(np.asarray(got[k])).all(), "%s%s %s holds a non-finite element" % (what, c["id"], k)
        zero = ~want[k].any(axis=1) & (S > 1)     # rows whose gradient is exactly zero stay exactly zero
        assert not np.asarray(got[k])[zero].any(), "%s%s %s: a row that must be zero is not" % (what, c["id"], k)
    if S == 1:                                  # exact cancellation: zero up to rounding (see the b33-n33-s1 case)
        x = want["x"]
        sq = min(float((x["s"].astype(np.float64) ** 2).sum(1).min()), float((x["t"].astype(np.float64) ** 2).sum(1).min()))
        bound = 16 * 2.0 ** -24 / np.sqrt(max(sq, 1e-12)) * x_scale * x["inv_rows"] * float(np.abs(z).max())
        worst = max(float(np.abs(np.asarray(got[k], np.float64)).max()) for k in ("d_src", "d_table"))
        assert worst <= bound, "%s%s: |gradient| %.3g above the rounding bound %.3g at S = 1" % (what, c["id"], worst, bound)
        return 0.0, 0.0
    rel, elem = head_errors(got, want)
    assert rel <= bars[0] and elem <= bars[1], "%s%s gradients: ||d||/||g|| %.3g (bar %.1e), max|d|/max|g| %.3g (bar %.1e)" % (
        what, c["id"], rel, bars[0], elem, bars[1])
    return rel, elem


# ---- the whole step ---------------------------------------------------------------------------------------------------
def _step_gradients(p, cfg, src, tgt, labels, inv_rows, scale):
    """The oracle's gradients of the two table modes with the class head in place of the pair loss, from the oracle's own
    forward and backward pieces, in the oracle's current precision (F32).  The table's gradient is dense."""
    F = O.F32
    mode = cfg["network_mode"]
    emb = p["word_embedding"]
    E = emb.shape[1]
    labels = np.asarray(labels, F)
    ks = _row_keys(src)
    table = p[TABLE]
    rows = O.check_ids(np.asarray(tgt).reshape(-1), table.shape[0])
    ids = O.check_ids(src, emb.shape[0])
    if mode == "source-encoder-only":
        scope = O.lstm_scope(mode, "src")
        K, b = p[scope + "/rnn/basic_lstm_cell/kernel"], p[scope + "/rnn/basic_lstm_cell/bias"]
        h, tape = O.lstm_forward(emb, K, b, ids, keep_tape=True)
        M = p[O.proj_name(mode, "src")]
        r = head((h @ M).astype(F), table, rows, labels, ks, scale, inv_rows, dtype=F)
        dK, db, dX = O._lstm_backward(K, tape, (r["d_src"] @ M.T).astype(F), E)
        grads = {O.proj_name(mode, "src"): (h.T @ r["d_src"]).astype(F), scope + "/rnn/basic_lstm_cell/kernel": dK,
                 scope + "/rnn/basic_lstm_cell/bias": db, TABLE: r["d_table"].astype(F),
                 "word_embedding": (ids.reshape(-1), dX.reshape(-1, E).astype(F))}
        return r, grads
    assert mode == "source_only_cnn"
    B, T = ids.shape
    pool, tape = O.cnn_forward(p, ids, keep_tape=True)
    M = p["source_only_cnn/src_M"]
    r = head((pool @ M).astype(F), table, rows, labels, ks, scale, inv_rows, dtype=F)
    d_s = r["d_src"]
    grads = {"source_only_cnn/src_M": (pool.T @ d_s).astype(F), TABLE: r["d_table"].astype(F)}
    dpool = (d_s @ M.T).astype(F)
    dX = np.zeros((B, T, E), F)
    off = 0
    for (fs, nf), (win, hconv) in zip(zip(O.CNN_FILTER_SIZES, O.CNN_NUM_FILTERS), tape):
        W = p["source_only_cnn/conv-maxpool-%d/W" % fs]
        pstar = hconv.argmax(axis=1)
        g = dpool[:, off:off + nf] * (np.take_along_axis(hconv, pstar[:, None, :], 1)[:, 0, :] > 0)
        sel = win[np.arange(B)[:, None], pstar]
        grads["source_only_cnn/conv-maxpool-%d/W" % fs] = np.einsum("bf,bfk->kf", g, sel).astype(F).reshape(W.shape)
        grads["source_only_cnn/conv-maxpool-%d/b" % fs] = g.sum(axis=0).astype(F)
        dwin = np.einsum("bf,kf->bfk", g, W.reshape(-1, nf)).reshape(B, nf, fs, E)
        for j in range(fs):
            np.add.at(dX, (np.arange(B)[:, None], pstar + j), dwin[:, :, j, :])
        off += nf
    grads["word_embedding"] = (ids.reshape(-1), dX.reshape(-1, E).astype(F))
    return r, grads


def step_reference(params, cfg, src, tgt, labels, rows_global=None, scale=64.0, float64=True):
    """What sse_train_grads leaves in the arena under train_class_loss = 1: ({variable: dense gradient}, tail[4]) with tail[0]
    the slice norm of word_embedding alone (the table's gradient is dense); also the head's own result."""
    import contextlib
    B = len(labels)
    inv_rows = 1.0 / float(rows_global or B)
    ctx = oracle_float64() if float64 else contextlib.nullcontext()
    with ctx:
        p = {k: np.asarray(v, O.F32) for k, v in params.items()}
        r, g = _step_gradients(p, cfg, src, tgt, labels, inv_rows, scale)
        dense, sq = {}, 0.0
        for name, v in g.items():
            if isinstance(v, tuple):
                sq += float(np.sum(np.square(v[1].astype(np.float64))))
                v = O.dense_embedding_grad(v, p[name].shape[0])
            dense[name] = np.asarray(v, np.float64).reshape(p[name].shape)
    return dense, np.array([sq, float(r["loss"]), float(r["acc"]), B], np.float64), r


def reference_apply(grads, tail, variables, slots, lr, max_norm=5.0):
    """clip_by_global_norm + Adagrad in float64 on GIVEN arena gradients of a class step: the global norm from tail[0]
    (word_embedding's slices) plus every other variable whole, the table among them.  Returns (variables, slots, clip scale)."""
    tot = float(tail[0]) + sum(float(np.sum(np.square(np.asarray(grads[n], np.float64)))) for n in grads if n != "word_embedding")
    gn = np.sqrt(tot)
    scale = max_norm * min(1.0 / gn, 1.0 / max_norm) if gn > 0 else 1.0
    lr = float(np.float32(lr))
    new_v, new_s = {}, {}
    for n, g in grads.items():
        g = np.asarray(g, np.float64) * scale
        new_s[n] = np.asarray(slots[n], np.float64) + g * g
        new_v[n] = np.asarray(variables[n], np.float64) - lr * g / np.sqrt(new_s[n])
    return new_v, new_s, scale


def _sc(cid, mode, V, E, H, S, T, B, N, opts=None, by_rows=False, seed=0, scale=64, path="fused", paired=False, bars=None, f32_err=None):
    return dict(id=cid, mode=mode, V=V, E=E, Hs=H, Ht=H, S=S, T=T, B=B, N=N, opts=dict(opts or {}), by_rows=by_rows, seed=seed,
                scale=scale, path=path, paired=paired, rows_factor=1, bars=bars or GRAD_BARS_EXACT, f32_err=f32_err)


# the smallest shapes that keep every kernel's tiles partial: 6 and 70 pair rows, 40 and 571 classes, T = 8
STEP_CASES = [
    _sc("seo-fused-b6-n40", "source-encoder-only", 80, 12, 16, 16, 8, 6, 40),
    _sc("seo-fused-b70-n40", "source-encoder-only", 80, 12, 16, 16, 8, 70, 40),
    _sc("seo-fused-b70-n571", "source-encoder-only", 80, 12, 16, 24, 8, 70, 571),
    _sc("seo-fused-rows-b70-n40", "source-encoder-only", 80, 12, 16, 16, 8, 70, 40, by_rows=True),
    _sc("seo-generic-b70-n40", "source-encoder-only", 80, 12, 16, 16, 8, 70, 40, opts=dict(train_generic=1), path="generic"),
    _sc("seo-generic-rows-b6-n571", "source-encoder-only", 80, 12, 16, 16, 8, 6, 571, opts=dict(train_generic=1), path="generic", by_rows=True),
    _sc("cnn-b6-n571", "source_only_cnn", 90, 16, 16, 32, 8, 6, 571, path="cnn", seed=1),
    _sc("cnn-rows-b70-n40", "source_only_cnn", 90, 16, 16, 32, 8, 70, 40, path="cnn", by_rows=True, seed=1),
]
STEP_CASES_BY_ID = {c["id"]: c for c in STEP_CASES}


def step_params(c):
    params = model_params(c["mode"], c["V"], c["E"], c["Hs"], c["Ht"], c["S"], c["T"], N=c["N"], lr=0.9)
    return params, oracle_params(params, seed=3 + c["seed"])


def step_batch(c, seed=None, B=None):
    """(src, tgt rows, labels): pair rows as the reference builds them -- every source twice, label 1 with its class and label 0
    with another -- and some sources a second time with another verified class."""
    rng = np.random.RandomState(70 + (c["seed"] if seed is None else seed))
    B, T, V, N = B or c["B"], c["T"], c["V"], c["N"]
    Vb = max(3, V * 4 // 5)
    src = np.repeat(random_ids(rng, (B + 1) // 2, T, Vb, 0.5), 2, axis=0)[:B]
    z = np.tile(np.array([1.0, 0.0], np.float32), (B + 1) // 2)[:B]
    tgt = rng.randint(0, N, size=B).astype(np.int32)
    for _ in range(max(1, B // 10)):              # a source again with a verified class, anywhere in the batch
        i, j = rng.randint(0, B, size=2)
        src[j] = src[i]
        z[j] = 1.0
    z[0] = 1.0
    return src, tgt, z


_STEP_SEEDED = {}


def step_case_seeded(c):
    """(params, oracle parameters, src, tgt, z, want, want_tail, head) at the first batch seed that meets the accuracy
    precondition on every active row (float64 logits of the float64 step).  Computed once and shared: leave it unchanged."""
    if c["id"] not in _STEP_SEEDED:
        params, p = step_params(c)
        for k in range(32):
            src, tgt, z = step_batch(c, c["seed"] + k)
            want, tail, r = step_reference(p, params, src, tgt, z, c["rows_factor"] * len(z), c["scale"])
            if min_accuracy_gap(r, tgt, z) > accuracy_gap_bound(c["scale"], c["S"]):
                _STEP_SEEDED[c["id"]] = (params, p, src, tgt, z, want, tail, r)
                break
        else:
            raise AssertionError("no seed meets the accuracy precondition for %s" % c["id"])
    return _STEP_SEEDED[c["id"]]


def check_step(got, tail, want, want_tail, c, what=""):
    errs = check_grads(got, want, c["bars"], what="%s%s: " % (what, c["id"]))
    check_tail(tail, want_tail, c["bars"], LOSS_REL_EXACT, what="%s%s: " % (what, c["id"]))
    return errs


# ---- the learning run -------------------------------------------------------------------------------------------------
# 60 steps on one batch of 32 pair rows over 40 classes, against a float64 reference run FREELY from the same initial weights
# (float64 gradients, float64 clip and Adagrad with the table dense).  A free-running comparison holds only where a
# rounding-sized difference in one update is not amplified by the updates after it.  At lr 0.05 it is: the float32 restatement
# of this very run leaves the float64 curve by 0.5 in mid-run (tests/test_class_loss_cases_host.py shows it), so no device
# could be held there.  At LEARN_LR the loss still falls a hundredfold, the clip engages on most steps, and the bars below hold.
LEARN_LR, LEARN_STEPS, LEARN_SCALE = 0.003, 60, 64


def learn_setup(lr=LEARN_LR):
    """(params, oracle parameters, src, tgt rows, labels) of the learning run."""
    params = model_params("source-encoder-only", 200, 50, 96, 96, 64, 12, N=40, lr=lr)
    rng = np.random.RandomState(2)
    src = np.repeat(random_ids(rng, 16, 12, 200, 0.6), 2, axis=0)
    tgt = rng.randint(0, 40, size=32).astype(np.int32)
    z = np.tile(np.array([1.0, 0.0], np.float32), 16)
    return params, oracle_params(params, seed=5), src, tgt, z


_FREE = {}


def learn_free_run(float64=True, lr=LEARN_LR):
    """The restatement run freely in float64 (or float32: gradients, clip, Adagrad and storage): dict(loss [steps], v = the final
    variables, v0, path = per variable the sum over the steps of the largest element's move, clips).  Computed once per
    argument pair and shared: leave it unchanged."""
    key = (bool(float64), float(lr))
    if key not in _FREE:
        params, p, src, tgt, z = learn_setup(lr)
        dt = np.float64 if float64 else np.float32
        v = {n: np.asarray(p[n], dt) for n in p}
        v0 = dict(v)
        slots = {n: np.full(v[n].shape, 0.1, dt) for n in v}
        path = {n: 0.0 for n in v}
        loss, clips = [], []
        for _ in range(LEARN_STEPS):
            g, tail, _ = step_reference(v, params, src, tgt, z, scale=LEARN_SCALE, float64=float64)
            loss.append(float(tail[1]))
            nv, ns, clip = reference_apply(g, tail, v, slots, lr)
            clips.append(clip)
            for n in v:
                path[n] += float(np.abs(nv[n] - v[n]).max())
            v = {n: nv[n].astype(dt) for n in nv}
            slots = {n: ns[n].astype(dt) for n in ns}
        _FREE[key] = dict(loss=np.array(loss), v=v, v0=v0, path=path, clips=np.array(clips))
    return _FREE[key]


def learn_loss_bar(want, z):
    """Per step: LOSS_REL_EXACT |want| plus the mean over the rows of the row_loss bar z_i 2 c (S + 2) 2^-24 (S = 64)."""
    return LOSS_REL_EXACT * np.abs(want) + float(np.abs(z).mean()) * 2 * LEARN_SCALE * (64 + 2) * 2.0 ** -24


def learn_variable_bar(ref, name):
    """Largest |final variable - float64 reference| a float32 run may show, per element: every update rounds the stored float32
    variable by at most half an ulp, 2^-24 max|v|, once per step; and an update computed from gradients within
    GRAD_BARS_EXACT[1] of the largest element is off by at most that share of the step's largest move, summed over the steps.
    No amplification is allowed for: that is what shaping the run buys."""
    return LEARN_STEPS * 2.0 ** -24 * float(np.abs(ref["v"][name]).max()) + GRAD_BARS_EXACT[1] * ref["path"][name]


def check_learning_run(loss, final, ref, z, what=""):
    """A free run's loss curve and final variables against the float64 free run `ref`; returns (worst loss share of its bar,
    worst variable share of its bar)."""
    loss = np.asarray(loss, np.float64)
    bar = learn_loss_bar(ref["loss"], z)
    diff = np.abs(loss - ref["loss"])
    assert (diff <= bar).all(), "%sloss curve leaves the free-running float64 curve at steps %s: |diff| %s, bar %s" % (
        what, np.nonzero(diff > bar)[0][:5], diff[diff > bar][:5], bar[diff > bar][:5])
    worst = 0.0
    for n in sorted(ref["v"]):
        err = float(np.abs(np.asarray(final[n], np.float64).reshape(ref["v"][n].shape) - ref["v"][n]).max())
        vb = learn_variable_bar(ref, n)
        assert err <= vb, "%s%s: final |variable - free-running float64| %.3g above %.3g" % (what, n, err, vb)
        worst = max(worst, err / vb)
    assert loss[-1] < loss[0] and ref["loss"][-1] < ref["loss"][0]
    return float((diff / bar).max()), worst
