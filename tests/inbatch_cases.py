"""The in-batch softmax loss (sse_inbatch_loss_dev; the train step under option train_loss = 1): its definition restated in
numpy, the cases of the head and of the whole step, and the checks.  Shared by tests/test_inbatch_cases_host.py (CPU),
tests/test_gpu_inbatch_loss.py (the head alone) and tests/test_gpu_inbatch_train.py (the whole step).

Definition (include/sse_hip.h):  ns_i = s_i / sqrt(max(|s_i|^2, 1e-12)), nt_j likewise;  L_ij = c ns_i . nt_j;  column j is
admitted for row i when j == i, or kt_j != kt_i and not (ks_j == ks_i and z_j != 0);  lse_i = log sum_admitted exp(L_ij);
row_loss_i = z_i (lse_i - L_ii);  row_acc_i = [z_i != 0 and no admitted j != i has L_ij > L_ii];
G_ij = z_i c inv_rows (p_ij - [i == j]);  d ns_i = sum_j G_ij nt_j, d nt_j = sum_i G_ij ns_i, then the l2_normalize backward.

Bars.  Gradients are held to util.GRAD_BARS_EXACT unless the float32 restatement of this very definition (head(..,
dtype=float32)) is not 10x inside it; such a case carries bars of its own = 10 x the restatement's error, rounded up, with the
measured value beside it (tests/test_inbatch_cases_host.py asserts the 10x margin for every case).  A logit carries an
absolute float32 error of about c * 2e-7, which the softmax turns into a RELATIVE error of every p_ij: at c = 64 that is 1e-5
by itself.  row_loss_i = z_i (lse_i - L_ii) is a difference of two logit-sized numbers, so it is held to
LOSS_REL_EXACT |want| + z_i * 2 c (S + 2) 2^-24 (the worst float32 error of two logits)."""
import numpy as np

from oracle import sse_oracle as O
from tests.util import (GRAD_BARS_EXACT, GRAD_BARS_SPLIT, LOSS_REL_EXACT, LOSS_REL_SPLIT, check_grads, check_tail, model_params,
                        oracle_float64, oracle_params, random_ids)

DEFECTS = ("equal-targets-unmasked", "same-source-unmasked", "label0-row-has-loss", "label0-column-dropped", "no-delta",
           "mean-over-active", "no-max-subtraction", "clamp-ignored", "tail-columns-admitted")


def admitted(z, ks, kt, defect=None):
    """[B][B] bool: column j admitted for row i."""
    B = len(z)
    ks = np.arange(B) if ks is None else np.asarray(ks)
    kt = np.arange(B) if kt is None else np.asarray(kt)
    eye = np.eye(B, dtype=bool)
    same_t = kt[None, :] == kt[:, None]
    same_s_verified = (ks[None, :] == ks[:, None]) & (np.asarray(z)[None, :] != 0)
    if defect == "equal-targets-unmasked":
        same_t = np.zeros_like(same_t)
    if defect == "same-source-unmasked":
        same_s_verified = np.zeros_like(same_s_verified)
    adm = eye | (~same_t & ~same_s_verified)
    if defect == "label0-column-dropped":
        adm = eye | (adm & (np.asarray(z)[None, :] != 0))
    return adm


def head(s, t, z, ks=None, kt=None, scale=64.0, inv_rows=None, dtype=np.float64, defect=None):
    """The head in `dtype` arithmetic.  Returns dict(row_loss, row_acc, d_src, d_tgt, logits, adm).  defect: one of DEFECTS (a
    planted error, for the CPU self-test)."""
    dt = dtype
    s, t, z = np.asarray(s, dt), np.asarray(t, dt), np.asarray(z, dt)
    B, S = s.shape
    c = dt(scale)
    inv = dt(1.0 / B if inv_rows is None else inv_rows)
    if defect == "mean-over-active":
        inv = dt(1.0 / max(1, int((z != 0).sum())))
    eps = dt(1e-12)
    if defect == "tail-columns-admitted":   # a partial 32-column tile whose zero padding enters the sums as logits of 0
        pad = (-B) % 32
    else:
        pad = 0
    ss, tt = np.sum(s * s, axis=1, dtype=dt), np.sum(t * t, axis=1, dtype=dt)
    rs, rt = dt(1) / np.sqrt(np.maximum(ss, eps)), dt(1) / np.sqrt(np.maximum(tt, eps))
    ns, nt = (s * rs[:, None]).astype(dt), (t * rt[:, None]).astype(dt)
    L = (c * (ns @ nt.T)).astype(dt)
    adm = admitted(z, ks, kt, defect)
    eye = np.eye(B, dtype=bool)
    neg = dt(-np.inf)
    Lm = np.where(adm, L, neg)
    with np.errstate(over="ignore", invalid="ignore"):
        mx = np.zeros(B, dt) if defect == "no-max-subtraction" else Lm.max(axis=1)
        e = np.where(adm, np.exp(L - mx[:, None]), dt(0)).astype(dt)
        tot = e.sum(axis=1, dtype=dt) + dt(pad) * np.exp(-mx)
        lse = mx + np.log(tot)
        p = (e / tot[:, None]).astype(dt)
    d = np.diag(L)
    zl = np.ones_like(z) if defect == "label0-row-has-loss" else z
    row_loss = (zl * (lse - d)).astype(dt)
    others = np.where(adm & ~eye, L, neg).max(axis=1) if B > 1 else np.full(B, neg)
    row_acc = ((z != 0) & ~(others > d)).astype(dt)
    delta = dt(0) if defect == "no-delta" else eye.astype(dt)
    G = (zl[:, None] * c * inv * (p - delta)).astype(dt)
    dns, dnt = (G @ nt).astype(dt), (G.T @ ns).astype(dt)

    def l2_bwd(n, dn, r, sq):
        full = r[:, None] * (dn - n * np.sum(n * dn, axis=1, keepdims=True, dtype=dt))
        if defect == "clamp-ignored":
            return full.astype(dt)
        return np.where((sq < eps)[:, None], r[:, None] * dn, full).astype(dt)
    return dict(row_loss=row_loss, row_acc=row_acc, d_src=l2_bwd(ns, dns, rs, ss), d_tgt=l2_bwd(nt, dnt, rt, tt), logits=L, adm=adm,
                loss=dt(inv * row_loss.sum(dtype=dt)), acc=dt(inv * row_acc.sum(dtype=dt)))


def accuracy_gap_bound(scale, S):
    """Twice the worst float32 error of two logits: 4 c (S + 2) 2^-24."""
    return 4.0 * scale * (S + 2) * 2.0 ** -24


def min_accuracy_gap(s, t, z, ks, kt, scale):
    """Smallest float64 |L_ii - best other admitted logit| over the active rows (inf when no row has another column)."""
    r = head(s, t, z, ks, kt, scale)
    L, adm = r["logits"], r["adm"]
    B = len(z)
    others = np.where(adm & ~np.eye(B, dtype=bool), L, -np.inf).max(axis=1) if B > 1 else np.full(B, -np.inf)
    gap = np.abs(np.diag(L) - others)[np.asarray(z) != 0]
    return float(gap.min()) if gap.size else np.inf


# ---- head cases ---------------------------------------------------------------------------------------------------------
def _hc(cid, B, S, kind="plain", scale=64.0, rows_factor=1, seed=0, bars=None, f32_err=None):
    return dict(id=cid, B=B, S=S, kind=kind, scale=scale, rows_factor=rows_factor, seed=seed, bars=bars or GRAD_BARS_EXACT,
                f32_err=f32_err)


# bars = (norm-relative, max-element-relative) over d_src and d_tgt.  A case whose float32 restatement is not 10x inside
# GRAD_BARS_EXACT carries 10 x its restatement's error, rounded up; f32_err = that measured error (CPU, numpy float32).
HEAD_CASES = [
    _hc("b1-s3", 1, 3),
    _hc("b2-s64", 2, 64),
    _hc("b31-s130", 31, 130, kind="keys"),
    _hc("b33-s64", 33, 64, kind="keys"),
    _hc("b65-s3", 65, 3, kind="keys"),
    _hc("b100-s130-rows-global", 100, 130, kind="keys", rows_factor=2, bars=(1.1e-5, 2.1e-5), f32_err=(1.10e-6, 2.03e-6)),
    # more than 8 row tiles: a wave of a workgroup walks two tiles (its running max / sum and its gradient accumulators carry
    # over), with the 128-column and the 256-column gradient workgroup
    _hc("b300-s64-two-tiles-per-wave", 300, 64, kind="keys"),
    _hc("b300-s130-two-tiles-per-wave", 300, 130, kind="keys", bars=(1e-5, 2.3e-5), f32_err=(9.39e-7, 2.20e-6)),
    # S = 1: ns = +-1, so the l2_normalize backward cancels exactly and both gradients are zero up to rounding -- held to
    # 16 * 2^-24 * max(1 / norm) * c * inv_rows instead of a relative bar; scale 1 keeps the softmax off saturation (logits +-1)
    _hc("b33-s1", 33, 1, kind="s1", scale=1.0),
    _hc("all-logits-negative", 33, 64, kind="negative", bars=(1.6e-5, 3.5e-5), f32_err=(1.50e-6, 3.40e-6)),
    _hc("labels-all-0", 33, 64, kind="labels0"),
    _hc("one-target-key", 33, 64, kind="one-target"),
    _hc("same-source-pairs", 100, 64, kind="pairs"),
    _hc("null-keys", 65, 64, kind="null"),
    _hc("zero-rows", 33, 64, kind="zeros"),
    _hc("s-equals-t-scale256", 33, 64, kind="equal", scale=256.0, bars=(1.1e-4, 1.4e-4), f32_err=(1.08e-5, 1.36e-5)),
    _hc("fractional-labels", 31, 64, kind="fractional"),
]
HEAD_CASES_BY_ID = {c["id"]: c for c in HEAD_CASES}


def head_inputs(c, seed=None):
    """dict(s, t, z, ks, kt, scale, inv_rows) of a head case (float32 inputs, int64 keys or None)."""
    B, S, kind = c["B"], c["S"], c["kind"]
    rng = np.random.RandomState(1000 + (c["seed"] if seed is None else seed))
    # the own target is the best column of about half the rows: a softmax that saturates (p_ii = 1 to rounding) leaves a
    # gradient of rounding noise and nothing to compare.  Two rows: one other column, so hardly any correlation.
    corr = 0.02 if B <= 2 else 0.3
    s = rng.normal(size=(B, S)).astype(np.float32)
    t = (corr * s + rng.normal(size=(B, S))).astype(np.float32)
    z = (rng.uniform(size=B) < 0.6).astype(np.float32)
    z[0] = 1.0
    ks = np.arange(B, dtype=np.int64) * 7 + 3                           # distinct, not the row numbers
    kt = np.arange(B, dtype=np.int64) * 5 + 11
    if kind == "keys" and B > 4:                                        # a few repeated sources and targets, anywhere in the batch
        for _ in range(max(2, B // 8)):
            i, j = rng.randint(0, B, size=2)
            ks[j] = ks[i]
        for _ in range(max(2, B // 8)):
            i, j = rng.randint(0, B, size=2)
            kt[j] = kt[i]
            t[j] = t[i]
    elif kind == "s1":           # S = 1: every logit is +-c, so active rows share one target key and see only label-0 columns
        s = np.abs(s) + 0.5
        act = z != 0
        t = np.where(act[:, None], np.abs(t) + 0.5, -np.abs(t) - 0.5).astype(np.float32)
        kt[act] = 4
    elif kind == "negative":     # every logit near -0.9 c: a zero logit let in by mistake (padding) would own the softmax
        u = rng.normal(size=(1, S))
        s = (u + 0.3 * rng.normal(size=(B, S))).astype(np.float32)
        t = (-u + 0.3 * rng.normal(size=(B, S))).astype(np.float32)
    elif kind == "labels0":
        z[:] = 0.0
    elif kind == "one-target":
        kt[:] = 7
        z[:] = 1.0
    elif kind == "pairs":        # rows 2i, 2i + 1 carry one source: labels (1, 1) on even pairs, (1, 0) on odd ones
        ks = np.repeat(np.arange(B // 2, dtype=np.int64) * 3 + 1, 2)
        s = np.repeat(s[: B // 2], 2, axis=0)
        t = (corr * s + rng.normal(size=(B, S))).astype(np.float32)
        z = np.tile(np.array([1, 1, 1, 0], np.float32), B // 4)
    elif kind == "null":
        ks = kt = None
    elif kind == "zeros":        # exact zeros on rows with label 0 (an active all-zero source row ties every logit at 0), and
        z[3] = z[5] = 0.0        # rows below the clamp on active rows: the clamp rule carries gradient on both sides
        s[3] = 0.0
        t[5] = 0.0
        z[8] = z[9] = 1.0
        s[8] = (s[8] * 1e-8).astype(np.float32)
        t[9] = (t[9] * 1e-8).astype(np.float32)
    elif kind == "equal":        # L_ii = c exactly; odd rows lie close to their even neighbour, so that row's softmax has a
        s[1::2] = (s[0:B - 1:2] + 0.02 * s[1::2]).astype(np.float32)   # second column within a fraction of a logit of c
        t = s.copy()
        z[:] = 1.0
    elif kind == "fractional":
        z = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 1.5], np.float32), size=B).astype(np.float32)
        z[0] = 0.5
    return dict(s=s, t=t, z=z, ks=ks, kt=kt, scale=c["scale"], inv_rows=1.0 / (c["rows_factor"] * B))


def head_case_seeded(c):
    """The inputs of a case at the first seed (from the case's own upwards) that meets the accuracy precondition on every row."""
    for k in range(64):
        x = head_inputs(c, c["seed"] + k)
        if min_accuracy_gap(x["s"], x["t"], x["z"], x["ks"], x["kt"], x["scale"]) >= accuracy_gap_bound(x["scale"], c["S"]):
            return x
    raise AssertionError("no seed meets the accuracy precondition for %s" % c["id"])


def head_errors(got, want):
    """(norm-relative, max-element-relative) error over d_src and d_tgt together."""
    g = np.concatenate([np.asarray(got["d_src"], np.float64).ravel(), np.asarray(got["d_tgt"], np.float64).ravel()])
    w = np.concatenate([want["d_src"].ravel(), want["d_tgt"].ravel()])
    d = np.abs(g - w)
    if not w.any():
        return (0.0, 0.0) if not d.any() else (np.inf, np.inf)
    return float(np.linalg.norm(g - w) / np.linalg.norm(w)), float(d.max() / np.abs(w).max())


def check_head(got, want, c, bars=None, what=""):
    """got: dict(row_loss, row_acc[, d_src, d_tgt]) against the float64 head `want`; every row and element compared."""
    bars = bars or c["bars"]
    x_scale, S = c["scale"], c["S"]
    z = np.asarray(want["z"], np.float64)
    rl = np.asarray(got["row_loss"], np.float64)
    tol = LOSS_REL_EXACT * np.abs(want["row_loss"]) + np.abs(z) * 2 * x_scale * (S + 2) * 2.0 ** -24
    bad = np.abs(rl - want["row_loss"]) > tol
    assert np.isfinite(rl).all() and not bad.any(), "%s%s row_loss: rows %s got %s want %s" % (
        what, c["id"], np.nonzero(bad)[0][:5], rl[bad][:5], want["row_loss"][bad][:5])
    assert np.array_equal(np.asarray(got["row_acc"], np.float64), want["row_acc"]), "%s%s row_acc differs at rows %s" % (
        what, c["id"], np.nonzero(np.asarray(got["row_acc"]) != want["row_acc"])[0][:8])
    if "d_src" not in got:
        return None
    for k in ("d_src", "d_tgt"):
        assert np.isfinite(np.asarray(got[k])).all(), "%s%s %s holds a non-finite element" % (what, c["id"], k)
        zero = ~want[k].any(axis=1) & (S > 1)     # rows whose gradient is exactly zero stay exactly zero
        assert not np.asarray(got[k])[zero].any(), "%s%s %s: a row that must be zero is not" % (what, c["id"], k)
    if S == 1:                                  # exact cancellation: zero up to rounding (see the b33-s1 case)
        x = want["x"]
        r = 1.0 / np.sqrt(np.maximum(np.minimum((x["s"].astype(np.float64) ** 2).sum(1), (x["t"].astype(np.float64) ** 2).sum(1)), 1e-12))
        bound = 16 * 2.0 ** -24 * float(r.max()) * x_scale * x["inv_rows"] * float(np.abs(z).max())
        worst = max(float(np.abs(np.asarray(got[k], np.float64)).max()) for k in ("d_src", "d_tgt"))
        assert worst <= bound, "%s%s: |gradient| %.3g above the rounding bound %.3g at S = 1" % (what, c["id"], worst, bound)
        return 0.0, 0.0
    rel, elem = head_errors(got, want)
    assert rel <= bars[0] and elem <= bars[1], "%s%s gradients: ||d||/||g|| %.3g (bar %.1e), max|d|/max|g| %.3g (bar %.1e)" % (
        what, c["id"], rel, bars[0], elem, bars[1])
    return rel, elem


def head_want(x):
    w = head(x["s"], x["t"], x["z"], x["ks"], x["kt"], x["scale"], x["inv_rows"])
    w["z"] = x["z"]
    w["x"] = x
    return w


# ---- the whole step ---------------------------------------------------------------------------------------------------
def _row_keys(a):
    """Key per row: the first row holding the same values."""
    a = np.asarray(a)
    a = a.reshape(len(a), -1)
    _, first, inv = np.unique(a, axis=0, return_index=True, return_inverse=True)
    return first[inv.ravel()].astype(np.int64)


def _step_gradients(p, cfg, src, tgt, labels, inv_rows, scale):
    """oracle.gradients / _source_only_gradients / _cnn_gradients with the in-batch loss in place of the pair loss, from the
    oracle's own forward and backward pieces, in the oracle's current precision (F32)."""
    F = O.F32
    mode = cfg["network_mode"]
    emb = p["word_embedding"]
    E = emb.shape[1]
    labels = np.asarray(labels, F)
    ks = _row_keys(src)
    kt = _row_keys(tgt)
    grads = {}
    if mode in ("dual-encoder", "shared-encoder"):
        fw = {}
        for side, ids in (("src", src), ("tgt", tgt)):
            scope = O.lstm_scope(mode, side)
            K, b = p[scope + "/rnn/basic_lstm_cell/kernel"], p[scope + "/rnn/basic_lstm_cell/bias"]
            h, tape = O.lstm_forward(emb, K, b, ids, keep_tape=True)
            M = p[O.proj_name(mode, side)]
            fw[side] = dict(scope=scope, K=K, h=h, tape=tape, M=M, raw=(h @ M).astype(F), ids=O.check_ids(ids, emb.shape[0]))
        r = head(fw["src"]["raw"], fw["tgt"]["raw"], labels, ks, kt, scale, inv_rows, dtype=F)
        sl_ids, sl_rows = [], []
        for side, draw in (("src", r["d_src"]), ("tgt", r["d_tgt"])):
            f = fw[side]
            grads[O.proj_name(mode, side)] = (f["h"].T @ draw).astype(F)
            dK, db, dX = O._lstm_backward(f["K"], f["tape"], (draw @ f["M"].T).astype(F), E)
            kname, bname = f["scope"] + "/rnn/basic_lstm_cell/kernel", f["scope"] + "/rnn/basic_lstm_cell/bias"
            grads[kname] = grads.get(kname, 0) + dK
            grads[bname] = grads.get(bname, 0) + db
            sl_ids.append(f["ids"].reshape(-1))
            sl_rows.append(dX.reshape(-1, E))
        grads["word_embedding"] = (np.concatenate(sl_ids), np.concatenate(sl_rows).astype(F))
        return r, grads
    table = p["target_embedding/tgt_seq_embedding"]
    rows = O.check_ids(np.asarray(tgt).reshape(-1), table.shape[0])
    ids = O.check_ids(src, emb.shape[0])
    raw_t = table[rows]
    if mode == "source-encoder-only":
        scope = O.lstm_scope(mode, "src")
        K, b = p[scope + "/rnn/basic_lstm_cell/kernel"], p[scope + "/rnn/basic_lstm_cell/bias"]
        h, tape = O.lstm_forward(emb, K, b, ids, keep_tape=True)
        M = p[O.proj_name(mode, "src")]
        r = head((h @ M).astype(F), raw_t, labels, ks, kt, scale, inv_rows, dtype=F)
        dK, db, dX = O._lstm_backward(K, tape, (r["d_src"] @ M.T).astype(F), E)
        grads = {O.proj_name(mode, "src"): (h.T @ r["d_src"]).astype(F), scope + "/rnn/basic_lstm_cell/kernel": dK,
                 scope + "/rnn/basic_lstm_cell/bias": db, "target_embedding/tgt_seq_embedding": (rows, r["d_tgt"].astype(F)),
                 "word_embedding": (ids.reshape(-1), dX.reshape(-1, E).astype(F))}
        return r, grads
    assert mode == "source_only_cnn"
    B, T = ids.shape
    pool, tape = O.cnn_forward(p, ids, keep_tape=True)
    M = p["source_only_cnn/src_M"]
    r = head((pool @ M).astype(F), raw_t, labels, ks, kt, scale, inv_rows, dtype=F)
    d_s = r["d_src"]
    grads = {"source_only_cnn/src_M": (pool.T @ d_s).astype(F), "target_embedding/tgt_seq_embedding": (rows, r["d_tgt"].astype(F))}
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
    """What sse_train_grads leaves in the arena under train_loss = 1, as util.reference_grads returns it for the pair loss:
    ({variable: dense gradient}, tail[4]); also the head's own result (logits, adm) for the accuracy precondition."""
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


def _sc(cid, mode, V, E, Hs, Ht, S, T, B, N=13, batch="paired", opts=None, rows_factor=1, by_rows=False, seed=0, scale=64,
        bars=None, f32_err=None, path="fused", paired=False):
    opts = dict(opts or {})
    split = any(opts.get(k) for k in ("train_fwd_x3", "train_bwd_x3", "train_dk_x3"))
    return dict(id=cid, mode=mode, V=V, E=E, Hs=Hs, Ht=Ht, S=S, T=T, B=B, N=N, batch=batch, opts=opts, split=split,
                rows_factor=rows_factor, by_rows=by_rows, seed=seed, scale=scale, path=path, paired=paired,
                bars=bars or (GRAD_BARS_SPLIT if split else GRAD_BARS_EXACT), f32_err=f32_err)


# bars: as for the head cases -- a component whose float32 restatement (the whole step in the float32 oracle) is not 10x
# inside GRAD_BARS_EXACT is 10 x that restatement's error, rounded up; f32_err = the measured (norm, element) errors
STEP_CASES = [
    _sc("dual-paired-b128", "dual-encoder", 90, 16, 16, 16, 32, 8, 128, paired=True, bars=(1.2e-5, 2e-5), f32_err=(1.20e-6, 1.17e-6)),
    _sc("dual-unpaired-b40", "dual-encoder", 90, 16, 16, 16, 32, 8, 40, batch="unpaired", bars=(1.1e-5, 2e-5), f32_err=(1.04e-6, 1.10e-6)),
    _sc("shared-b64", "shared-encoder", 80, 12, 16, 16, 24, 7, 64, batch="unpaired"),
    _sc("seo-b40", "source-encoder-only", 80, 12, 16, 16, 16, 6, 40, N=11, batch="unpaired"),   # 40 rows over 11 target rows: repeats
    _sc("by-rows-equal-tokens", "dual-encoder", 90, 16, 16, 16, 32, 8, 40, batch="unpaired", by_rows=True, bars=(1.1e-5, 2e-5),
        f32_err=(1.04e-6, 1.10e-6)),
    _sc("generic-forced", "dual-encoder", 70, 8, 16, 16, 8, 6, 24, batch="unpaired", opts=dict(train_generic=1), path="generic",
        bars=(1.4e-5, 2e-5), f32_err=(1.31e-6, 1.62e-6)),
    _sc("cnn-b10", "source_only_cnn", 90, 16, 16, 16, 32, 12, 10, N=7, batch="unpaired", path="cnn", seed=1),
    _sc("rows-global-2b", "dual-encoder", 90, 16, 16, 16, 32, 8, 40, batch="unpaired", rows_factor=2, bars=(1.1e-5, 2e-5),
        f32_err=(1.04e-6, 1.10e-6)),
    _sc("split-operands", "dual-encoder", 90, 16, 64, 64, 32, 8, 64, batch="unpaired",
        opts=dict(train_fwd_x3=1, train_bwd_x3=1, train_dk_x3=1)),
]
STEP_CASES_BY_ID = {c["id"]: c for c in STEP_CASES}


def step_params(c):
    params = model_params(c["mode"], c["V"], c["E"], c["Hs"], c["Ht"], c["S"], c["T"], N=c["N"], lr=0.9)
    return params, oracle_params(params, seed=3 + c["seed"])


def step_batch(c, seed=None):
    """(src, tgt, labels): the reference's batch shape -- every source twice in a paired batch, label 1 with its own target and
    label 0 with another row's; some rows repeat a source or a target of an earlier row."""
    rng = np.random.RandomState(50 + (c["seed"] if seed is None else seed))
    B, T, V = c["B"], c["T"], c["V"]
    Vb = max(3, V * 4 // 5)
    if c["batch"] == "paired":
        src = np.repeat(random_ids(rng, B // 2, T, Vb, 0.5), 2, axis=0)
        z = np.tile(np.array([1.0, 0.0], np.float32), B // 2)
    else:
        src = random_ids(rng, B, T, Vb, 0.5)
        z = (rng.uniform(size=B) < 0.6).astype(np.float32)
        z[0] = 1.0
        for _ in range(max(1, B // 10)):          # a source twice, anywhere in the batch
            i, j = rng.randint(0, B, size=2)
            src[j] = src[i]
    if c["mode"] in ("source-encoder-only", "source_only_cnn"):
        tgt = rng.randint(0, c["N"], size=B).astype(np.int32)
    else:
        tgt = random_ids(rng, B, T, Vb, 0.5)
        for _ in range(max(1, B // 10)):          # a target twice
            i, j = rng.randint(0, B, size=2)
            tgt[j] = tgt[i]
    return src, tgt, z


def step_case_seeded(c):
    """(params, oracle parameters, src, tgt, z, want, want_tail, head) at the first batch seed that meets the accuracy
    precondition on every active row (float64 logits of the float64 step)."""
    params, p = step_params(c)
    for k in range(32):
        src, tgt, z = step_batch(c, c["seed"] + k)
        want, tail, r = step_reference(p, params, src, tgt, z, c["rows_factor"] * len(z), c["scale"])
        L, adm = r["logits"], r["adm"]
        B = len(z)
        others = np.where(adm & ~np.eye(B, dtype=bool), L, -np.inf).max(axis=1)
        gap = np.abs(np.diag(L) - others)[z != 0]
        if gap.min() >= accuracy_gap_bound(c["scale"], c["S"]):
            return params, p, src, tgt, z, want, tail, r
    raise AssertionError("no seed meets the accuracy precondition for %s" % c["id"])


def check_step(got, tail, want, want_tail, c, what=""):
    errs = check_grads(got, want, c["bars"], what="%s%s: " % (what, c["id"]))
    check_tail(tail, want_tail, c["bars"], LOSS_REL_SPLIT if c["split"] else LOSS_REL_EXACT, what="%s%s: " % (what, c["id"]))
    return errs
