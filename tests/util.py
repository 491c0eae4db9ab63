"""Shared helpers for the GPU parity tests."""
import contextlib

import numpy as np

from oracle import sse_oracle as O


def model_params(mode="dual-encoder", V=500, E=50, Hs=256, Ht=256, S=256, T=32, N=7, lr=0.9):
    return dict(forward_only=False, network_mode=mode, predict_nbest=10, max_seq_length=T, vocab_size=V,
                embedding_size=E, encoding_size=S, src_cell_size=Hs, tgt_cell_size=Ht, learning_rate=lr,
                learning_rate_decay_factor=0.99, targetSpaceSize=N)


def oracle_params(params, seed=0, bias_scale=0.2):
    """The oracle parameter dict make_pair loads (reference initialisers, LSTM biases drawn instead of zero)."""
    p = O.init_params(params, seed=seed)
    rng = np.random.RandomState(seed + 100)
    for k in p:
        if k.endswith("/bias"):
            p[k] = rng.uniform(-bias_scale, bias_scale, size=p[k].shape).astype(np.float32)
    return p


def make_pair(params, seed=0, bias_scale=0.2):
    """(sse_amd.SSEModel on the GPU, oracle parameter dict) holding identical weights."""
    import sse_amd
    p = oracle_params(params, seed, bias_scale)
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    return m, p


def random_ids(rng, B, T, V, pad_frac=0.0):
    ids = rng.randint(2, V, size=(B, T)).astype(np.int32)
    ids[:, -1] = 1
    if pad_frac > 0:
        for b in range(B):
            npad = rng.randint(0, max(1, int(T * pad_frac)) + 1)
            ids[b, :npad] = 0
    return ids


# Loss tolerance of the LSTM train step against the oracle.  The DEFAULT train step is fp32 MFMA throughout -- the
# reference's arithmetic (tf.float32, sse_model.py:355-364) -- and is held to LOSS_REL = LOSS_REL_EXACT.  The opt-in
# split-operand path (options train_fwd_x3 / train_bwd_x3 / train_dk_x3: the three GEMM families on the bf16 matrix pipe
# with hi + lo split fp32 operands) leaves encodings within ~2e-6 of the fp32 path, i.e. <= 64 * 2 * 2e-6 on a logit;
# relative to the north-star budget (1e-3 on a cosine = 6e-2 on a logit) that is 1/250: LOSS_REL_SPLIT.
LOSS_REL_EXACT = 1e-5
LOSS_REL = LOSS_REL_EXACT
LOSS_REL_SPLIT = 1e-4


def exact_fp32_training(model):
    """A model's train step on the fp32-MFMA kernels throughout (the library default since round 4; explicit here)."""
    for opt in ("train_fwd_x3", "train_bwd_x3", "train_dk_x3"):
        model.handle.set_option(opt, 0)


def split_bf16_training(model):
    """Opt a model's train step into the split-operand bf16-pipe GEMMs (forward, BPTT recurrence + dX, weight gradient)."""
    for opt in ("train_dk_x3", "train_fwd_x3", "train_bwd_x3"):
        model.handle.set_option(opt, 1)


# ---- raw train-step gradients against a float64 oracle (tests/test_gpu_train_grads.py, tests/test_grad_check.py) --------
# Bars per variable: (||got - want|| / ||want||, max|got - want| / max|want|).  The float32 oracle is within ~4e-7 / ~6e-7
# of its float64 run (checked in tests/test_grad_check.py at every shape the GPU test uses), so the exact fp32 paths get
# 25x room for a different summation order; the split-bf16 options (hi + lo operands, ~2^-17 per product) 10x that.
GRAD_BARS_EXACT = (1e-5, 2e-5)
GRAD_BARS_SPLIT = (1e-4, 2e-4)
TABLES = ("word_embedding", "target_embedding/tgt_seq_embedding")    # IndexedSlices gradients: their norm enters via tail[0]


@contextlib.contextmanager
def oracle_float64():
    """oracle/sse_oracle.py in float64 for the duration: F32 and the float32 constants switched, restored whatever happens
    (a leak would turn every later test's oracle into float64)."""
    names = ("F32", "FORGET_BIAS", "L2_EPS", "LOGIT_SCALE", "MAX_GRAD_NORM", "ADAGRAD_INIT_ACC")
    saved = {n: getattr(O, n) for n in names}
    try:
        O.F32 = np.float64
        for n in names[1:]:
            setattr(O, n, np.float64(saved[n]))
        yield O
    finally:
        for n in names:
            setattr(O, n, saved[n])


def reference_grads(params, cfg, src, tgt, labels, rows_global=None, cnn_bf16=False, float64=True):
    """What sse_train_grads leaves in the gradient arena, from the oracle: ({variable: dense gradient (float64 array of the
    variable's shape)}, tail[4] = {sum of squares of the un-deduplicated IndexedSlices values, loss, acc, rows}).  Gradients,
    loss and acc are scaled by B / rows_global (the arena holds this rank's share of a mean over rows_global rows).
    float64: the float32 parameters taken as float64 and the whole oracle run in float64 (float64=False: the float32 oracle,
    for tests/test_grad_check.py).  cnn_bf16: the gradient of the bf16 CNN, i.e. the float32 function's gradient at the
    bf16-rounded embedding and filters (tests/test_oracle.py::test_cnn_bf16_gradients_are_the_fp32_gradients_at_the_rounded_weights)."""
    B = len(labels)
    w = float(B) / float(rows_global or B)
    if cnn_bf16:
        params = {k: (O.bf16_round(v) if k == "word_embedding" or k.endswith("/W") else v) for k, v in params.items()}
    cfg = dict(cfg, cnn_bf16=False)
    ctx = oracle_float64() if float64 else contextlib.nullcontext()
    with ctx:
        p = {k: np.asarray(v, O.F32) for k, v in params.items()}
        loss, acc, g = O.gradients(p, cfg, src, tgt, np.asarray(labels, O.F32))
        dense, sq = {}, 0.0
        for name, v in g.items():
            if isinstance(v, tuple):
                sq += float(np.sum(np.square(v[1].astype(np.float64) * w)))
                v = O.dense_embedding_grad(v, p[name].shape[0])
            dense[name] = np.asarray(v, np.float64).reshape(p[name].shape) * w
    return dense, np.array([sq, float(loss) * w, float(acc) * w, B], np.float64)


def arena_grads(model, src, tgt, labels, rows_global=None, rows=False):
    """sse_train_grads (rows=True: sse_train_grads_rows; src / tgt are then corpus row numbers) into a bound torch arena that
    starts as NaN, so that an element no kernel writes shows.  Returns ({variable: gradient in the variable's shape}, tail)."""
    import torch
    h = model.handle
    arena = torch.full((h.train_grad_count(),), float("nan"), dtype=torch.float32, device="cuda:0")
    h.train_bind_arena(arena)
    rg = int(rows_global or len(labels))
    if rows:
        h.train_grads_rows(src, tgt, labels, rg)
    else:
        h.train_grads(src, tgt, labels, rows_global=rg)
    torch.cuda.synchronize()
    return split_arena(model, arena.cpu().numpy())


def split_arena(model, flat):
    """The flat arena as ({variable: [rows, cols] block, in sse_variable_info order}, tail[4])."""
    out, off = {}, 0
    for name, cnt, r, c in model.handle.variables():
        out[name] = flat[off:off + cnt].reshape(r, c)
        off += cnt
    assert off + 4 == flat.size
    return out, flat[off:].copy()


def grad_error(got, want):
    """(||got - want|| / ||want||, max|got - want| / max|want|, index of the largest |got - want|) in float64."""
    d = np.asarray(got, np.float64) - want
    ad = np.abs(d)
    worst = np.unravel_index(int(np.argmax(ad)), d.shape) if d.size else ()
    n, m = float(np.linalg.norm(want)), float(np.abs(want).max()) if want.size else 0.0
    if m == 0.0:
        return (0.0 if not ad.any() else np.inf), (0.0 if not ad.any() else np.inf), worst
    return float(np.linalg.norm(d)) / n, float(ad.max()) / m, worst


def check_grads(got, want, bars, what="", var_bars=None):
    """Asserts every variable within bars = (norm-relative, max-element-relative), a variable named in var_bars within the
    bars given there; returns {variable: (rel, elem)}.
    A failure names the variable, both numbers, the bars and the worst index with its two values."""
    errs, bad = {}, []
    case_bars = bars
    for name in sorted(want):
        bars = (var_bars or {}).get(name, case_bars)
        g = np.asarray(got[name]).reshape(want[name].shape)
        rel, elem, worst = grad_error(g, want[name])
        errs[name] = (rel, elem)
        if not (rel <= bars[0] and elem <= bars[1]):
            bad.append("%s%s: ||d||/||g|| %.3g (bar %.0e), max|d|/max|g| %.3g (bar %.0e), worst at %s: got %r, want %r"
                       % (what, name, rel, bars[0], elem, bars[1], worst, float(g[worst]), float(want[name][worst])))
    assert not bad, "\n".join(bad)
    return errs


def check_tail(got, want, bars, loss_rel, what=""):
    """tail = {sum of squares of the raw slices, loss, acc, rows} against reference_grads' tail; the sum of squares at twice
    the norm-relative gradient bar."""
    assert abs(got[0] - want[0]) <= 2 * bars[0] * want[0], "%stail[0] %r, want %r" % (what, got[0], want[0])
    assert abs(got[1] - want[1]) <= loss_rel * abs(want[1]) + 1e-7, "%stail[1] (loss) %r, want %r" % (what, got[1], want[1])
    assert abs(got[2] - want[2]) <= 1e-6, "%stail[2] (acc) %r, want %r" % (what, got[2], want[2])
    assert got[3] == want[3], "%stail[3] (rows) %r, want %r" % (what, got[3], want[3])


def reference_apply(grads, tail, variables, slots, lr, max_norm=5.0):
    """clip_by_global_norm + Adagrad in float64 on GIVEN (e.g. the device's own) arena gradients: the global norm from
    tail[0] (the IndexedSlices) plus every dense variable, then slot += g^2, var -= lr g / sqrt(slot) per variable.
    Returns (variables, slots) as float64 dicts."""
    tot = float(tail[0]) + sum(float(np.sum(np.square(grads[n].astype(np.float64)))) for n in grads if n not in TABLES)
    gn = np.sqrt(tot)
    scale = max_norm * min(1.0 / gn, 1.0 / max_norm) if gn > 0 else 1.0
    lr = float(np.float32(lr))
    new_v, new_s = {}, {}
    for n, g in grads.items():
        g = g.astype(np.float64) * scale
        new_s[n] = slots[n].astype(np.float64) + g * g
        new_v[n] = variables[n].astype(np.float64) - lr * g / np.sqrt(new_s[n])
    return new_v, new_s
