"""Raw train-step gradients (the arena sse_train_grads leaves) against the float64 oracle, on every training path.

The other training tests see the backward pass only through the weights after one Adagrad step, where a gradient error
below ~7e-5 absolute disappears (tests/test_grad_check.py measures how coarse that is).  Here every variable's gradient,
the dense embedding block and the tail {sum of squares of the raw embedding slices, loss, acc, rows} are held to
util.GRAD_BARS_EXACT (the exact fp32 paths, the bf16 CNN against its rounded-weight reference) or util.GRAD_BARS_SPLIT (the
split-bf16 train_*_x3 options); then sse_train_apply is checked on its own, against a float64 clip + Adagrad of the
device's own arena.  CASES is shared with the CPU self-test, which checks that the float32 oracle passes these bars with
10x margin at every case and that known backward defects do not."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import (GRAD_BARS_EXACT, GRAD_BARS_SPLIT, LOSS_REL_EXACT, LOSS_REL_SPLIT, arena_grads, check_grads,
                        check_tail, model_params, oracle_params, random_ids, reference_apply, reference_grads)

pytestmark = pytest.mark.gpu


def _case(cid, mode, V, E, Hs, Ht, S, T, B, N=13, batch="paired", opts=None, rows_factor=1, by_rows=False, seed=0, **extra):
    opts = dict(opts or {})
    split = any(opts.get(k) for k in ("train_fwd_x3", "train_bwd_x3", "train_dk_x3"))
    return pytest.param(dict(id=cid, mode=mode, V=V, E=E, Hs=Hs, Ht=Ht, S=S, T=T, B=B, N=N, batch=batch, opts=opts, split=split,
                             rows_factor=rows_factor, by_rows=by_rows, seed=seed, **extra), id=cid)


def _cnn(cid, V, E, S, T, B, N=17, seed=0, bf16=False, **kw):
    """A text-CNN case.  Extra keys: distinct = D (batch kind "tiled": D distinct sequences tiled over the batch), conv_bias = v
    (every conv bias set to v), dead = (lo, hi) (the share of pooled features that are exactly 0 must lie in [lo, hi]),
    bars = a bar of the case's own, var_bars = {variable: bars}."""
    return _case(cid, "source_only_cnn", V, E, 96, 96, S, T, B, N=N, seed=seed, opts=dict(cnn_bf16=1) if bf16 else None, **kw)


def _x3(fwd, bwd, dk):
    return dict(train_fwd_x3=fwd, train_bwd_x3=bwd, train_dk_x3=dk)


# Text-CNN, one case per backward branch.  The kernel a case takes, read from the launchers: cnn_dw_kernel<R,X16> with R = 8
# (T <= 64), 12 (T <= 96), 0 (longer), X16 = bf16 with even E; dX by cnn_dx_mfma_kernel<ceil(T/32), ceil(E/32)> in bf16 mode up
# to T = 96, else by the gather cnn_dx_kernel + dx_hot_reduce; NCH = min(ceil(B/32), 128) chunks; the training forward
# conv_pool_kernel<true,NB> / conv_pool_bf16_kernel<NB,true> with NB = 8 sequences per workgroup while T * Ep <= ~3,940 (fp32,
# Ep = E rounded up to 4) or T * Ep8 <= ~7,900 (bf16), else 4.  Seeds searched on the CPU so that no max-pool is within 1e-5 of
# a tie and no pooled feature within 1e-5 of 0 (both asserted).  Left out on purpose: ids_fit == false with T <= 96 (the
# chunk's ids no longer in LDS), which needs B above about 17,800 at T = 96.
CNN_CASES = [
    _cnn("cnn-t5", 60, 8, 16, 5, 24, N=64, seed=1),                       # ONE position for width 5; dw<8,false>; conv_pool<true,8>
    _cnn("cnn-e3", 80, 3, 24, 12, 10, seed=4),                           # E < 4 (Ep 4): k-groups mostly padding
    _cnn("cnn-t80-e50", 200, 50, 64, 80, 26, N=33, seed=6),              # reference default T; dw<12,false>; conv_pool<true,4>
    _cnn("cnn-t96-e64", 150, 64, 64, 96, 20, seed=3),                    # dw<12,false> at its upper edge; E 64 (the training limit)
    _cnn("cnn-t140-e64", 150, 64, 32, 140, 8),                   # dw<0,false>; training forward ~750 B below its LDS limit
    _cnn("cnn-t150-e50", 120, 50, 32, 150, 12, seed=2),                  # dw<0,false>; 5 position tiles
    _cnn("cnn-b9", 90, 24, 64, 20, 9, batch="unpaired", seed=7),         # odd B: DW_G tail, partial dX workgroup, Bp padding rows
    _cnn("cnn-chunks", 90, 24, 64, 20, 200, N=400, batch="tiled", distinct=24, seed=2),        # 7 chunks, the last one partial; reduce order
    # chunk cap: per = 33, chunks 125-127 empty.  A bar of its own: the float32 oracle itself is 1.47e-6 norm-relative (conv-
    # maxpool-4/b; every conv variable and the embedding ~1.2e-6 alike) / 4.13e-6 per element (word_embedding) from float64 here
    # -- the 4100-term float32 sums -- so 10x that, rounded up, instead of 25x 4e-7; still well inside GRAD_BARS_SPLIT
    _cnn("cnn-b4100", 90, 16, 32, 12, 4100, N=6000, batch="tiled", distinct=24, seed=15, bars=(1.5e-5, 4.2e-5)),
    _cnn("cnn-hot", 90, 24, 64, 20, 40, N=64, batch="cnn-hot", seed=12),        # hot_part + dx_hot_reduce, all-PAD pair, one repeated id
    _cnn("cnn-dead", 90, 24, 64, 20, 10, conv_bias=-0.15, dead=(0.3, 0.7)),     # ReLU mask in db / dW / dX
    _cnn("cnn-all-dead", 90, 24, 64, 20, 10, conv_bias=-10.0, dead=(1.0, 1.0)), # zero encodings through the 1e-12 clamp
    _cnn("cnn-rows-global-3b", 90, 24, 64, 20, 10, rows_factor=3, seed=2),      # this rank's share of a mean over 3 B rows
    _cnn("cnn-by-rows", 90, 24, 64, 20, 10, by_rows=True, seed=2),       # sse_train_grads_rows: uploaded source corpus, free-matrix rows
    _cnn("cnn-bf16-11", 90, 24, 64, 20, 10, bf16=True),          # dx_mfma<1,1>; dw<8,true>
    _cnn("cnn-bf16-12", 200, 50, 64, 30, 16, N=33, bf16=True, seed=7),   # dx_mfma<1,2>
    _cnn("cnn-bf16-21", 200, 32, 64, 40, 16, N=33, bf16=True, seed=4),   # dx_mfma<2,1>
    _cnn("cnn-bf16-31", 200, 30, 64, 96, 12, N=33, bf16=True, seed=1),   # dx_mfma<3,1>; dw<12,true>
    _cnn("cnn-bf16-32", 200, 50, 64, 80, 26, N=33, bf16=True, seed=9),   # dx_mfma<3,2>; dw<12,true>
    _cnn("cnn-bf16-e25", 200, 25, 64, 33, 18, N=33, bf16=True, seed=3),  # odd E: x16 false, dw<8,false> rounding while staging; dx_mfma<2,1>
    _cnn("cnn-bf16-t100", 200, 50, 64, 100, 12, N=33, bf16=True, seed=1),               # gather dX over rounded filters; dw<0,true>
    _cnn("cnn-bf16-t96-e64", 150, 64, 64, 96, 16, bf16=True, seed=2),    # dw<12,true>, dx_mfma<3,2> at both upper edges
    _cnn("cnn-bf16-t140-e64", 150, 64, 32, 140, 8, bf16=True, seed=3),   # conv_pool_bf16<4,true> (T * Ep8 = 8,960); dw<0,true>; gather dX
    _cnn("cnn-bf16-chunks", 90, 24, 64, 20, 200, N=400, batch="tiled", distinct=24, bf16=True, seed=30),   # chunks through dx_mfma, hot_part[workgroup]
]

CASES = [
    # configs[1] shape: paired (B % 128 == 0: source forward and dK on B/2 rows, dk_gemm2 pair) and the same batch unpaired
    _case("c1-paired", "dual-encoder", 400, 50, 256, 256, 256, 32, 128),
    _case("c1-unpaired", "dual-encoder", 400, 50, 256, 256, 256, 32, 128, batch="unpaired"),
    # Bp > 256: the projection backward in several row chunks plus its reduce
    _case("d256-b512-paired", "dual-encoder", 600, 50, 256, 256, 256, 8, 512),
    _case("d256-b320-unpaired", "dual-encoder", 600, 50, 256, 256, 256, 8, 320, batch="unpaired"),
    # Hp 128 with H < Hp, S % 8 != 0 (VALU proj_bwd_dh), T 50
    _case("shared96-s50", "shared-encoder", 300, 40, 96, 96, 50, 50, 64),
    # both lstm_bwd2 widths: H == Hp (128) and H < Hp (200 in 256)
    _case("h128", "dual-encoder", 300, 50, 128, 128, 64, 10, 96),
    _case("h200", "dual-encoder", 300, 40, 200, 200, 64, 10, 64),
    # embedding widths around the KT 6 / 10 boundary and the constant-1 column; E 64 runs the first generation by itself
    _case("e7", "shared-encoder", 200, 7, 40, 40, 24, 5, 130),
    _case("e31", "dual-encoder", 300, 31, 128, 96, 48, 8, 64),
    _case("e32", "dual-encoder", 300, 32, 96, 64, 40, 7, 66),
    _case("e63", "dual-encoder", 300, 63, 128, 256, 64, 9, 128),
    _case("e64", "dual-encoder", 300, 64, 128, 256, 64, 9, 128),
    # zero LSTM biases (the reference initialiser) and a small embedding: cell states ~1e-3, where the training forward's and the
    # BPTT recompute's tanh (sse_tanh, shared with the inference kernels) takes its small-argument branch; fused fp32 path
    _case("small-preactivations", "dual-encoder", 300, 50, 128, 128, 64, 10, 128, zero_bias=True, emb_scale=1e-2),
    # first-generation kernels (lstm_bwd_kernel, dx_kernel, bias partials)
    _case("gen1-c1", "dual-encoder", 400, 50, 256, 256, 256, 16, 128, opts=dict(train_gen1=1)),
    _case("gen1-shared96", "shared-encoder", 300, 40, 96, 96, 50, 50, 64, opts=dict(train_gen1=1)),
    # split-bf16 GEMMs (forward, BPTT, weight gradient), kernel by kernel
    _case("x3-111", "dual-encoder", 300, 50, 256, 96, 64, 9, 128, opts=_x3(1, 1, 1)),
    _case("x3-001", "dual-encoder", 300, 50, 256, 96, 64, 9, 128, opts=_x3(0, 0, 1)),
    _case("x3-011", "dual-encoder", 300, 50, 256, 96, 64, 9, 128, opts=_x3(0, 1, 1)),
    _case("x3-101", "dual-encoder", 300, 50, 256, 96, 64, 9, 128, opts=_x3(1, 0, 1)),
    # any-shape path: forced on a fused shape, H > 256, E > 64, odd cell sizes with S 19
    _case("generic-forced", "dual-encoder", 300, 50, 96, 64, 64, 12, 32, opts=dict(train_generic=1)),
    _case("generic-h300", "dual-encoder", 200, 50, 300, 300, 64, 10, 32),
    _case("generic-e100", "dual-encoder", 120, 100, 128, 96, 64, 8, 24),
    _case("generic-h33-129", "dual-encoder", 150, 7, 33, 129, 19, 5, 6),
    # source-encoder-only: rows_scatter into the free target matrix, its IndexedSlices in tail[0]
    _case("seo-h128", "source-encoder-only", 200, 50, 128, 128, 64, 12, 40, N=17),
    _case("seo-e70", "source-encoder-only", 90, 70, 64, 64, 40, 6, 10, N=13),
    # CNN: cnn_dw, cnn_dx(_mfma); seeds chosen so that no max-pool is within rounding of a tie (asserted below)
    _case("cnn", "source_only_cnn", 90, 24, 96, 96, 64, 20, 10, N=17, seed=1),
    _case("cnn-bf16", "source_only_cnn", 200, 50, 96, 96, 64, 33, 26, N=33, opts=dict(cnn_bf16=1), seed=0),
] + CNN_CASES + [
    # BPTT edges, repeated / hot ids (dx_hot_reduce, the atomics scatter), labels all 1
    _case("t1", "dual-encoder", 100, 16, 64, 64, 32, 1, 64),
    _case("t2", "shared-encoder", 100, 16, 64, 64, 32, 2, 64),
    _case("edges", "dual-encoder", 300, 50, 128, 128, 64, 10, 128, batch="edges"),
    _case("hot-ids", "dual-encoder", 300, 50, 128, 96, 64, 12, 128, batch="hot"),
    _case("labels-1", "shared-encoder", 300, 40, 96, 96, 64, 10, 64, batch="ones"),
    # this rank's share of a mean over 3 B rows; batches by row number from uploaded corpora (device id gather)
    _case("rows-global-3b", "dual-encoder", 300, 50, 128, 128, 64, 10, 64, rows_factor=3),
    _case("by-rows", "dual-encoder", 300, 50, 128, 128, 64, 10, 64, by_rows=True),
    # Branches of the step frame that the three paths share and that no case above reaches: every paired case above (a pair
    # needs B % 128 == 0) is dual-encoder with id matrices.  B 128 is the smallest paired shape; everything else is small.
    # permuted free-matrix rows together with rows_scatter and its offset behind the encoder's partial sums (N 300: more rows
    # than the batch, so that some stay untouched -- asserted)
    _case("seo-paired", "source-encoder-only", 200, 32, 96, 96, 48, 6, 128, N=300),
    # the half-row source side accumulating onto the shared kernel gradient on one stream
    _case("shared-paired", "shared-encoder", 200, 24, 64, 64, 32, 7, 128),
    # row numbers under the pair permutation, then the device gather (pair_rows: the two rows of a pair name ONE corpus row,
    # which is how a batch by row numbers is recognised as paired)
    _case("by-rows-paired", "dual-encoder", 200, 40, 96, 64, 64, 8, 128, by_rows=True, pair_rows=True),
    _case("seo-by-rows-paired", "source-encoder-only", 200, 16, 64, 64, 40, 5, 128, N=300, by_rows=True, pair_rows=True),
    # both encoders on one stream (the h128 shape)
    _case("serial", "dual-encoder", 300, 50, 128, 128, 64, 10, 96, opts=dict(train_serial=1)),
    # a pairable batch with the pair deduplication switched off (the c1 shape at T 8)
    _case("pair-dedup-off", "dual-encoder", 400, 50, 256, 256, 256, 8, 128, opts=dict(train_pair_dedup=0)),
]


def case_params(c):
    """(model params, oracle parameter dict) of a case: what _model loads into the GPU model."""
    params = model_params(c["mode"], c["V"], c["E"], c["Hs"], c["Ht"], c["S"], c["T"], N=c["N"], lr=0.9)
    p = oracle_params(params, seed=3 + c["seed"], bias_scale=0.0 if c.get("zero_bias") else 0.2)
    if c.get("emb_scale"):
        p["word_embedding"] = (p["word_embedding"] * np.float32(c["emb_scale"])).astype(np.float32)
    if c.get("conv_bias") is not None:             # lowered conv biases: dead filters (pooled value exactly 0)
        for k in p:
            if k.endswith("/b"):
                p[k] = np.full_like(p[k], c["conv_bias"])
    return params, p


def _ids(rng, B, T, V):
    Vb = max(3, V * 4 // 5)                        # the top fifth of the vocabulary stays untouched
    if T <= 2:
        return rng.randint(0, Vb, size=(B, T)).astype(np.int32)
    return random_ids(rng, B, T, Vb, 0.6)


def case_batch(c):
    """(src, tgt, labels) of a case: src / tgt are id matrices, tgt rows of the free target matrix in the table modes."""
    rng = np.random.RandomState(11 + c["seed"])
    B, T, V = c["B"], c["T"], c["V"]
    kind = c["batch"]
    if kind in ("tiled", "cnn-hot"):               # the CNN-only kinds draw in an order of their own; every other kind as before
        return _cnn_batch(c, rng)
    src = _ids(rng, B, T, V) if kind == "unpaired" else np.repeat(_ids(rng, B // 2, T, V), 2, axis=0)
    if c["mode"] in ("source-encoder-only", "source_only_cnn"):
        tgt = rng.randint(0, c["N"], size=B).astype(np.int32)
    else:
        tgt = _ids(rng, B, T, V)
    z = np.tile(np.array([1.0, 0.0], np.float32), (B + 1) // 2)[:B]     # odd B (unpaired only): one more positive row
    if kind == "edges":
        src[0:2] = 0                               # an all-PAD pair
        tgt[0] = 0
        tgt[2] = 7                                 # a row of one repeated id
        src[4:6] = 9
    elif kind == "hot":                            # most tokens PAD / EOS: the hot rows of the embedding scatter
        hot = rng.uniform(size=src.shape) < 0.8
        src[hot] = rng.randint(0, 2, size=int(hot.sum()))
        src[1::2] = src[0::2]
        hot = rng.uniform(size=tgt.shape) < 0.8
        tgt[hot] = rng.randint(0, 2, size=int(hot.sum()))
    elif kind == "ones":
        z[:] = 1.0
    return src, tgt, z


def _cnn_batch(c, rng):
    """tiled: c["distinct"] (<= 24) distinct sequences repeated over the batch, target rows and labels drawn per row -- the
    near-tie preconditions cannot hold for thousands of random sequences (the smallest gap over B * 576 features shrinks like
    1 / B), while the weight gradients still sum a different g per row over every chunk.
    cnn-hot: 80 % of the tokens PAD / EOS (the hot rows of the embedding scatter), an all-PAD pair, a pair of one repeated id."""
    B, T, V, N = c["B"], c["T"], c["V"], c["N"]
    if c["batch"] == "tiled":
        D = c["distinct"]
        assert D <= 24
        src = _ids(rng, D, T, V)[np.arange(B) % D]
        tgt = rng.randint(0, N, size=B).astype(np.int32)
        return src, tgt, (rng.uniform(size=B) < 0.5).astype(np.float32)
    half = _ids(rng, B // 2, T, V)
    hot = rng.uniform(size=half.shape) < 0.8
    half[hot] = rng.randint(0, 2, size=int(hot.sum()))
    half[0] = 0
    half[2] = 9
    src = np.repeat(half, 2, axis=0)
    tgt = rng.randint(0, N, size=B).astype(np.int32)
    return src, tgt, np.tile(np.array([1.0, 0.0], np.float32), B // 2)


def cnn_min_positive_pool(params, src, bf16):
    """Smallest strictly positive pooled feature (inf if there is none): a feature that is 1e-8 here and 0 on the device (or
    the reverse) switches a whole window of gradient on or off."""
    pool = O.cnn_forward(params, np.unique(src, axis=0), bf16=bf16)
    return float(pool[pool > 0].min()) if (pool > 0).any() else np.inf


def cnn_dead_share(params, src, bf16):
    """Share of the pooled features that are exactly 0 (ReLU closed at every position)."""
    return float(np.mean(O.cnn_forward(params, src, bf16=bf16) == 0))


def cnn_min_pool_gap(params, src, bf16):
    """Smallest (best - second best) over every sequence and filter whose pooled value is > 0, second best taken over the
    positions whose value differs from the best (bit-equal values come from equal windows: the same gradient either way).
    Taken over the distinct sequences: a sequence's pooling does not depend on its batch."""
    _, tape = O.cnn_forward(params, np.unique(src, axis=0), keep_tape=True, bf16=bf16)
    gap = np.inf
    for _, hconv in tape:
        h = hconv.astype(np.float64)
        best = h.max(axis=1)
        second = np.where(h < best[:, None], h, -np.inf).max(axis=1)
        live = best > 0
        if live.any():
            gap = min(gap, float((best - second)[live].min()))
    return gap


def cnn_preconditions(c, p, src):
    """What makes the comparison meaningful in CNN mode (asserted here and in the CPU self-test): float32 and float64 agree on
    which position wins every max-pool and on whether the winner is above 0; and the share of dead features the case is for."""
    if c["mode"] != "source_only_cnn":
        return
    bf16 = bool(c["opts"].get("cnn_bf16"))
    assert cnn_min_pool_gap(p, src, bf16) > 1e-5
    assert cnn_min_positive_pool(p, src, bf16) > 1e-5
    if c.get("dead"):
        lo, hi = c["dead"]
        assert lo <= cnn_dead_share(p, src, bf16) <= hi


def case_bars(c):
    return c.get("bars") or (GRAD_BARS_SPLIT if c["split"] else GRAD_BARS_EXACT)


def _model(c):
    import sse_amd
    params, p = case_params(c)
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    for k, v in c["opts"].items():
        m.handle.set_option(k, v)
    return params, m, p


def case_arena(c, m, src, tgt, z, rows_global):
    """The raw arena of the case's batch: sse_train_grads, or -- by_rows -- sse_train_grads_rows on uploaded, shuffled corpora."""
    if not c["by_rows"]:
        return arena_grads(m, src, tgt, z, rows_global)
    B = len(z)
    order = np.random.RandomState(5).permutation(B).astype(np.int32)
    inv = np.argsort(order).astype(np.int32)        # row numbers into the shuffled corpora that give back the batch
    src_rows = inv
    if c.get("pair_rows"):                          # a source corpus of the B / 2 distinct sequences: rows 2i, 2i + 1 share a number
        assert np.array_equal(src[0::2], src[1::2])
        half = np.random.RandomState(6).permutation(B // 2).astype(np.int32)
        m.handle.corpus_upload(0, src[0::2][half])
        src_rows = np.repeat(np.argsort(half).astype(np.int32), 2)
    else:
        m.handle.corpus_upload(0, src[order])
    if tgt.ndim == 2:
        m.handle.corpus_upload(1, tgt[order])
        return arena_grads(m, src_rows, inv, z, rows_global, rows=True)
    return arena_grads(m, src_rows, tgt, z, rows_global, rows=True)   # table modes: the target side stays row numbers of the free matrix


@pytest.mark.parametrize("c", CASES)
def test_raw_gradients_and_apply_match_float64(c):
    params, m, p = _model(c)
    src, tgt, z = case_batch(c)
    B = len(z)
    rows_global = c["rows_factor"] * B
    cnn_bf16 = bool(c["opts"].get("cnn_bf16"))
    cnn_preconditions(c, p, src)
    bars = case_bars(c)
    want, want_tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=cnn_bf16)
    got, tail = case_arena(c, m, src, tgt, z, rows_global)
    errs = check_grads(got, want, bars, what="%s: " % c["id"], var_bars=c.get("var_bars"))
    check_tail(tail, want_tail, bars, LOSS_REL_SPLIT if c["opts"].get("train_fwd_x3") else LOSS_REL_EXACT)
    if c.get("dead") == (1.0, 1.0):                 # nothing alive: the clamp's 1e6 slope reaches only masked features
        for name in want:
            assert not want[name].any() and not np.asarray(got[name]).any(), name
    # rows of the lookup tables that the batch never touches: exactly zero
    touched = {"word_embedding": np.unique(np.concatenate([src.ravel(), tgt.ravel()]) if tgt.ndim == 2 else src.ravel())}
    if "target_embedding/tgt_seq_embedding" in got:
        touched["target_embedding/tgt_seq_embedding"] = np.unique(tgt)
    for name, ids in touched.items():
        untouched = np.setdiff1d(np.arange(got[name].shape[0]), ids)
        assert len(untouched) > 0 and not got[name][untouched].any(), name
    # sse_train_apply on its own: float64 clip + Adagrad of the device's own arena
    before = m.get_variables(with_slots=True)
    names = [n for n, _, _, _ in m.handle.variables()]
    wv, ws = reference_apply(got, tail, {n: before[n] for n in names}, {n: before[n + "/Adagrad"] for n in names},
                             m.handle.learning_rate)
    loss, acc = m.handle.train_apply()
    assert (loss, acc) == (float(tail[1]), float(tail[2]))
    after = m.get_variables(with_slots=True)
    worst_apply = 0.0
    for n in names:
        for have, ref, what in ((after[n], wv[n], n), (after[n + "/Adagrad"], ws[n], n + "/Adagrad")):
            d = np.abs(have.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
            worst_apply = max(worst_apply, float(d.max()))
            assert d.max() <= 1e-6, (what, float(d.max()))
    rel_name = max(errs, key=lambda n: errs[n][0])
    elem_name = max(errs, key=lambda n: errs[n][1])
    print("GRADERR %s bars %.0e/%.0e: norm %.2e (%s), element %.2e (%s), apply %.2e"
          % (c["id"], bars[0], bars[1], errs[rel_name][0], rel_name, errs[elem_name][1], elem_name, worst_apply))


BAD_ID_CASES = [
    pytest.param(("dual-encoder", 300, 50, 128, 128, 64, 10, 64, {}, "src"), id="fused"),
    pytest.param(("dual-encoder", 300, 50, 128, 128, 64, 10, 64, {"train_gen1": 1}, "tgt"), id="gen1"),
    pytest.param(("dual-encoder", 300, 50, 128, 128, 64, 10, 64, {"train_generic": 1}, "src"), id="generic-forced"),
    pytest.param(("dual-encoder", 200, 70, 96, 96, 64, 6, 16, {}, "tgt"), id="generic-e70"),
    pytest.param(("shared-encoder", 200, 50, 300, 300, 64, 6, 16, {}, "src"), id="generic-h300"),
    pytest.param(("source-encoder-only", 200, 50, 128, 128, 64, 12, 40, {}, "row"), id="source-only-row"),
    pytest.param(("source-encoder-only", 90, 70, 64, 64, 40, 6, 10, {}, "row"), id="source-only-generic-row"),
    pytest.param(("source_only_cnn", 90, 24, 96, 96, 64, 20, 10, {}, "src"), id="cnn"),
]


@pytest.mark.parametrize("case", BAD_ID_CASES)
def test_train_grads_reports_a_bad_id_on_every_path(case):
    """sse_train_grads with a token id (or free-target-matrix row) out of range fails on every path -- the any-shape path
    used to return success and leave the failure to that rank's sse_train_apply, so data-parallel replicas diverged.  No
    gradients are then pending (sse_train_apply changes nothing), and the next good call gives the right arena."""
    import sse_amd
    mode, V, E, Hs, Ht, S, T, B, opts, where = case
    c = dict(id="bad-id", mode=mode, V=V, E=E, Hs=Hs, Ht=Ht, S=S, T=T, B=B, N=13, batch="paired", opts=opts, seed=1)
    params, m, p = _model(c)
    src, tgt, z = case_batch(c)
    bad_src, bad_tgt = src.copy(), tgt.copy()
    if where == "src":
        bad_src[3, T - 2] = V
    elif where == "tgt":
        bad_tgt[B - 1, 0] = V
    else:
        bad_tgt[5] = c["N"]
    before = m.get_variables(with_slots=True)
    with pytest.raises(sse_amd.SSEError, match="out of range"):
        arena_grads(m, bad_src, bad_tgt, z)
    with pytest.raises(sse_amd.SSEError):
        m.handle.train_apply()
    after = m.get_variables(with_slots=True)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    want, want_tail = reference_grads(p, params, src, tgt, z)
    got, tail = arena_grads(m, src, tgt, z)
    check_grads(got, want, GRAD_BARS_EXACT)
    check_tail(tail, want_tail, GRAD_BARS_EXACT, LOSS_REL_EXACT)


@pytest.mark.parametrize("bf16,start", [(False, 150), (True, 300)], ids=["fp32", "bf16"])
def test_largest_accepted_cnn_shape_matches_float64(bf16, start):
    """E = 64 (the training limit): T walked down from one the library rejects to the first it accepts -- the boundary is the
    library's, not restated here.  A rejection is a host-side check whose message names LDS, never a launch error.  At the
    accepted T (every LDS tile of the training forward and of cnn_dw_kernel<0,*> as full as it gets) the raw gradients are held
    to the exact bar like any other case; the seed is the first whose batch meets the near-tie preconditions, and the float32
    oracle has to be 10x inside the bar there, as tests/test_grad_check.py asserts for the listed cases."""
    import sse_amd
    c = dict(id="cnn-largest-%s" % ("bf16" if bf16 else "fp32"), mode="source_only_cnn", V=150, E=64, Hs=96, Ht=96, S=32, B=6,
             N=17, batch="paired", opts=dict(cnn_bf16=1) if bf16 else {}, split=False, rows_factor=1, by_rows=False, seed=0)
    rejected = 0
    for T in range(start, 4, -1):
        c["T"] = T
        params, m, p = _model(c)
        src, tgt, z = case_batch(c)
        try:
            arena_grads(m, src, tgt, z)
        except sse_amd.SSEError as e:
            assert "LDS" in str(e), str(e)
            rejected += 1
            continue
        break
    assert rejected > 0, "T = %d was expected to be rejected" % start
    print("largest accepted T for E = 64 (%s): %d" % ("bf16" if bf16 else "fp32", T))
    for seed in range(16):
        c["seed"] = seed
        params, p = case_params(c)
        src, tgt, z = case_batch(c)
        if cnn_min_pool_gap(p, src, bf16) > 1e-5 and cnn_min_positive_pool(p, src, bf16) > 1e-5:
            break
    cnn_preconditions(c, p, src)
    want, want_tail = reference_grads(p, params, src, tgt, z, cnn_bf16=bf16)
    f32, f32_tail = reference_grads(p, params, src, tgt, z, cnn_bf16=bf16, float64=False)
    check_grads(f32, want, (GRAD_BARS_EXACT[0] / 10, GRAD_BARS_EXACT[1] / 10), what="float32 oracle: ")
    params, m, p = _model(c)
    got, tail = arena_grads(m, src, tgt, z)
    errs = check_grads(got, want, GRAD_BARS_EXACT, what="%s T %d: " % (c["id"], T))
    check_tail(tail, want_tail, GRAD_BARS_EXACT, LOSS_REL_EXACT)
    rel_name = max(errs, key=lambda n: errs[n][0])
    elem_name = max(errs, key=lambda n: errs[n][1])
    print("GRADERR %s T %d seed %d: norm %.2e (%s), element %.2e (%s)"
          % (c["id"], T, seed, errs[rel_name][0], rel_name, errs[elem_name][1], elem_name))
