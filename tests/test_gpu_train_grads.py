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
                        check_tail, make_pair, model_params, oracle_params, random_ids, reference_apply, reference_grads)

pytestmark = pytest.mark.gpu


def _case(cid, mode, V, E, Hs, Ht, S, T, B, N=13, batch="paired", opts=None, rows_factor=1, by_rows=False, seed=0):
    opts = dict(opts or {})
    split = any(opts.get(k) for k in ("train_fwd_x3", "train_bwd_x3", "train_dk_x3"))
    return pytest.param(dict(id=cid, mode=mode, V=V, E=E, Hs=Hs, Ht=Ht, S=S, T=T, B=B, N=N, batch=batch, opts=opts, split=split,
                             rows_factor=rows_factor, by_rows=by_rows, seed=seed), id=cid)


def _x3(fwd, bwd, dk):
    return dict(train_fwd_x3=fwd, train_bwd_x3=bwd, train_dk_x3=dk)


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
    # BPTT edges, repeated / hot ids (dx_hot_reduce, the atomics scatter), labels all 1
    _case("t1", "dual-encoder", 100, 16, 64, 64, 32, 1, 64),
    _case("t2", "shared-encoder", 100, 16, 64, 64, 32, 2, 64),
    _case("edges", "dual-encoder", 300, 50, 128, 128, 64, 10, 128, batch="edges"),
    _case("hot-ids", "dual-encoder", 300, 50, 128, 96, 64, 12, 128, batch="hot"),
    _case("labels-1", "shared-encoder", 300, 40, 96, 96, 64, 10, 64, batch="ones"),
    # this rank's share of a mean over 3 B rows; batches by row number from uploaded corpora (device id gather)
    _case("rows-global-3b", "dual-encoder", 300, 50, 128, 128, 64, 10, 64, rows_factor=3),
    _case("by-rows", "dual-encoder", 300, 50, 128, 128, 64, 10, 64, by_rows=True),
]


def case_params(c):
    """(model params, oracle parameter dict) of a case: what make_pair loads into the GPU model."""
    params = model_params(c["mode"], c["V"], c["E"], c["Hs"], c["Ht"], c["S"], c["T"], N=c["N"], lr=0.9)
    return params, oracle_params(params, seed=3 + c["seed"])


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
    src = _ids(rng, B, T, V) if kind == "unpaired" else np.repeat(_ids(rng, B // 2, T, V), 2, axis=0)
    if c["mode"] in ("source-encoder-only", "source_only_cnn"):
        tgt = rng.randint(0, c["N"], size=B).astype(np.int32)
    else:
        tgt = _ids(rng, B, T, V)
    z = np.tile(np.array([1.0, 0.0], np.float32), B // 2)
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


def cnn_min_pool_gap(params, src, bf16):
    """Smallest (best - second best) over every sequence and filter whose pooled value is > 0, second best taken over the
    positions whose value differs from the best (bit-equal values come from equal windows: the same gradient either way)."""
    _, tape = O.cnn_forward(params, src, keep_tape=True, bf16=bf16)
    gap = np.inf
    for _, hconv in tape:
        h = hconv.astype(np.float64)
        best = h.max(axis=1)
        second = np.where(h < best[:, None], h, -np.inf).max(axis=1)
        live = best > 0
        if live.any():
            gap = min(gap, float((best - second)[live].min()))
    return gap


def _model(c):
    params, _ = case_params(c)
    m, p = make_pair(params, seed=3 + c["seed"])
    for k, v in c["opts"].items():
        m.handle.set_option(k, v)
    return params, m, p


@pytest.mark.parametrize("c", CASES)
def test_raw_gradients_and_apply_match_float64(c):
    params, m, p = _model(c)
    src, tgt, z = case_batch(c)
    B = len(z)
    rows_global = c["rows_factor"] * B
    cnn_bf16 = bool(c["opts"].get("cnn_bf16"))
    if c["mode"] == "source_only_cnn":
        assert cnn_min_pool_gap(p, src, cnn_bf16) > 1e-5
    bars = GRAD_BARS_SPLIT if c["split"] else GRAD_BARS_EXACT
    want, want_tail = reference_grads(p, params, src, tgt, z, rows_global, cnn_bf16=cnn_bf16)
    if c["by_rows"]:
        order = np.random.RandomState(5).permutation(B).astype(np.int32)
        inv = np.argsort(order).astype(np.int32)    # row numbers into the shuffled corpora that give back the batch
        m.handle.corpus_upload(0, src[order])
        m.handle.corpus_upload(1, tgt[order])
        got, tail = arena_grads(m, inv, inv, z, rows_global, rows=True)
    else:
        got, tail = arena_grads(m, src, tgt, z, rows_global)
    errs = check_grads(got, want, bars, what="%s: " % c["id"])
    check_tail(tail, want_tail, bars, LOSS_REL_SPLIT if c["opts"].get("train_fwd_x3") else LOSS_REL_EXACT)
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
