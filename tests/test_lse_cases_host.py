"""CPU proof of tests/lse_cases.py, the yardstick of sse_score_lse (DESIGN K6m): the numpy model of the kernel's arithmetic
passes check() on every case, every planted defect is rejected by a named case, the float32-dot restatement uses at most a
tenth of the dot bound (so the GPU bar has room and still means something), and the pure helpers built on the call --
softmax_probs, softmax_nll_from, merge_lse_lists -- equal their direct float64 formulas."""
import os

import numpy as np
import pytest

from tests import lse_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the case that rejects each planted defect
DEFECT_CASE = {
    "pad_counted": "n33",
    "none_ignored": "tags_none_only",
    "any0_nothing": "tags_mixed",
    "bias_dropped": "bias_mixed",
    "bias_outside_scale": "bias_mixed",
    "split_dropped": "two_splits",
    "merge_adds_logs": "two_splits",
    "no_reference": "scale256",
    "empty_nan": "tags_mixed",
    "bound_without_qnorm": "short_query",
}

# (the model costs a Python loop per tile: the two largest cases run on the GPU only)
MODEL_CASES = [c for c in LC.CASES if c.Q * c.N <= 400_000 and c.N <= 4000]


def test_cases_reach_what_they_claim():
    names = [c.name for c in LC.CASES]
    assert len(set(names)) == len(names)
    assert set(DEFECT_CASE) == set(LC.DEFECTS) and set(DEFECT_CASE.values()) <= set(names)
    for c in LC.CASES:
        if c.nsplit is not None:
            assert LC.nsplit_of(c.Q, c.N) == c.nsplit, (c, LC.nsplit_of(c.Q, c.N))
    assert LC.BY_NAME["two_splits"].nsplit > 1 and LC.BY_NAME["folded_decode"].nsplit > 8
    c = LC.BY_NAME["tags_mixed"]
    cnt = LC.reference(c)[1]
    assert cnt[0] == 0 and cnt[2] == 1 and LC.inputs(c)["any"][1] == 0 and 0 < cnt[1] < c.N
    assert LC.eligible(c)[2, c.N - 1] and c.N % 32 == 1                  # the one eligible row sits alone in the tail tile
    for name in ("bias_and_tags", "shard_f64", "shard_dev"):
        assert LC.reference(LC.BY_NAME[name])[1][0] == 0
    c = LC.BY_NAME["scale256"]
    z = LC.logits(c)
    assert z.max() > 89.0, "no logit of the case overflows exp in fp32"   # exp(88.7) = FLT_MAX
    a, d = LC.BY_NAME["ascending"], LC.BY_NAME["descending"]
    za = LC.logits(a)[0]
    assert (np.diff(za) >= 0).all() and (np.diff(LC.logits(d)[0]) <= 0).all()
    tile_max = za.reshape(-1, 32).max(1)
    assert (np.diff(np.ceil(tile_max * LC.LOG2E)) >= 0).all() and len(set(np.ceil(tile_max * LC.LOG2E))) > 10, "the reference hardly moves"
    assert np.abs(LC.reference(a)[0] - LC.reference(d)[0]).max() < 1e-9
    c = LC.BY_NAME["bias_log_prior"]
    I = LC.inputs(c)
    assert (I["bias"] < 0).all() and abs(np.exp(c.scale * I["bias"].astype(np.float64)).sum() - 1.0) < 1e-3
    assert (LC.inputs(LC.BY_NAME["bias_mixed"])["w"] < 0).any()
    c = LC.BY_NAME["tags_skip"]
    e = LC.eligible(c)
    assert (~e.reshape(c.Q, -1, 32).any(2).any(0)).sum() > 10, "no tile is skippable"


@pytest.mark.parametrize("case", MODEL_CASES, ids=repr)
def test_model_of_the_kernel_passes_check(case):
    used, over = LC.check(case, *LC.model(case))
    assert used <= 0.5, "%s: the model uses %.2f of its bound" % (case.name, used)


def test_model_is_independent_of_the_split_count():
    case = LC.BY_NAME["two_splits"]
    a, b = LC.model(case, nsplit=1), LC.model(case, nsplit=4)
    LC.check(case, *a)
    LC.check(case, *b)
    assert np.array_equal(a[1], b[1]) and np.abs(a[0] - b[0]).max() < 1e-6


@pytest.mark.parametrize("defect", LC.DEFECTS)
def test_planted_defect_is_rejected(defect):
    case = LC.BY_NAME[DEFECT_CASE[defect]]
    LC.check(case, *LC.model(case))
    with pytest.raises(AssertionError):
        LC.check(case, *LC.model(case, defect))


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_float32_dots_use_a_tenth_of_the_dot_bound(case):
    """the restatement with float32 dot products (and the fused bias in float32), reduced in float64"""
    I = LC.inputs(case)
    y = I["q"] @ np.asarray(I["t"]).astype(np.float32).T
    if I["w"] is not None:
        y = (y.astype(np.float64) + I["w"].astype(np.float64)[:, None] * I["bias"].astype(np.float64)[None, :]).astype(np.float32)
    got, cnt = LC.lse_of(case.scale * y.astype(np.float64), LC.eligible(case))
    want, wc = LC.reference(case)
    live = wc > 0
    assert np.array_equal(cnt, wc)
    err = np.abs(got[live] - want[live])
    d = LC.dot_bounds(case)[live]
    assert (err <= 0.1 * d).all(), "%s: float32 dots move the lse by %.3e, d_q = %.3e" % (case.name, err.max(), d[np.argmax(err / d)])


def test_softmax_probs_against_the_direct_formula():
    from sse_amd.sse_index import softmax_probs
    case = LC.BY_NAME["tags_mixed"]
    z, e = LC.logits(case), LC.eligible(case)
    lse, cnt = LC.reference(case)
    s = np.where(e, z / case.scale, -np.inf)                            # ineligible columns as padding
    p = softmax_probs(s, lse, case.scale)
    assert p.shape == s.shape and p.dtype == np.float64 and not np.isnan(p).any()
    assert (p[~e] == 0).all() and (p[0] == 0).all() and cnt[0] == 0
    live = cnt > 0
    assert np.abs(p[live].sum(1) - 1.0).max() < 1e-12
    assert abs(p[2].max() - 1.0) < 1e-12                                 # the only eligible row
    with np.errstate(under="ignore"):
        direct = np.exp(z - lse[:, None])
    assert np.abs(p[e] - direct[e]).max() < 1e-15


def test_softmax_nll_from_against_the_direct_formula():
    from sse_amd.sse_evaluator import softmax_nll_from
    rng = np.random.RandomState(5)
    scale = 64.0
    s = rng.uniform(-1, 1, (3, 40))
    lse = np.log(np.exp(scale * s).sum(1))
    labels = [[3, 17], [5], [0]]                                         # a source with two labels
    nll = softmax_nll_from(lse, [s[i, l] for i, l in enumerate(labels)], scale)
    for i, l in enumerate(labels):
        p = np.exp(scale * s[i]) / np.exp(scale * s[i]).sum()
        assert abs(nll[i] - -np.log(p[l].sum())) < 1e-10
    assert (nll > 0).all()
    # a label that is the only eligible row: nll = 0
    one = softmax_nll_from(np.array([scale * 0.37]), [np.array([0.37])], scale)
    assert one[0] == 0.0


def test_merge_lse_lists_three_uneven_shards():
    import torch
    from sse_amd.sharded import merge_lse_lists
    case = LC.BY_NAME["bias_and_tags"]
    z, e = LC.logits(case), LC.eligible(case)
    cuts = [0, 7, 200, case.N]                                           # three uneven shards
    ls, cs, bs = [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        l, c = LC.lse_of(z[:, a:b], e[:, a:b])
        ls.append(l)
        cs.append(c)
        bs.append(np.where(c > 0, 1e-4 * (1 + a), 0.0))
    # every shard perturbed by less than its own bound
    rng = np.random.RandomState(3)
    pert = [l + rng.uniform(-1, 1, case.Q) * b for l, b in zip(ls, bs)]
    lse, cnt, bound = merge_lse_lists(torch.from_numpy(np.stack(pert)), torch.from_numpy(np.stack(cs)), torch.from_numpy(np.stack(bs)))
    lse, cnt, bound = lse.numpy(), cnt.numpy(), bound.numpy()
    want, wc = LC.reference(case)
    assert np.array_equal(cnt, wc) and np.array_equal(lse == -np.inf, wc == 0) and not np.isnan(lse).any()
    live = wc > 0
    assert (np.abs(lse[live] - want[live]) <= bound[live]).all()
    assert (bound <= np.stack(bs).max(0) + 1e-12).all() and (bound >= np.stack(bs).max(0)).all()
    # unperturbed: the unsharded reference to float64 rounding
    exact = merge_lse_lists(torch.from_numpy(np.stack(ls)), torch.from_numpy(np.stack(cs)), torch.zeros(3, case.Q, dtype=torch.float64))
    assert np.abs(exact[0].numpy()[live] - want[live]).max() <= exact[2].numpy()[live].max() < 1e-12


def test_header_and_library_carry_the_call():
    hdr = open(os.path.join(ROOT, "include", "sse_hip.h")).read()
    for word in ("sse_score_lse(", "sse_score_lse_dev(", '"score_lse_calls"', '"score_lse_tiles_skipped"'):
        assert word in hdr, word
    import sse_amd
    assert "sse_score_lse" in sse_amd.SYMBOLS and "sse_score_lse_dev" in sse_amd.SYMBOLS
    for name in ("score_lse", "score_lse_dev"):
        assert hasattr(sse_amd._lib.Handle, name), name
    from sse_amd import sse_train
    assert sse_train.FLAGS.parse([]).eval_nll == 0
