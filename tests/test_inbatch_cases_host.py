"""CPU self-test of tests/inbatch_cases.py: the float64 head against torch autograd, the float32 restatement against the bars
of every case (10x margin), planted defects, the accuracy precondition, and the C ABI surface of the feature."""
import os
import re

import numpy as np
import pytest

from tests import inbatch_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sequence-semantic-embedding_amd")


@pytest.mark.parametrize("c", IC.HEAD_CASES, ids=[c["id"] for c in IC.HEAD_CASES])
def test_float64_head_equals_torch_autograd(c):
    """Masked logsumexp on normalised rows, differentiated by torch in float64: loss terms and both gradients within 1e-12."""
    import torch
    x = IC.head_case_seeded(c)
    want = IC.head_want(x)
    s = torch.tensor(x["s"], dtype=torch.float64, requires_grad=True)
    t = torch.tensor(x["t"], dtype=torch.float64, requires_grad=True)
    z = torch.tensor(x["z"], dtype=torch.float64)

    def normalize(v):
        return v / torch.sqrt(torch.clamp((v * v).sum(dim=1, keepdim=True), min=1e-12))
    L = x["scale"] * normalize(s) @ normalize(t).T
    adm = torch.tensor(IC.admitted(x["z"], x["ks"], x["kt"]))
    lse = torch.logsumexp(torch.where(adm, L, torch.full_like(L, -float("inf"))), dim=1)
    row_loss = z * (lse - torch.diagonal(L))
    (x["inv_rows"] * row_loss.sum()).backward()

    def close(got, ref, what):
        scale = max(1.0, float(np.abs(ref).max()))
        assert float(np.abs(got - ref).max()) <= 1e-12 * scale, (c["id"], what, float(np.abs(got - ref).max()), scale)
    close(want["row_loss"], row_loss.detach().numpy(), "row_loss")
    close(want["d_src"], s.grad.numpy(), "d_src")
    close(want["d_tgt"], t.grad.numpy(), "d_tgt")


def _own_bars_are_10x_the_recorded_error(c, default):
    """A bar of the case's own is 10 x its recorded restatement error, rounded up (at most 13 x), never wider."""
    for k in (0, 1):
        if c["bars"][k] != default[k]:
            assert c["f32_err"] is not None and default[k] < c["bars"][k] <= 13 * c["f32_err"][k], (c["id"], k)


@pytest.mark.parametrize("c", IC.HEAD_CASES, ids=[c["id"] for c in IC.HEAD_CASES])
def test_float32_restatement_is_10x_inside_the_head_bars(c):
    x = IC.head_case_seeded(c)
    want = IC.head_want(x)
    f32 = IC.head(x["s"], x["t"], x["z"], x["ks"], x["kt"], x["scale"], x["inv_rows"], dtype=np.float32)
    rel, elem = IC.head_errors(f32, want)
    print("F32ERR head %s: norm %.3g element %.3g (bars %.1e / %.1e)" % (c["id"], rel, elem, c["bars"][0], c["bars"][1]))
    IC.check_head(f32, want, c, bars=(c["bars"][0] / 10, c["bars"][1] / 10), what="float32 restatement: ")
    _own_bars_are_10x_the_recorded_error(c, IC.GRAD_BARS_EXACT)


@pytest.mark.parametrize("c", IC.STEP_CASES, ids=[c["id"] for c in IC.STEP_CASES])
def test_float32_restatement_is_10x_inside_the_step_bars(c):
    params, p, src, tgt, z, want, want_tail, _ = IC.step_case_seeded(c)
    f32, f32_tail, _ = IC.step_reference(p, params, src, tgt, z, c["rows_factor"] * len(z), c["scale"], float64=False)
    errs = IC.check_grads(f32, want, (np.inf, np.inf))
    print("F32ERR step %s: norm %.3g element %.3g" % (c["id"], max(e[0] for e in errs.values()), max(e[1] for e in errs.values())))
    IC.check_grads(f32, want, (c["bars"][0] / 10, c["bars"][1] / 10), what="float32 restatement %s: " % c["id"])
    _own_bars_are_10x_the_recorded_error(c, IC.GRAD_BARS_SPLIT if c["split"] else IC.GRAD_BARS_EXACT)
    print("F32ERR step %s: loss %.3g rel" % (c["id"], abs(f32_tail[1] - want_tail[1]) / abs(want_tail[1])))
    assert abs(f32_tail[1] - want_tail[1]) <= IC.LOSS_REL_EXACT / 10 * abs(want_tail[1]) + 1e-8
    assert abs(f32_tail[2] - want_tail[2]) <= 1e-7


def test_accuracy_precondition_holds_on_every_row_of_every_case():
    for c in IC.HEAD_CASES:
        x = IC.head_case_seeded(c)
        assert IC.min_accuracy_gap(x["s"], x["t"], x["z"], x["ks"], x["kt"], x["scale"]) >= IC.accuracy_gap_bound(x["scale"], c["S"]), c["id"]
    for c in IC.STEP_CASES:
        IC.step_case_seeded(c)                     # raises when no seed meets it


PLANTED = [("equal-targets-unmasked", "b33-s64"), ("same-source-unmasked", "same-source-pairs"), ("label0-row-has-loss", "b33-s64"),
           ("label0-column-dropped", "b33-s64"), ("no-delta", "b33-s64"), ("mean-over-active", "b33-s64"),
           ("no-max-subtraction", "s-equals-t-scale256"), ("clamp-ignored", "zero-rows"), ("tail-columns-admitted", "all-logits-negative")]


@pytest.mark.parametrize("defect,cid", PLANTED, ids=[d for d, _ in PLANTED])
def test_planted_defect_is_rejected(defect, cid):
    assert defect in IC.DEFECTS
    c = IC.HEAD_CASES_BY_ID[cid]
    x = IC.head_case_seeded(c)
    want = IC.head_want(x)
    IC.check_head(want, want, c)                   # the check itself passes on the definition
    # (exp(256) is finite in float64: the missing maximum shows in the arithmetic the kernel uses)
    dtype = np.float32 if defect == "no-max-subtraction" else np.float64
    bad = IC.head(x["s"], x["t"], x["z"], x["ks"], x["kt"], x["scale"], x["inv_rows"], dtype=dtype, defect=defect)
    with pytest.raises(AssertionError):
        IC.check_head(bad, want, c)


def test_every_listed_defect_is_planted():
    assert sorted(d for d, _ in PLANTED) == sorted(IC.DEFECTS)


def test_head_shapes_cover_the_listed_sizes():
    assert {1, 2, 31, 33, 65, 100} <= {c["B"] for c in IC.HEAD_CASES}
    assert {1, 3, 64, 130} <= {c["S"] for c in IC.HEAD_CASES}


def test_sse_train_flags_and_trainer_option_pass_through():
    from sse_amd import sse_train
    f = sse_train.FLAGS.parse([])
    assert (f.loss, f.loss_scale) == ("pair", 64)
    f = sse_train.FLAGS.parse(["--loss", "inbatch", "--loss_scale=32"])
    assert (f.loss, f.loss_scale) == ("inbatch", 32)

    class Engine:                                   # what DataParallelTrainer needs of a handle, recording its options
        def __init__(self):
            self.options = {}

        def set_option(self, name, value):
            self.options[name] = value

        def train_grad_count(self):
            return 8

        def train_bind_arena(self, arena):
            self.arena = arena
    import sse_amd
    eng = Engine()
    sse_amd.DataParallelTrainer(eng, options={"train_loss": 1, "train_loss_scale": 32})
    assert eng.options == {"train_loss": 1, "train_loss_scale": 32}
    eng = Engine()
    sse_amd.DataParallelTrainer(eng)
    assert eng.options == {}


def test_symbol_and_options_exist_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "sse_hip.h")).read()
    assert re.search(r"\bint\s+sse_inbatch_loss_dev\s*\(", header)
    for word in ('"train_loss"', '"train_loss_scale"', '"train_inbatch_steps"'):
        assert word in header, word
    lib = os.path.join(PKG, "libsse_hip.so")
    assert os.path.exists(lib), "libsse_hip.so is not built"
    blob = open(lib, "rb").read()
    for word in (b"sse_inbatch_loss_dev", b"train_loss must be 0 (pair) or 1 (in-batch softmax)", b"train_loss_scale", b"train_inbatch_steps"):
        assert word in blob, word
    import sse_amd
    assert "sse_inbatch_loss_dev" in sse_amd.SYMBOLS
    assert hasattr(sse_amd.load_library(), "sse_inbatch_loss_dev")
    assert hasattr(sse_amd.Handle, "inbatch_loss_dev")
