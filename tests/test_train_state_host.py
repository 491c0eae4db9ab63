"""tests/train_state_script.py can see what it is for (CPU).  The runner drives TrainStateModel, the numpy model of the
handle's training interface: the clean model passes every step of every script; every step that follows a weight change is
sensitive enough that a stale layout could not pass the gradient bars (the runner's _check_sensitivity: the gradient at the
previous weights is at least 100 bars from the current one, in both measures, for every variable a stale layout feeds); every
planted defect -- one stale piece of per-handle training state each -- is rejected, at the step named here; and the counter
deltas the GPU test expects, which the clean model produces, agree with a table written by hand for fused-dual."""
import numpy as np
import pytest

from tests import train_state_script as TS
from tests.test_gpu_train_grads import cnn_min_pool_gap, cnn_min_positive_pool
from tests.util import check_grads, reference_grads


def _run(script, defect=None, sensitivity=False, name="host"):
    cfg, seed, steps, marks = script
    return TS.Runner(TS.TrainStateModel(cfg, seed, defect), cfg, seed, name=name, sensitivity=sensitivity).run(steps)


def _rejected(script, defect):
    with pytest.raises(TS.StepFailed) as e:
        _run(script, defect)
    return e.value


@pytest.mark.parametrize("name", list(TS.SCRIPTS))
def test_clean_model_passes_and_every_step_after_a_weight_change_is_sensitive(name):
    for script in TS.SCRIPTS[name]():
        r = _run(script, sensitivity=True, name=name)
        assert len(r.done) == len(script[2])
        assert r.worst["least_sensitive"] >= TS.SENSITIVITY          # (asserted per variable and step by the runner)
        assert r.worst["f32_oracle"] <= 0.1                          # the float32 oracle 10x inside the bars at every step
        assert r.worst["rel"][0] <= 1e-12 and r.worst["apply"] <= 1e-7 # the model against itself: float64 and one float32 rounding


def test_scripts_reach_the_branches_they_are_for():
    def routes(script):
        cfg, seed, steps, _ = script
        m, out = TS.TrainStateModel(cfg, seed), []
        r = TS.Runner(m, cfg, seed)
        for st in steps:
            r.step(st)
            if st.kind in TS.TRAIN_CALLS:
                out.append((st, dict(r.truth.last_route)))
        return out
    for script in (TS.fused_dual_script(), TS.fused_shared_script()):
        rs = routes(script)
        assert all(r["path"] == "fused" for _, r in rs)
        assert any(r["paired"] for _, r in rs) and any(not r["paired"] for _, r in rs)
        assert any(r["all_x3"] for _, r in rs) and any(r["bwd2"] for _, r in rs)
        assert any(r["any_bwd_x3"] and not r["all_x3"] for _, r in rs)                       # fp32 forward, split BPTT
        assert any(r["split"] and not r["any_bwd_x3"] for _, r in rs)                        # the weight gradient alone
        assert any(not r["bwd2"] and not r["split"] for _, r in rs)                          # first generation
        assert {st.batch.B % 64 != 0 for st, _ in rs} == {True, False}                       # padding rows, and none
        assert {st.batch.T for st, _ in rs} == {1, 5, 12, 20}
    a, b = TS.generic_scripts()
    assert [r["path"] for _, r in routes(a)] == ["fused", "generic", "fused", "generic", "generic", "generic", "fused"]
    assert all(r["path"] == "generic" for _, r in routes(b))
    assert all(r["path"] == "cnn" for _, r in routes(TS.cnn_script()))
    rs = routes(TS.by_rows_script())
    assert [r["paired"] for _, r in rs] == [True, False, False, False, False, True]
    rs = routes(TS.table_target_script())
    assert [r["paired"] for _, r in rs][:4] == [True, False, True, True]


def test_mixed_grads_without_stale_layouts_is_reference_grads():
    for script in (TS.fused_dual_script(), TS.fused_shared_script(), TS.table_target_script()):
        cfg, seed, steps, _ = script
        m = TS.TrainStateModel(cfg, seed)
        b = next(st for st in steps if st.kind == "grads").batch
        for rg in (b.B, 3 * b.B):
            want, want_tail = reference_grads(m.w, cfg, b.src, b.tgt, b.z, rg)
            got, tail = TS.mixed_grads(m.w, cfg, b.src, b.tgt, b.z, rg)
            check_grads(got, want, (1e-12, 1e-12))
            assert np.allclose(tail, want_tail, rtol=1e-12, atol=0)


def test_cnn_seeds_meet_the_preconditions_with_margin():
    """CNN_SEEDS are the first seeds find_cnn_seeds accepts, and every batch of the script meets the near-tie preconditions at
    the weights the clean model holds then, with twice the room the runner asks for at the driver's weights"""
    assert tuple(TS.find_cnn_seeds()) == tuple(TS.CNN_SEEDS)
    cfg, seed, steps, _ = TS.cnn_script()
    r = TS.Runner(TS.TrainStateModel(cfg, seed), cfg, seed)
    checked = 0
    for st in steps:
        if st.kind in TS.TRAIN_CALLS:
            bf16 = bool(r.truth.opts["cnn_bf16"])
            assert cnn_min_pool_gap(r.truth.w, st.batch.src, bf16) > 2e-5 and cnn_min_positive_pool(r.truth.w, st.batch.src, bf16) > 2e-5
            checked += 1
        r.step(st)
    assert checked == 10


def test_expected_counter_deltas_of_fused_dual_match_the_hand_written_table():
    cfg, seed, steps, marks = TS.fused_dual_script()
    r = _run((cfg, seed, steps, marks))
    calls = [i for i, st in enumerate(steps) if st.kind in TS.TRAIN_CALLS + ("apply", "encode", "eval_loss", "refused")]
    assert len(calls) == len(r.deltas)
    by_step = {i + 1: d for i, d in zip(calls, r.deltas)}
    for mark, off, want in TS.FUSED_DUAL_DELTAS:
        n = marks[mark] + off
        assert steps[n - 1].kind in TS.TRAIN_CALLS or steps[n - 1].kind == "refused", (mark, off, steps[n - 1])
        assert by_step[n] == dict(dict.fromkeys(TS.TRAIN_COUNTERS, 0), **want), (mark, off, steps[n - 1], by_step[n])
    # and no call but a train call moves a counter
    for n, d in by_step.items():
        if steps[n - 1].kind in ("apply", "encode", "eval_loss") or (steps[n - 1].kind == "refused" and steps[n - 1].step.kind == "apply"):
            assert not any(d.values()), (n, steps[n - 1])


# ---- planted defects: (defect, script, the mark and offset of the step that must reject it, a piece of the message)

def _generic(i):
    return lambda: TS.generic_scripts()[i]


PLANTED = [
    ("fp32_stale_after_split_step", TS.fused_dual_script, "fp32_two_updates_old", 3, "against the float64 oracle"),
    ("split_not_rebuilt_after_fp32_step", TS.fused_dual_script, "bwd_split_same_weights", 1, "against the float64 oracle"),
    ("generic_packs_survive_set_vars", _generic(0), "set_vars", 1, "against the float64 oracle"),
    ("generic_packs_survive_set_vars", _generic(1), "set_vars", 1, "against the float64 oracle"),
    ("perm_of_previous_B", TS.fused_dual_script, "paired_b256", 0, "against the float64 oracle"),
    ("table_rows_not_permuted", TS.table_target_script, "paired_after_unpaired", 0, "against the float64 oracle"),
    ("corpus_N_kept", TS.by_rows_script, "row_out_of_range", 0, "was accepted"),
    ("corpus_T_kept", TS.by_rows_script, "t5", 0, "against the float64 oracle"),
    ("cancelled_leaves_pending", TS.fused_dual_script, "apply_after_cancelled", 0, "was accepted"),
    ("padding_rows_enter", TS.fused_dual_script, "unpaired_b70", 0, "against the float64 oracle"),
    ("padding_rows_enter", _generic(1), "b6_t5_again", 0, "against the float64 oracle"),
    ("eval_overwrites_pending", TS.fused_dual_script, "pending_survives", 3, "the bound arena's bytes changed"),
    ("table_grad_not_zeroed", TS.fused_dual_script, "unpaired_b70", 0, "word_embedding"),
    ("table_grad_not_zeroed", TS.table_target_script, "unpaired", 0, "against the float64 oracle"),
    ("unbind_leaves_pointers", TS.arena_script, "fresh_internal", 0, "the external arena B is not bound and its bytes changed"),
]


@pytest.mark.parametrize("defect,script,mark,off,text", PLANTED, ids=["%s-%d" % (p[0], i) for i, p in enumerate(PLANTED)])
def test_planted_defect_is_rejected_at_its_step(defect, script, mark, off, text):
    s = script()
    f = _rejected(s, defect)
    assert f.number == s[3][mark] + off, (f.number, str(f)[:400])
    assert text in str(f), str(f)[:600]
    assert " step %d " % f.number in str(f) and "opts" in str(f) and "route" in str(f)       # what a failure names


def test_the_weight_copies_a_defect_leaves_stale_are_the_ones_its_step_reads():
    """fp32_stale_after_split_step and split_not_rebuilt_after_fp32_step are rejected by the gradient, not by a counter: the
    defective model reports the counters of the clean one"""
    for defect, mark, off in (("fp32_stale_after_split_step", "fp32_two_updates_old", 3), ("split_not_rebuilt_after_fp32_step", "bwd_split_same_weights", 1)):
        cfg, seed, steps, marks = TS.fused_dual_script()
        m = TS.TrainStateModel(cfg, seed, defect)
        clean = TS.TrainStateModel(cfg, seed)
        for st in steps[:marks[mark] + off]:
            for model in (m, clean):
                if st.kind == "set_option":
                    model.set_option(st.name, st.value)
                elif st.kind == "bind_arena":
                    model.bind_arena(st.arena)
                elif st.kind == "set_vars":
                    model.set_variables(TS.scaled_variables(cfg, model.variables(), st.which))
                else:
                    try:
                        model.call(st.step if st.kind == "refused" else st)
                    except TS.Refused:
                        pass
        assert m.last_delta == clean.last_delta
        which = "fp32" if defect.startswith("fp32") else "split"
        assert m.lay[which] is not m.w and clean.lay[which] is clean.w


def test_every_defect_has_a_test():
    assert {p[0] for p in PLANTED} == set(TS.DEFECTS) and len(TS.DEFECTS) >= 12
