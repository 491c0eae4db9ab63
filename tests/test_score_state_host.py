"""tests/score_state_script.py can see what it is for (CPU).  The runner drives StateOracle, the numpy model of the handle's
scoring interface: the clean model passes every step of transitions 1, 4, 6 (refused calls and refused uploads) and 7 (and the reference of every call of every
transition is one a device must reproduce id for id: preconditions()), and every planted defect -- one stale piece of
per-index state each -- is rejected, at the step named here."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests import score_state_script as SS
from tests import topk_cases as TC


def _run(steps, defect=None, preconditions=False, name="host"):
    return SS.Runner(SS.StateOracle(defect), name=name, check_preconditions=preconditions).run(steps)


def _calls(r):
    return sum(1 for st in r.done if st.kind == "call")


def test_clean_model_passes_the_replacement_chain():
    steps, where = SS.chain_script()
    r = _run(steps, preconditions=True)
    assert len(r.done) == len(steps) and _calls(r) >= 7 * len(SS.CHAIN)
    # Bu holds B's rows at another alignment: the same queries, the same results
    b, bu = where[SS.CHAIN.index("B")], where[SS.CHAIN.index("Bu")]
    assert b[1] - b[0] == bu[1] - bu[0]
    for i, j in zip(range(b[0], b[1] + 1), range(bu[0], bu[1] + 1)):
        assert SS.same_outputs(r.results[i - 1], r.results[j - 1]), (i, j)
    # D64 -> D32 changes the scores by what the oracle says (tests/test_gpu_score_large_k.py::
    # test_f64_rows_and_their_rounding_differ_on_the_device_as_in_the_oracle: more than 1e3 bars)
    d64, d32 = where[SS.CHAIN.index("D64")], where[SS.CHAIN.index("D32")]
    a, b = r.results[d64[0] - 1], r.results[d32[0] - 1]
    assert np.array_equal(a[1], b[1])
    assert np.abs(a[0] - b[0]).max() > 1e3 * TC.score_bar(TC.BY_NAME["f64_rows"])


def test_clean_model_passes_tags_and_groups():
    steps, info = SS.tags_script()
    r = _run(steps, preconditions=True)
    for group in info["same_as_topk"]:                       # calls without masks equal score_topk
        first = r.results[group[0] - 1]
        for j in group[1:]:
            assert SS.same_outputs(first[:2], r.results[j - 1][:2]) and (r.results[j - 1][2] == first[0].shape[1]).all()


def test_clean_model_passes_refused_calls():
    r = _run(SS.refused_script(), preconditions=True)
    assert sum(1 for st in r.done if st.kind == "refused") == 8


def test_clean_model_passes_refused_uploads():
    steps = SS.refused_upload_script()
    r = _run(steps, preconditions=True)
    assert sum(1 for st in r.done if st.kind == "refused") == 3
    for name in ("W32", "W64", "Wd"):
        assert SS.index(name).S > SS.MAX_INDEX_DIM
    assert SS.index("W64").rows.size >= SS.index("D64").rows.size and SS.index("W64").rows.dtype == np.float64


def test_a_refused_upload_that_dropped_the_float64_rows_is_rejected():
    steps = SS.refused_upload_script()
    f = _rejected(steps, "refused_upload_drops_f64")
    assert f.step.kind == "call" and f.step.entry == "topk" and steps[f.number - 2].kind == "refused" and "score off by" in str(f)


def test_case_module_preconditions_of_the_rows_the_script_takes():
    """D64 / D32 are the rows of topk_cases' f64_rows / f64_rows_rounded"""
    for name in ("f64_rows", "f64_rows_rounded"):
        assert TC.preconditions(TC.BY_NAME[name])


def test_clean_model_passes_two_handles():
    x, y = SS.two_handles_script()
    runners = [SS.Runner(SS.StateOracle(), name="X", check_preconditions=True), SS.Runner(SS.StateOracle(), name="Y", check_preconditions=True)]
    for who, st in SS.alternate(x, y):
        runners[who].step(st)
    assert len(runners[0].done) == len(x) and len(runners[1].done) == len(y)


def test_references_of_the_gpu_only_transitions_are_reproducible():
    """transitions 2, 3 and 5 run on the GPU only; their references are proven here"""
    steps, _ = SS.bf16_script()
    _run(steps, preconditions=True)
    _run(SS.norm_script(), preconditions=True)
    for form in ("host",):
        setup, calls, q = SS.scratch_script(form)
        _run(setup + [c for c in calls if c is not None], preconditions=True)


def _rejected(steps, defect):
    with pytest.raises(SS.StepFailed) as e:
        _run(steps, defect)
    return e.value


def _index_at(steps, number):
    return [st.name for st in steps[:number] if st.kind == "set_index"][-1]


def test_tags_kept_across_an_upload_is_rejected():
    steps, _ = SS.tags_script()
    f = _rejected(steps, "tags_kept")
    assert f.step.kind == "refused" and f.step.step.entry == "filtered" and _index_at(steps, f.number) == "A2" and "was served" in str(f)
    assert steps[f.number - 2].kind == "set_index"            # the first step after the upload


def test_group_keys_kept_across_an_upload_is_rejected():
    steps, _ = SS.tags_script()
    f = _rejected(steps, "groups_kept")
    assert f.step.kind == "refused" and f.step.step.entry == "grouped" and _index_at(steps, f.number) == "A2" and "was served" in str(f)


def test_id_base_kept_is_rejected():
    steps, where = SS.chain_script()
    f = _rejected(steps, "id_base_kept")
    assert f.number == where[SS.CHAIN.index("B")][0] and f.step.entry == "topk"       # the first call on B (id_base BASE after 0)
    assert "against the float64 oracle" in str(f)


def test_float64_rows_kept_after_a_float32_upload_is_rejected():
    steps, where = SS.chain_script()
    f = _rejected(steps, "f64_kept")
    assert f.number == where[SS.CHAIN.index("D32")][0] and "score off by" in str(f)


def test_rows_of_the_larger_index_behind_row_n_are_rejected():
    steps, where = SS.chain_script()
    f = _rejected(steps, "rows_behind_n")
    assert f.number == where[SS.CHAIN.index("B")][0] and f.step.entry == "topk"


def test_tag_words_behind_row_n_are_rejected():
    steps, _ = SS.tags_script()
    f = _rejected(steps, "tag_words_behind_n")
    assert f.step.kind == "call" and f.step.entry == "filtered" and f.step.args["k"] == 100 and _index_at(steps, f.number) == "B"
    assert steps[f.number - 2].kind == "set_tags"             # the first call on the smaller index


def test_stale_tile_sums_are_rejected():
    steps, _ = SS.tags_script()
    f = _rejected(steps, "tile_sums_stale")
    # the first filtered call with masks after the second accepted set_tags (the sums are those of the first)
    second = [i for i, st in enumerate(steps) if st.kind == "set_tags"][1]
    want = next(i for i in range(second + 1, len(steps))
                if steps[i].kind == "call" and steps[i].entry == "filtered" and steps[i].args.get("any_of") is not None)
    assert f.number == want + 1 and f.step is steps[want] and _index_at(steps, f.number) == "A2"
    assert "against the float64 oracle" in str(f)


def test_a_refused_set_tags_that_changed_the_tags_is_rejected():
    steps, _ = SS.tags_script()
    f = _rejected(steps, "refused_set_tags_changes")
    assert f.step.kind == "call" and f.step.entry == "filtered"
    assert [st.kind for st in steps[f.number - 3:f.number - 1]] == ["refused", "refused"]     # the call after the two refusals


def test_a_refused_rank_that_wrote_output_is_rejected():
    steps = SS.refused_script()
    f = _rejected(steps, "refused_rank_writes")
    assert f.step.kind == "refused" and f.step.step.entry == "rank" and "wrote output" in str(f)


def test_every_defect_has_a_test():
    import sys
    src = open(sys.modules[__name__].__file__).read()
    for d in SS.DEFECTS:
        assert '"%s"' % d in src, d


def test_band_preconditions():
    """Transition 3: distances of the planted rows from the rank label and from the score_above threshold, in units of
    e_g = score_eps32(norm 1) |q_g| (group 0) and e_g / 16 (group 1), and no other row of the index near either."""
    q, t, groups, labels = SS.planted()
    t64 = t.astype(np.float64)
    norm = float(np.linalg.norm(t64, axis=1).max())
    assert abs(norm - 1.0) < 1e-4                              # idx_norm_max of A2; A16: 16 times that
    s = O.scores_f64(q, t64)
    thr = [c.args["thr"] for c in SS.norm_script() if c.kind == "call" and c.entry == "above"][0]
    for g in range(SS.PLANT_Q):
        e1 = SS.score_eps32(64, norm) * float(np.linalg.norm(q[g].astype(np.float64)))      # eps taken at norm 1 (A2's own) ...
        e16 = SS.score_eps32(64, 16 * norm) * float(np.linalg.norm(q[g].astype(np.float64)))  # ... and at norm 16
        rows = groups[g]
        assert len(rows) == SS.PLANT and labels[g] not in rows
        for ref in (s[g, labels[g]], thr[g]):
            d = np.abs(s[g, rows] - ref)
            others = np.abs(np.delete(s[g], np.concatenate([rows, [labels[g]]])) - ref)
            if g == 0:
                # index A2: none within the band of norm 1, all within the band of norm 16, none within 20 % of an edge
                assert d.min() > 1.2 * e1 and d.max() < 0.8 * e16
                assert 3.0 * e1 <= np.abs(s[g, rows] - s[g, labels[g]]).min() and np.abs(s[g, rows] - s[g, labels[g]]).max() <= 10.0 * e1
                assert others.min() > 1.2 * e16                   # nothing else decides the count
            else:
                # index A16 (scores x 16): all within the band of norm 16, none within the band of norm 1
                assert 16 * d.min() > 1.2 * e1 and 16 * d.max() < 0.8 * e16
                assert d.max() < 0.8 * e1                         # index A2: all within its own band
                assert 16 * others.min() > 1.2 * e16
        # and group 0 on A16: none within the band of norm 16
        if g == 0:
            assert 16 * np.abs(s[g, rows] - s[g, labels[g]]).min() > 1.2 * e16
    # a count of 64 rows moves when the wrong bound is used: both groups are whole on one side of both edges
    assert np.array_equal(O.scores_f64(q, t64 * 16.0), 16.0 * s)


def test_a_and_a2_share_almost_no_top_rows():
    """Transition 2: candidates taken from the bf16 image of the other index cannot certify by luck."""
    steps, q = SS.bf16_script()
    k = 10
    assert q.shape[0] == 129
    ia = O.topk(O.scores_f64(q, np.asarray(SS.index("A").rows, np.float64)), k)[1]
    ib = O.topk(O.scores_f64(q, np.asarray(SS.index("A2").rows, np.float64)), k)[1]
    fewer = sum(1 for qi in range(129) if len(set(ia[qi].tolist()) & set(ib[qi].tolist())) < k)
    assert fewer >= 120
    shared = max(len(set(ia[qi].tolist()) & set(ib[qi].tolist())) for qi in range(129))
    assert shared <= 2


def test_indexes_sit_where_the_script_says():
    """the shapes' side of the thresholds the script quotes (the thresholds themselves are the library's)"""
    I = SS.index
    assert I("A").N >= 8192 and I("A").N % 32 == 8 and I("A").S % 4 == 0
    assert I("B").N % 32 == 9 and (I("B").S + 7) // 8 == 5 and I("B").id_base == TC.BASE and I("B").how == "dev"
    assert np.array_equal(I("Bu").rows, I("B").rows) and I("Bu").how == "dev_unaligned"
    assert I("Bx").N <= 1024 and (I("Bx").S + 7) // 8 == 8
    assert I("C").S % 4 != 0 and (I("C").S + 7) // 8 == 6
    assert I("D64").rows.dtype == np.float64 and not np.array_equal(I("D64").rows, I("D64").rows.astype(np.float32))
    assert np.array_equal(I("D32").rows, I("D64").rows.astype(np.float32))
    assert I("E").S > 616 and 296 < I("F").S <= 616
    assert I("G").N % 32 == 1 and I("G").S < 8
    assert np.array_equal(I("A16").rows, I("A2").rows * np.float32(16)) and I("A16").rows.dtype == np.float32
