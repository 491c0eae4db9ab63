"""CPU side of the in-place index updates (DESIGN K6n): IndexModel of tests/index_update_script.py, the numpy model of the
images a handle keeps, is driven through one scripted sequence of updates and appends; after every step its observation (what
each route would read) must equal a fresh model's that was given the final arrays.  The clean model passes every step; every
planted defect is rejected at the step named for it.  Then the C ABI: the six entry points are declared, exported and bound,
and refuse a null handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import index_update_script as US

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8
RM_LIMIT = 150 * S * 4        # the model's "64 MiB": 150 rows of this script


def script():
    """(name, kind, args) steps on a 70-row index with id_base 1000 and all three columns"""
    u = lambda seed, n, scale=1.0: US.unit(seed, n, S) * np.float32(scale)
    c = lambda n, seed: dict(zip(("tags", "groups", "bias"), US.columns(n, seed)))
    return [
        ("update one row", "update", dict(ids=[1005], rows=u(1, 1))),
        ("bf16 call", "bf16", {}),
        ("update the seam", "update", dict(ids=[1031, 1032], rows=u(2, 2), **c(2, 2))),
        ("largest row", "update", dict(ids=[1000], rows=u(3, 1, 16.0))),
        ("largest row made small", "update", dict(ids=[1000], rows=u(4, 1, 0.5))),
        ("set a tag bit", "update", dict(ids=[1040], tags=[1 << 40])),
        ("clear the tag bit", "update", dict(ids=[1040], tags=[2])),
        ("large bias", "update", dict(ids=[1041], bias=[9.0])),
        ("large bias made small", "update", dict(ids=[1041], bias=[0.01])),
        ("duplicate ids", "update_unsorted", dict(ids=[1009, 1003, 1009], rows=u(5, 3))),
        ("refused: id out of range", "refused", dict(ids=[1003, 1070], rows=u(6, 2))),
        ("refused: column not given on append", "refused_append", dict(rows=u(7, 2))),
        ("append inside the tail tile", "append", dict(rows=u(8, 3), **c(3, 8))),
        ("append into new tiles", "append", dict(rows=u(9, 40), **c(40, 9))),
        ("append past capacity", "append", dict(rows=u(10, 30), **c(30, 10))),
        ("append past the row-major limit", "append", dict(rows=u(11, 20), **c(20, 11))),
        ("append past the small-index scorer", "append", dict(rows=u(12, 900), **c(900, 12))),
    ]


def run(defect):
    """None, or (step name, image) of the first step after which the model differs from the fresh one"""
    rows = US.unit(0, 70, S)
    tags, groups, bias = US.columns(70, 0)
    garbage = np.float32(7.5)
    m = US.IndexModel(defect, rm_limit=RM_LIMIT).upload(rows, 1000, garbage=garbage).set_columns(tags, groups, bias)
    state = dict(index="m", rows=rows.copy(), how="f32", id_base=1000, tags=tags.copy(), groups=groups.copy(), bias=bias.copy())
    had_bf16 = False
    for name, kind, a in script():
        if kind == "bf16":
            m.bf16_call()
            had_bf16 = True
        elif kind in ("update", "update_unsorted"):
            st = US.update(**a)
            ids, r_, t_, g_, b_ = m.sort_ids(st.ids, st.rows, st.tags, st.groups, st.bias)
            assert m.update(ids, r_, t_, g_, b_) is None, name
            US.apply_to_arrays(state, st)
        elif kind == "refused":
            st = US.update(**a)
            assert m.update(st.ids, st.rows) is not None, name
        elif kind == "refused_append":
            assert m.append(a["rows"]) is not None, name
        else:
            st = US.append(**a)
            assert m.append(st.rows, st.tags, st.groups, st.bias) is None, name
            US.apply_to_arrays(state, st)
        bad = US.first_mismatch(m.observe(), US.fresh_like(m, state, had_bf16).observe())
        if bad is not None:
            return name, bad
    return None


def test_clean_model_passes_every_step():
    assert run(None) is None


WHERE = {
    "idx_rm_stale": ("update one row", "idx_rm"),
    "idx64_stale": None,                       # (its own script below: the float64 index)
    "idxp16_stale": ("update the seam", "idxp16"),
    "idx_x3_stale": ("update one row", "idx_x3"),
    "norm2_stale": ("largest row", "norm_max"),
    "norm_max_only_rises": ("largest row made small", "norm_max"),
    "tile_sum_keeps_bit": ("clear the tag bit", "tile_sum"),
    "absmax_only_rises": ("large bias made small", "absmax"),
    "tail_padding_not_zeroed": ("append into new tiles", "idxp"),
    "idx_x3_valid_past_limit": ("append past the small-index scorer", "idx_x3"),
    "idx_rm_valid_past_limit": ("append past the row-major limit", "idx_rm"),
    "realloc_loses_contents": ("append inside the tail tile", "idx_rm"),     # (the row-major images hold exactly N rows: they grow first)
    "first_duplicate_wins": ("duplicate ids", "idxp"),
    "refused_call_applies": ("refused: id out of range", "idxp"),
}


@pytest.mark.parametrize("defect", [d for d in US.DEFECTS if WHERE[d] is not None])
def test_every_planted_defect_is_rejected_at_its_step(defect):
    got = run(defect)
    assert got is not None, "the defect %s went unnoticed" % defect
    assert got[0] == WHERE[defect][0], got
    assert got[1].startswith(WHERE[defect][1]), got


@pytest.mark.parametrize("defect", [None, "idx64_stale"])
def test_float64_index(defect):
    rows = US.unit(20, 40, S).astype(np.float64) * (1.0 + 1e-9)
    m = US.IndexModel(defect).upload(rows, 0, f64=True)
    state = dict(index="m", rows=rows.copy(), how="f64", id_base=0, tags=None, groups=None, bias=None)
    assert m.update([3], US.unit(21, 1, S)) == "float64"            # an f32 form on an index that holds idx64
    st = US.update([3, 39], US.unit(22, 2, S).astype(np.float64) * (1.0 - 1e-9))
    assert m.update(st.ids, st.rows, f64=True) is None
    US.apply_to_arrays(state, st)
    bad = US.first_mismatch(m.observe(), US.fresh_like(m, state, False).observe())
    assert (bad is None) if defect is None else (bad == "idx64")


def test_model_refusals():
    rows = US.unit(30, 70, S)
    assert US.IndexModel().update([0], rows[:1]) == "no index uploaded"
    m = US.IndexModel().upload(rows, 10).set_columns(bias=np.zeros(70, np.float32))
    one = rows[:1]
    assert m.update([9], one) == "outside the index" and m.update([80], one) == "outside the index"
    assert m.update([11, 11], rows[:2]) == "strictly increasing" and m.update([12, 11], rows[:2]) == "strictly increasing"
    assert m.update([11], one.astype(np.float64), f64=True) == "float64"
    assert m.update([11], tags=[1]) == "not set" and m.update([11]) == "nothing to update"
    assert m.update([11], bias=[np.inf]) == "not finite"
    assert m.append(one) == "exactly when" and m.append(one, tags=[1], bias=[0.0]) == "exactly when"
    assert m.append(one, bias=[np.nan]) == "not finite"
    before = m.observe()
    assert US.first_mismatch(before, m.observe()) is None and m.N == 70


NEW = ("sse_index_update", "sse_index_update_f64", "sse_index_update_dev", "sse_index_append", "sse_index_append_f64",
       "sse_index_append_dev")


def test_new_entry_points_are_declared_exported_and_refuse_a_null_handle():
    import __graft_entry__ as g
    g.build()
    import sse_amd
    lib = sse_amd.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sse_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in sse_amd.SYMBOLS and hasattr(lib, name), name
    ids = np.zeros(1, np.int64)
    rows = np.zeros((1, 8), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.sse_index_update(None, p(ids), p(rows), 1, None, None, None) != 0
    assert lib.sse_index_update_f64(None, p(ids), p(rows.astype(np.float64)), 1, None, None, None) != 0
    assert lib.sse_index_append(None, p(rows), 1, None, None, None) != 0
    assert lib.sse_index_append_f64(None, p(rows.astype(np.float64)), 1, None, None, None) != 0
    assert lib.sse_index_update_dev(None, None, None, 0, None, None, None, None) != 0
    assert lib.sse_index_append_dev(None, None, 0, None, None, None, None) != 0


def test_header_documents_hiding_a_row_and_the_counters():
    txt = open(os.path.join(ROOT, "include", "sse_hip.h")).read()
    for word in ("none_of", "no removal and no compaction", '"index_update_calls"', '"index_grow_copies"'):
        assert word in txt, word
