"""sse_inbatch_loss_dev and sse_class_loss_dev on guarded, skewed caller buffers (tests/guard_bands.py): every input
(encodings, table, target rows, labels, keys) and every output (d_src, d_tgt / d_table, row_loss, row_acc) sits between
guards, with no skew and one element off 16-byte alignment, under both fills.

The shapes are the issue's -- (B, S) = (33, 50) and (32, 64) for the in-batch head, (B, N, S) = (33, 45, 50) and (128, 571, 64)
(the class walk split over workgroups) for the class head -- built by the case builders of tests/inbatch_cases.py and
tests/class_loss_cases.py (kind "keys": repeated sources and targets) and held by their check_head at their bars, against
their float64 heads.  The float32 restatement of each new shape is asserted 10x inside the bars here, which is the rule those
files give for a case on the default bars.  Both heads sum in an order fixed by the shape, no atomics, so every output must
also be bit-identical to the same call on whole allocations."""
import functools

import numpy as np
import pytest

from tests import class_loss_cases as CL
from tests import guard_bands as GB
from tests import inbatch_cases as IC

pytestmark = pytest.mark.gpu
F32 = np.float32

INBATCH = [IC._hc("guard-b33-s50", 33, 50, kind="keys"), IC._hc("guard-b32-s64", 32, 64, kind="keys")]
CLASS = [CL._hc("guard-b33-n45-s50", 33, 45, 50, kind="keys"), CL._hc("guard-b128-n571-s64-split", 128, 571, 64, kind="keys")]


def _scorer():
    from tests.test_gpu_score import _scorer as s
    return s()


def _guard(rows, cols, itemsize=4):
    return GB.guard_bytes(rows, cols, itemsize, 64, 64)


def _in(a, valid=None):
    a = np.ascontiguousarray(a)
    rows = a.shape[0]
    return GB.spec(a.dtype, a.size, "in", init=a, valid=valid, guard=_guard(rows, a.size // rows, a.dtype.itemsize))


def _out(rows, cols):
    return GB.spec(F32, rows * cols, "out", guard=_guard(rows, cols))


@functools.lru_cache(maxsize=None)
def _inbatch(cid):
    c = next(c for c in INBATCH if c["id"] == cid)
    x = IC.head_case_seeded(c)
    want = IC.head_want(x)
    f32 = IC.head(x["s"], x["t"], x["z"], x["ks"], x["kt"], x["scale"], x["inv_rows"], dtype=np.float32)
    rel, elem = IC.head_errors(f32, want)
    assert 10 * rel <= c["bars"][0] and 10 * elem <= c["bars"][1], (cid, rel, elem)
    return c, x, want


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("cid", [c["id"] for c in INBATCH])
def test_inbatch_loss_on_guarded_buffers(cid, skew):
    c, x, want = _inbatch(cid)
    B, S = c["B"], c["S"]
    h = _scorer()
    specs = dict(s=_in(x["s"]), t=_in(x["t"]), z=_in(x["z"]), ks=_in(x["ks"], valid=int(x["ks"][0])), kt=_in(x["kt"], valid=int(x["kt"][0])),
                 d_src=_out(B, S), d_tgt=_out(B, S), row_loss=_out(B, 1), row_acc=_out(B, 1))

    def call(b):
        h.inbatch_loss_dev(b["s"].ptr, b["t"].ptr, b["z"].ptr, b["ks"].ptr, b["kt"].ptr, B, S, x["scale"], x["inv_rows"], b["d_src"].ptr,
                           b["d_tgt"].ptr, b["row_loss"].ptr, b["row_acc"].ptr)
        h.synchronize()

    def check(o):
        IC.check_head(dict(row_loss=o["row_loss"], row_acc=o["row_acc"], d_src=o["d_src"].reshape(B, S), d_tgt=o["d_tgt"].reshape(B, S)),
                      want, c, what="skew %d: " % skew)
    calls = GB.run_guarded.calls
    GB.drive(GB.TorchBackend(), specs, call, skew, check)
    # forward only: both gradient pointers NULL
    fwd = {k: v for k, v in specs.items() if k not in ("d_src", "d_tgt")}

    def call_fwd(b):
        h.inbatch_loss_dev(b["s"].ptr, b["t"].ptr, b["z"].ptr, b["ks"].ptr, b["kt"].ptr, B, S, x["scale"], x["inv_rows"], None, None,
                           b["row_loss"].ptr, b["row_acc"].ptr)
        h.synchronize()
    GB.drive(GB.TorchBackend(), fwd, call_fwd, skew, lambda o: IC.check_head(dict(row_loss=o["row_loss"], row_acc=o["row_acc"]), want, c))
    print("GUARDCALLS loss_heads %d" % (GB.run_guarded.calls - calls))
    h.close()


@functools.lru_cache(maxsize=None)
def _class(cid):
    c = next(c for c in CLASS if c["id"] == cid)
    x, want = CL.head_case_seeded(c)
    f32 = CL.head(x["s"], x["t"], x["y"], x["z"], x["ks"], x["scale"], x["inv_rows"], dtype=np.float32)
    rel, elem = CL.head_errors(f32, want)
    assert 10 * rel <= c["bars"][0] and 10 * elem <= c["bars"][1], (cid, rel, elem)
    return c, x, want


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("cid", [c["id"] for c in CLASS])
def test_class_loss_on_guarded_buffers(cid, skew):
    c, x, want = _class(cid)
    B, N, S = c["B"], c["N"], c["S"]
    h = _scorer()
    specs = dict(s=_in(x["s"]), table=_in(x["t"]), y=_in(x["y"], valid=1), z=_in(x["z"]), ks=_in(x["ks"], valid=int(x["ks"][0])),
                 d_src=_out(B, S), d_table=_out(N, S), row_loss=_out(B, 1), row_acc=_out(B, 1))

    def call(b):
        h.class_loss_dev(b["s"].ptr, b["table"].ptr, b["y"].ptr, b["z"].ptr, b["ks"].ptr, B, N, S, x["scale"], x["inv_rows"], b["d_src"].ptr,
                         b["d_table"].ptr, b["row_loss"].ptr, b["row_acc"].ptr)
        h.synchronize()                                # (a target row picked up from outside its array would raise the error flag)

    def check(o):
        CL.check_head(dict(row_loss=o["row_loss"], row_acc=o["row_acc"], d_src=o["d_src"].reshape(B, S), d_table=o["d_table"].reshape(N, S)),
                      want, c, what="skew %d: " % skew)
    calls = GB.run_guarded.calls
    GB.drive(GB.TorchBackend(), specs, call, skew, check)
    fwd = {k: v for k, v in specs.items() if k not in ("d_src", "d_table")}

    def call_fwd(b):
        h.class_loss_dev(b["s"].ptr, b["table"].ptr, b["y"].ptr, b["z"].ptr, b["ks"].ptr, B, N, S, x["scale"], x["inv_rows"], None, None,
                         b["row_loss"].ptr, b["row_acc"].ptr)
        h.synchronize()
    GB.drive(GB.TorchBackend(), fwd, call_fwd, skew, lambda o: CL.check_head(dict(row_loss=o["row_loss"], row_acc=o["row_acc"]), want, c))
    print("GUARDCALLS loss_heads %d" % (GB.run_guarded.calls - calls))
    h.close()
