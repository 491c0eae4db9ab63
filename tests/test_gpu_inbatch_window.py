"""sse_inbatch_loss_window_dev (csrc/inbatch_loss.hip): the in-batch softmax head with its outputs cut to a window of rows.
Every output row must carry the BITS of the same row of sse_inbatch_loss_dev on the same inputs -- windows not aligned to the
32-row tile and windows inside one tile included --, nothing outside the window's outputs is written, and the window [0, B) is
the full head.  Bit-for-bit claims carry no tolerance; the comparison with the float64 head uses the bars of the case
(tests/inbatch_cases.py)."""
import numpy as np
import pytest

from tests import inbatch_cases as IC
from tests.test_gpu_inbatch_loss import run_head

pytestmark = pytest.mark.gpu

CASES = ("b33-s64", "b100-s130-rows-global", "b300-s130-two-tiles-per-wave")      # B x S: 33 x 64, 100 x 130, 300 x 130
# the whole batch, one row, across a tile boundary up to an unaligned end, unaligned start to the end, the batch's partial last
# tile, and a window inside one tile; a window is run on every case whose batch holds it ("B" = the case's row count)
WINDOWS = ((0, "B"), (0, 1), (31, 33), (37, 100), (96, 100), (40, 50), (5, 20))
GUARD = 3          # rows of NaN kept behind every output: the head must not write past its window


@pytest.fixture(scope="module")
def handle():
    import sse_amd
    from tests.util import model_params
    return sse_amd.SSEModel(model_params("dual-encoder", V=20, E=8, Hs=16, Ht=16, S=8, T=4)).handle


_full = {}


def full_head(handle, cid):
    """(inputs, outputs of sse_inbatch_loss_dev) of a case, computed once."""
    if cid not in _full:
        x = IC.head_case_seeded(IC.HEAD_CASES_BY_ID[cid])
        _full[cid] = (x, run_head(handle, x))
    return _full[cid]


def run_window(h, x, lo, hi, grads=True, drop=(), **over):
    """One call on NaN-filled outputs with GUARD extra rows; returns dict of numpy arrays (guard rows included)."""
    import torch
    dev = "cuda:0"
    B, S = x["s"].shape
    n = max(hi - lo, 0) + GUARD
    s, t, z = (torch.tensor(x[k], dtype=torch.float32, device=dev) for k in ("s", "t", "z"))
    ks = None if x["ks"] is None else torch.tensor(x["ks"], dtype=torch.int64, device=dev)
    kt = None if x["kt"] is None else torch.tensor(x["kt"], dtype=torch.int64, device=dev)
    out = dict(row_loss=torch.full((n,), float("nan"), device=dev), row_acc=torch.full((n,), float("nan"), device=dev))
    if grads:
        out["d_src"] = torch.full((n, S), float("nan"), device=dev)
        out["d_tgt"] = torch.full((n, S), float("nan"), device=dev)
    args = dict(src_raw=s, tgt_raw=t, labels=z, src_key=ks, tgt_key=kt, d_src=out.get("d_src"), d_tgt=out.get("d_tgt"),
                row_loss=out["row_loss"], row_acc=out["row_acc"])
    for k in drop:
        args[k] = None
    h.inbatch_loss_window_dev(args["src_raw"], args["tgt_raw"], args["labels"], args["src_key"], args["tgt_key"], over.get("B", B),
                              over.get("S", S), lo, hi, over.get("scale", x["scale"]), x["inv_rows"], args["d_src"], args["d_tgt"],
                              args["row_loss"], args["row_acc"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _windows(B):
    out = []
    for lo, hi in WINDOWS:
        hi = B if hi == "B" else hi
        if hi <= B and (lo, hi) not in out:
            out.append((lo, hi))
    return out


@pytest.mark.parametrize("cid", CASES)
def test_every_window_row_carries_the_bits_of_the_full_head(handle, cid):
    x, full = full_head(handle, cid)
    B = x["s"].shape[0]
    wins = _windows(B)
    assert (0, B) in wins and any(lo % 32 and hi % 32 for lo, hi in wins) and any(lo // 32 == (hi - 1) // 32 and hi - lo > 1 for lo, hi in wins)
    for lo, hi in wins:
        got = run_window(handle, x, lo, hi)
        n = hi - lo
        for k, v in got.items():
            assert np.array_equal(v[:n].view(np.uint32), full[k][lo:hi].view(np.uint32)), (cid, lo, hi, k)
            assert np.isnan(v[n:]).all(), "%s window [%d, %d): %s written behind the window" % (cid, lo, hi, k)
        # forward only: the same loss and accuracy bits
        fwd = run_window(handle, x, lo, hi, grads=False)
        for k in ("row_loss", "row_acc"):
            assert np.array_equal(fwd[k][:n].view(np.uint32), full[k][lo:hi].view(np.uint32)), (cid, lo, hi, k)
            assert np.isnan(fwd[k][n:]).all()
        # the same call again: the same bits
        again = run_window(handle, x, lo, hi)
        for k in got:
            assert np.array_equal(again[k].view(np.uint32), got[k].view(np.uint32)), (cid, lo, hi, k)


@pytest.mark.parametrize("cid", CASES)
def test_whole_window_matches_float64(handle, cid):
    c = IC.HEAD_CASES_BY_ID[cid]
    x, _ = full_head(handle, cid)
    B = x["s"].shape[0]
    got = {k: v[:B] for k, v in run_window(handle, x, 0, B).items()}
    errs = IC.check_head(got, IC.head_want(x), c, what="window [0, B) ")
    print("WINDOWERR %s bars %.1e/%.1e: norm %.2e element %.2e" % ((cid,) + tuple(c["bars"]) + tuple(errs)))


def test_window_after_full_head_of_another_shape_leaves_no_stale_scratch(handle):
    """The scratch only grows: a window of a small batch after a large one, and back, against a fresh handle."""
    import sse_amd
    from tests.util import model_params
    for cid, (lo, hi) in (("b300-s130-two-tiles-per-wave", (37, 100)), ("b33-s64", (31, 33)), ("b300-s130-two-tiles-per-wave", (96, 100))):
        x, _ = full_head(handle, cid)
        fresh = sse_amd.SSEModel(model_params("dual-encoder", V=20, E=8, Hs=16, Ht=16, S=8, T=4)).handle
        a, b = run_window(handle, x, lo, hi), run_window(fresh, x, lo, hi)
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (cid, k)


REFUSALS = [
    (dict(lo=-1, hi=2), "row_lo = -1 is negative"),
    (dict(lo=0, hi=3), "row_hi = 3 lies behind the 2 rows"),
    (dict(lo=1, hi=1), r"window \[1, 1\) is empty or inverted"),
    (dict(lo=2, hi=1), r"window \[2, 1\) is empty or inverted"),
    (dict(B=0), "B and S must be >= 1"),
    (dict(S=0), "B and S must be >= 1"),
    (dict(drop=("src_raw",)), "must not be NULL"),
    (dict(drop=("tgt_raw",)), "must not be NULL"),
    (dict(drop=("labels",)), "must not be NULL"),
    (dict(drop=("row_loss",)), "must not be NULL"),
    (dict(drop=("row_acc",)), "must not be NULL"),
    (dict(drop=("d_src",)), "both be given, or both be NULL"),
    (dict(drop=("d_tgt",)), "both be given, or both be NULL"),
    (dict(scale=0.0), r"scale must be in \(0, 256\]"),
    (dict(scale=256.5), r"scale must be in \(0, 256\]"),
    (dict(scale=float("nan")), r"scale must be in \(0, 256\]"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_bad_arguments_are_refused_with_their_text(handle, kw, text):
    import sse_amd
    x = IC.head_case_seeded(IC.HEAD_CASES_BY_ID["b2-s64"])
    kw = dict(kw)
    lo, hi = kw.pop("lo", 0), kw.pop("hi", 2)
    if kw.get("B") == 0:
        hi = 0          # (so that the batch size, not the window, is what is wrong)
    with pytest.raises(sse_amd.SSEError, match=text):
        run_window(handle, x, lo, hi, **kw)
    # nothing was queued and the handle still serves
    got = run_window(handle, x, 0, 2)
    assert np.isfinite(got["row_loss"][:2]).all()
