"""sse_inbatch_loss_dev (csrc/inbatch_loss.hip) alone, against the float64 head of tests/inbatch_cases.py: per-row loss and
accuracy on every row, both gradients on every element, with outputs pre-filled with NaN so that an unwritten element shows."""
import numpy as np
import pytest

from tests import inbatch_cases as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    import sse_amd
    from tests.util import model_params
    return sse_amd.SSEModel(model_params("dual-encoder", V=20, E=8, Hs=16, Ht=16, S=8, T=4)).handle


def run_head(h, x, grads=True, scale=None, inv_rows=None, B=None, S=None, drop=()):
    """One call on NaN-filled outputs; returns dict of numpy arrays.  drop: argument names passed as NULL."""
    import torch
    dev = "cuda:0"
    Bx, Sx = x["s"].shape
    s, t, z = (torch.tensor(x[k], dtype=torch.float32, device=dev) for k in ("s", "t", "z"))
    ks = None if x["ks"] is None else torch.tensor(x["ks"], dtype=torch.int64, device=dev)
    kt = None if x["kt"] is None else torch.tensor(x["kt"], dtype=torch.int64, device=dev)
    out = dict(row_loss=torch.full((Bx,), float("nan"), device=dev), row_acc=torch.full((Bx,), float("nan"), device=dev))
    if grads:
        out["d_src"] = torch.full((Bx, Sx), float("nan"), device=dev)
        out["d_tgt"] = torch.full((Bx, Sx), float("nan"), device=dev)
    args = dict(src_raw=s, tgt_raw=t, labels=z, src_key=ks, tgt_key=kt, d_src=out.get("d_src"), d_tgt=out.get("d_tgt"),
                row_loss=out["row_loss"], row_acc=out["row_acc"])
    for k in drop:
        args[k] = None
    h.inbatch_loss_dev(args["src_raw"], args["tgt_raw"], args["labels"], args["src_key"], args["tgt_key"], Bx if B is None else B,
                       Sx if S is None else S, x["scale"] if scale is None else scale, x["inv_rows"] if inv_rows is None else inv_rows,
                       args["d_src"], args["d_tgt"], args["row_loss"], args["row_acc"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("c", IC.HEAD_CASES, ids=[c["id"] for c in IC.HEAD_CASES])
def test_head_matches_float64(handle, c):
    x = IC.head_case_seeded(c)
    want = IC.head_want(x)
    got = run_head(handle, x)
    errs = IC.check_head(got, want, c)
    print("HEADERR %s bars %.1e/%.1e: norm %.2e element %.2e" % ((c["id"],) + tuple(c["bars"]) + tuple(errs)))
    if c["kind"] in ("labels0", "one-target") or c["B"] == 1:     # nothing to learn: loss 0, gradients 0, exactly
        assert not got["row_loss"].any() and not got["d_src"].any() and not got["d_tgt"].any()
    if c["kind"] == "labels0":
        assert not got["row_acc"].any()
    # forward only: the same loss and accuracy bits, nothing else touched
    fwd = run_head(handle, x, grads=False)
    assert np.array_equal(fwd["row_loss"], got["row_loss"]) and np.array_equal(fwd["row_acc"], got["row_acc"])
    # the same call again: the same bits
    again = run_head(handle, x)
    for k in got:
        assert np.array_equal(again[k], got[k]), k


def test_shrinking_and_growing_batches_leave_no_stale_scratch(handle):
    """One handle, B 100 -> 31 -> 100 and S 130 -> 64: the scratch only grows, rows past B and columns past S of an earlier
    call must not reach a later one."""
    import sse_amd
    from tests.util import model_params
    for cid in ("b100-s130-rows-global", "fractional-labels", "b100-s130-rows-global", "b33-s64"):
        c = IC.HEAD_CASES_BY_ID[cid]
        x = IC.head_case_seeded(c)
        fresh = sse_amd.SSEModel(model_params("dual-encoder", V=20, E=8, Hs=16, Ht=16, S=8, T=4)).handle
        a, b = run_head(handle, x), run_head(fresh, x)
        for k in a:
            assert np.array_equal(a[k], b[k]), (cid, k)


REFUSALS = [
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
    (dict(scale=-1.0), r"scale must be in \(0, 256\]"),
    (dict(scale=256.5), r"scale must be in \(0, 256\]"),
    (dict(scale=float("nan")), r"scale must be in \(0, 256\]"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_bad_arguments_are_refused_with_their_text(handle, kw, text):
    import sse_amd
    x = IC.head_case_seeded(IC.HEAD_CASES_BY_ID["b2-s64"])
    with pytest.raises(sse_amd.SSEError, match=text):
        run_head(handle, x, **kw)


def test_option_refusals(handle):
    import sse_amd
    for v in (-1, 2, 7):
        with pytest.raises(sse_amd.SSEError, match=r"train_loss must be 0 \(pair\) or 1 \(in-batch softmax\)"):
            handle.set_option("train_loss", v)
    for v in (0, 257, -64):
        with pytest.raises(sse_amd.SSEError, match=r"train_loss_scale must be in 1 \.\. 256"):
            handle.set_option("train_loss_scale", v)
    for v in (1, 64, 256):
        handle.set_option("train_loss_scale", v)
    handle.set_option("train_loss_scale", 64)
    assert handle.get_counter("train_inbatch_steps") == 0
