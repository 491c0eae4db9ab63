"""sse_class_loss_dev (csrc/class_loss.hip) alone, against the float64 head of tests/class_loss_cases.py: per-row loss and
accuracy on every row, both gradients on every element (the table's on every class), with outputs pre-filled with NaN so that an
unwritten element shows."""
import numpy as np
import pytest

from tests import class_loss_cases as CC

pytestmark = pytest.mark.gpu


def _fresh_handle():
    import sse_amd
    from tests.util import model_params
    return sse_amd.SSEModel(model_params("dual-encoder", V=20, E=8, Hs=16, Ht=16, S=8, T=4)).handle


@pytest.fixture(scope="module")
def handle():
    return _fresh_handle()


def run_head(h, x, grads=True, scale=None, B=None, N=None, S=None, drop=(), y=None, sync=True):
    """One call on NaN-filled outputs; returns dict of numpy arrays.  drop: argument names passed as NULL."""
    import torch
    dev = "cuda:0"
    Bx, Sx = x["s"].shape
    Nx = x["t"].shape[0]
    s, t, z = (torch.tensor(x[k], dtype=torch.float32, device=dev) for k in ("s", "t", "z"))
    rows = torch.tensor(x["y"] if y is None else y, dtype=torch.int32, device=dev)
    ks = None if x["ks"] is None else torch.tensor(x["ks"], dtype=torch.int64, device=dev)
    out = dict(row_loss=torch.full((Bx,), float("nan"), device=dev), row_acc=torch.full((Bx,), float("nan"), device=dev))
    if grads:
        out["d_src"] = torch.full((Bx, Sx), float("nan"), device=dev)
        out["d_table"] = torch.full((Nx, Sx), float("nan"), device=dev)
    args = dict(src_raw=s, table=t, tgt_row=rows, labels=z, src_key=ks, d_src=out.get("d_src"), d_table=out.get("d_table"),
                row_loss=out["row_loss"], row_acc=out["row_acc"])
    for k in drop:
        args[k] = None
    h.class_loss_dev(args["src_raw"], args["table"], args["tgt_row"], args["labels"], args["src_key"], Bx if B is None else B,
                     Nx if N is None else N, Sx if S is None else S, x["scale"] if scale is None else scale, x["inv_rows"],
                     args["d_src"], args["d_table"], args["row_loss"], args["row_acc"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if sync:
        h.synchronize()         # reports the device error flag
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("c", CC.HEAD_CASES, ids=[c["id"] for c in CC.HEAD_CASES])
def test_head_matches_float64(handle, c):
    x, want = CC.head_case_seeded(c)
    got = run_head(handle, x)
    for k, v in got.items():
        assert not np.isnan(v).any(), "%s: an element of %s was not written" % (c["id"], k)
    errs = CC.check_head(got, want, c)
    print("CLASS HEADERR %s bars %.1e/%.1e: norm %.2e element %.2e" % ((c["id"],) + tuple(c["bars"]) + tuple(errs)))
    if c["kind"] == "labels0" or c["N"] == 1:     # nothing to learn: loss 0, gradients 0, exactly
        assert not got["row_loss"].any() and not got["d_src"].any() and not got["d_table"].any()
    if c["kind"] == "labels0":
        assert not got["row_acc"].any()
    if c["N"] > 2 and c["kind"] not in ("labels0", "s1"):    # classes no row names carry gradient too
        unnamed = ~np.isin(np.arange(c["N"]), x["y"])
        assert not unnamed.any() or np.abs(got["d_table"][unnamed]).max() > 0
    # forward only: the same loss and accuracy bits, nothing else touched
    fwd = run_head(handle, x, grads=False)
    assert np.array_equal(fwd["row_loss"], got["row_loss"]) and np.array_equal(fwd["row_acc"], got["row_acc"])
    # the same call again: the same bits
    again = run_head(handle, x)
    for k in got:
        assert np.array_equal(again[k], got[k]), k


def test_shrinking_and_growing_shapes_leave_no_stale_scratch(handle):
    """One handle, (B, N, S) up and down: the scratch only grows, and rows past B, classes past N, columns past S, exclusion
    lists or split partials of an earlier call must not reach a later one."""
    for cid in ("b100-n300-s130-rows-global", "forty-class-source", "b33-n31-s64", "b300-n65-s64", "three-class-source",
                "b100-n300-s130-rows-global"):
        x, _ = CC.head_case_seeded(CC.HEAD_CASES_BY_ID[cid])
        a, b = run_head(handle, x), run_head(_fresh_handle(), x)
        for k in a:
            assert np.array_equal(a[k], b[k]), (cid, k)


REFUSALS = [
    (dict(B=0), "B, N and S must be >= 1"),
    (dict(N=0), "B, N and S must be >= 1"),
    (dict(S=0), "B, N and S must be >= 1"),
    (dict(drop=("src_raw",)), "must not be NULL"),
    (dict(drop=("table",)), "must not be NULL"),
    (dict(drop=("tgt_row",)), "must not be NULL"),
    (dict(drop=("labels",)), "must not be NULL"),
    (dict(drop=("row_loss",)), "must not be NULL"),
    (dict(drop=("row_acc",)), "must not be NULL"),
    (dict(drop=("d_src",)), "both be given, or both be NULL"),
    (dict(drop=("d_table",)), "both be given, or both be NULL"),
    (dict(scale=0.0), r"scale must be in \(0, 256\]"),
    (dict(scale=-1.0), r"scale must be in \(0, 256\]"),
    (dict(scale=256.5), r"scale must be in \(0, 256\]"),
    (dict(scale=float("nan")), r"scale must be in \(0, 256\]"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_bad_arguments_are_refused_with_their_text(handle, kw, text):
    import sse_amd
    x, _ = CC.head_case_seeded(CC.HEAD_CASES_BY_ID["b2-n5-s64"])
    with pytest.raises(sse_amd.SSEError, match="sse_class_loss_dev: .*" + text):
        run_head(handle, x, **kw)


def test_option_refusals_and_counter(handle):
    import sse_amd
    for v in (-1, 2, 7):
        with pytest.raises(sse_amd.SSEError, match=r"train_class_loss must be 0 \(off\) or 1 \(softmax over the free target matrix\)"):
            handle.set_option("train_class_loss", v)
    handle.set_option("train_class_loss", 1)
    handle.set_option("train_class_loss", 0)
    assert handle.get_counter("train_class_steps") == 0


@pytest.mark.parametrize("bad", [-1, 31, 1 << 30])
def test_bad_target_row_raises_the_flag_contributes_nothing_and_leaves_the_handle_usable(bad):
    """A target row outside [0, N) on a label-1 row: the error flag reports it, that row's loss, accuracy and d_src are 0, the
    other rows are those of the batch without it (the mean still over B rows), and the next call on the handle is right."""
    import sse_amd
    h = _fresh_handle()
    c = CC.HEAD_CASES_BY_ID["b33-n31-s64"]
    x, want = CC.head_case_seeded(c)
    y = x["y"].copy()
    y[0] = bad
    assert x["z"][0] != 0
    with pytest.raises(sse_amd.SSEError, match="out of range"):
        run_head(h, x, y=y)
    got = run_head(h, x, y=y, sync=False)
    with pytest.raises(sse_amd.SSEError):
        h.synchronize()                            # (reports and resets the flag of the second call)
    keep = np.arange(c["B"]) != 0
    sub = dict(x, s=x["s"][keep], y=x["y"][keep], z=x["z"][keep], ks=x["ks"][keep])
    ref = CC.head(sub["s"], sub["t"], sub["y"], sub["z"], sub["ks"], sub["scale"], sub["inv_rows"])
    ref["z"], ref["x"] = sub["z"], sub
    assert got["row_loss"][0] == 0 and got["row_acc"][0] == 0 and not got["d_src"][0].any()
    CC.check_head(dict(row_loss=got["row_loss"][keep], row_acc=got["row_acc"][keep], d_src=got["d_src"][keep], d_table=got["d_table"]),
                  ref, c, what="without the bad row: ")
    CC.check_head(run_head(h, x), want, c, what="after the bad row: ")
