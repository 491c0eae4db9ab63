"""CPU self-test of the bars tests/test_gpu_eval_loss.py holds sse_eval_loss to: the float32 oracle against its float64 run
over the same case list.  The cosine bar follows the 25x rule (25 x the float32 oracle's distance must not exceed it); the
loss bar is check_tail's LOSS_REL_EXACT, which the float32 oracle has to pass with 10x room (as tests/test_grad_check.py
asks of the gradient bars); the accuracy is exact once no row's logit is within LN9_MARGIN of ln 9, the margins the GPU
test asserts."""
import numpy as np
import pytest

from tests.test_gpu_eval_loss import ACC_BAR, CASES, COS_BAR, LN9_MARGIN, build_case, ln9_margin, oracle_eval
from tests.util import LOSS_REL_EXACT

# smallest | |64 cos| - ln 9 | per case in the float64 oracle, rounded down (measured with this construction)
MARGINS = {"A": 0.038, "B": 0.049, "C": 1.0, "D": 0.040, "E": 2.1, "F": 0.032, "G": 3.5}


@pytest.fixture(scope="module")
def runs():
    out = {}
    for cid in sorted(CASES):
        cfg, p, src, tgt, labels = build_case(cid)
        out[cid] = (oracle_eval(p, cfg, src, tgt, labels, float64=True), oracle_eval(p, cfg, src, tgt, labels, float64=False))
    return out


def test_float32_oracle_distance_leaves_the_bars_their_room(runs):
    d_cos = max(float(np.abs(f32[2] - f64[2]).max()) for f64, f32 in runs.values())
    d_loss = max(abs(f32[0] - f64[0]) / abs(f64[0]) for f64, f32 in runs.values())
    d_acc = max(abs(f32[1] - f64[1]) for f64, f32 in runs.values())
    print("\nfloat32 oracle vs float64 over %s: cos %.3g, loss rel %.3g, acc %.3g" % (sorted(runs), d_cos, d_loss, d_acc))
    assert 25 * d_cos <= COS_BAR * 1.05, d_cos                       # COS_BAR is 25 x this, rounded to one digit
    assert COS_BAR <= 50 * d_cos                                     # ... and not a bar set generously
    assert 10 * d_loss <= LOSS_REL_EXACT, d_loss
    assert d_acc <= ACC_BAR


def test_no_row_sits_where_the_accuracy_flips(runs):
    for cid, (f64, f32) in runs.items():
        got = ln9_margin(f64[2])
        print("\n%s: ln 9 margin %.4f, loss %.6f acc %.4f" % (cid, got, f64[0], f64[1]))
        assert got >= MARGINS[cid] >= LN9_MARGIN, (cid, got)
        assert 64 * COS_BAR * 10 < LN9_MARGIN                        # a cosine at its bar moves the logit far less than the margin
    for cid in ("A", "F"):                                           # both outcomes of the accuracy occur
        assert 0.0 < runs[cid][0][1] < 1.0
    assert abs(runs["A"][0][1] - 0.28) < 0.01 and abs(runs["F"][0][1] - 0.24) < 0.01
