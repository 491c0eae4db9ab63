"""The truncation term of the split-bf16 candidate bound of the small-index scorer (option score_small_x3, DESIGN K6),
checked on the CPU.

The scorer carries every fp32 operand as hi = bf16(x), lo = bf16(x - hi) (round to nearest even, sse_bf16_rne) and keeps
qh.th + qh.tl + ql.th of a product.  bf16 has 8 significant bits, so |x - hi| <= 2^-8 |x| and |x - hi - lo| <= 2^-17 |x|;
the dropped terms ql.tl + eq.t + (q - eq).et are at most

    TRUNC * sum|q_i t_i| <= TRUNC * |q||t|,     TRUNC = 2^-15 (1 + 2^-6).

Here the split is restated in numpy and the three kept products are summed EXACTLY (math.fsum of float64 products, each of
which is exact), so the distance to the exact dot product is the truncation alone.  The accumulation term of the bound --
(3 S + 2) fp32 additions in an order the matrix pipe chooses -- cannot be emulated: the hardware's order is not specified.
That term rests on the derivation in DESIGN K6 and its factor 2.
"""
import math

import numpy as np
import pytest

TRUNC = 2.0 ** -15 * (1.0 + 2.0 ** -6)


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even) as float32: the integer restatement of sse_bf16_rne."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split(x):
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    lo = bf16_rne(x - hi)          # x - hi is exact in float32
    return hi, lo


def kept_dot(q, t, drop_lo_hi=False, no_lo=False):
    qh, ql = split(q)
    th, tl = split(t)
    if no_lo:
        ql, tl = np.zeros_like(ql), np.zeros_like(tl)
    qh, ql, th, tl = (v.astype(np.float64) for v in (qh, ql, th, tl))
    terms = [qh * th, qh * tl] + ([] if drop_lo_hi else [ql * th])
    return math.fsum(np.concatenate(terms))


def exact_dot(q, t):
    return math.fsum(np.asarray(q, np.float64) * np.asarray(t, np.float64))


def norms(q, t):
    return float(np.linalg.norm(np.asarray(q, np.float64)) * np.linalg.norm(np.asarray(t, np.float64)))


def worst_mantissas(S, odd=5):
    """x = 2^e (1 + 2^-7 - (2^-8 - odd * 2^-17)): hi rounds UP over almost half a bf16 step, and the remainder sits halfway
    between two bf16 values of its own binade: both roundings at their maximum.  odd = 5: the tie of the second rounding
    goes the way that lets ql.tl and the two e.x terms add up; odd = 3: the other way, they cancel."""
    m = np.float32(1.0 + 2.0 ** -7 - (2.0 ** -8 - odd * 2.0 ** -17))
    e = np.float32(2.0) ** (np.arange(S) % 5).astype(np.float32)
    return (m * e / np.float32(16.0)).astype(np.float32)


def _cases():
    rng = np.random.RandomState(0)
    out = []
    for S in (256, 249, 64, 49):
        for _ in range(40):
            q, t = rng.standard_normal(S).astype(np.float32), rng.standard_normal(S).astype(np.float32)
            out.append(("random", q, t))
            out.append(("positive", np.abs(q), np.abs(t)))        # sum|q_i t_i| = |q.t|: nothing cancels
            out.append(("scaled", q * np.float32(23.0), t * np.float32(0.02)))
        w = worst_mantissas(S)
        out.append(("worst", w, w))
        out.append(("worst, mixed", w, worst_mantissas(S)[::-1].copy()))
        out.append(("worst, other tie", worst_mantissas(S, 3), worst_mantissas(S, 3)))
        out.append(("worst, both ties", w, worst_mantissas(S, 3)))
    return out


CASES = _cases()


def test_split_matches_its_claims():
    rng = np.random.RandomState(1)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32), worst_mantissas(64), np.float32([1.0, 1.0 + 2.0 ** -8])])
    hi, lo = split(x)
    x64 = x.astype(np.float64)
    assert np.all(np.abs(x64 - hi) <= 2.0 ** -8 * np.abs(x64))
    assert np.all(np.abs(x64 - hi - lo) <= 2.0 ** -17 * np.abs(x64))
    # 8 significant bits, not 9: halfway between 1 and the next bf16 the error IS 2^-8 (ties to even: down)
    assert bf16_rne(np.float32([1.0 + 2.0 ** -8]))[0] == np.float32(1.0)


def test_truncation_stays_below_the_documented_term():
    worst = 0.0
    for name, q, t in CASES:
        err = abs(kept_dot(q, t) - exact_dot(q, t))
        bound = TRUNC * norms(q, t)
        assert err <= bound, (name, err, bound)
        worst = max(worst, err / bound)
    # the bound is not slack: the worst-case mantissas come within a few per cent of it
    assert worst > 0.9, worst
    # ... and they exceed 3 * 2^-18, the figure a 9-bit reading of bf16 would give
    w = worst_mantissas(256)
    assert abs(kept_dot(w, w) - exact_dot(w, w)) > 3.02 * 2.0 ** -18 * norms(w, w)


@pytest.mark.parametrize("defect", ["drop_lo_hi", "no_lo"])
def test_a_missing_term_exceeds_the_bound(defect):
    """The check can see a defect: without the lo.hi product, or with lo rounded to zero, typical vectors leave the bound."""
    over = 0
    for name, q, t in CASES:
        err = abs(kept_dot(q, t, **{defect: True}) - exact_dot(q, t))
        over += err > TRUNC * norms(q, t)
    assert over >= len(CASES) // 2, (over, len(CASES))
    w = worst_mantissas(256)
    assert abs(kept_dot(w, w, **{defect: True}) - exact_dot(w, w)) > TRUNC * norms(w, w)
