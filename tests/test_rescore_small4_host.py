"""The summation order of rescore_small4_kernel (four queries per wave, one per 16-lane row; DESIGN K6) restated in numpy
float64: a row's lane l plays the virtual lanes l, l + 16, l + 32, l + 48 of the 64-lane form (wave_exact_dot), combines its
four accumulators as (acc0 + acc2) + (acc1 + acc3) and finishes with a xor 8, 4, 2, 1 butterfly.  That has to give the BITS
of the 64-lane xor 32, 16, 8, 4, 2, 1 butterfly over the same accumulators, in every lane, for the dot product's
dimension map (lane v: dimensions 4v .. 4v+3) and for the norm's (lane v: dimensions v, v + 64, ...).

A float32 x float32 product is exact in float64, so `acc + q * v` here is the kernels' fused multiply-add."""
import numpy as np
import pytest


def _accumulate(q, v, dims):
    """acc[r][lane] over rows r: the products of dims[lane][0], dims[lane][1], ... added in that order to +0.0; a dimension
    >= S is skipped (no addition), a lane without dimensions stays +0.0."""
    R, S = q.shape
    acc = np.zeros((R, 64), np.float64)
    for step in range(dims.shape[1]):
        d = dims[:, step]
        ok = d < S
        dc = np.minimum(d, S - 1)
        p = q[:, dc].astype(np.float64) * v[:, dc].astype(np.float64)
        acc = np.where(ok[None, :], acc + p, acc)
    return acc


def _butterfly(x, steps):
    idx = np.arange(x.shape[1])
    for m in steps:
        x = x + x[:, idx ^ m]
    return x


def _wave64(acc):
    return _butterfly(acc, (32, 16, 8, 4, 2, 1))                       # [R][64], every lane the total


def _row16(acc):
    a = [acc[:, 16 * i:16 * i + 16] for i in range(4)]                 # accumulator i of row lane l = virtual lane l + 16 i
    return _butterfly((a[0] + a[2]) + (a[1] + a[3]), (8, 4, 2, 1))     # [R][16]


DOT_DIMS = np.arange(64)[:, None] * 4 + np.arange(4)[None, :]          # wave_exact_dot: j = lane -> dimensions 4j .. 4j+3
NORM_DIMS = np.arange(64)[:, None] + 64 * np.arange(4)[None, :]        # |q|: d = lane, lane + 64, ...


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _rows(kind, rng, R, S):
    q = rng.standard_normal((R, S)).astype(np.float32)
    v = rng.standard_normal((R, S)).astype(np.float32)
    if kind == "cancellation":
        # huge terms of both signs around small ones: every grouping of the additions rounds differently
        big = (rng.randint(0, 2, (R, S)) * 2 - 1) * np.exp2(rng.randint(20, 60, (R, S)))
        mask = rng.rand(R, S) < 0.3
        q = np.where(mask, big, q).astype(np.float32)
        pair = rng.rand(R, S // 2) < 0.5                              # (S is even) exactly cancelling neighbours
        q[:, 1::2] = np.where(pair, q[:, 0::2], q[:, 1::2])
        v[:, 1::2] = np.where(pair, -v[:, 0::2], v[:, 1::2])
    elif kind == "signed_zeros":
        z = rng.rand(R, S)
        q = np.where(z < 0.4, np.float32(-0.0), np.where(z < 0.8, np.float32(0.0), q)).astype(np.float32)
        v[rng.rand(R, S) < 0.3] = np.float32(-0.0)
        q[0] = np.float32(-0.0)                                       # all products -0.0: the totals must be +0.0 both ways
        v[0] = np.float32(1.0)
        q[1] = np.float32(0.0)
    elif kind == "denormals":
        q = (q * np.float32(2.0 ** -140)).astype(np.float32)          # float32 subnormals (kept, not flushed)
        sel = rng.rand(R, S) < 0.5
        v = np.where(sel, v * np.float32(2.0 ** -130), v).astype(np.float32)
        assert (np.abs(q[q != 0]) < np.finfo(np.float32).tiny).any()
    return q, v


@pytest.mark.parametrize("S", [256, 64, 50])
@pytest.mark.parametrize("kind", ["random", "cancellation", "signed_zeros", "denormals"])
def test_four_accumulators_per_row_lane_equal_the_64_lane_butterfly_bit_for_bit(S, kind):
    rng = np.random.RandomState(S * 7 + len(kind))
    q, v = _rows(kind, rng, 400, S)
    with np.errstate(over="ignore", invalid="ignore"):
        for dims in (DOT_DIMS, NORM_DIMS):
            acc = _accumulate(q, v if dims is DOT_DIMS else q, dims)
            want, got = _wave64(acc), _row16(acc)
            assert np.array_equal(_bits(want), _bits(np.tile(got, (1, 4))))   # every lane of the row holds the 64-lane total
    if kind == "signed_zeros":
        assert _bits(_row16(_accumulate(q, v, DOT_DIMS)))[0, 0] == 0          # +0.0, not -0.0


def test_the_test_can_tell_summation_orders_apart():
    """The same accumulators combined as ((acc0 + acc1) + acc2) + acc3 differ in the last bits on cancelling rows: the
    comparison above is not vacuous."""
    rng = np.random.RandomState(1)
    q, v = _rows("cancellation", rng, 400, 256)
    acc = _accumulate(q, v, DOT_DIMS)
    a = [acc[:, 16 * i:16 * i + 16] for i in range(4)]
    other = _butterfly(((a[0] + a[1]) + a[2]) + a[3], (8, 4, 2, 1))
    assert not np.array_equal(_bits(_wave64(acc)[:, :16]), _bits(other))


def test_empty_virtual_lanes_are_explicit_zero_terms():
    """S = 64 and 50 leave virtual lanes 16 .. 63 (14 .. 63) without dimensions: their accumulators are +0.0 and take part
    in every addition of both forms."""
    for S in (64, 50):
        acc = _accumulate(np.ones((1, S), np.float32), np.ones((1, S), np.float32), DOT_DIMS)
        assert np.all(acc[0, (S + 3) // 4:] == 0.0) and not np.signbit(acc[0, (S + 3) // 4:]).any()
        assert _row16(acc)[0, 0] == float(S) == _wave64(acc)[0, 0]
