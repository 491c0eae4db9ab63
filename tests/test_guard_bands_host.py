"""tests/guard_bands.py proved on the CPU: a numpy fake entry point (tiled copy, row reduce and top-k, all with tile
rounding, working on raw allocations the way a kernel works on pointers) passes when it is correct and is rejected, by the
check meant for it, under each planted defect.  No GPU."""
import numpy as np
import pytest

from tests import guard_bands as GB

TR, TC = 4, 8                                       # the fake's tile: rows and columns are rounded up to these
R, C, K = 5, 11, 3                                  # neither a multiple of the tile; more than one tile each way


def _mem(g):
    """(typed view of the whole allocation, index of the payload's first element): a pointer, as a kernel sees it."""
    return g.buf.view(g.spec.dtype), g.offset // g.spec.dtype.itemsize


def fake_entry(b, rows, cols, k, defect=None):
    """copy[r][c] = x[r][c]; sums[r] = sum_c x[r][c] (float64 accumulation, in column order); ids[r][:k] = the columns of the k
    largest x[r][c], ties by lower column, NaN never chosen.  `keep` is an output this call is documented to leave alone."""
    x, xo = _mem(b["x"])
    cp, co = _mem(b["copy"])
    sm, so = _mem(b["sums"])
    ids, io = _mem(b["ids"])
    keep, ko = _mem(b["keep"])
    rp, cpad = GB.round_up(rows, TR), GB.round_up(cols, TC)
    skewed = b["x"].ptr % 16 != 0
    overread = defect == "overread" or (defect == "overread_skewed" and skewed)
    for r0 in range(0, rp, TR):
        for c0 in range(0, cpad, TC):
            for r in range(r0, r0 + TR):
                for c in range(c0, c0 + TC):
                    if r < rows and c < cols:
                        cp[co + r * cols + c] = x[xo + r * cols + c]
                    elif defect == "pad_row_after" and c < cols:       # the bound on r is missing: the padding rows are stored
                        cp[co + r * cols + c] = 0.0
    for r in range(rows):
        n = cols + 1 if (overread and r == rows - 1) else cols         # `<=` for `<` on the last row
        acc = np.float64(0)
        for c in range(n):
            acc += np.float64(x[xo + r * cols + c])
        sm[so + r] = acc
        width = cpad if (defect == "guard_id" and r == rows - 1) else cols   # top-k over the padded width
        vals = np.array([x[xo + r * cols + c] for c in range(width)], np.float64)
        vals[np.isnan(vals)] = -np.inf
        order = np.argsort(-vals, kind="stable")[:k]
        for j in range(k):
            ids[io + r * k + j] = order[j]
    if defect == "store_before":
        cp[co - 1] = 0.0
    if defect == "store_after":
        cp[co + rows * cols] = 0.0
    if defect == "store_input":
        x[xo + 2] = x[xo + 2] + 1.0
    if defect == "store_untouched":
        keep[ko + 1] = 0.0
    return 0


def _specs(x):
    g = GB.guard_bytes(R, C, 8, TR, TC)
    return dict(x=GB.spec(np.float32, R * C, "in", init=x, guard=g),
                copy=GB.spec(np.float32, R * C, "out", guard=g),
                sums=GB.spec(np.float64, R, "out", guard=g),
                ids=GB.spec(np.int64, R * K, "out", valid=2, guard=g, id_range=(0, C, ())),
                keep=GB.spec(np.float32, R, "untouched", guard=g))


def _x():
    return np.random.RandomState(5).uniform(0.0, 0.5, size=(R, C)).astype(np.float32)   # below the valid fill 1.0f


def _run(defect, skew):
    return GB.run_guarded(GB.NumpyBackend(), _specs(_x()), lambda b: fake_entry(b, R, C, K, defect), skew)


@pytest.mark.parametrize("skew", (0, 1))
def test_correct_fake_passes_and_is_right(skew):
    x = _x()
    before = GB.run_guarded.calls
    outs, status = _run(None, skew)
    assert GB.run_guarded.calls - before == len(GB.FILLS) == 2 and status == 0
    assert GB.same_bits(outs["copy"].reshape(R, C), x)
    assert np.array_equal(outs["sums"], np.array([np.sum(row.astype(np.float64)) for row in x]))
    assert np.array_equal(outs["ids"].reshape(R, K), np.argsort(-x.astype(np.float64), axis=1, kind="stable")[:, :K])


def test_placement_is_what_the_module_says():
    be = GB.NumpyBackend()
    for skew in (0, 1):
        for dt, step in ((np.float32, 4), (np.int32, 4), (np.float64, 8), (np.int64, 8), (np.uint64, 8)):
            g = GB.Guarded(be, "b", GB.spec(dt, 7, "out", valid=1), skew, "ones")
            assert g.ptr % 16 == skew * step and g.ptr % step == 0
            assert g.offset >= GB.MIN_GUARD and g.buf.size - g.offset - 7 * step >= GB.MIN_GUARD
    assert GB.guard_bytes(65, 500, 4) == 128 * 512 * 4 and GB.guard_bytes(65, 50, 4) == GB.MIN_GUARD == GB.guard_bytes(1, 1, 4)
    assert GB.guard_bytes(129, 40, 8, tile_rows=128, tile_cols=1) == GB.round_up(256 * 40 * 8, GB.ALIGN)
    ones = GB.Guarded(be, "b", GB.spec(np.float32, 3, "out"), 1, "ones")
    assert np.isnan(ones.buf.view(np.float32)).all() and (ones.buf.view(np.int32) == -1).all()
    valid = GB.Guarded(be, "b", GB.spec(np.int32, 3, "in", init=[4, 5, 6], valid=7), 1, "valid")
    cells = valid.buf.view(np.int32)
    o = valid.offset // 4
    assert list(cells[o:o + 3]) == [4, 5, 6] and (np.delete(cells, range(o, o + 3)) == 7).all()
    with pytest.raises(AssertionError):                      # a guard narrower than the payload is no guard
        GB.spec(np.float32, 1 << 20, "out", guard=GB.MIN_GUARD)


# defect -> (the check that must reject it, the skews at which it must; at the others the call must pass)
DEFECTS = {
    "store_before": ("skew gap", (1,)),              # with no skew the element before the payload is the front guard's last
    "store_after": ("back guard", (0, 1)),
    "pad_row_after": ("back guard", (0, 1)),
    "store_input": ("input payload", (0, 1)),
    "store_untouched": ("untouched region", (0, 1)),
    "overread": ("fill dependence", (0, 1)),
    "overread_skewed": ("fill dependence", (1,)),
    "guard_id": ("id out of range", (0, 1)),
}


@pytest.mark.parametrize("skew", (0, 1))
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_is_rejected_by_name(defect, skew):
    kind, skews = DEFECTS[defect]
    if defect == "store_before" and skew == 0:
        kind, skews = "front guard", (0,)
    if skew not in skews:
        _run(defect, skew)                                  # the defect is not active here: the harness must not cry wolf
        return
    with pytest.raises(GB.GuardViolation) as e:
        _run(defect, skew)
    assert e.value.kind == kind, str(e.value)
    want_buffer = dict(store_before="copy", store_after="copy", pad_row_after="copy", store_input="x", store_untouched="keep",
                       overread="sums", overread_skewed="sums", guard_id="ids")[defect]
    assert e.value.buffer == want_buffer, str(e.value)


def test_a_whole_padding_row_is_reported_with_its_extent():
    with pytest.raises(GB.GuardViolation) as e:
        _run("pad_row_after", 0)
    # rows 5 .. 7 of the padded 8 x 11 copy: the first store lands on element R * C, the last on 8 * C - 1
    assert "first at element %d, last at element %d" % (R * C, GB.round_up(R, TR) * C - 1) in str(e.value)


def test_a_status_raised_under_one_fill_only_is_a_failure():
    def call(b):
        fake_entry(b, R, C, K)
        x, xo = _mem(b["x"])
        return 1 if np.isnan(x[xo + R * C]) else 0          # an "error flag" that depends on the element behind the input
    with pytest.raises(GB.GuardViolation) as e:
        GB.run_guarded(GB.NumpyBackend(), _specs(_x()), call, 0)
    assert e.value.kind == "fill dependence" and e.value.buffer == "status"


def test_a_named_comparison_replaces_bit_identity_for_that_buffer_only():
    seen = []

    def call(b):
        fake_entry(b, R, C, K)
        sm, so = _mem(b["sums"])
        if b["sums"].fill == "valid":
            sm[so] = np.nextafter(sm[so], np.inf)            # a last-bit difference, as float atomics make
    with pytest.raises(GB.GuardViolation):
        GB.run_guarded(GB.NumpyBackend(), _specs(_x()), call, 0)
    GB.run_guarded(GB.NumpyBackend(), _specs(_x()), call, 0,
                   compare=dict(sums=lambda name, a, b: (seen.append(name), np.testing.assert_allclose(a, b, rtol=1e-12))))
    assert seen == ["sums"]
