"""Text-CNN encodings against the float64 oracle, on every forward branch.

encode_source in network_mode source_only_cnn runs conv_pool_kernel<false,NB> + proj_norm_kernel (fp32) or
conv_pool_bf16_kernel<NB,false> + the split-operand projection (option cnn_bf16), NB = 8 or 4 sequences per workgroup by
(T, E).  tests/test_gpu_cnn.py holds them to 1e-4 against the float32 oracle at six shapes; here the reference is the oracle
run in float64 on the float32 (for bf16: the bf16-rounded) parameters, the shapes sit on the kernels' edges -- position tiles
exactly full and one over, Ep / Ep8 padding, the half k-group, partial workgroups and projection tiles -- and the data is
asserted to put a winning position on each side of every tile boundary, so that a masking or off-by-one defect there cannot
hide.  The bars follow the rule of the gradient bars (tests/util.py): 25x what the float32 oracle differs from float64
(<= 3.2e-7 on normalised rows, <= 8.7e-7 * max|raw| on raw ones), i.e. FWD_BAR_NORM absolute on normalised encodings and
FWD_BAR_RAW * max|want| on raw ones.  tests/test_cnn_forward_check.py (CPU) re-measures the float32 oracle on this case list
with 10x margin, asserts the preconditions and shows that known forward defects exceed the bars."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import model_params, oracle_float64, oracle_params, random_ids

pytestmark = pytest.mark.gpu

FWD_BAR_NORM = 1e-5
FWD_BAR_RAW = 2e-5
BOUNDARY_POSITIONS = (0, 31, 32, 63, 64, 95, 96)


def _fc(cid, V, E, S, T, B, seed=0, **kw):
    return dict(id=cid, V=V, E=E, S=S, T=T, B=B, seed=seed, **kw)


# Sequences per workgroup, from the launchers: fp32 inference 8 while T * Ep <= ~4,540 (Ep = E rounded up to 4; the training
# layout, with the arg-max keys, only to ~3,940), bf16 inference 8 while T * Ep8 <= ~9,080; else 4.  A case with T >= 33 has at
# least B rows: rows without left padding are added until every tile-boundary position wins somewhere (boundary_misses).
FORWARD_CASES = [
    _fc("t5-e1-b1", 40, 1, 4, 5, 1),                      # one position for width 5; E 1 (Ep 4, Ep8 8); one row, S 4
    _fc("t31-e3-b7", 60, 3, 50, 31, 7),                   # one position short of a full tile; partial workgroup of 8
    _fc("t32-e4-b8", 80, 4, 100, 32, 8),                  # P = 31..28; E 4: fs * E % 8 == 4 with no padding column (fs 3, 5)
    _fc("t12-e7-b9", 80, 7, 50, 12, 9),                   # one row into a second workgroup
    _fc("t20-e24-b33", 90, 24, 64, 20, 33),               # one row into a second 32-row projection tile
    _fc("t12-e7-b1093", 90, 7, 100, 12, 1093),            # many workgroups and projection tiles, the last ones partial
    _fc("t33-e7", 80, 7, 50, 33, 8),                      # P = 32 for width 2 only: position 32 exists for no other width
    _fc("t36-e60", 150, 60, 64, 36, 8),                   # P = 35..32 straddles the tile; E 60: the half k-group (fs 3, 5)
    _fc("t64-e50-s512", 200, 50, 512, 64, 8),             # two tiles, the second one short by fs - 1; 16 column tiles
    _fc("t68-e63", 150, 63, 100, 68, 8),                  # P = 67..64: a third tile for some widths only; 8 per workgroup in
                                                          # the inference layout where the training layout takes 4
    _fc("t96-e64", 150, 64, 64, 96, 8),                   # three tiles; E 64; 4 per workgroup (fp32), 8 (bf16)
    _fc("t144-e64", 150, 64, 32, 144, 8),                 # 4 per workgroup in both precisions (T * Ep8 = 9,216)
    _fc("t150-e50", 120, 50, 32, 150, 8),                 # five tiles, P = 149..146
    _fc("pads", 80, 24, 64, 33, 12, kind="pads"),         # all-PAD rows, rows of one repeated id, duplicate rows
    # features exactly 0 (about half), an all-zero row; the seed keeps the smallest live feature above 5e-5 in both precisions
    _fc("dead", 80, 24, 64, 20, 8, seed=1, kind="dead", conv_bias=-0.15, zero_pad_row=True),
    _fc("scale-1e3", 80, 24, 64, 20, 8, scale=1e3),       # nothing in the kernels may depend on magnitude
    _fc("scale-1e-3", 80, 24, 64, 20, 8, scale=1e-3),
]


def boundary_misses(p, ids):
    """[(filter width, position)] of the positions 0, 31, 32, 63, 64, 95, 96 (those < P) and P - 1 that are NOT the arg-max of a
    live feature of any sequence without left padding.  p as the oracle is to read it (rounded beforehand for bf16)."""
    rows = ids[ids[:, 0] != 0]
    if len(rows) == 0:
        return [(fs, -1) for fs in O.CNN_FILTER_SIZES]
    _, tape = O.cnn_forward(p, rows, keep_tape=True)
    out = []
    for fs, (_, hconv) in zip(O.CNN_FILTER_SIZES, tape):
        P = hconv.shape[1]
        best = hconv.argmax(axis=1)
        won = set(best[hconv.max(axis=1) > 0].tolist())
        out += [(fs, pos) for pos in sorted(set(BOUNDARY_POSITIONS + (P - 1,))) if pos < P and pos not in won]
    return out


def rounded(p):
    """The parameters the bf16 variant computes with: embedding and filters rounded to bf16 (done in float32, before any
    float64 mode: bf16_round works on float32 bits)."""
    return {k: (O.bf16_round(v) if k == "word_embedding" or k.endswith("/W") else v) for k, v in p.items()}


def forward_case(c):
    """(model params, oracle parameter dict, ids) of a forward case."""
    params = model_params("source_only_cnn", c["V"], c["E"], 96, 96, c["S"], c["T"], N=11)
    p = oracle_params(params, seed=2 + c["seed"])
    if c.get("scale"):
        p["word_embedding"] = (p["word_embedding"] * np.float32(c["scale"])).astype(np.float32)
    if c.get("conv_bias") is not None:
        for k in p:
            if k.endswith("/b"):
                p[k] = np.full_like(p[k], c["conv_bias"])
    if c.get("zero_pad_row"):
        p["word_embedding"][0] = 0.0               # with biases below 0 an all-PAD row has no live feature at all
    rng = np.random.RandomState(40 + c["seed"])
    B, T, V = c["B"], c["T"], c["V"]
    ids = random_ids(rng, B, T, V, pad_frac=0.5)
    kind = c.get("kind")
    if kind == "pads":
        ids[0] = 0                                 # all PAD
        ids[1] = 0
        ids[2] = 7                                 # one repeated id
        ids[3] = 1                                 # all EOS
        ids[5] = ids[4]                            # duplicate rows, far apart too
        ids[B - 1] = ids[4]
    elif kind == "dead":
        ids[3] = 0
    if T >= 33 and kind is None:
        p16 = rounded(p)
        for _ in range(40):
            if not boundary_misses(p, ids) and not boundary_misses(p16, ids):
                break
            ids = np.concatenate([ids, random_ids(rng, 4, T, V)])
    return params, p, ids


def reference_encode(p, params, ids, normalize, bf16, float64=True):
    """The oracle's encoding; float64: run in float64 on the float32 (bf16: rounded) parameters."""
    if not float64:
        return O.encode(p, params, "src", ids, normalize=normalize, cnn_bf16=bf16)
    if bf16:
        p = rounded(p)
    with oracle_float64():
        return O.encode({k: np.asarray(v, np.float64) for k, v in p.items()}, params, "src", ids, normalize=normalize)


def encoding_error(got, want, normalize):
    """(error in units of the bar's scale, the scale, worst index): absolute on normalised rows, relative to max|want| on raw."""
    scale = 1.0 if normalize else float(np.abs(want).max())
    d = np.abs(np.asarray(got, np.float64) - want)
    worst = np.unravel_index(int(np.argmax(d)), d.shape)
    return (float(d.max()) / scale if scale > 0 else (0.0 if not d.any() else np.inf)), scale, worst


def check_encoding(got, want, normalize, what="", margin=1.0):
    """Asserts the bar (divided by margin); a failure names the case, the worst element and its two values."""
    err, scale, worst = encoding_error(got, want, normalize)
    bar = (FWD_BAR_NORM if normalize else FWD_BAR_RAW) / margin
    assert got.shape == want.shape and np.isfinite(got).all(), what
    assert err <= bar, ("%s%s: max|d| %.3g of scale %.3g (bar %.1e), worst at row %d column %d: got %r, want %r"
                        % (what, "normalised" if normalize else "raw", err, scale, bar, worst[0], worst[1],
                           float(got[worst]), float(want[worst])))
    return err


def _model(params, p, bf16):
    import sse_amd
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    if bf16:
        m.handle.set_option("cnn_bf16", 1)
    return m


def _compare(m, p, params, ids, bf16, what):
    errs = []
    for normalize in (True, False):
        want = reference_encode(p, params, ids, normalize, bf16)
        got = m.encode_source(ids, normalize=normalize)
        errs.append(check_encoding(got, want, normalize, what))
    print("FWDERR %s: normalised %.2e, raw %.2e (of max|want|), %d rows" % (what.strip(": "), errs[0], errs[1], len(ids)))
    return errs


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in FORWARD_CASES])
def test_encodings_match_float64(c, bf16):
    params, p, ids = forward_case(c)
    if c["T"] >= 33 and c.get("kind") is None:     # every tile boundary carries a winning position, in float64 as well
        with oracle_float64():
            pp = rounded(p) if bf16 else p
            assert boundary_misses({k: np.asarray(v, np.float64) for k, v in pp.items()}, ids) == []
    m = _model(params, p, bf16)
    _compare(m, p, params, ids, bf16, "%s %s: " % (c["id"], "bf16" if bf16 else "fp32"))
    if c.get("kind") == "dead":
        pool = O.cnn_forward(rounded(p) if bf16 else p, ids)
        assert 0.2 < np.mean(pool == 0) < 0.8 and not pool[3].any() and pool[0].any()
        for normalize in (True, False):            # no live feature: zeros through the normalise clamp, exactly
            assert not m.encode_source(ids, normalize=normalize)[3].any()
    if c.get("kind") == "pads":
        got = m.encode_source(ids)
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[4], got[5]) and np.array_equal(got[4], got[-1])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_largest_accepted_length_matches_float64(bf16):
    """E = 64: T walked down from a rejected one (the message names LDS) to the first that encode_source accepts; the boundary
    is the library's, not restated here.  There the LDS tile of the 4-sequence kernel is as full as it gets."""
    import sse_amd
    c = _fc("largest", 150, 64, 32, 0, 9)
    rejected = 0
    for T in range(150, 4, -1):
        c["T"] = T
        params, p, ids = forward_case(dict(c, kind="plain"))        # (no boundary search while walking)
        m = _model(params, p, bf16)
        try:
            m.encode_source(ids[:2])
        except sse_amd.SSEError as e:
            assert "LDS" in str(e), str(e)
            rejected += 1
            continue
        break
    assert rejected > 0, "T = 150 was expected to be rejected"
    params, p, ids = forward_case(c)
    with oracle_float64():
        pp = rounded(p) if bf16 else p
        assert boundary_misses({k: np.asarray(v, np.float64) for k, v in pp.items()}, ids) == []
    for normalize in (True, False):                # the float32 oracle is 10x inside the bar here too
        check_encoding(reference_encode(p, params, ids, normalize, bf16, float64=False),
                       reference_encode(p, params, ids, normalize, bf16), normalize, "float32 oracle: ", margin=10.0)
    _compare(_model(params, p, bf16), p, params, ids, bf16, "largest T %d %s: " % (T, "bf16" if bf16 else "fp32"))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_a_row_does_not_depend_on_its_batch(bf16):
    c = next(c for c in FORWARD_CASES if c["id"] == "t12-e7-b1093")
    params, p, ids = forward_case(c)
    m = _model(params, p, bf16)
    for normalize in (True, False):
        whole = m.encode_source(ids, normalize=normalize)
        for r in (0, 7, 8, 31, 32, 1087, 1088, 1092):
            alone = m.encode_source(ids[r:r + 1], normalize=normalize)
            assert np.array_equal(alone[0], whole[r]), (r, normalize)
        part = m.encode_source(ids[1000:1093], normalize=normalize)
        assert np.array_equal(part, whole[1000:1093]), normalize


@pytest.mark.parametrize("cid", ["t36-e60", "t96-e64"])
def test_bf16_option_off_again_gives_the_fp32_bits(cid):
    params, p, ids = forward_case(next(c for c in FORWARD_CASES if c["id"] == cid))
    m = _model(params, p, False)
    exact = m.encode_source(ids)
    m.handle.set_option("cnn_bf16", 1)
    assert not np.array_equal(m.encode_source(ids), exact)
    m.handle.set_option("cnn_bf16", 0)
    assert np.array_equal(m.encode_source(ids), exact)
