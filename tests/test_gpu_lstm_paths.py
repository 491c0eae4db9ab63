"""LSTM inference encodings against the float64 oracle, kernel by kernel, each case proving by counter which kernel ran.

An LSTM encode goes to one of six kernels (choose_lstm_path in csrc/sse_api.hip, then the matrix kernel's launcher): the
single-query cluster kernel (lstm_persist.hip), the MFMA cluster kernel (lstm_cluster.hip), the few-sequences kernel
(lstm_small.hip), the fp32 matrix kernel (lstm_fwd.hip at 32- or 64-row tiles, unit-block or gate-split (lstm_fwd_gs.hip),
embedding gather or x-projection table), the split-bf16 matrix kernel (lstm_fwd_x3.hip, opt-in) and the any-shape path
(lstm_generic.hip).  The chooser falls through silently, so every case here forces its kernel with the library's options and
then ASSERTS through the counters lstm_path_* / lstm_fwd_* (include/sse_hip.h) that exactly this kernel ran, once per
encode, and that lstm_persist_fallbacks did not move: a cluster kernel that gives up on a busy device fails the case, it
does not pass on another kernel.  tests/test_gpu_encode.py holds the kernels to each other bit for bit and to the float32
oracle at 1e-4; here the reference is the oracle run in float64 on the float32 parameters, the shapes sit on the launchers'
edges, and the magnitude cases (zero LSTM biases, the reference's initialiser, with the embedding scaled by 1 .. 1e-5 and by
1e2 and 1e3) hold the kernels to the principle of tests/test_gpu_cnn_paths.py: nothing may depend on magnitude.

The bars follow the rule of tests/util.py and tests/test_gpu_cnn_paths.py: 25x what the float32 oracle differs from its
float64 run over this file's whole case list (3.62e-7 on normalised rows, 1.09e-6 * max|raw| on raw ones, both at the
8,250-row case xt64-h256; re-measured by tests/test_lstm_forward_check.py), rounded to one significant digit: 9e-6 absolute
on normalised encodings, 3e-5 * max|want| on raw ones; the 1e3 cases run on bars of their own, see BARS_EXACT_OVERFLOW.  (The
text-CNN file's constants, 1e-5 and 2e-5, come from the same rule on its own list; they are not these.)  The split-bf16 kernel
gets 10x that, the ratio of GRAD_BARS_SPLIT to GRAD_BARS_EXACT for the same hi + lo arithmetic; a numpy emulation of the
documented split stays inside it with margin (same CPU file, which also asserts every case's preconditions and shows that
planted defects exceed the bars, that the exponential-only tanh the kernels had before exceeds them from an embedding scale
of 1e-2 down, and that the formula they have now stays 2.5x inside).

Largest device errors (the LSTMFWDERR lines) per kernel over the case list on an MI355X, normalised / raw of max|want|, the
1e3 cases apart (DESIGN.md K2a has the same table):
    few-sequences (14 cases) 3.34e-7 / 9.67e-7       single-query cluster (15) 1.90e-7 / 7.77e-7    MFMA cluster (12) 4.12e-7 / 9.92e-7
    matrix 32-row (25) 2.96e-7 / 1.05e-6             matrix 64-row, unit-block (6) and gate-split (7) 3.42e-7 / 1.05e-6
    x-table 32-row (12) 3.39e-7 / 1.12e-6            x-table 64-row (1) 3.84e-7 / 1.17e-6           any-shape (3) 2.92e-7 / 7.53e-7
    split-bf16 (10) 3.16e-6 / 1.13e-5                1e3: exact kernels (5) 4.34e-7 / 1.03e-6       1e3: split-bf16 (1) 1.02e-5 / 3.88e-5
Every exact kernel is within 1.2x of the float32 oracle's own distance.  The same magnitude cases with the exponential-only
tanh the kernels had before (normalised error, every exact kernel alike): 0.1 -> 6e-6 .. 8e-6 (inside the bar), 1e-2 -> 6e-5 ..
7e-5, 1e-3 -> 5e-4 (9e-4 at 8,257 rows), 1e-5 -> 5e-2 .. 6e-2."""
import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.test_gpu_cnn_paths import encoding_error
from tests.util import model_params, oracle_float64, oracle_params, random_ids

pytestmark = pytest.mark.gpu

BARS_EXACT = (9e-6, 3e-5)                         # (normalised: absolute, raw: of max|want|)
BARS_SPLIT = (9e-5, 3e-4)
# The 1e3 magnitude cases, added to the issue's list for the overflow of exp2, on bars of their own by the same rule: gates that
# are 0 or 1 almost everywhere leave the few that are not badly conditioned, and the float32 oracle itself is 8.0e-7 / 1.84e-6 from
# float64 there -- inside the list they would have widened everybody's bar to 2e-5 / 5e-5.
BARS_EXACT_OVERFLOW = (2e-5, 5e-5)
BARS_SPLIT_OVERFLOW = (2e-4, 5e-4)

PATH_COUNTERS = ("lstm_path_persist", "lstm_path_cluster", "lstm_path_small", "lstm_path_x3", "lstm_path_generic", "lstm_path_fwd",
                 "lstm_fwd_rows32", "lstm_fwd_rows64", "lstm_fwd_gate_split", "lstm_fwd_x_table")
_MATRIX = dict(lstm_small_rows=0, lstm_persist_rows=0, lstm_cluster_rows=0)
# kernel -> (options that force it, the counters that move by one per encode; every other one stays, entry point)
KERNELS = {
    "persist": (dict(), ("lstm_path_persist",), "host"),
    "cluster": (dict(), ("lstm_path_cluster",), "host"),
    "small": (dict(lstm_persist_rows=0, lstm_cluster_rows=0), ("lstm_path_small",), "host"),
    "fwd32": (dict(_MATRIX, lstm_x_table=0), ("lstm_path_fwd", "lstm_fwd_rows32"), "host"),
    "fwd64": (dict(_MATRIX, lstm_x_table=0, pad_sort_dev=0), ("lstm_path_fwd", "lstm_fwd_rows64"), "dev"),
    "fwd64gs": (dict(_MATRIX, lstm_x_table=0, pad_sort_dev=0), ("lstm_path_fwd", "lstm_fwd_rows64", "lstm_fwd_gate_split"), "dev"),
    "xt32": (dict(_MATRIX, lstm_x_table=2), ("lstm_path_fwd", "lstm_fwd_rows32", "lstm_fwd_x_table"), "host"),
    "xt64": (dict(_MATRIX, lstm_x_table=2, pad_sort_dev=0), ("lstm_path_fwd", "lstm_fwd_rows64", "lstm_fwd_x_table"), "dev"),
    "x3": (dict(_MATRIX, lstm_x3=1), ("lstm_path_x3",), "host"),
    "generic": (dict(), ("lstm_path_generic",), "host"),
}


def _lc(cid, kernel, V, E, H, S, T, B, seed=0, pad=0.6, **kw):
    return dict(id=cid, kernel=kernel, V=V, E=E, H=H, S=S, T=T, B=B, seed=seed, pad=pad, **kw)


def _magnitude(prefix, kernel, V, E, H, S, T, B, **kw):
    """Zero LSTM biases (the reference initialiser: pre-activations as small as the embedding makes them) and the embedding
    scaled.  1e2 saturates the gates (tanh = +-1 to the last bit), but with pre-activations of 16 .. 29 no exp2 overflows
    yet -- the issue expected that of 1e2; 1e3 is added for it: exp2 = inf in both exponential forms, which must still give
    +-1 / 0 / 1, finite."""
    return [_lc("%s-mag-%s" % (prefix, name), kernel, V, E, H, S, T, B, zero_bias=True, scale=scale, overflow=scale > 1e2, **kw)
            for name, scale in (("1", 1.0), ("0.1", 0.1), ("1e-2", 1e-2), ("1e-3", 1e-3), ("1e-5", 1e-5), ("1e2", 1e2), ("1e3", 1e3))]


# The edges are the launchers'.  Where the list of the issue and the code disagree the comment says so.
LSTM_CASES = (
    # ---- few-sequences kernel: 4 rows per workgroup (LS_RB), up to lstm_small_rows = 1024 rows
    [_lc("small-b%d" % B, "small", 300, 50, 96, 64, 12, B) for B in (1, 3, 4, 5)] +
    [_lc("small-b1023", "small", 300, 50, 96, 64, 6, 1023), _lc("small-b1024", "small", 300, 50, 96, 64, 6, 1024),
     _lc("small-h256-pads", "small", 500, 50, 256, 256, 32, 37, kind="pads"),
     # ---- single-query cluster kernel: 4 sequences x 8 clusters (B <= 32), 16 workgroups per cluster
     _lc("persist-b1", "persist", 500, 50, 256, 256, 32, 1, pad=0.0),
     _lc("persist-b4", "persist", 500, 50, 256, 256, 32, 4), _lc("persist-b5", "persist", 500, 50, 256, 256, 32, 5),
     _lc("persist-b29", "persist", 300, 50, 96, 64, 20, 29, kind="pads"), _lc("persist-b32", "persist", 300, 50, 96, 64, 20, 32),
     # H = 200: 13 units per workgroup, the last one owns 5 (uneven).  The issue names H = 300 for this: 300 units need 32
     # workgroups per cluster, 8 x 32 x 2 = 512 compute units for the co-residency rule of choose_lstm_path, and the device has
     # 256 -- the chooser sends H = 300 to the few-sequences kernel (case persist-h300-goes-small pins that).
     _lc("persist-h200", "persist", 200, 50, 200, 128, 12, 7),
     _lc("persist-h300-goes-small", "small", 200, 50, 300, 128, 12, 7, opts=dict(lstm_persist_rows=32, lstm_cluster_rows=1024)),
     # The issue names H = 16 for workgroups that own no unit; with 16 workgroups per cluster H = 16 gives each exactly one.
     # H = 40 is ceil(40 / 16) = 3 units per workgroup: workgroups 14 and 15 own none.  Both are here.
     _lc("persist-h16", "persist", 90, 8, 16, 64, 9, 6), _lc("persist-h40", "persist", 90, 8, 40, 64, 9, 6),
     _lc("persist-s512", "persist", 90, 8, 16, 512, 9, 3),
     # ---- MFMA cluster kernel: 64-row tiles, launches of lstm_cluster_rows = 1024 rows, up to 3 of them
     _lc("cluster-b33", "cluster", 500, 50, 256, 256, 32, 33), _lc("cluster-b64", "cluster", 300, 50, 128, 64, 12, 64),
     _lc("cluster-b65", "cluster", 300, 50, 129, 64, 12, 65, kind="pads"),
     _lc("cluster-b1024", "cluster", 300, 50, 128, 64, 6, 1024), _lc("cluster-b1025", "cluster", 300, 40, 200, 50, 6, 1025),
     _lc("cluster-b3072", "cluster", 300, 40, 72, 50, 6, 3072),
     # ---- matrix kernel, 32-row tiles (B <= 8192), embedding gather
     _lc("fwd32-b1", "fwd32", 500, 50, 256, 256, 32, 1), _lc("fwd32-b31", "fwd32", 300, 50, 96, 64, 12, 31),
     _lc("fwd32-b32", "fwd32", 300, 50, 128, 64, 12, 32), _lc("fwd32-b33", "fwd32", 300, 50, 129, 64, 12, 33),
     _lc("fwd32-h32-e1-s1", "fwd32", 40, 1, 32, 1, 9, 5), _lc("fwd32-h64-e7-s31", "fwd32", 80, 7, 64, 31, 9, 9),
     _lc("fwd32-h65-e8-s32", "fwd32", 80, 8, 65, 32, 9, 9), _lc("fwd32-h200-e9-s33", "fwd32", 80, 9, 200, 33, 9, 9),
     _lc("fwd32-h257-e63-s50", "fwd32", 150, 63, 257, 50, 9, 9), _lc("fwd32-h300-e64", "fwd32", 150, 64, 300, 64, 9, 40),
     _lc("fwd32-h512-s512", "fwd32", 200, 50, 512, 512, 12, 45),
     _lc("fwd32-t1", "fwd32", 300, 50, 96, 64, 1, 40), _lc("fwd32-t2", "fwd32", 300, 50, 256, 64, 2, 40),
     _lc("fwd32-t1000", "fwd32", 200, 50, 96, 64, 1000, 3, pad=0.9),
     _lc("fwd32-pads-host", "fwd32", 300, 50, 256, 64, 40, 200, kind="pads"),                    # host counting sort, row_map
     _lc("fwd32-pads-noskip", "fwd32", 300, 50, 96, 64, 40, 200, kind="pads", opts=dict(pad_skip=0)),
     _lc("fwd32-pads-dev-sorted", "fwd32", 300, 50, 256, 64, 40, 200, kind="pads", entry="dev", opts=dict(pad_sort_dev=2), pad_sorted=1),
     _lc("fwd32-pads-dev-unsorted", "fwd32", 300, 50, 96, 64, 40, 200, kind="pads", entry="dev", opts=dict(pad_sort_dev=0), pad_sorted=0),
     # a heavily padded batch above 8192 rows through the host entry: padded_hint -> force_rows 32 where a dense one takes 64
     _lc("fwd32-pads-host-forced", "fwd32", 300, 50, 96, 64, 10, 8300, pad=0.95, kind="pads", padded_hint=True),
     # ---- matrix kernel, 64-row tiles (B > 8192, not a multiple of 64), gate-split kernel on and off
     ] +
    [_lc("fwd64-gs-h%d" % H, "fwd64gs", 300, 50, H, 64, 6, 8200 + H) for H in (40, 64, 72, 96, 128)] +
    [_lc("fwd64-h%d" % H, "fwd64", 300, 50, H, 64, 6, 8200 + H, opts=dict(lstm_gate_split=0)) for H in (40, 64, 72, 96, 128)] +
    [_lc("fwd64-h256", "fwd64", 300, 50, 256, 64, 6, 8250),
     # ---- x-projection table (Hp = 256 / 512): V not a multiple of 32, ids hold V - 1 and 0
     _lc("xt32-h129", "xt32", 203, 50, 129, 64, 12, 70, kind="vmax"), _lc("xt32-h256", "xt32", 501, 50, 256, 256, 32, 70, kind="vmax"),
     _lc("xt32-h300", "xt32", 203, 50, 300, 64, 12, 70, kind="vmax"), _lc("xt32-h512", "xt32", 203, 50, 512, 128, 12, 45, kind="vmax"),
     _lc("xt64-h256", "xt64", 203, 50, 256, 64, 6, 8250, kind="vmax"),
     # ---- any-shape path: cell or encoding beyond 512, an embedding beyond the fused LDS tile (Hp = 128: E >= 383)
     _lc("generic-h513", "generic", 100, 20, 513, 64, 6, 9), _lc("generic-s513", "generic", 100, 20, 64, 513, 6, 9),
     _lc("generic-e400", "generic", 100, 400, 64, 64, 6, 9),
     # ---- split-bf16 matrix kernel (cells 64 .. 256, E < 64)
     _lc("x3-h64-e8", "x3", 300, 8, 64, 64, 12, 70), _lc("x3-h96-e50", "x3", 300, 50, 96, 64, 12, 70, kind="pads"),
     _lc("x3-h256-e63", "x3", 300, 63, 256, 256, 32, 70), _lc("x3-h256-dense", "x3", 300, 50, 256, 64, 12, 1100, pad=0.0),
     ] +
    # ---- magnitude, on every kernel family
    _magnitude("fwd32", "fwd32", 500, 50, 256, 256, 32, 64) + _magnitude("small", "small", 300, 50, 96, 64, 80, 9) +
    _magnitude("cluster", "cluster", 500, 50, 256, 256, 32, 70) + _magnitude("persist", "persist", 500, 50, 256, 256, 32, 5) +
    _magnitude("xt32", "xt32", 501, 50, 256, 256, 32, 64, kind="vmax") + _magnitude("x3", "x3", 500, 50, 256, 256, 32, 64) +
    [_lc("fwd64-gs-mag-1e-3", "fwd64gs", 300, 50, 96, 64, 6, 8257, zero_bias=True, scale=1e-3)]
)


def lstm_case(c):
    """(model params, oracle parameter dict, ids) of a case."""
    params = model_params("dual-encoder", c["V"], c["E"], c["H"], c["H"], c["S"], c["T"])
    p = oracle_params(params, seed=3 + c["seed"], bias_scale=0.0 if c.get("zero_bias") else 0.2)
    if c.get("scale"):
        p["word_embedding"] = (p["word_embedding"] * np.float32(c["scale"])).astype(np.float32)
    rng = np.random.RandomState(50 + c["seed"])
    B, T, V = c["B"], c["T"], c["V"]
    ids = random_ids(rng, B, T, V, pad_frac=c["pad"])
    if c.get("kind") == "pads":                    # every prefix length 0 .. T - 1, an all-PAD row, a PAD inside a sequence
        assert B >= T + 3
        for r in range(T + 1):
            ids[B - 1 - r] = rng.randint(2, V, size=T)
            ids[B - 1 - r, :r] = 0
        ids[0] = rng.randint(2, V, size=T)
        ids[0, T // 2] = 0
    if c.get("kind") == "vmax":
        ids[1, -2:] = V - 1
        ids[2, 0] = V - 1
        ids[3, :] = 0
    return params, p, ids


def lead_counts(ids):
    """Leading-PAD count per row."""
    nz = ids != 0
    return np.where(nz.any(axis=1), nz.argmax(axis=1), ids.shape[1])


def reference_encodings(p, params, side, ids, float64=True):
    """{normalize: encoding} from the oracle; float64: run in float64 on the float32 parameters."""
    with np.errstate(over="ignore"):               # (the oracle's exp(-x) at the saturated cases: inf, sigmoid 0)
        if not float64:
            raw = O.encode(p, params, side, ids, normalize=False)
            return {True: O.l2_normalize(raw), False: raw}
        with oracle_float64():
            raw = O.encode({k: np.asarray(v, np.float64) for k, v in p.items()}, params, side, ids, normalize=False)
            return {True: O.l2_normalize(raw), False: raw}


def bars_of(c, kernel=None):
    """The bars of a case on its kernel (kernel="exact": on the exact fp32 arithmetic whatever its kernel)."""
    if (kernel or c["kernel"]) == "x3":
        return BARS_SPLIT_OVERFLOW if c.get("overflow") else BARS_SPLIT
    return BARS_EXACT_OVERFLOW if c.get("overflow") else BARS_EXACT


def check_encoding(got, want, normalize, bars, what="", margin=1.0):
    """Asserts the bar (divided by margin); a failure names the case, the worst element and its two values."""
    err, scale, worst = encoding_error(got, want, normalize)
    bar = (bars[0] if normalize else bars[1]) / margin
    assert got.shape == want.shape and np.isfinite(got).all(), "%snot finite / wrong shape" % what
    assert err <= bar, ("%s%s: max|d| %.3g of scale %.3g (bar %.1e), worst at row %d column %d: got %r, want %r"
                        % (what, "normalised" if normalize else "raw", err, scale, bar, worst[0], worst[1],
                           float(got[worst]), float(want[worst])))
    return err


def options_of(c):
    opts = dict(KERNELS[c["kernel"]][0])
    opts.update(c.get("opts", {}))
    return opts


def _model(c, params, p):
    import sse_amd
    m = sse_amd.SSEModel(params)
    m.set_variables(p)
    for k, v in options_of(c).items():
        m.handle.set_option(k, v)
    return m


def _counters(h):
    return {n: h.get_counter(n) for n in PATH_COUNTERS + ("lstm_persist_fallbacks", "lstm_x_table_builds", "pad_sorted_calls")}


def _encode(m, c, side, ids, normalize):
    entry = c.get("entry", KERNELS[c["kernel"]][2])
    if entry == "host":
        return (m.encode_source if side == "src" else m.encode_target)(ids, normalize=normalize)
    import torch
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(ids).to(dev)
    out = torch.full((len(ids), c["S"]), float("nan"), dtype=torch.float32, device=dev)
    m.handle.encode_dev(0 if side == "src" else 1, d.data_ptr(), len(ids), ids.shape[1], normalize, out.data_ptr())
    m.handle.synchronize()
    return out.cpu().numpy()


def assert_kernel_ran(c, before, after, calls, what):
    """The path counters moved by `calls` for the case's kernel and not at all for any other; no cluster give-up."""
    moved = {n: after[n] - before[n] for n in before}
    assert moved["lstm_persist_fallbacks"] == 0, \
        "%sa cluster kernel gave up (device busy?) and the batch was re-run on another kernel: %r" % (what, moved)
    want = {n: (calls if n in KERNELS[c["kernel"]][1] else 0) for n in PATH_COUNTERS}
    got = {n: moved[n] for n in PATH_COUNTERS}
    assert got == want, "%sthe encode did not take the %s kernel: counters moved %r, expected %r" % (what, c["kernel"], got, want)
    if "pad_sorted" in c:
        assert moved["pad_sorted_calls"] == c["pad_sorted"] * calls, (what, moved)


def compare(m, c, params, p, ids, what):
    """Both sides, normalised and raw, against float64; returns the two maxima."""
    before = _counters(m.handle)
    errs = {True: 0.0, False: 0.0}
    for side in ("src", "tgt"):
        want = reference_encodings(p, params, side, ids)
        for normalize in (True, False):
            got = _encode(m, c, side, ids, normalize)
            errs[normalize] = max(errs[normalize], check_encoding(got, want[normalize], normalize, bars_of(c),
                                                                  "%s%s " % (what, side)))
    after = _counters(m.handle)
    assert_kernel_ran(c, before, after, 4, what)
    print("LSTMFWDERR %s [%s]: normalised %.2e, raw %.2e (of max|want|), %d rows"
          % (c["id"], c["kernel"], errs[True], errs[False], len(ids)))
    return errs, before, after


@pytest.mark.parametrize("c", [pytest.param(c, id=c["id"]) for c in LSTM_CASES])
def test_encodings_match_float64_on_the_kernel_meant(c):
    params, p, ids = lstm_case(c)
    m = _model(c, params, p)
    what = "%s: " % c["id"]
    errs, before, after = compare(m, c, params, p, ids, what)
    if c["kernel"] in ("xt32", "xt64"):            # one table per encoder, built once
        assert after["lstm_x_table_builds"] - before["lstm_x_table_builds"] == 2, what


def test_x_table_is_rebuilt_after_new_weights():
    """set_variables invalidates the x-projection table: the next encode builds it again (counter lstm_x_table_builds) and
    matches float64 on the NEW weights."""
    c = next(c for c in LSTM_CASES if c["id"] == "xt32-h129")
    params, p, ids = lstm_case(c)
    m = _model(c, params, p)
    compare(m, c, params, p, ids, "first weights: ")
    assert m.handle.get_counter("lstm_x_table_builds") == 2
    _, p2, _ = lstm_case(dict(c, seed=c["seed"] + 7))
    m.set_variables(p2)
    compare(m, c, params, p2, ids, "new weights: ")
    assert m.handle.get_counter("lstm_x_table_builds") == 4


def test_dense_batch_above_8192_rows_through_the_host_entry_keeps_64_row_tiles():
    """The counterpart of fwd32-pads-host-forced: the same shape without the padding is not forced to 32-row tiles."""
    c = next(c for c in LSTM_CASES if c["id"] == "fwd32-pads-host-forced")
    c = dict(c, id="fwd64-dense-host", kernel="fwd64gs", pad=0.0, kind=None, entry="host")
    params, p, ids = lstm_case(c)
    compare(_model(c, params, p), c, params, p, ids, "%s: " % c["id"])
