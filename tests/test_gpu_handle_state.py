"""State a handle keeps from one call to the next: the layouts derived from the weights (padded embedding, packed kernels,
Waug, Wc, Wx3 / emb16, the x-projection table, the any-shape packs, the CNN packs), the three pad-prefix tables (pad_small,
pad_fwd, pad_x3) and the policy state (cluster back-off, adaptive device pad sort, x-table build policy).

A long-lived handle runs a scripted sequence of encodes, weight changes and option toggles.  Every encode is compared with
  (a) a fresh handle holding the same variables and options, bit for bit -- a stale cache shows up here;
  (b) the same long-lived handle with pad_skip = 0, bit for bit -- the header's claim; no pad-prefix table is read there;
  (c) the oracle on a sample of rows at the encoder tolerance (lstm_x3 also within 5e-5 of the exact fp32 kernel).
The T orderings that matter for the pad-prefix tables: a batch longer than max_seq_length, a weight change, a batch of at
most max_seq_length steps, then the long batch again.  Every row of a long batch has more leading PADs than max_seq_length,
so every tile of every kernel starts from a table row beyond what the short batch re-recorded."""
import os

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.util import exact_fp32_training, make_pair, model_params, split_bf16_training

pytestmark = pytest.mark.gpu

TOL = 1e-4            # every encoder against the oracle (tests/test_gpu_encode.py)
X3_TOL_EXACT = 5e-5   # lstm_x3 against the exact fp32 kernel (test_split_bf16_matrix_path_stays_within_the_encoder_tolerance)


def lead_ids(rng, B, T, V, lo, hi=None):
    """B x T ids, row b left-padded by lo .. hi (default T - 1) PADs, the rest tokens ending in EOS.  Row 0 is all PAD
    without EOS (lead = T), row 1 all PAD but its EOS."""
    hi = T - 1 if hi is None else hi
    ids = rng.randint(2, V, size=(B, T)).astype(np.int32)
    lead = rng.randint(lo, hi + 1, size=B)
    for b in range(B):
        ids[b, :lead[b]] = 0
    ids[:, -1] = 1
    ids[0, :] = 0
    if B > 1:
        ids[1, :-1] = 0
    return ids


def short_ids(rng, B, T, V):
    """T <= max_seq_length: leads 0 .. T, so that the short batch re-records the table (T = 1: no table at all)."""
    ids = lead_ids(rng, B, T, V, 0) if T > 1 else rng.randint(2, V, size=(B, T)).astype(np.int32)
    if T == 1:
        ids[0, 0] = 0
        if B > 1:
            ids[1, 0] = 1
    return ids


class Script(object):
    """One long-lived handle, the options it runs with, and a fresh handle per weight state for comparison (a)."""

    def __init__(self, params, seed=0, **opts):
        self.params = params
        self.m, _ = make_pair(params, seed=seed)
        self.opts = {}
        self.fresh = None
        self.steps = 0
        self.log = []
        self.set(**opts)

    def set(self, **opts):
        for k, v in opts.items():
            self.m.handle.set_option(k, v)
            self.opts[k] = v

    def changed(self, route):
        """The weights changed by `route`: later comparisons use a new fresh handle."""
        self.fresh = None
        self.log.append(route)

    def _fresh(self):
        import sse_amd
        if self.fresh is None:
            self.fresh = sse_amd.SSEModel(self.params)
            self.fresh.set_variables(self.m.get_variables(with_slots=True))
        for k, v in self.opts.items():
            self.fresh.handle.set_option(k, v)
        return self.fresh

    @staticmethod
    def _encode(m, side, ids, normalize, dev):
        if not dev:
            return (m.encode_source if side == "src" else m.encode_target)(ids, normalize=normalize)
        import torch
        d = torch.from_numpy(np.ascontiguousarray(ids)).to("cuda:0")
        out = torch.empty((ids.shape[0], int(m.seq_embed_size)), dtype=torch.float32, device="cuda:0")
        m.handle.encode_dev(0 if side == "src" else 1, d.data_ptr(), ids.shape[0], ids.shape[1], normalize, out.data_ptr())
        m.handle.synchronize()
        return out.cpu().numpy()

    def check(self, path, side, ids, normalize=True, dev=False):
        """(a), (b) and (c) for one encode of the long-lived handle; returns its encodings."""
        self.steps += 1
        B, T = ids.shape
        tag = "step %d [%s] %s side=%s B=%d T=%d normalize=%d opts=%s after %s" % (
            self.steps, path, "encode_dev" if dev else "encode", side, B, T, normalize, self.opts, " -> ".join(self.log) or "-")
        got = self._encode(self.m, side, ids, normalize, dev)
        want = self._encode(self._fresh(), side, ids, normalize, dev)
        assert np.array_equal(got, want), "%s: differs from a fresh handle with the same variables (max |d| %.3g, rows %s)" % (
            tag, float(np.abs(got - want).max()), np.nonzero((got != want).any(axis=1))[0][:8].tolist())
        self.m.handle.set_option("pad_skip", 0)
        full = self._encode(self.m, side, ids, normalize, dev)
        self.m.handle.set_option("pad_skip", self.opts.get("pad_skip", 1))
        assert np.array_equal(got, full), "%s: differs from pad_skip = 0 (max |d| %.3g, rows %s)" % (
            tag, float(np.abs(got - full).max()), np.nonzero((got != full).any(axis=1))[0][:8].tolist())
        rows = np.unique(np.r_[0:min(B, 4), np.random.RandomState(B + T).randint(0, B, size=8)])
        ref = O.encode(self.m.get_variables(), self.params, side, ids[rows], normalize=normalize,
                       cnn_bf16=bool(self.opts.get("cnn_bf16", 0)))
        scale = 1.0 if normalize else max(1.0, float(np.abs(ref).max()))
        d = float(np.abs(got[rows] - ref).max()) / scale
        assert d <= TOL, "%s: %.3g from the oracle" % (tag, d)
        if self.opts.get("lstm_x3", 0):
            self.m.handle.set_option("lstm_x3", 0)
            exact = self._encode(self.m, side, ids, normalize, dev)
            self.m.handle.set_option("lstm_x3", 1)
            d = float(np.abs(got - exact).max()) / scale
            assert d <= X3_TOL_EXACT, "%s: %.3g from the exact fp32 kernel" % (tag, d)
        return got


def _var(mode, side, what):
    scope = O.lstm_scope(mode, side)
    return {"kernel": scope + "/rnn/basic_lstm_cell/kernel", "bias": scope + "/rnn/basic_lstm_cell/bias",
            "proj": O.proj_name(mode, side)}[what]


def _scaled(w, name, f):
    return {name: (w[name] * np.float32(f)).astype(np.float32)}


def _train_batch(rng, mode, B, T, V, N):
    src = np.repeat(lead_ids(rng, B // 2, T, V, 0)[:, :], 2, axis=0)
    src[:2] = src[2:4]                                     # (no all-PAD rows in a train batch)
    z = np.tile(np.array([1.0, 0.0], np.float32), B // 2)
    if mode in ("source-encoder-only", "source_only_cnn"):
        return src, rng.randint(0, N, size=B).astype(np.int32), z
    tgt = lead_ids(rng, B, T, V, 0)
    tgt[:2] = tgt[2:4]
    return src, tgt, z


def apply_route(s, route, rng, tmp_path=None):
    """Change (or, for 'slot' and 'cancelled', deliberately not change) the weights of s.m by one route."""
    import sse_amd
    m, p = s.m, s.params
    mode, V, T, N = p["network_mode"], p["vocab_size"], p["max_seq_length"], p["targetSpaceSize"]
    w = m.get_variables()
    lstm_sides = [] if mode == "source_only_cnn" else (["src"] if mode == "source-encoder-only" else ["src", "tgt"])
    if route == "set_all":
        m.set_variables({k: (v * np.float32(0.97)).astype(np.float32) for k, v in w.items()})
    elif route == "embedding":
        m.set_variables(_scaled(w, "word_embedding", 1.05))
    elif route in ("kernel", "bias", "proj"):
        for side in lstm_sides:
            m.set_variables(_scaled(w, _var(mode, side, route), 1.04 if route != "bias" else -1.0))
        if not lstm_sides:                                 # text CNN: every filter, bias and the projection one by one
            for k in sorted(w):
                m.set_variables(_scaled(w, k, 1.03))
    elif route == "slot":
        k = sorted(w)[0]
        m.set_variables({k + "/Adagrad": np.full(w[k].shape, 0.37, np.float32)})
    elif route in ("train_fp32", "train_split"):
        if route == "train_split":
            split_bf16_training(m)
        try:
            m.train_step(*_train_batch(rng, mode, 32, T, V, N))
        finally:
            exact_fp32_training(m)
    elif route == "train_rows":
        src = lead_ids(rng, 20, T, V, 0)
        src[:2] = src[2:4]
        m.handle.corpus_upload(0, src)
        sr = np.repeat(rng.randint(0, 20, size=8), 2).astype(np.int32)
        if mode in ("source-encoder-only", "source_only_cnn"):
            tr = rng.randint(0, N, size=16).astype(np.int32)
        else:
            tgt = lead_ids(rng, 24, T, V, 0)
            tgt[:2] = tgt[2:4]
            m.handle.corpus_upload(1, tgt)
            tr = rng.randint(0, 24, size=16).astype(np.int32)
        m.handle.train_step_rows(sr, tr, np.tile(np.array([1.0, 0.0], np.float32), 8))
    elif route == "grads_apply":
        m.handle.train_grads(*_train_batch(rng, mode, 32, T, V, N))
        m.handle.train_apply()
    elif route == "cancelled":
        src, tgt, z = _train_batch(rng, mode, 32, T, V, N)
        src[5, T - 2] = V                                  # out of range: the step cancels its own update
        with pytest.raises(sse_amd.SSEError):
            m.train_step(src, tgt, z)
    elif route == "checkpoint":
        path = m.save(None, os.path.join(str(tmp_path), "ck"))
        m.train_step(*_train_batch(rng, mode, 32, T, V, N))
        m.load(None, path)                                 # back to the weights saved: a change from what the handle holds
    else:
        raise ValueError(route)
    s.changed(route)


# Routes that change the LSTM recurrence (pad-prefix tables go stale); the projection alone leaves them right.
RECURRENT = ["set_all", "kernel", "bias", "embedding", "train_fp32", "train_split", "train_rows", "grads_apply", "checkpoint"]

# path family: name, mode, (V, E, Hs, Ht, S, max_seq_length), T_long, options, B, through sse_encode_dev (torch buffers)
FAMILIES = [
    ("persist", "dual-encoder", (300, 50, 256, 96, 64, 16), 48, {}, 9, False),
    ("cluster", "dual-encoder", (300, 50, 256, 96, 64, 16), 48, {}, 200, False),
    ("cluster_chunked", "shared-encoder", (300, 50, 200, 200, 64, 16), 48, {}, 2000, False),
    ("small", "dual-encoder", (300, 50, 256, 96, 64, 16), 48, dict(lstm_persist_rows=0, lstm_cluster_rows=0), 300, False),
    ("fwd32_host_sort", "dual-encoder", (300, 50, 256, 96, 64, 16), 48,
     dict(lstm_cluster_rows=0, lstm_small_rows=0, lstm_x_table=0), 1500, False),
    ("fwd64_gate_split", "dual-encoder", (300, 50, 256, 128, 64, 12), 60,
     dict(lstm_cluster_rows=0, lstm_small_rows=0), 8300, False),
    ("x_table1", "dual-encoder", (300, 50, 256, 200, 64, 16), 48,
     dict(lstm_cluster_rows=0, lstm_small_rows=0, lstm_x_table=1), 1500, False),
    ("x_table2_hp512", "dual-encoder", (200, 50, 512, 300, 64, 12), 36,
     dict(lstm_persist_rows=0, lstm_cluster_rows=0, lstm_small_rows=0, lstm_x_table=2), 700, False),
    ("x3", "dual-encoder", (300, 50, 256, 96, 64, 16), 48, dict(lstm_x3=1), 1500, False),
    ("dev_sort1", "dual-encoder", (300, 50, 256, 96, 64, 16), 48,
     dict(lstm_cluster_rows=0, lstm_small_rows=0, pad_sort_dev=1), 1500, True),
    ("dev_sort2_x3", "shared-encoder", (300, 50, 128, 128, 64, 16), 48,
     dict(lstm_cluster_rows=0, lstm_small_rows=0, pad_sort_dev=2, lstm_x3=1), 1500, True),
]


@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_pad_prefix_tables_follow_weight_changes_across_T(fam, tmp_path):
    """T_long -> weight change -> T <= max_seq_length (and T = 1, 2) -> T_long again, twice, with a different route that
    changes the recurrence each time; both sides (dual-encoder: two LSTM owners of different cell sizes)."""
    name, mode, (V, E, Hs, Ht, S, Tm), Tl, opts, B, dev = fam
    params = model_params(mode, V, E, Hs, Ht, S, Tm)
    s = Script(params, seed=len(name), **opts)
    rng = np.random.RandomState(B + Tl)
    # 64-row tiles on the host-sorted path need a mean lead below T / 4 (no 32-row hint): leads just above max_seq_length
    hi = Tm + 2 if name.startswith("fwd64") else None
    long_ids = lead_ids(rng, B, Tl, V, Tm + 1, hi)
    sides = ("src", "tgt")
    k = FAMILIES.index(fam)
    for r, route in enumerate((RECURRENT[k % len(RECURRENT)], RECURRENT[(k + 4) % len(RECURRENT)])):
        for side in sides:
            s.check(name, side, long_ids, dev=dev)
        apply_route(s, route, rng, tmp_path)
        for T in (Tm, 2, 1):
            for side in sides:
                s.check(name, side, short_ids(rng, B, T, V), normalize=(T != 2), dev=dev)
        for side in sides:
            s.check(name, side, long_ids, normalize=bool(r), dev=dev)     # stale table rows Tm + 1 .. Tl would show here
    if name.startswith("fwd64"):                         # the same tiles on lstm_fwd instead of the gate-split kernel
        s.set(lstm_gate_split=0)
        apply_route(s, "kernel", rng)
        s.check(name, "src", short_ids(rng, B, Tm, V))
        s.check(name, "tgt", long_ids)
    h = s.m.handle
    if name.startswith("dev_sort"):                      # the device pad sort did bucket these batches
        assert h.get_counter("pad_sorted_calls") > 0
    if name.startswith("x_table"):                       # the x-projection table was built, and rebuilt after each change
        assert h.get_counter("lstm_x_table_builds") >= 3


MODES = [
    # mode, (V, E, Hs, Ht, S, max_seq_length, N); dual-encoder: two LSTM owners of different sizes; shared-encoder: the
    # target reads the source's tables; any-shape: source cell size > 512 (lstm_generic.hip) beside a fused target
    ("dual-encoder", (300, 50, 256, 128, 64, 16, 40)),
    ("shared-encoder", (300, 50, 200, 200, 64, 16, 40)),
    ("source-encoder-only", (300, 50, 256, 256, 64, 16, 40)),
    ("source_only_cnn", (300, 50, 96, 96, 64, 16, 40)),
    ("any-shape", (120, 72, 600, 96, 64, 8, 40)),
]

# each route with the option toggled just before it (slot writes and cancelled steps keep the options: their encodings
# must equal the ones before them bit for bit)
ROUTES = [
    ("set_all", dict(lstm_x3=1), dict(cnn_bf16=1)),
    ("embedding", dict(lstm_x_table=2), {}),
    ("kernel", dict(lstm_gate_split=0), dict(cnn_bf16=0)),
    ("bias", dict(pad_sort_dev=2), {}),
    ("proj", dict(lstm_x_table=0), dict(cnn_bf16=1)),
    ("slot", {}, {}),
    ("train_fp32", dict(pad_skip=0), dict(pad_skip=0)),
    ("train_split", dict(pad_skip=1, lstm_x3=0), dict(pad_skip=1)),
    ("train_rows", dict(lstm_gate_split=1), dict(cnn_bf16=0)),
    ("grads_apply", dict(lstm_x_table=1, pad_sort_dev=1), {}),
    ("cancelled", {}, {}),
    ("checkpoint", dict(lstm_x3=1), dict(cnn_bf16=1)),
]


@pytest.mark.parametrize("mode,shape", MODES, ids=[m[0] for m in MODES])
def test_every_weight_route_refreshes_every_cache(mode, shape, tmp_path):
    """Each route that changes weights, after an option toggle, then the T orderings on the cluster kernel, the host-sorted
    and the device-sorted matrix kernels and the single-query kernel.  Adagrad-slot writes and a cancelled step change no
    weight: the encodings must equal the ones before, bit for bit."""
    V, E, Hs, Ht, S, Tm, N = shape
    real = "dual-encoder" if mode == "any-shape" else mode
    cnn = real == "source_only_cnn"
    params = model_params(real, V, E, Hs, Ht, S, Tm, N=N, lr=0.5)
    s = Script(params, seed=3)
    rng = np.random.RandomState(7)
    Tl = 3 * Tm
    sides = ("src",) if real in ("source-encoder-only", "source_only_cnn") else ("src", "tgt")
    if cnn:
        batches = [("long", lead_ids(rng, 70, Tl, V, Tm + 1), False), ("short", lead_ids(rng, 40, Tm, V, 0), False)]
    else:
        batches = [("long_cluster", lead_ids(rng, 200, Tl, V, Tm + 1), False),
                   ("short_sorted", lead_ids(rng, 3100, Tm, V, 0), False),       # above the cluster kernel's 3 x 1024
                   ("long_persist", lead_ids(rng, 6, Tl, V, Tm + 1), False),
                   ("long_sorted", lead_ids(rng, 3100, Tl, V, Tm + 1), False),
                   ("long_dev", lead_ids(rng, 1500, Tl, V, Tm + 1), True),
                   ("T2", short_ids(rng, 50, 2, V), False)]

    def run(label):
        return {(b, side): s.check("%s/%s" % (label, b), side, ids, dev=dev) for b, ids, dev in batches for side in sides}

    before = run("initial")
    for route, lstm_opts, cnn_opts in ROUTES:
        opts = cnn_opts if cnn else lstm_opts
        if opts:
            s.set(**opts)
            s.log.append(",".join("%s=%d" % kv for kv in sorted(opts.items())))
        apply_route(s, route, rng, tmp_path)
        got = run(route)
        if route in ("slot", "cancelled"):
            for key in got:
                assert np.array_equal(got[key], before[key]), "%s after %s: encodings moved (%s)" % (key, route, s.log)
        before = got


def test_cluster_backoff_counts_down_for_host_sorted_batches():
    """A give-up of the cluster kernel arms the back-off (lstm_cluster_backoff = N calls).  Batches of 1025 .. 3072 rows
    that the back-off sends to the matrix kernel take the host pad-prefix sort; each of them must still count the back-off
    down, so that the call after N of them tries the cluster kernel again (one more injected miss, one more fallback)."""
    V, T, N = 300, 16, 3
    params = model_params("dual-encoder", V, 50, 256, 96, 64, T)
    m, _ = make_pair(params, seed=5)
    f, _ = make_pair(params, seed=5)
    ids = lead_ids(np.random.RandomState(9), 2000, T, V, 0)
    want = f.encode_source(ids)
    h = m.handle
    h.set_option("lstm_cluster_backoff", N)
    h.set_option("lstm_persist_inject_miss", 1)
    try:
        assert np.array_equal(m.encode_source(ids), want)
        assert h.get_counter("lstm_persist_fallbacks") == 1
        for i in range(N):                               # backed off: the matrix kernel on host-sorted rows
            assert np.array_equal(m.encode_source(ids), want), i
            assert h.get_counter("lstm_persist_fallbacks") == 1, i
        for rnd in range(2):                             # tried again after N calls, every time
            assert np.array_equal(m.encode_source(ids), want)
            assert h.get_counter("lstm_persist_fallbacks") == 2 + rnd, "the cluster kernel was not tried again after %d calls" % N
            for _ in range(N):
                assert np.array_equal(m.encode_source(ids), want)
            assert h.get_counter("lstm_persist_fallbacks") == 2 + rnd
    finally:
        h.set_option("lstm_persist_inject_miss", 0)
        h.set_option("lstm_cluster_backoff", -1)
