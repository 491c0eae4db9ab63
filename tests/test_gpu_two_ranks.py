"""The product's multi-rank classes as REAL ranks: 2 and 3 processes on the one GPU of a test box, a `gloo` group between
them, the HIP handle behind ShardedIndex.score_topk and DataParallelTrainer.train_step on every rank.

What no other test runs with the device library behind it: id_base = start on a rank that is not the first, the share
B / rows_global of a batch another process holds the rest of, the packed sparse embedding exchange between processes that
touched different rows, the row-count all-gather of uneven batches, the query-block pipeline of the sharded index, shards
shorter than k and an empty shard, and the ordering between the library's raw-pointer writes and a collective (host-staged
under gloo: sse_amd/collectives.py; RCCL refuses two ranks on one device).

Each of the four launches (sharded x {2, 3} ranks, data-parallel x {2, 3} ranks) starts fresh children running
tests/two_rank_worker.py on a job file; the children write <case>_rank<r>.npz, every assertion is made here.  A child that
fails, or the 300 s cap, ends the launch: the remaining children are killed (a rank that lost its peer would sit in a
collective); a child that died of a signal ends the whole pytest session -- nothing more starts on the GPU after a fault.

Bars are the project's: ids exact and scores within 1e-12 of the float64 oracle (tests/test_gpu_score.py); the reduced
arena at util.GRAD_BARS_EXACT / LOSS_REL_EXACT against the float64 gradient of the WHOLE batch and sse_train_apply within 1e-6
of a float64 clip + Adagrad of that arena (tests/test_gpu_train_grads.py); on the `even` shape the bars of
tests/test_gpu_train.py::test_data_parallel_two_logical_ranks; three free-running oracle steps at the bars of
tests/test_gpu_rccl.py::test_data_parallel_step_through_rccl_all_reduce on `even` and `three`."""
import os
import time

import numpy as np
import pytest

from oracle import sse_oracle as O
from tests.test_gpu_train_grads import case_batch, cnn_min_pool_gap
from tests.util import (GRAD_BARS_EXACT, LOSS_REL_EXACT, check_grads, check_tail, make_pair, model_params, oracle_params,
                        random_ids, reference_apply, reference_grads)
from tests.rank_launch import free_port, run_ranks

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "two_rank_worker.py")
LAUNCH_CAP_S = 300                      # safety limit of one launch, not a measurement


# ---- launching ---------------------------------------------------------------------------------------------------------
def _launch(tmp, kind, world, cases, inputs):
    """Runs `world` workers on one job; returns [{case id: loaded npz} per rank].  Fails with every rank's stderr tail when a
    rank fails or the cap passes; ends the session when a rank died of a signal."""
    assert world <= 3, "three children plus pytest is the most this module puts on the GPU"
    tmp = str(tmp)
    np.savez(os.path.join(tmp, "inputs.npz"), **inputs)
    job = dict(kind=kind, world=world, port=free_port(), cases=cases, inputs=os.path.join(tmp, "inputs.npz"), out_dir=tmp)
    run_ranks(WORKER, tmp, world, job, LAUNCH_CAP_S)
    return [{c["id"]: np.load(os.path.join(tmp, "%s_rank%d.npz" % (c["id"], r))) for c in cases} for r in range(world)]


# ---- sharded scoring ---------------------------------------------------------------------------------------------------
def _unit(rng, n, s):                                            # as tests/test_gpu_score.py
    x = rng.standard_normal((n, s)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


#                id        world  N     S    Q    k   block  seed
SHARDED = [dict(id="basic", world=2, N=20011, S=64, Q=300, k=10, block=128, seed=0, score_bf16=[0, 1], plant=True, gather_lists=True),
           dict(id="three", world=3, N=9001, S=256, Q=37, k=16, block=16, seed=1, score_bf16=[0], plant=True, side_stream=True),
           dict(id="large-k", world=2, N=571, S=64, Q=40, k=100, block=8192, seed=2, score_bf16=[0]),
           dict(id="short", world=3, N=25, S=16, Q=33, k=10, block=8, seed=3, score_bf16=[0]),       # shards of 9 / 8 / 8 rows
           dict(id="empty", world=3, N=2, S=16, Q=5, k=2, block=8, seed=4, score_bf16=[0])]          # rank 2 holds no row


def sharded_inputs(c):
    """(t [N,S], q [Q,S], planted): unit rows and queries; with c["plant"], per shard boundary b an exact tie between rows b-1 and
    b (entries that are multiples of 1/4: the float64 dot is the same in any summation order) under a query that equals the row,
    one query whose whole top-k lies in rank 0's shard and one whose whole top-k lies in the last rank's.
    planted = dict(ties=[(query, row b-1, row b)], first=query, last=query)."""
    from sse_amd.sharded import shard_bounds
    rng = np.random.RandomState(c["seed"])
    N, S, Q, k = c["N"], c["S"], c["Q"], c["k"]
    t, q = _unit(rng, N, S), _unit(rng, Q, S)
    planted = dict(ties=[], first=None, last=None)
    if c.get("plant"):
        bounds = shard_bounds(N, c["world"])
        for j, (b, _) in enumerate(bounds[1:]):
            t[b - 1] = rng.choice([-0.25, 0.0, 0.25], size=S)
            t[b] = t[b - 1]
            q[1 + j] = t[b]
            planted["ties"].append((1 + j, b - 1, b))
        for name, qi, (a, b) in (("first", 5, bounds[0]), ("last", 6, bounds[-1])):
            rows = a + 10 + 3 * np.arange(k)                      # inside the shard, away from its boundaries
            assert rows.max() < b - 1
            near = q[qi][None, :] + 0.02 * rng.standard_normal((k, S)).astype(np.float32)
            t[rows] = (near / np.linalg.norm(near, axis=1, keepdims=True)).astype(np.float32)
            planted[name] = qi
    return t, q, planted


def sharded_guard(c, t, q, planted):
    """The oracle's top-k and the smallest gap between adjacent scores of its top k+1 outside the planted ties, which must exceed
    1e-10 -- 50x what two 1e-12 errors need to swap two rows.  Rows of one planted tie must score EXACTLY alike in the oracle."""
    k, N = c["k"], c["N"]
    ws, wi = O.topk(O.scores_f64(q, t.astype(np.float64)), min(k + 1, N))
    group = {}
    for _, a, b in planted["ties"]:
        group[a] = group[b] = a
    gap = np.inf
    for row_s, row_i in zip(ws, wi):
        for j in range(len(row_i) - 1):
            ga, gb = group.get(int(row_i[j])), group.get(int(row_i[j + 1]))
            if ga is not None and ga == gb:
                assert row_s[j] == row_s[j + 1], "a planted tie is not exact in the oracle"
            else:
                gap = min(gap, float(row_s[j] - row_s[j + 1]))
    assert gap > 1e-10, "oracle gap %.3g: the inputs do not separate the ranks" % gap
    return ws[:, :k], wi[:, :k], gap


def _unsharded(c, t, q, bf):
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, c["S"], 4))
    m.handle.set_option("score_bf16", bf)
    m.handle.index_upload(t)
    out = m.handle.score_topk(q, c["k"])
    m.handle.close()
    return out


def _sharded_launch(tmp_path_factory, world):
    from sse_amd.sharded import shard_bounds
    cases = [dict(c, bounds=shard_bounds(c["N"], world)) for c in SHARDED if c["world"] == world]
    inputs, data = {}, {}
    for c in cases:
        t, q, planted = sharded_inputs(c)
        inputs[c["id"] + "/t"], inputs[c["id"] + "/q"] = t, q
        data[c["id"]] = (c, t, q, planted)
    t0 = time.monotonic()
    ranks = _launch(tmp_path_factory.mktemp("sharded%d" % world), "sharded", world, cases, inputs)
    print("TWORANKS sharded x %d ranks: %.1f s" % (world, time.monotonic() - t0))
    return data, ranks


@pytest.fixture(scope="module")
def sharded2(tmp_path_factory):
    return _sharded_launch(tmp_path_factory, 2)


@pytest.fixture(scope="module")
def sharded3(tmp_path_factory):
    return _sharded_launch(tmp_path_factory, 3)


@pytest.mark.parametrize("cid", [c["id"] for c in SHARDED])
def test_sharded_scoring_as_real_ranks(cid, request):
    world = next(c["world"] for c in SHARDED if c["id"] == cid)
    data, ranks = request.getfixturevalue("sharded%d" % world)
    c, t, q, planted = data[cid]
    k, bounds = c["k"], c["bounds"]
    wsc, wids, gap = sharded_guard(c, t, q, planted)
    for qi, a, b in planted["ties"]:
        assert wids[qi, :2].tolist() == [a, b]                    # the lower row id first, across the shard boundary
    if planted["first"] is not None:
        assert wids[planted["first"]].max() < bounds[0][1] and wids[planted["last"]].min() >= bounds[-1][0]
    worst = 0.0
    for bf in c["score_bf16"]:
        us, ui = _unsharded(c, t, q, bf)
        for r in range(world):
            z = ranks[r][cid]
            s, i = z["s%d" % bf], z["i%d" % bf]
            assert np.array_equal(i, wids), "rank %d score_bf16 %d" % (r, bf)
            assert np.isfinite(s).all()
            worst = max(worst, float(np.abs(s - wsc).max()))
            assert np.abs(s - wsc).max() < 1e-12
            assert np.array_equal(s, ranks[0][cid]["s%d" % bf]) and np.array_equal(i, ranks[0][cid]["i%d" % bf])
            assert np.array_equal(i, ui) and np.array_equal(s, us)     # the same handle's unsharded call: bit for bit
    for r in range(world):
        assert str(ranks[r][cid]["k_too_large"]).startswith("ValueError"), ranks[r][cid]["k_too_large"]
    if c.get("gather_lists"):                                     # all_gather_topk on device tensors: shard-major per-shard lists
        for r in range(world):
            gs, gi = ranks[r][cid]["gs"], ranks[r][cid]["gi"]
            assert gs.shape == gi.shape == (world, c["Q"], k)
            for p, (a, b) in enumerate(bounds):
                ps, pi = O.topk(O.scores_f64(q, t[a:b].astype(np.float64)), k)
                assert np.array_equal(gi[p], pi + a) and np.abs(gs[p] - ps).max() < 1e-12
            assert np.array_equal(gs, ranks[0][cid]["gs"]) and np.array_equal(gi, ranks[0][cid]["gi"])
    print("SHARDERR %s x %d ranks: oracle gap %.2e, max |score - oracle| %.2e" % (cid, world, gap, worst))


# ---- data-parallel train step ------------------------------------------------------------------------------------------
def _pairs(rng, B, T, V, pad_frac=0.6):                           # as tests/test_gpu_train.py::_batch
    src = np.repeat(random_ids(rng, B // 2, T, V, pad_frac), 2, axis=0)
    tgt = random_ids(rng, B, T, V, pad_frac)
    return src, tgt, np.tile(np.array([1.0, 0.0], np.float32), B // 2)


def _dp(cid, world, mode, V, E, Hs, Ht, S, T, N=13, seed=3, sparse=False, want_kinds=("dense",) * 3, **kw):
    return dict(dict(id=cid, world=world, mode=mode, V=V, E=E, Hs=Hs, Ht=Ht, S=S, T=T, N=N, seed=seed, sparse=sparse,
                     want_kinds=list(want_kinds), by_rows=False, steps=3), **kw)


DP = [_dp("even", 2, "dual-encoder", 300, 50, 128, 128, 64, 10, seed=7),
      _dp("mixed-paths", 2, "dual-encoder", 400, 50, 256, 256, 256, 16),
      _dp("sparse", 2, "dual-encoder", 5000, 50, 128, 128, 64, 12, sparse=True, want_kinds=("sparse",) * 3),
      _dp("auto", 2, "dual-encoder", 2000, 8, 40, 40, 24, 6, sparse=None, want_kinds=("sparse", "dense", "dense")),
      _dp("three", 3, "shared-encoder", 300, 40, 96, 96, 50, 50, side_stream=True),
      _dp("by-rows", 2, "dual-encoder", 300, 50, 128, 128, 64, 10, by_rows=True),
      _dp("cnn", 2, "source_only_cnn", 90, 24, 96, 96, 64, 20, N=17, seed=4),
      _dp("seo", 2, "source-encoder-only", 200, 50, 128, 128, 64, 12, N=17, sparse=True, want_kinds=("sparse",) * 3)]


def _gen(c, B, kind="paired", seed=0):
    return case_batch(dict(mode=c["mode"], V=c["V"], T=c["T"], N=c["N"], B=B, batch=kind, seed=seed))


def dp_batches(c):
    """[per step: (per rank: (src, tgt, z) as handed to train_step, whole batch (src, tgt, z) in rank order, rows_global argument)]
    and extra inputs (the corpora of `by-rows`)."""
    from sse_amd.sharded import shard_bounds
    cid, world = c["id"], c["world"]
    extra = {}

    def split(whole, sizes=None, rows_global=None):
        src, tgt, z = whole
        cuts = shard_bounds(len(z), world) if sizes is None else list(zip(np.cumsum([0] + sizes[:-1]), np.cumsum(sizes)))
        return [(src[a:b], tgt[a:b], z[a:b]) for a, b in cuts], whole, rows_global

    def cat(parts):
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))

    if cid == "even":                                             # the batch of test_data_parallel_two_logical_ranks, 48 / 48
        one = split(_pairs(np.random.RandomState(4), 96, 10, 300), rows_global=96)
    elif cid == "mixed-paths":                                    # rank 0: B % 128 == 0 and (pos, neg) rows share a source; rank 1: neither
        parts = [_gen(c, 128, "paired", 0), _gen(c, 70, "unpaired", 1)]
        assert np.array_equal(parts[0][0][0::2], parts[0][0][1::2]) and len(parts[0][2]) % 128 == 0
        one = (parts, cat(parts), None)
    elif cid == "sparse":                                         # 40 / 24, PAD / EOS heavy on both ranks
        parts = [_gen(c, 40, "hot", 0), _gen(c, 24, "hot", 1)]
        touched = [np.unique(np.concatenate([p[0].ravel(), p[1].ravel()])) for p in parts]
        assert {0, 1} <= set(touched[0]) & set(touched[1])
        assert len(np.setdiff1d(touched[0], touched[1])) > 10 and len(np.setdiff1d(touched[1], touched[0])) > 10
        one = (parts, cat(parts), None)
    elif cid == "auto":                                           # 2 * 41 * 6 = 492 < 2000 // 4 <= 2 * 42 * 6
        steps = []
        for seed, rows in enumerate((41, 42, 42)):
            rng = np.random.RandomState(40 + seed)
            whole = (rng.randint(2, 2000, size=(rows, 6)).astype(np.int32), rng.randint(2, 2000, size=(rows, 6)).astype(np.int32),
                     (np.arange(rows) % 2 == 0).astype(np.float32))
            steps.append(split(whole, rows_global=rows))
        return steps, extra
    elif cid == "three":                                          # 34 / 33 / 33
        one = split(_gen(c, 100), rows_global=100)
    elif cid == "by-rows":                                        # 32 / 32 row numbers into shuffled corpora every rank uploaded
        src, tgt, z = _gen(c, 64)
        order = np.random.RandomState(5).permutation(64).astype(np.int32)
        inv = np.argsort(order).astype(np.int32)
        extra = {"corpus_src": src[order], "corpus_tgt": tgt[order]}
        parts, _, _ = split((inv, inv, z))
        one = (parts, (src, tgt, z), 64)
    elif cid == "cnn":                                            # the batch of test_gpu_train_grads' `cnn` case, 6 / 4
        one = split(_gen(c, 10, seed=1), sizes=[6, 4])
    elif cid == "seo":                                            # 24 / 16
        one = split(_gen(c, 40), sizes=[24, 16])
    else:
        raise KeyError(cid)
    return [one] * c["steps"], extra


def _dp_launch(tmp_path_factory, world):
    cases, inputs, data = [], {}, {}
    for c in DP:
        if c["world"] != world:
            continue
        steps, extra = dp_batches(c)
        c = dict(c, rows_global=[s[2] for s in steps])
        for name, v in extra.items():
            inputs["%s/%s" % (c["id"], name)] = v
        for i, (parts, _, _) in enumerate(steps):
            assert len(parts) == world
            for r, (src, tgt, z) in enumerate(parts):
                key = "%s/step%d/rank%d/" % (c["id"], i, r)
                inputs[key + "src"], inputs[key + "tgt"], inputs[key + "z"] = src, tgt, z
        cases.append(c)
        data[c["id"]] = (c, steps)
    t0 = time.monotonic()
    ranks = _launch(tmp_path_factory.mktemp("dp%d" % world), "dp", world, cases, inputs)
    print("TWORANKS data-parallel x %d ranks: %.1f s" % (world, time.monotonic() - t0))
    return data, ranks


@pytest.fixture(scope="module")
def dp2(tmp_path_factory):
    return _dp_launch(tmp_path_factory, 2)


@pytest.fixture(scope="module")
def dp3(tmp_path_factory):
    return _dp_launch(tmp_path_factory, 3)


def _named(z, prefix):
    return {n[len(prefix):]: z[n] for n in z.files if n.startswith(prefix)}


@pytest.mark.parametrize("cid", [c["id"] for c in DP])
def test_data_parallel_steps_as_real_ranks(cid, request):
    world = next(c["world"] for c in DP if c["id"] == cid)
    data, ranks = request.getfixturevalue("dp%d" % world)
    c, steps = data[cid]
    Z = [ranks[r][cid] for r in range(world)]
    params = model_params(c["mode"], c["V"], c["E"], c["Hs"], c["Ht"], c["S"], c["T"], N=c["N"], lr=0.9)
    p = oracle_params(params, seed=c["seed"])
    parts, (src, tgt, z), _ = steps[0]
    assert [len(x[2]) for x in parts] == {"even": [48, 48], "mixed-paths": [128, 70], "sparse": [40, 24], "auto": [21, 20],
                                         "three": [34, 33, 33], "by-rows": [32, 32], "cnn": [6, 4], "seo": [24, 16]}[cid]
    if c["mode"] == "source_only_cnn":
        assert cnn_min_pool_gap(p, src, False) > 1e-5
    # ---- first step: the reduced arena is the float64 gradient of the WHOLE batch, the same bits on every rank
    want, want_tail = reference_grads(p, params, src, tgt, z)
    assert want_tail[3] == len(z)
    names = sorted(want)
    worst_apply = 0.0
    for r in range(world):
        got, tail = _named(Z[r], "g/"), Z[r]["tail"]
        assert sorted(got) == names
        errs = check_grads(got, want, GRAD_BARS_EXACT, what="%s rank %d: " % (cid, r))
        check_tail(tail, want_tail, GRAD_BARS_EXACT, LOSS_REL_EXACT, what="%s rank %d: " % (cid, r))
        assert tail[3] == len(z)
        assert np.array_equal(tail, Z[0]["tail"])
        for n in names:
            assert np.array_equal(got[n], Z[0]["g/" + n]), "arena of rank %d differs from rank 0 in %s" % (r, n)
        # sse_train_apply on that arena: float64 clip + Adagrad
        v0, v1 = _named(Z[r], "v0/"), _named(Z[r], "v1/")
        wv, ws = reference_apply(got, tail, {n: v0[n] for n in names}, {n: v0[n + "/Adagrad"] for n in names}, np.float32(0.9))
        for n in names:
            for have, ref, what in ((v1[n], wv[n], n), (v1[n + "/Adagrad"], ws[n], n + "/Adagrad")):
                d = float((np.abs(have.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())
                worst_apply = max(worst_apply, d)
                assert d <= 1e-6, (cid, r, what, d)
        assert tuple(Z[r]["hist"][0]) == (float(tail[1]), float(tail[2]))
    rel_name, elem_name = max(errs, key=lambda n: errs[n][0]), max(errs, key=lambda n: errs[n][1])
    print("GRADERR two-ranks %s x %d bars %.0e/%.0e: norm %.2e (%s), element %.2e (%s), apply %.2e"
          % (cid, world, GRAD_BARS_EXACT[0], GRAD_BARS_EXACT[1], errs[rel_name][0], rel_name, errs[elem_name][1], elem_name, worst_apply))
    # ---- after the last step: the ranks are in lock-step, bit for bit
    last = "v%d/" % c["steps"]
    for r in range(world):
        assert Z[r]["kinds"].tolist() == c["want_kinds"], (r, Z[r]["kinds"].tolist())
        assert int(Z[r]["global_step"]) == c["steps"]
        assert np.array_equal(Z[r]["hist"], Z[0]["hist"])
        vr, v0 = _named(Z[r], last), _named(Z[0], last)
        assert sorted(vr) == sorted(v0) and len(vr) == 2 * len(names)
        for n in vr:
            assert np.array_equal(vr[n], v0[n]), "rank %d differs from rank 0 in %s after %d steps" % (r, n, c["steps"])
    # ---- comparisons whose bars were set on one shape stay on that shape
    if cid == "even":                                             # bars of test_data_parallel_two_logical_ranks
        mf, _ = make_pair(params, seed=c["seed"])
        full = mf.train_step(src, tgt, z)
        gf = mf.get_variables(with_slots=True)
        p1 = {n: v.copy() for n, v in p.items()}
        st1 = O.new_optimizer_state(p1)
        w1 = O.train_step(p1, st1, params, src, tgt, z, 0.9)
        v1 = _named(Z[0], "v1/")
        assert Z[0]["hist"][0][0] == pytest.approx(float(w1[0]), rel=LOSS_REL_EXACT) and Z[0]["hist"][0][1] == pytest.approx(float(w1[1]), abs=1e-6)
        assert Z[0]["hist"][0][0] == pytest.approx(full[0], rel=1e-5)
        d_dev = max(float(np.abs(v1[n] - gf[n]).max()) for n in p)
        d_orc = max(max(float(np.abs(v1[n].reshape(w.shape) - w).max()), float(np.abs(v1[n + "/Adagrad"].reshape(w.shape) - st1[n]).max()))
                    for n, w in p1.items())
        print("GRADERR two-ranks even step 1: max |var - single-process device step| %.2e (bar 2e-5), |var, slot - oracle step| %.2e (bar 2e-4)"
              % (d_dev, d_orc))
        assert d_dev < 2e-5 and d_orc < 2e-4
        mf.handle.close()
    if cid in ("even", "three"):                                  # bars of test_data_parallel_step_through_rccl_all_reduce
        pf = {n: v.copy() for n, v in p.items()}
        st = O.new_optimizer_state(pf)
        d_loss = 0.0
        for i, (_, whole, _) in enumerate(steps):
            w = O.train_step(pf, st, params, whole[0], whole[1], whole[2], 0.9)
            d_loss = max(d_loss, abs(Z[0]["hist"][i][0] - float(w[0])) / abs(float(w[0])))
        v3 = _named(Z[0], last)
        d_var = max(float(np.abs(v3[n].reshape(w.shape) - w).max()) for n, w in pf.items())
        print("GRADERR two-ranks %s 3 free-running oracle steps: loss rel %.2e (bar 1e-4), variables %.2e (bar 1e-3)" % (cid, d_loss, d_var))
        assert d_loss <= 1e-4 and d_var < 1e-3
