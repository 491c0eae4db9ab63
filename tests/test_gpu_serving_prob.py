"""Probabilities of the serving routes (sse_serving.py; DESIGN K6m): Ranker.rank(prob_scale=64) appends to every tuple the
softmax probability over the WHOLE index -- softmax_probs of its own scores and one Handle.score_lse on the encodings of the
call --, the four routes accept prob_scale and add "prob" per result, and a route without the argument returns exactly what it
returned before, byte for byte.  The ranker is a real one on an untrained model, as in tests/test_gpu_serving_after.py."""
import json

import numpy as np
import pytest

from tests.test_gpu_serving_after import N, _get, _ranker

pytestmark = pytest.mark.gpu

ROUTES = [("/api/classify", "keywords", True, "ClassificationResults", "targetCategoryId", "confidenceScore"),
          ("/api/search", "query", False, "SearchRankingResults", "ListingId", "rankingScore"),
          ("/api/qna", "question", False, "Answers", "answerDocId", "confidenceScore"),
          ("/api/crosslingual", "query", False, "SearchResults", "documentId", "confScore")]


def test_rank_probabilities_are_softmax_probs_of_its_own_scores():
    from sse_amd.sse_index import softmax_probs
    r = _ranker()
    h = r.model.handle
    toks = [r.tokens("red nike shoes"), r.tokens("hello kitty sunglasses"), r.tokens("a")]
    for normalize in (True, False):
        plain = r.rank(toks, 7, normalize)
        calls0 = h.get_counter("score_lse_calls")
        got = r.rank(toks, 7, normalize, prob_scale=64)
        assert h.get_counter("score_lse_calls") == calls0 + 1               # one call for all rows
        assert [[t[:3] for t in row] for row in got] == plain and all(len(t) == 4 for row in got for t in row)
        enc = h.encode(0, np.asarray(toks, np.int32), normalize)
        lse, cnt, bound = h.score_lse(enc, 64.0)
        assert (cnt == N).all()
        scores = np.array([[t[0] for t in row] for row in got])
        assert np.array_equal(np.array([[t[3] for t in row] for row in got]), softmax_probs(scores, lse, 64.0))
        # the whole ranked list sums to one
        full = r.rank(toks, N, normalize, prob_scale=64)
        total = np.array([sum(t[3] for t in row) for row in full])
        assert (np.abs(total - 1.0) <= np.expm1(bound) + 1e-12).all(), (total, bound)
        # paged: the tuples keep the row id in front of the probability
        cs, ci = [row[6][0] for row in plain], [r.targetIDs.index(row[6][1]) for row in plain]
        page = r.rank(toks, 5, normalize, after=(cs, ci), prob_scale=64)
        unpaged = r.rank(toks, 5, normalize, after=(cs, ci))
        assert [[t[:4] for t in row] for row in page] == unpaged
        assert [[t[4] for t in row] for row in page] == [[t[3] for t in row[7:12]] for row in full]
    h.close()


@pytest.mark.parametrize("batch", [False, True])
def test_routes_add_prob_when_asked_and_keep_their_keys_otherwise(batch):
    from sse_amd import sse_serving
    from sse_amd.sse_index import softmax_probs
    r = _ranker()
    h = r.model.handle
    app = sse_serving.create_app(ranker=r, batch=batch)
    text = "red nike shoes"
    tok = np.array([r.tokens(text)], np.int32)
    for path, arg, normalize, rkey, idk, scorek in ROUTES:
        route = sse_serving.ROUTES[path]
        # without the parameter: today's JSON, byte for byte
        st, body = _get(app, path, "%s=red+nike+shoes&nbest=7" % arg)
        assert st.startswith("200")
        ts, ti = h.encode_score_topk(0, tok, normalize, 7)
        want = {route[3]: text, rkey: [{idk: r.targetIDs[ti[0, j]], route[5][1]: r.targetNames[ti[0, j]], scorek: float(ts[0, j])} for j in range(7)]}
        assert body == json.dumps(want).encode("utf-8")
        # with it: the same results, each with its probability
        st, body = _get(app, path, "%s=red+nike+shoes&nbest=7&prob_scale=64" % arg)
        assert st.startswith("200"), body
        d = json.loads(body)
        assert set(d) == {route[3], rkey} and all(set(x) == {idk, route[5][1], scorek, "prob"} for x in d[rkey])
        assert [{k: v for k, v in x.items() if k != "prob"} for x in d[rkey]] == want[rkey]
        lse, _, _ = h.score_lse(h.encode(0, tok, normalize), 64.0)
        assert [x["prob"] for x in d[rkey]] == softmax_probs(ts, lse, 64.0)[0].tolist()
        # paged with probabilities
        st, body = _get(app, path, "%s=red+nike+shoes&nbest=3&prob_scale=64&after_score=%r&after_id=%d" % (arg, float(ts[0, 6]), int(ti[0, 6])))
        d = json.loads(body)
        assert st.startswith("200") and len(d[rkey]) == 3 and all(0.0 <= x["prob"] <= 1.0 for x in d[rkey])
        assert set(d) == {route[3], rkey, "next_after_score", "next_after_id"}
        for bad in ("0", "300", "abc", "nan"):
            assert _get(app, path, "%s=x&prob_scale=%s" % (arg, bad))[0].startswith("400")
    h.close()
