"""Paged requests of the serving routes (sse_serving.py; DESIGN K6j): a route called with after_score / after_id returns the rows
a direct Handle.score_topk_after call returns for the same encoding, plus next_after_score / next_after_id, which round-trip
through JSON bit for bit and lead through the whole ranked list; the same route without them returns exactly what it returned
before (Ranker.rank's encode + top-k call).  The ranker is a real one on an untrained model: a serving shell ranks whatever
encoder it is given."""
import json

import numpy as np
import pytest

from tests.util import make_pair, model_params

pytestmark = pytest.mark.gpu

N, T = 300, 8


def _ranker():
    from sse_amd import sse_serving
    m, _ = make_pair(model_params("dual-encoder", 50, 8, 16, 16, 16, T))
    rng = np.random.RandomState(5)
    enc = rng.standard_normal((N, 16))
    enc /= np.linalg.norm(enc, axis=1, keepdims=True)
    r = object.__new__(sse_serving.Ranker)                   # (no model directory: the attributes __init__ would have set)
    r.model, r.max_seq_length = m, T
    r.targetIDs, r.targetNames = ["id%d" % i for i in range(N)], ["name %d" % i for i in range(N)]
    m.handle.index_upload(enc)
    r._index_gen, r._encodings = m.handle.index_gen, enc
    r.tokens = lambda text: [0] * (T - 1 - len(text.split())) + [2 + (sum(map(ord, w)) % 48) for w in text.lower().split()] + [1]
    return r


def _get(app, path, qs):
    out = {}
    body = b"".join(app({"PATH_INFO": path, "QUERY_STRING": qs}, lambda st, hd: out.update(status=st)))
    return out["status"], body


@pytest.mark.parametrize("batch", [False, True])
def test_paged_routes_follow_the_direct_call_and_unpaged_ones_stay(batch):
    from sse_amd import sse_serving
    r = _ranker()
    h = r.model.handle
    app = sse_serving.create_app(ranker=r, batch=batch)
    text = "red nike shoes"
    tok = np.array([r.tokens(text)], np.int32)
    for path, arg, normalize, rkey, idk, scorek in [("/api/classify", "keywords", True, "ClassificationResults", "targetCategoryId", "confidenceScore"),
                                                    ("/api/search", "query", False, "SearchRankingResults", "ListingId", "rankingScore"),
                                                    ("/api/qna", "question", False, "Answers", "answerDocId", "confidenceScore"),
                                                    ("/api/crosslingual", "query", False, "SearchResults", "documentId", "confScore")]:
        route = sse_serving.ROUTES[path]
        enc = h.encode(0, tok, normalize)
        fs, fi = h.score_topk(enc, N)
        # without a cursor: today's JSON, byte for byte what the unpaged code path builds
        st, body = _get(app, path, "%s=red+nike+shoes&nbest=7" % arg)
        assert st.startswith("200")
        ts, ti = h.encode_score_topk(0, tok, normalize, 7)
        want = {route[3]: text, rkey: [{idk: r.targetIDs[ti[0, j]], route[5][1]: r.targetNames[ti[0, j]], scorek: float(ts[0, j])} for j in range(7)]}
        assert body == json.dumps(want).encode("utf-8")
        # with one: the direct call's rows and the cursor of the page after
        cs, ci = float(fs[0, 6]), int(fi[0, 6])
        seen = list(zip(fs[0, :7].tolist(), fi[0, :7].tolist()))
        while True:
            st, body = _get(app, path, "%s=red+nike+shoes&nbest=64&after_score=%r&after_id=%d" % (arg, cs, ci))
            assert st.startswith("200"), body
            d = json.loads(body)
            ds, di, dc = h.score_topk_after(enc, 64, after=([cs], [ci]))
            c = int(dc[0])
            assert [x[idk] for x in d[rkey]] == [r.targetIDs[j] for j in di[0, :c]]
            assert [x[scorek] for x in d[rkey]] == ds[0, :c].tolist()            # repr round-trips: the same bits
            assert set(d) == {route[3], rkey, "next_after_score", "next_after_id"}
            if c == 0:
                assert (d["next_after_score"], d["next_after_id"]) == (cs, ci)
                break
            assert (d["next_after_score"], d["next_after_id"]) == (float(ds[0, c - 1]), int(di[0, c - 1]))
            seen += list(zip(ds[0, :c].tolist(), di[0, :c].tolist()))
            cs, ci = d["next_after_score"], d["next_after_id"]
        assert seen == list(zip(fs[0].tolist(), fi[0].tolist()))                 # the pages are the whole ranked list
        st, body = _get(app, path, "%s=x&after_score=inf&after_id=0&nbest=3" % arg)   # 'inf' starts at the top
        assert st.startswith("200") and len(json.loads(body)[rkey]) == 3
        assert _get(app, path, "%s=x&after_score=0.5" % arg)[0].startswith("400")
        assert _get(app, path, "%s=x&after_id=3" % arg)[0].startswith("400")
        assert _get(app, path, "%s=x&after_score=abc&after_id=3" % arg)[0].startswith("400")
    h.close()
