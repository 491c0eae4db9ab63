"""sse_set_option and sse_get_counter by name: every option's accepted range and the exact text of every refusal, every
counter's name, and the check order of the filtered / grouped / after calls on a handle without an index.

Two tiny handles, created once; nothing here encodes, scores or trains.  The option and counter names are the C ABI's
(csrc/sse_api.hip: OPTIONS, COUNTERS); everything else is what the calls answer."""
import numpy as np
import pytest

from tests.util import model_params

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ANY = (0, 1, I32_MIN, I32_MAX)           # a switch takes any value: on unless 0

# option -> (default, legal values with the extremes)
OPTIONS = {
    "score_small_index": (1, ANY), "score_small_x3": (1, ANY), "score_filtered_skip": (1, ANY), "score_bf16": (1, ANY),
    "train_bwd_x3": (0, ANY), "train_fwd_x3": (0, ANY), "train_dk_x3": (0, ANY), "train_generic": (0, ANY),
    "train_gen1": (0, ANY), "train_pair_dedup": (1, ANY), "train_serial": (0, ANY), "pad_skip": (1, ANY),
    "lstm_gate_split": (1, ANY), "lstm_x3": (0, ANY), "lstm_persist_inject_miss": (0, ANY),
    "lstm_cluster_drop_wg": (0, ANY), "lstm_cluster_coop": (1, ANY), "lstm_cluster_write_through": (0, ANY),
    "lstm_train_rows": (0, (0, 32, 64)),
    "eval_chunk_rows": (65536, (2, 3, I32_MAX)),
    "score_two_pass_min_rows": (49152, (0, I32_MAX)), "score_two_pass_rows": (524288, (0, I32_MAX)),
    "pad_sort_dev": (1, (0, 1, 2)),
    "lstm_persist_epoch": (0, (0, 2 ** 20 - 1)),
    "lstm_persist_rows": (32, (0, I32_MAX)),
    "lstm_cluster_backoff": (-1, (-1, 0, I32_MAX)),
    "lstm_cluster_chunks": (3, (1, I32_MAX)),
    "lstm_cluster_rows": (1024, (0, I32_MAX)), "lstm_small_rows": (1024, (0, I32_MAX)),
    "lstm_x_table": (1, (0, 1, 2)), "lstm_x_table_mb": (256, (0, I32_MAX)),
}
CNN_OPTIONS = {"cnn_bf16": (0, ANY)}

REFUSED = [
    ("lstm_train_rows", 16, "lstm_train_rows must be 0, 32 or 64"),
    ("eval_chunk_rows", 1, "eval_chunk_rows must be >= 2"),
    ("score_two_pass_min_rows", -1, "score_two_pass_min_rows must be >= 0"),
    ("score_two_pass_rows", -1, "score_two_pass_rows must be >= 0"),
    ("lstm_persist_rows", -1, "lstm_persist_rows must be >= 0"),
    ("lstm_cluster_rows", -1, "lstm_cluster_rows must be >= 0"),
    ("lstm_small_rows", -1, "lstm_small_rows must be >= 0"),
    ("lstm_x_table_mb", -1, "lstm_x_table_mb must be >= 0"),
    ("pad_sort_dev", 3, "pad_sort_dev must be 0 (off), 1 (adaptive) or 2 (always)"),
    ("lstm_x_table", 3, "lstm_x_table must be 0 (off), 1 (batches with B * T >= vocab_size) or 2 (always)"),
    ("lstm_persist_epoch", -1, "lstm_persist_epoch must be in [0, 2^20)"),
    ("lstm_persist_epoch", 2 ** 20, "lstm_persist_epoch must be in [0, 2^20)"),
    ("lstm_cluster_backoff", -2, "lstm_cluster_backoff must be >= 0 (or -1: automatic)"),
    ("lstm_cluster_chunks", 0, "lstm_cluster_chunks must be >= 1"),
]

COUNTERS = [
    "lstm_persist_fallbacks", "score_two_pass_calls", "pad_sorted_calls", "eval_paired_calls", "lstm_x_table_builds",
    "lstm_path_persist", "lstm_path_cluster", "lstm_path_small", "lstm_path_x3", "lstm_path_generic", "lstm_path_fwd",
    "lstm_fwd_rows32", "lstm_fwd_rows64", "lstm_fwd_gate_split", "lstm_fwd_x_table",
    "score_rank_band_rows", "score_rank_bruteforce_pairs",
    "score_above_band_rows", "score_above_bruteforce_pairs", "score_above_long_segments",
    "score_filtered_collected_rows", "score_filtered_bruteforce_queries", "score_filtered_tiles_skipped",
    "score_grouped_collected_rows", "score_grouped_bruteforce_queries",
    "score_after_collected_rows", "score_after_bruteforce_queries",
    "score_bf16_second_chance_queries", "score_collect_queries", "score_bruteforce_queries",
    "train_path_fused", "train_path_generic", "train_path_cnn", "train_paired_steps",
    "train_fp32_repacks", "train_split_repacks", "train_generic_repacks",
]


@pytest.fixture(scope="module")
def handles():
    import sse_amd
    dual = sse_amd.SSEModel(model_params("dual-encoder", 50, 8, 16, 16, 8, 8))
    cnn = sse_amd.SSEModel(model_params("source_only_cnn", 50, 8, 16, 16, 8, 8, N=11))
    yield {"dual": dual.handle, "cnn": cnn.handle}
    dual.handle.close()
    cnn.handle.close()


def _refused(call, *args):
    import sse_amd
    with pytest.raises(sse_amd.SSEError) as e:
        call(*args)
    return str(e.value)


@pytest.mark.parametrize("which", ["dual", "cnn"])
def test_every_counter_of_a_fresh_handle(handles, which):
    h = handles[which]
    assert len(COUNTERS) == 37 and len(set(COUNTERS)) == 37
    for name in COUNTERS:
        assert h.get_counter(name) == 0, name
    assert h.get_counter("lstm_coop_refused") >= 0      # process-wide
    assert _refused(h.get_counter, "x") == "unknown counter 'x'"


@pytest.mark.parametrize("which", ["dual", "cnn"])
def test_every_option_takes_its_range_and_refuses_the_rest(handles, which):
    h = handles[which]
    options = dict(OPTIONS, **CNN_OPTIONS) if which == "cnn" else OPTIONS
    for name, (default, legal) in options.items():
        try:
            for v in (default,) + tuple(legal):
                h.set_option(name, v)
        finally:
            h.set_option(name, default)
    for name, value, text in REFUSED:
        assert _refused(h.set_option, name, value) == text, (name, value)
        h.set_option(name, OPTIONS[name][0])             # a refusal leaves the handle usable
    assert _refused(h.set_option, "x", 1) == "unknown option 'x'"
    if which == "dual":
        for v in (0, 1):
            assert _refused(h.set_option, "cnn_bf16", v) == "option cnn_bf16 needs network_mode source_only_cnn"


def test_filtered_grouped_after_ask_for_the_index_first(handles):
    """Without an index every other argument error waits: k out of range, tag masks without tags, half a cursor."""
    h = handles["dual"]
    q = np.zeros((2, 8), np.float32)
    masks = np.ones(2, np.uint64)
    got = {
        "sse_score_topk_filtered": _refused(h.score_topk_filtered, q, 0, masks, masks, np.zeros((2, 65), np.int64)),
        "sse_score_topk_grouped": _refused(h.score_topk_grouped, q, 0, masks, masks),
        "sse_score_topk_after": _refused(h.score_topk_after, q, 0, None, masks, masks),
    }
    for name, text in got.items():
        assert text.startswith(name + ":") and text.endswith("no index uploaded"), text
