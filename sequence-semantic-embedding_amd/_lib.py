"""ctypes binding of libsse_hip.so (C ABI in include/sse_hip.h).

There is NO CPU fallback: if the library is missing or no HIP device is
visible, loading / handle creation raises.
"""
import atexit
import ctypes as C
import weakref
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SSE_HIP_LIB: developer knob for A/B timing of two builds of the same C ABI (tools/ab); never a CPU fallback
LIB_PATH = os.environ.get("SSE_HIP_LIB") or os.path.join(HERE, "libsse_hip.so")

MODE_IDS = {"dual-encoder": 0, "shared-encoder": 1, "source-encoder-only": 2, "source_only_cnn": 3}
SIDE_SOURCE, SIDE_TARGET = 0, 1


class SSEConfig(C.Structure):
    _fields_ = [("network_mode", C.c_int32), ("vocab_size", C.c_int32), ("embedding_size", C.c_int32),
                ("encoding_size", C.c_int32), ("src_cell_size", C.c_int32), ("tgt_cell_size", C.c_int32),
                ("max_seq_length", C.c_int32), ("target_space_size", C.c_int32), ("device", C.c_int32),
                ("learning_rate", C.c_float), ("learning_rate_decay_factor", C.c_float)]


# every symbol declared in include/sse_hip.h: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "sse_create": (C.c_int, [C.POINTER(SSEConfig), C.POINTER(_P)]),
    "sse_destroy": (None, [_P]),
    "sse_last_error": (C.c_char_p, [_P]),
    "sse_num_variables": (C.c_int, [_P]),
    "sse_variable_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sse_set_variable": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "sse_get_variable": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "sse_encode": (C.c_int, [_P, C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "sse_encode_dev": (C.c_int, [_P, C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "sse_set_option": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "sse_get_counter": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "sse_l2_normalize_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, _P]),
    "sse_inbatch_loss_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P, _P]),
    "sse_inbatch_loss_window_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                              _P, _P, _P, _P, _P]),
    "sse_class_loss_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P, _P]),
    "sse_index_upload": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64]),
    "sse_index_upload_f64": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64]),
    "sse_index_set_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int64, _P]),
    "sse_index_shape": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)]),
    "sse_index_update": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P]),
    "sse_index_update_f64": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P]),
    "sse_index_update_dev": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "sse_index_append": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "sse_index_append_f64": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "sse_index_append_dev": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P]),
    "sse_score_topk": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "sse_score_topk_dev": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "sse_score_rank": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, _P, _P, _P]),
    "sse_score_rank_dev": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "sse_score_above": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P, _P]),
    "sse_score_above_dev": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "sse_index_set_tags": (C.c_int, [_P, _P, C.c_int64]),
    "sse_index_set_tags_dev": (C.c_int, [_P, _P, C.c_int64, _P]),
    "sse_score_topk_filtered": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P]),
    "sse_score_topk_filtered_dev": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, _P]),
    "sse_index_set_groups": (C.c_int, [_P, _P, C.c_int64]),
    "sse_index_set_groups_dev": (C.c_int, [_P, _P, C.c_int64, _P]),
    "sse_score_topk_grouped": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "sse_score_topk_grouped_dev": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "sse_score_topk_after": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "sse_score_topk_after_dev": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sse_score_confusions": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_double, _P, _P, _P, _P, _P]),
    "sse_score_confusions_dev": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_double, _P, _P, _P, _P, _P, _P]),
    "sse_index_set_bias": (C.c_int, [_P, _P, C.c_int64]),
    "sse_index_set_bias_dev": (C.c_int, [_P, _P, C.c_int64, _P]),
    "sse_score_topk_biased": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "sse_score_topk_biased_dev": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "sse_score_lse": (C.c_int, [_P, _P, C.c_int32, C.c_float, _P, _P, _P, _P, _P, _P]),
    "sse_score_lse_dev": (C.c_int, [_P, _P, C.c_int32, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    "sse_encode_score_topk": (C.c_int, [_P, C.c_int, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "sse_merge_topk_dev": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "sse_merge_topk_strided_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "sse_rccl_library_path": (C.c_char_p, []),
    "sse_rccl_group_start": (C.c_int, []),
    "sse_rccl_group_end": (C.c_int, []),
    "sse_rccl_get_unique_id": (C.c_int, [_P]),
    "sse_rccl_comm_init_rank": (C.c_int, [_P, C.POINTER(_P), C.c_int32, C.c_int32, _P]),
    "sse_rccl_comm_destroy": (C.c_int, [_P, _P]),
    "sse_allgather_merge_topk_dev": (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "sse_score_topk_sharded_dev": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "sse_train_step": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sse_set_stream": (C.c_int, [_P, _P]),
    "sse_train_grad_count": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "sse_train_set_grad_arena": (C.c_int, [_P, _P, C.c_int64]),
    "sse_train_grads": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64]),
    "sse_train_apply": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sse_train_packed_embedding_floats": (C.c_int64, [_P, C.c_int32]),
    "sse_train_pack_embedding_grad": (C.c_int, [_P, C.c_int32, _P]),
    "sse_train_unpack_embedding_grad": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "sse_corpus_upload": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.c_int32]),
    "sse_train_step_rows": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sse_train_grads_rows": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int64]),
    "sse_train_forward": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int64]),
    "sse_train_forward_rows": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int64]),
    "sse_train_open_encodings_dev": (C.c_int, [_P, C.c_int, _P, _P]),
    "sse_train_backward_dev": (C.c_int, [_P, _P, _P, C.c_float, C.c_float]),
    "sse_train_exchange_floats": (C.c_int64, [_P, C.c_int32, C.c_int32]),
    "sse_train_pack_exchange": (C.c_int, [_P, C.c_int32, _P]),
    "sse_train_backward_inbatch_global": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "sse_eval_loss": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(C.c_double), _P]),
    "sse_eval_loss_rows": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(C.c_double), _P]),
    "sse_get_learning_rate": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "sse_set_learning_rate": (C.c_int, [_P, C.c_float]),
    "sse_decay_learning_rate": (C.c_int, [_P]),
    "sse_get_global_step": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "sse_set_global_step": (C.c_int, [_P, C.c_int64]),
    "sse_timer_record": (C.c_int, [_P, C.c_int32, _P]),
    "sse_timer_elapsed_ms": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    "sse_synchronize": (C.c_int, [_P]),
    "sse_format_rows_stride": (C.c_int64, [C.c_int32]),
    "sse_format_rows_f32": (C.c_int, [_P, C.c_int64, C.c_int32, _P, _P]),
    "sse_parse_rows_f64": (C.c_int, [C.c_char_p, _P, C.c_int64, C.c_int32, _P, C.POINTER(C.c_int64)]),
    "sse_crc32c": (C.c_uint32, [_P, C.c_int64, C.c_uint32]),
}

_lib = None
_host_lib = None
HOST_LIB_PATH = os.path.join(HERE, "libsse_host.so")
HOST_SYMBOLS = ("sse_format_rows_stride", "sse_format_rows_f32", "sse_parse_rows_f64", "sse_crc32c")


def load_host_library():
    """The host-only entry points of include/sse_hip.h (index text I/O, CRC-32C) from libsse_host.so: the same C code
    (csrc/index_io.cpp) linked WITHOUT the HIP runtime, so that reading a TF checkpoint or an index file neither imports
    torch nor touches a GPU.  Falls back to the full library when only that one is built."""
    global _host_lib
    if _host_lib is not None:
        return _host_lib
    if _lib is not None or not os.path.exists(HOST_LIB_PATH):
        _host_lib = load_library()
        return _host_lib
    lib = C.CDLL(HOST_LIB_PATH)
    for name in HOST_SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = SYMBOLS[name]
    _host_lib = lib
    return lib


def load_library():
    """dlopen libsse_hip.so (once).  When torch is importable it is imported
    FIRST so that both share one HIP runtime (torch bundles its own
    libamdhip64.so.7; two copies in one process cannot share device memory)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libsse_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    if "torch" not in sys.modules and os.environ.get("SSE_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# The argument checks and output buffers the host forms of the scoring family share (score_topk_filtered, _grouped, _after,
# _biased, score_lse, score_confusions, score_rank, score_above): one copy of each message.

def _opt(a):
    return _ptr(a) if a is not None else None


def _queries(queries):
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim != 2:
        raise ValueError("queries must be [Q,S]")
    return q


def _masks(any_of, none_of, Q):
    """[any_of, none_of] as uint64 [Q] arrays (None stays None), any_of checked first."""
    masks = []
    for m in (any_of, none_of):
        if m is not None:
            m = np.ascontiguousarray(m, dtype=np.uint64).reshape(-1)
            if m.shape[0] != Q:
                raise ValueError("any_of / none_of must be uint64 [Q]")
        masks.append(m)
    return masks


def _weights(weight, Q):
    """None, a scalar or float32 [Q] -> None or float32 [Q]."""
    if weight is None:
        return None
    w = np.asarray(weight, dtype=np.float32)
    w = np.full(Q, w, np.float32) if w.ndim == 0 else np.ascontiguousarray(w.reshape(-1))
    if w.shape[0] != Q:
        raise ValueError("weight must be a scalar or float32 [Q]")
    return w


def _topk_out(Q, k):
    """(scores float64 [Q,k], ids int64 [Q,k], counts int32 [Q]); a negative k is left to the library to refuse."""
    return np.empty((Q, max(k, 0)), np.float64), np.empty((Q, max(k, 0)), np.int64), np.empty(Q, np.int32)


class SSEError(RuntimeError):
    pass


# Handles still alive when the interpreter exits are closed by an atexit hook, i.e. BEFORE module teardown and before the C-level
# exit handlers: Handle.__del__ otherwise runs during interpreter finalisation, when the HIP runtime (and, under rocprofv3, the
# profiler's intercept layer) may already be on its way out.
_live_handles = weakref.WeakSet()


def _close_live_handles():
    for h in list(_live_handles):
        try:
            h.close()
        except Exception:
            pass


atexit.register(_close_live_handles)


class Handle(object):
    """Owner of one `sse_handle*`."""

    def __init__(self, cfg):
        self.lib = load_library()
        self._h = C.c_void_p()
        _live_handles.add(self)
        self.index_gen = 0          # bumped by every index upload: lets holders of "their" index notice a replacement
        rc = self.lib.sse_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise SSEError(self.lib.sse_last_error(None).decode())
        self.cfg = cfg
        # SSE_OPTIONS="name=value,name=value": library options (sse_set_option) for any command line without touching it,
        # e.g. SSE_OPTIONS=lstm_x3=1 python sse_index.py ...; an option the network mode rejects fails loudly
        for item in filter(None, (x.strip() for x in os.environ.get("SSE_OPTIONS", "").split(","))):
            name, _, value = item.partition("=")
            self.set_option(name.strip(), int(value or "1"))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.sse_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise SSEError(self.lib.sse_last_error(self._h).decode())

    # -- variables ---------------------------------------------------------
    def variables(self):
        out = []
        name, cnt, r, c = C.c_char_p(), C.c_int64(), C.c_int32(), C.c_int32()
        for i in range(self.lib.sse_num_variables(self._h)):
            self.check(self.lib.sse_variable_info(self._h, i, C.byref(name), C.byref(cnt), C.byref(r), C.byref(c)))
            out.append((name.value.decode(), int(cnt.value), int(r.value), int(c.value)))
        return out

    def set_variable(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        self.check(self.lib.sse_set_variable(self._h, name.encode(), _ptr(a), a.size))

    def get_variable(self, name, count):
        a = np.empty(count, np.float32)
        self.check(self.lib.sse_get_variable(self._h, name.encode(), _ptr(a), a.size))
        return a

    # -- encode ------------------------------------------------------------
    def encode(self, side, ids, normalize=True):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim != 2:
            raise ValueError("ids must be [B,T]")
        B, T = ids.shape
        out = np.empty((B, self.cfg.encoding_size), np.float32)
        self.check(self.lib.sse_encode(self._h, side, _ptr(ids), B, T, 1 if normalize else 0, _ptr(out)))
        return out

    def encode_dev(self, side, ids_ptr, B, T, normalize, out_ptr, stream=0):
        self.check(self.lib.sse_encode_dev(self._h, side, ids_ptr, B, T, 1 if normalize else 0, out_ptr, stream))

    def set_option(self, name, value):
        self.check(self.lib.sse_set_option(self._h, name.encode(), int(value)))

    def get_counter(self, name):
        v = C.c_int64()
        self.check(self.lib.sse_get_counter(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def l2_normalize_dev(self, x_ptr, out_ptr, rows, cols, stream=0):
        self.check(self.lib.sse_l2_normalize_dev(self._h, x_ptr, out_ptr, rows, cols, stream))

    def inbatch_loss_dev(self, src_raw, tgt_raw, labels, src_key, tgt_key, B, S, scale, inv_rows, d_src, d_tgt, row_loss,
                         row_acc, stream=0):
        """sse_inbatch_loss_dev: the in-batch softmax loss head on device buffers.  Every buffer is a torch CUDA tensor
        (contiguous; float32, keys int64) or a raw device pointer; src_key / tgt_key None = every row distinct; d_src and
        d_tgt both None = loss and accuracy only.  Queued on `stream`, nothing is synchronised."""
        def dev(x):
            if x is None:
                return None
            return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        self.check(self.lib.sse_inbatch_loss_dev(self._h, dev(src_raw), dev(tgt_raw), dev(labels), dev(src_key), dev(tgt_key),
                                                 int(B), int(S), float(scale), float(inv_rows), dev(d_src), dev(d_tgt),
                                                 dev(row_loss), dev(row_acc), stream))

    def inbatch_loss_window_dev(self, src_raw, tgt_raw, labels, src_key, tgt_key, B, S, row_lo, row_hi, scale, inv_rows, d_src,
                                d_tgt, row_loss, row_acc, stream=0):
        """sse_inbatch_loss_window_dev: inbatch_loss_dev over the B rows, its outputs cut to the rows [row_lo, row_hi): d_src /
        d_tgt [row_hi - row_lo][S], row_loss / row_acc [row_hi - row_lo]; every output row carries the bits of the same row of
        inbatch_loss_dev.  What a rank of a data-parallel step runs over the gathered global batch."""
        def dev(x):
            if x is None:
                return None
            return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        self.check(self.lib.sse_inbatch_loss_window_dev(self._h, dev(src_raw), dev(tgt_raw), dev(labels), dev(src_key), dev(tgt_key),
                                                        int(B), int(S), int(row_lo), int(row_hi), float(scale), float(inv_rows),
                                                        dev(d_src), dev(d_tgt), dev(row_loss), dev(row_acc), stream))

    def class_loss_dev(self, src_raw, table, tgt_row, labels, src_key, B, N, S, scale, inv_rows, d_src, d_table, row_loss,
                       row_acc, stream=0):
        """sse_class_loss_dev: the class softmax loss head (softmax over all N rows of `table`) on device buffers.  Every
        buffer is a torch CUDA tensor (contiguous; float32, tgt_row int32, src_key int64) or a raw device pointer; src_key
        None = every row a source of its own; d_src and d_table both None = loss and accuracy only.  Queued on `stream`,
        nothing is synchronised; a target row outside [0, N) raises the handle's error flag (reported by synchronize())."""
        def dev(x):
            if x is None:
                return None
            return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))
        self.check(self.lib.sse_class_loss_dev(self._h, dev(src_raw), dev(table), dev(tgt_row), dev(labels), dev(src_key),
                                               int(B), int(N), int(S), float(scale), float(inv_rows), dev(d_src), dev(d_table),
                                               dev(row_loss), dev(row_acc), stream))

    # -- index / scoring -----------------------------------------------------
    def index_upload(self, rows, id_base=0):
        rows = np.ascontiguousarray(rows)
        if rows.ndim != 2:
            raise ValueError("index rows must be [N,S]")
        N, S = rows.shape
        if rows.dtype == np.float64:
            self.check(self.lib.sse_index_upload_f64(self._h, _ptr(rows), N, S, id_base))
        else:
            rows = np.ascontiguousarray(rows, dtype=np.float32)
            self.check(self.lib.sse_index_upload(self._h, _ptr(rows), N, S, id_base))
        self.index_gen += 1

    def index_set_dev(self, rows_ptr, N, S, id_base=0, stream=0):
        self.check(self.lib.sse_index_set_dev(self._h, rows_ptr, N, S, id_base, stream))
        self.index_gen += 1

    def index_shape(self):
        """(rows, dimension, id_base) of the resident index as the library holds them; zeros when none is resident."""
        n, s, b = C.c_int64(), C.c_int32(), C.c_int64()
        self.check(self.lib.sse_index_shape(self._h, C.byref(n), C.byref(s), C.byref(b), None))
        return int(n.value), int(s.value), int(b.value)

    def index_norm_max(self):
        """The largest row norm of the resident index as the library formed it (float32), the bound its certificates use."""
        v = C.c_float()
        self.check(self.lib.sse_index_shape(self._h, None, None, None, C.byref(v)))
        return np.float32(v.value)

    index_rows = property(lambda self: self.index_shape()[0])
    index_base = property(lambda self: self.index_shape()[2])

    # In-place updates (sse_index_update* / sse_index_append*).  They change the holder's own index, so index_gen stays.
    @staticmethod
    def _index_delta_args(rows, M, tags, groups, bias):
        """rows [M,S] float32 / float64 (or None) and the three optional columns of M values, contiguous."""
        if rows is not None:
            rows = np.ascontiguousarray(rows)
            if rows.dtype != np.float64:
                rows = np.ascontiguousarray(rows, dtype=np.float32)
            if rows.ndim != 2 or (M is not None and rows.shape[0] != M):
                raise ValueError("rows must be [M,S], one row per id")
            M = rows.shape[0]
        cols = []
        for name, v, dt in (("tags", tags, np.uint64), ("groups", groups, np.int64), ("bias", bias, np.float32)):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=dt).reshape(-1)
                if M is not None and v.shape[0] != M:
                    raise ValueError("%s must hold one value per row (%d), got %d" % (name, M, v.shape[0]))
                M = v.shape[0]
            cols.append(v)
        return rows, cols, M

    def index_update(self, ids, rows=None, tags=None, groups=None, bias=None):
        """Replace rows of the resident index in place: ids int64 [M] global ids (any order; of a repeated id the LAST
        entry wins), rows [M,S] (float64 selects the _f64 form, for an index uploaded as float64) and / or one tag word,
        group key or bias value per id.  rows=None changes the given columns only.  After the call the handle answers as
        one freshly given the final rows and columns."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        rows, cols, M = self._index_delta_args(rows, ids.shape[0], tags, groups, bias)
        # sorted, the last of equal ids kept: a stable sort of the reversed list puts it first in its run
        order = (ids.shape[0] - 1 - np.argsort(ids[::-1], kind="stable")).astype(np.int64)
        keep = np.ones(order.shape[0], bool)
        keep[1:] = ids[order][1:] != ids[order][:-1]
        order = order[keep]
        if order.shape[0] != ids.shape[0] or (order[1:] < order[:-1]).any():   # (ids already strictly increasing: no copies)
            ids = np.ascontiguousarray(ids[order])
            if rows is not None:
                rows = np.ascontiguousarray(rows[order])
            cols = [None if c is None else np.ascontiguousarray(c[order]) for c in cols]
        fn = self.lib.sse_index_update_f64 if rows is not None and rows.dtype == np.float64 else self.lib.sse_index_update
        self.check(fn(self._h, _ptr(ids), _opt(rows), ids.shape[0], _opt(cols[0]), _opt(cols[1]), _opt(cols[2])))

    def index_update_dev(self, ids_ptr, rows_ptr, M, tags_ptr=None, groups_ptr=None, bias_ptr=None, stream=0):
        """index_update on device pointers: ids int64 [M] strictly increasing (checked on the device: a bad list changes
        nothing and raises), rows float32 [M,S] or None / 0.  Runs on `stream`, which is synchronised once."""
        self.check(self.lib.sse_index_update_dev(self._h, ids_ptr, rows_ptr or None, int(M), tags_ptr or None, groups_ptr or None,
                                                 bias_ptr or None, stream))

    def index_append(self, rows, tags=None, groups=None, bias=None):
        """Append rows [M,S] behind the resident index (float64 selects the _f64 form); each column must be given exactly
        when it is set on the index.  Returns the id of the first new row."""
        rows, cols, M = self._index_delta_args(rows, None, tags, groups, bias)
        if rows is None:
            raise ValueError("rows must be [M,S]")
        first = self.index_base + self.index_rows
        fn = self.lib.sse_index_append_f64 if rows.dtype == np.float64 else self.lib.sse_index_append
        self.check(fn(self._h, _ptr(rows), M, _opt(cols[0]), _opt(cols[1]), _opt(cols[2])))
        return first

    def index_append_dev(self, rows_ptr, M, tags_ptr=None, groups_ptr=None, bias_ptr=None, stream=0):
        """index_append on device pointers (rows float32 [M,S]), on `stream`, which is synchronised once.  Returns the id
        of the first new row."""
        first = self.index_base + self.index_rows
        self.check(self.lib.sse_index_append_dev(self._h, rows_ptr, int(M), tags_ptr or None, groups_ptr or None, bias_ptr or None,
                                                 stream))
        return first

    def score_topk(self, queries, k):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2:
            raise ValueError("queries must be [Q,S]")
        Q = q.shape[0]
        scores = np.empty((Q, k), np.float64)
        ids = np.empty((Q, k), np.int64)
        self.check(self.lib.sse_score_topk(self._h, _ptr(q), Q, k, _ptr(scores), _ptr(ids)))
        return scores, ids

    def encode_score_topk(self, side, ids, normalize, k, want_encodings=False):
        """encode + cosine top-k with the encodings staying on the device (sse_demo.py:121-129,
        sse_evaluator.py:107-111); returns (scores [B,k] f64, ids [B,k] i64[, encodings [B,S] f32])."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim != 2:
            raise ValueError("ids must be [B,T]")
        B, T = ids.shape
        scores = np.empty((B, k), np.float64)
        rows = np.empty((B, k), np.int64)
        enc = np.empty((B, self.cfg.encoding_size), np.float32) if want_encodings else None
        self.check(self.lib.sse_encode_score_topk(self._h, side, _ptr(ids), B, T, 1 if normalize else 0, int(k),
                                                  _ptr(scores), _ptr(rows), _ptr(enc) if want_encodings else None))
        return (scores, rows, enc) if want_encodings else (scores, rows)

    def score_topk_dev(self, q_ptr, Q, k, scores_ptr, ids_ptr, stream=0):
        self.check(self.lib.sse_score_topk_dev(self._h, q_ptr, Q, k, scores_ptr, ids_ptr, stream))

    def score_rank(self, queries, pair_q, pair_id, pair_score=None):
        """Exact rank over the whole resident index: for pair p (query row pair_q[p], row id pair_id[p]) the number of
        rows ranked before it in score_topk's order.  pair_score=None: pair_id are rows of this index, the result is
        their 0-based rank and their float64 score.  pair_score given: rows before the threshold (pair_score[p],
        pair_id[p]), any id -- what a shard counts for a label of another shard.  Returns (before int64 [L], score
        float64 [L]); the output arrays are handed back untouched (zeros) only on success -- an error raises."""
        q = _queries(queries)
        pq = np.ascontiguousarray(pair_q, dtype=np.int32).reshape(-1)
        pid = np.ascontiguousarray(pair_id, dtype=np.int64).reshape(-1)
        if pq.shape != pid.shape:
            raise ValueError("pair_q and pair_id must both be [L]")
        L = pq.shape[0]
        ps = None
        if pair_score is not None:
            ps = np.ascontiguousarray(pair_score, dtype=np.float64).reshape(-1)
            if ps.shape != pq.shape:
                raise ValueError("pair_score must be [L]")
        before = np.zeros(L, np.int64)
        score = np.zeros(L, np.float64) if ps is None else ps.copy()
        self.check(self.lib.sse_score_rank(self._h, _ptr(q), q.shape[0], _ptr(pq), _ptr(pid), L,
                                           _opt(ps), _ptr(before), _ptr(score)))
        return before, score

    def score_rank_dev(self, q_ptr, Q, pair_q_ptr, pair_id_ptr, L, pair_score_ptr, before_ptr, score_ptr, stream=0):
        """score_rank on device pointers (pair_score_ptr / score_ptr may be None / 0), enqueued on `stream`; a bad pair
        is reported by synchronize()."""
        self.check(self.lib.sse_score_rank_dev(self._h, q_ptr, Q, pair_q_ptr, pair_id_ptr, int(L), pair_score_ptr or None,
                                               before_ptr, score_ptr or None, stream))

    def _above_args(self, queries, thr, pair_q):
        q = _queries(queries)
        t = np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)
        pq = np.arange(q.shape[0], dtype=np.int32) if pair_q is None else np.ascontiguousarray(pair_q, dtype=np.int32).reshape(-1)
        if pq.shape != t.shape:
            raise ValueError("thr and pair_q must both be [L] (pair_q defaults to arange(Q))")
        return q, t, pq

    def score_above(self, queries, thr, pair_q=None, cap=None):
        """All rows of the resident index with float64 score >= thr[p] for query row pair_q[p] (default: pair p is query
        p).  Returns (offsets int64 [L+1], ids int64 [total], scores float64 [total]): segment offsets[p]:offsets[p+1] holds
        pair p's rows in score_topk's order (score descending, lower id first) with score_topk's score bits.  Without `cap`
        a capacity is guessed and, when the total turned out larger, the call repeated with exactly the total.  With `cap`
        the library's contract is handed through: one call, lists of `cap` entries, and when offsets[-1] > cap the lists
        come back as (None, None) -- read offsets[-1] and call again."""
        q, t, pq = self._above_args(queries, thr, pair_q)
        L = pq.shape[0]
        offsets = np.zeros(L + 1, np.int64)
        room = int(cap) if cap is not None else max(1024, 64 * L)
        while True:
            ids = np.empty(room, np.int64)
            scores = np.empty(room, np.float64)
            self.check(self.lib.sse_score_above(self._h, _ptr(q), q.shape[0], _ptr(pq), _ptr(t), L, room, _ptr(offsets),
                                                _ptr(ids), _ptr(scores)))
            total = int(offsets[-1])
            if total <= room:
                return offsets, ids[:total], scores[:total]
            if cap is not None:
                return offsets, None, None
            room = total

    def count_above(self, queries, thr, pair_q=None):
        """The counts alone: int64 [L], rows with float64 score >= thr[p] for query row pair_q[p]."""
        q, t, pq = self._above_args(queries, thr, pair_q)
        L = pq.shape[0]
        offsets = np.zeros(L + 1, np.int64)
        self.check(self.lib.sse_score_above(self._h, _ptr(q), q.shape[0], _ptr(pq), _ptr(t), L, 0, _ptr(offsets), None, None))
        return np.diff(offsets)

    def score_above_dev(self, q_ptr, Q, pair_q_ptr, pair_thr_ptr, L, cap, offsets_ptr, ids_ptr, scores_ptr, stream=0):
        """score_above on device pointers (ids_ptr / scores_ptr both None / 0: counts only), enqueued on `stream`; whether
        the total fits `cap` is decided on the device; a bad pair is reported by synchronize()."""
        self.check(self.lib.sse_score_above_dev(self._h, q_ptr, Q, pair_q_ptr, pair_thr_ptr, int(L), int(cap), offsets_ptr,
                                                ids_ptr or None, scores_ptr or None, stream))

    def index_set_tags(self, tags):
        """One uint64 tag word per row of the resident index (tags=None clears them); a new index clears them too."""
        self._index_set_column(self.lib.sse_index_set_tags, tags, np.uint64)

    def _index_set_column(self, fn, values, dtype):
        """index_set_tags / _groups / _bias: one value of `dtype` per row of the resident index; None clears the column."""
        if values is None:
            self.check(fn(self._h, None, 0))
            return
        v = np.ascontiguousarray(values, dtype=dtype).reshape(-1)
        self.check(fn(self._h, _ptr(v), v.shape[0]))

    def index_set_tags_dev(self, tags_ptr, N, stream=0):
        """index_set_tags from a device pointer of N uint64 words (None / 0 clears), copied on `stream`."""
        self.check(self.lib.sse_index_set_tags_dev(self._h, tags_ptr or None, int(N), stream))

    def score_topk_filtered(self, queries, k, any_of=None, none_of=None, exclude=None):
        """Exact top-k among the rows each query may return.  any_of / none_of: uint64 [Q] tag masks (a row is eligible
        when it carries a bit of any_of -- or any_of is 0 -- and no bit of none_of); exclude: int64 [Q, n] row ids a query
        must not return (n <= 64; ids outside the index, e.g. -1 padding, are ignored).  Returns (scores float64 [Q,k],
        ids int64 [Q,k], counts int32 [Q]): the first counts[q] columns are score_topk's columns with the ineligible rows
        removed, the rest hold (-inf, INT64_MAX)."""
        q = _queries(queries)
        Q, k = q.shape[0], int(k)
        masks = _masks(any_of, none_of, Q)
        ex, n_excl = None, 0
        if exclude is not None:
            ex = np.ascontiguousarray(exclude, dtype=np.int64)
            if ex.ndim != 2 or ex.shape[0] != Q:
                raise ValueError("exclude must be int64 [Q, n]")
            n_excl = ex.shape[1]
            if n_excl == 0:
                ex = None
        scores, ids, counts = _topk_out(Q, k)
        self.check(self.lib.sse_score_topk_filtered(self._h, _ptr(q), Q, k, _opt(masks[0]), _opt(masks[1]), _opt(ex), n_excl,
                                                    _ptr(scores), _ptr(ids), _ptr(counts)))
        return scores, ids, counts

    def score_topk_filtered_dev(self, q_ptr, Q, k, any_ptr, none_ptr, excl_ptr, n_excl, scores_ptr, ids_ptr, counts_ptr, stream=0):
        """score_topk_filtered on device pointers (any_ptr / none_ptr / excl_ptr may be None / 0), enqueued on `stream`."""
        self.check(self.lib.sse_score_topk_filtered_dev(self._h, q_ptr, int(Q), int(k), any_ptr or None, none_ptr or None,
                                                        excl_ptr or None, int(n_excl), scores_ptr, ids_ptr, counts_ptr, stream))

    def index_set_groups(self, groups):
        """One int64 group key per row of the resident index (groups=None clears them); a new index clears them too."""
        self._index_set_column(self.lib.sse_index_set_groups, groups, np.int64)

    def index_set_groups_dev(self, groups_ptr, N, stream=0):
        """index_set_groups from a device pointer of N int64 keys (None / 0 clears), copied on `stream`."""
        self.check(self.lib.sse_index_set_groups_dev(self._h, groups_ptr or None, int(N), stream))

    def score_topk_grouped(self, queries, k, any_of=None, none_of=None):
        """Exact top-k distinct groups of index rows (keys: index_set_groups).  any_of / none_of: uint64 [Q] tag masks, the
        eligibility rule of score_topk_filtered.  Returns (scores float64 [Q,k], ids int64 [Q,k], groups int64 [Q,k], counts
        int32 [Q]): the first counts[q] columns hold each group once, represented by its best eligible row (the lowest id
        among equal bests), best group first; the rest hold (-inf, INT64_MAX, INT64_MAX)."""
        q = _queries(queries)
        Q, k = q.shape[0], int(k)
        masks = _masks(any_of, none_of, Q)
        scores, ids, counts = _topk_out(Q, k)
        groups = np.empty((Q, max(k, 0)), np.int64)
        self.check(self.lib.sse_score_topk_grouped(self._h, _ptr(q), Q, k, _opt(masks[0]), _opt(masks[1]),
                                                   _ptr(scores), _ptr(ids), _ptr(groups), _ptr(counts)))
        return scores, ids, groups, counts

    def score_topk_grouped_dev(self, q_ptr, Q, k, any_ptr, none_ptr, scores_ptr, ids_ptr, groups_ptr, counts_ptr, stream=0):
        """score_topk_grouped on device pointers (any_ptr / none_ptr may be None / 0), enqueued on `stream`."""
        self.check(self.lib.sse_score_topk_grouped_dev(self._h, q_ptr, int(Q), int(k), any_ptr or None, none_ptr or None,
                                                       scores_ptr, ids_ptr, groups_ptr, counts_ptr, stream))

    def score_topk_after(self, queries, k, after=None, any_of=None, none_of=None):
        """The next k rows of score_topk's ranked list after a cursor.  after: None (no cursor: the first page) or (scores
        float64 [Q], ids int64 [Q]), the last (score, id) each query has seen -- a row is after it when its float64 score is
        lower, or equal with a higher id; +inf starts at the top, NaN / -inf leave nothing.  any_of / none_of: uint64 [Q] tag
        masks, the eligibility rule of score_topk_filtered.  Returns (scores float64 [Q,k], ids int64 [Q,k], counts int32
        [Q]): the first counts[q] columns are score_topk's columns with the ineligible rows and the rows not after the cursor
        removed, the rest hold (-inf, INT64_MAX)."""
        q = _queries(queries)
        Q, k = q.shape[0], int(k)
        cs = ci = None
        if after is not None:
            cs = np.ascontiguousarray(after[0], dtype=np.float64).reshape(-1)
            ci = np.ascontiguousarray(after[1], dtype=np.int64).reshape(-1)
            if cs.shape[0] != Q or ci.shape[0] != Q:
                raise ValueError("after must be (scores float64 [Q], ids int64 [Q])")
        masks = _masks(any_of, none_of, Q)
        scores, ids, counts = _topk_out(Q, k)
        self.check(self.lib.sse_score_topk_after(self._h, _ptr(q), Q, k, _opt(cs), _opt(ci), _opt(masks[0]), _opt(masks[1]),
                                                 _ptr(scores), _ptr(ids), _ptr(counts)))
        return scores, ids, counts

    def score_topk_after_dev(self, q_ptr, Q, k, after_score_ptr, after_id_ptr, any_ptr, none_ptr, scores_ptr, ids_ptr, counts_ptr,
                             stream=0):
        """score_topk_after on device pointers (the cursor pointers both None / 0: no cursor; any_ptr / none_ptr may be
        None / 0), enqueued on `stream`."""
        self.check(self.lib.sse_score_topk_after_dev(self._h, q_ptr, int(Q), int(k), after_score_ptr or None, after_id_ptr or None,
                                                     any_ptr or None, none_ptr or None, scores_ptr, ids_ptr, counts_ptr, stream))

    def score_confusions(self, queries, k, positives, margin=np.inf):
        """The k best rows that are not among a query's positives and score at or above (its best positive's score) - margin
        (data.py:124-129 declares the mining and leaves it empty).  positives: int64 [Q, n_pos] or a sequence of Q sequences
        of row ids, padded with -1 (1 <= n_pos <= 64 after padding; ids outside the index are ignored); margin: finite or
        +inf (no cut).  Returns (scores float64 [Q,k], ids int64 [Q,k], counts int32 [Q], pos_scores float64 [Q], pos_ids
        int64 [Q]): the first counts[q] columns are score_topk's columns with the positives and the rows below the floor
        removed, the rest hold (-inf, INT64_MAX); (pos_scores, pos_ids) is the best positive, (-inf, INT64_MAX) without one."""
        q = _queries(queries)
        Q, k = q.shape[0], int(k)
        if isinstance(positives, np.ndarray) and positives.ndim == 2:
            pos = np.ascontiguousarray(positives, dtype=np.int64)
        else:
            rows = [np.asarray(p, np.int64).reshape(-1) for p in positives]
            pos = np.full((len(rows), max([len(r) for r in rows] + [1])), -1, np.int64)   # -1: no row has this id
            for i, r in enumerate(rows):
                pos[i, :len(r)] = r
        if pos.shape[0] != Q:
            raise ValueError("positives must be int64 [Q, n_pos]")
        scores, ids, counts = _topk_out(Q, k)
        pos_scores = np.empty(Q, np.float64)
        pos_ids = np.empty(Q, np.int64)
        self.check(self.lib.sse_score_confusions(self._h, _ptr(q), Q, k, _ptr(pos), pos.shape[1], float(margin), _ptr(scores),
                                                 _ptr(ids), _ptr(counts), _ptr(pos_scores), _ptr(pos_ids)))
        return scores, ids, counts, pos_scores, pos_ids

    def score_confusions_dev(self, q_ptr, Q, k, pos_ptr, n_pos, margin, scores_ptr, ids_ptr, counts_ptr, pos_score_ptr=None,
                             pos_id_ptr=None, stream=0):
        """score_confusions on device pointers (pos_score_ptr / pos_id_ptr may be None / 0), enqueued on `stream`."""
        self.check(self.lib.sse_score_confusions_dev(self._h, q_ptr, int(Q), int(k), pos_ptr or None, int(n_pos), float(margin),
                                                     scores_ptr, ids_ptr, counts_ptr, pos_score_ptr or None, pos_id_ptr or None,
                                                     stream))

    def index_set_bias(self, bias):
        """One float32 bias per row of the resident index (bias=None clears it); a new index clears it too.  A non-finite
        value is refused."""
        self._index_set_column(self.lib.sse_index_set_bias, bias, np.float32)

    def index_set_bias_dev(self, bias_ptr, N, stream=0):
        """index_set_bias from a device pointer of N float32 values (None / 0 clears), copied on `stream`."""
        self.check(self.lib.sse_index_set_bias_dev(self._h, bias_ptr or None, int(N), stream))

    def score_topk_biased(self, queries, k, weight=None, any_of=None, none_of=None):
        """Exact top-k by score + weight * bias[row] (bias: index_set_bias).  weight: None (1.0), a scalar or float32 [Q];
        any_of / none_of: uint64 [Q] tag masks, the eligibility rule of score_topk_filtered.  Returns (scores float64 [Q,k],
        ids int64 [Q,k], counts int32 [Q]): the first counts[q] columns are the eligible rows by biased score descending,
        equal scores by ascending id, scores holding score_topk's float64 score + float64(weight) * float64(bias); the rest
        hold (-inf, INT64_MAX)."""
        q = _queries(queries)
        Q, k = q.shape[0], int(k)
        w = _weights(weight, Q)
        masks = _masks(any_of, none_of, Q)
        scores, ids, counts = _topk_out(Q, k)
        self.check(self.lib.sse_score_topk_biased(self._h, _ptr(q), Q, k, _opt(w), _opt(masks[0]), _opt(masks[1]),
                                                  _ptr(scores), _ptr(ids), _ptr(counts)))
        return scores, ids, counts

    def score_topk_biased_dev(self, q_ptr, Q, k, weight_ptr, any_ptr, none_ptr, scores_ptr, ids_ptr, counts_ptr, stream=0):
        """score_topk_biased on device pointers (weight_ptr: float32 [Q]; weight_ptr / any_ptr / none_ptr may be None / 0),
        enqueued on `stream`."""
        self.check(self.lib.sse_score_topk_biased_dev(self._h, q_ptr, int(Q), int(k), weight_ptr or None, any_ptr or None,
                                                      none_ptr or None, scores_ptr, ids_ptr, counts_ptr, stream))

    def score_lse(self, queries, scale, weight=None, any_of=None, none_of=None):
        """Softmax log-partition over the tag-eligible rows of the resident index: lse[q] = log sum_r exp(scale * (score +
        weight[q] * bias[r])), scores and biased scores as score_topk / score_topk_biased return them, so that
        exp(scale * returned_score - lse[q]) is P(row | q) (sse_index.softmax_probs).  weight: None (no bias term), a scalar
        or float32 [Q]; any_of / none_of: uint64 [Q] tag masks, the eligibility rule of score_topk_filtered; 0 < scale <= 256.
        Returns (lse float64 [Q], -inf where no row is eligible; count int64 [Q], the eligible rows; bound float64 [Q], a
        certified bound on |lse - its float64 value|)."""
        q = _queries(queries)
        Q = q.shape[0]
        w = _weights(weight, Q)
        masks = _masks(any_of, none_of, Q)
        lse = np.empty(Q, np.float64)
        count = np.empty(Q, np.int64)
        bound = np.empty(Q, np.float64)
        self.check(self.lib.sse_score_lse(self._h, _ptr(q), Q, float(scale), _opt(w), _opt(masks[0]), _opt(masks[1]),
                                          _ptr(lse), _ptr(count), _ptr(bound)))
        return lse, count, bound

    def score_lse_dev(self, q_ptr, Q, scale, weight_ptr, any_ptr, none_ptr, lse_ptr, count_ptr, bound_ptr=None, stream=0):
        """score_lse on device pointers (weight_ptr: float32 [Q]; weight_ptr / any_ptr / none_ptr / bound_ptr may be None / 0;
        lse_ptr / bound_ptr: float64 [Q], count_ptr: int64 [Q]), enqueued on `stream`."""
        self.check(self.lib.sse_score_lse_dev(self._h, q_ptr, int(Q), float(scale), weight_ptr or None, any_ptr or None,
                                              none_ptr or None, lse_ptr, count_ptr, bound_ptr or None, stream))

    def merge_topk_strided_dev(self, in_s, in_i, shard_stride, P, Q, k, out_s, out_i, stream=0):
        self.check(self.lib.sse_merge_topk_strided_dev(self._h, in_s, in_i, int(shard_stride), P, Q, k, out_s, out_i, stream))

    def merge_topk_dev(self, in_s, in_i, P, Q, k, out_s, out_i, stream=0):
        self.check(self.lib.sse_merge_topk_dev(self._h, in_s, in_i, P, Q, k, out_s, out_i, stream))

    # -- RCCL exchange without torch ------------------------------
    def rccl_unique_id(self):
        """A fresh 128-byte ncclUniqueId (rank 0 creates it; the other ranks receive the bytes)."""
        buf = C.create_string_buffer(128)
        if self.lib.sse_rccl_get_unique_id(buf) != 0:
            raise SSEError("RCCL (librccl.so.1) is not loadable in this process")
        return buf.raw

    def rccl_library_path(self):
        """The ONE RCCL instance the library bound ($SSE_RCCL_LIB, else one already mapped into the process, else
        librccl.so.1); None when no RCCL is loadable.  Communicators must come from this instance."""
        p = self.lib.sse_rccl_library_path()
        return p.decode() if p else None

    def rccl_group_start(self):
        if self.lib.sse_rccl_group_start() != 0:
            raise SSEError("ncclGroupStart failed (or RCCL is not loadable in this process)")

    def rccl_group_end(self):
        if self.lib.sse_rccl_group_end() != 0:
            raise SSEError("ncclGroupEnd failed (or RCCL is not loadable in this process)")

    def rccl_comm_init_rank(self, world, rank, unique_id):
        """ncclCommInitRank on the handle's device; returns the communicator as an integer handle (void*)."""
        comm = _P()
        self.check(self.lib.sse_rccl_comm_init_rank(self._h, C.byref(comm), int(world), int(rank), C.c_char_p(bytes(unique_id))))
        return comm.value

    def rccl_comm_destroy(self, comm):
        self.check(self.lib.sse_rccl_comm_destroy(self._h, comm))

    def allgather_merge_topk_dev(self, comm, world, loc_s, loc_i, Q, k, out_s, out_i, stream=0):
        self.check(self.lib.sse_allgather_merge_topk_dev(self._h, comm, int(world), loc_s, loc_i, Q, k, out_s, out_i, stream))

    def score_topk_sharded_dev(self, comm, world, q_ptr, Q, k, out_s, out_i, stream=0):
        self.check(self.lib.sse_score_topk_sharded_dev(self._h, comm, int(world), q_ptr, Q, k, out_s, out_i, stream))

    # -- training ------------------------------------------------------------
    @staticmethod
    def _train_batch(src_ids, tgt_ids, labels):
        """src [B,T] int32; tgt [B,T] token ids -- or, for source_only_cnn, [B] rows of the free target matrix
        (the library checks which one the network mode wants); labels float32 [B]."""
        s = np.ascontiguousarray(src_ids, dtype=np.int32)
        t = np.ascontiguousarray(tgt_ids, dtype=np.int32)
        z = np.ascontiguousarray(labels, dtype=np.float32)
        if t.ndim == 2 and t.shape[1] == 1 and s.ndim == 2 and s.shape[1] != 1:
            t = np.ascontiguousarray(t[:, 0])
        if s.ndim != 2 or z.shape != (s.shape[0],) or not (t.shape == s.shape or t.shape == (s.shape[0],)):
            raise ValueError("train batch shapes: src [B,T], tgt [B,T] (or [B] target rows), labels [B]")
        return s, t, z

    def _check_tgt_kind(self, t):
        table = self.cfg.network_mode in (2, 3)                    # source-encoder-only, source_only_cnn
        if table != (t.ndim == 1):
            raise ValueError("source-encoder-only / source_only_cnn train on [B] target-matrix rows, "
                             "dual- and shared-encoder on [B,T] target token ids")

    def embedding_slice(self):
        """(offset, V, E) of the dense word_embedding gradient inside the gradient arena (variable 0 comes first)."""
        return 0, int(self.cfg.vocab_size), int(self.cfg.embedding_size)

    @property
    def max_seq_length(self):
        return int(self.cfg.max_seq_length)

    def set_stream(self, stream=0):
        """The stream (hipStream_t as int; 0 = null stream) the train-step entry points enqueue on."""
        self.check(self.lib.sse_set_stream(self._h, C.c_void_p(stream) if stream else None))
        self._stream = int(stream or 0)

    def train_step(self, src_ids, tgt_ids, labels):
        s, t, z = self._train_batch(src_ids, tgt_ids, labels)
        self._check_tgt_kind(t)
        loss, acc = C.c_float(), C.c_float()
        self.check(self.lib.sse_train_step(self._h, _ptr(s), _ptr(t), _ptr(z), s.shape[0], s.shape[1],
                                           C.byref(loss), C.byref(acc)))
        return float(loss.value), float(acc.value)

    # ---- batches by row number: corpora resident on the device
    def corpus_upload(self, side, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim != 2:
            raise ValueError("corpus must be [N,T]")
        self.check(self.lib.sse_corpus_upload(self._h, int(side), _ptr(ids), ids.shape[0], ids.shape[1]))

    def _rows_batch(self, src_rows, tgt_rows, labels):
        s = np.ascontiguousarray(src_rows, dtype=np.int32).reshape(-1)
        t = np.ascontiguousarray(tgt_rows, dtype=np.int32).reshape(-1)
        z = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
        if not (s.shape == t.shape == z.shape):
            raise ValueError("src_rows, tgt_rows, labels must all be [B]")
        return s, t, z

    def train_step_rows(self, src_rows, tgt_rows, labels):
        s, t, z = self._rows_batch(src_rows, tgt_rows, labels)
        loss, acc = C.c_float(), C.c_float()
        self.check(self.lib.sse_train_step_rows(self._h, _ptr(s), _ptr(t), _ptr(z), s.shape[0], C.byref(loss), C.byref(acc)))
        return float(loss.value), float(acc.value)

    def train_grads_rows(self, src_rows, tgt_rows, labels, rows_global):
        s, t, z = self._rows_batch(src_rows, tgt_rows, labels)
        self.check(self.lib.sse_train_grads_rows(self._h, _ptr(s), _ptr(t), _ptr(z), s.shape[0], int(rows_global)))

    # ---- data-parallel split of the train step: grads -> all-reduce(arena) -> apply
    def train_grad_count(self):
        n = C.c_int64()
        self.check(self.lib.sse_train_grad_count(self._h, C.byref(n)))
        return int(n.value)

    def train_set_grad_arena(self, dev_ptr, count):
        """Hand the library a caller-owned float32 device buffer (e.g. tensor.data_ptr()) of train_grad_count()
        floats for the gradients; dev_ptr=None returns to a library-owned one.  The caller keeps it alive."""
        self.check(self.lib.sse_train_set_grad_arena(self._h, C.c_void_p(dev_ptr) if dev_ptr else None, int(count)))

    def train_bind_arena(self, tensor):
        """tensor: contiguous float32 CUDA tensor of train_grad_count() elements on the handle's device."""
        if not tensor.is_cuda or not tensor.is_contiguous() or str(tensor.dtype) != "torch.float32":
            raise ValueError("gradient arena must be a contiguous float32 CUDA tensor")
        self._arena = tensor                                       # keep it alive
        self.train_set_grad_arena(tensor.data_ptr(), tensor.numel())

    def train_grads(self, src_ids, tgt_ids, labels, rows_global=None):
        s, t, z = self._train_batch(src_ids, tgt_ids, labels)
        self._check_tgt_kind(t)
        self.check(self.lib.sse_train_grads(self._h, _ptr(s), _ptr(t), _ptr(z), s.shape[0], s.shape[1],
                                            int(rows_global if rows_global is not None else s.shape[0])))

    def train_apply(self):
        loss, acc = C.c_float(), C.c_float()
        self.check(self.lib.sse_train_apply(self._h, C.byref(loss), C.byref(acc)))
        return float(loss.value), float(acc.value)

    # ---- the open train step: forward -> (the caller's objective over the raw encodings) -> backward -> [exchange] -> apply
    def train_forward(self, src_ids, tgt_ids, labels, rows_global=None):
        """sse_train_forward: the forward half of train_grads; the step stays open for ONE closing call (train_backward,
        train_backward_inbatch_global).  The options train_loss / train_class_loss are not consulted."""
        s, t, z = self._train_batch(src_ids, tgt_ids, labels)
        self._check_tgt_kind(t)
        self.check(self.lib.sse_train_forward(self._h, _ptr(s), _ptr(t), _ptr(z), s.shape[0], s.shape[1],
                                              int(rows_global if rows_global is not None else s.shape[0])))

    def train_forward_rows(self, src_rows, tgt_rows, labels, rows_global=None):
        s, t, z = self._rows_batch(src_rows, tgt_rows, labels)
        self.check(self.lib.sse_train_forward_rows(self._h, _ptr(s), _ptr(t), _ptr(z), s.shape[0],
                                                   int(rows_global if rows_global is not None else s.shape[0])))

    def train_open_encodings(self, side, out, stream=0):
        """The un-normalised encodings [B][S] of the open step (side 0 source, 1 target; table modes: the gathered rows of
        the free target matrix) into `out`, a contiguous float32 CUDA tensor; queued on `stream`."""
        self.check(self.lib.sse_train_open_encodings_dev(self._h, int(side), C.c_void_p(out.data_ptr()), stream))

    def train_backward(self, d_src, d_tgt, loss_part=0.0, acc_part=0.0):
        """Closes the open step with the caller's gradients [B][S] of the GLOBAL mean objective with respect to this rank's
        un-normalised encodings (float32 CUDA tensors); loss_part / acc_part: this rank's share of the global loss and
        accuracy, summed over the ranks by the arena's all-reduce.  train_apply follows as after train_grads."""
        self.check(self.lib.sse_train_backward_dev(self._h, C.c_void_p(d_src.data_ptr()), C.c_void_p(d_tgt.data_ptr()),
                                                   float(loss_part), float(acc_part)))

    def train_exchange_floats(self, cap, T=None):
        return int(self.lib.sse_train_exchange_floats(self._h, int(cap), int(T if T is not None else self.cfg.max_seq_length)))

    def train_pack_exchange(self, cap, block):
        """block: contiguous float32 CUDA tensor of train_exchange_floats(cap, T) elements; the open step's rows for one all-gather."""
        self.check(self.lib.sse_train_pack_exchange(self._h, int(cap), C.c_void_p(block.data_ptr())))

    def train_backward_inbatch_global(self, gathered, world, cap, rank, rank_rows):
        """Closes the open step with the in-batch softmax loss over the GLOBAL batch: gathered = the `world` exchange blocks
        back to back (float32 CUDA), rank_rows = the ranks' row counts (host)."""
        rr = np.ascontiguousarray(rank_rows, dtype=np.int32).reshape(-1)
        if rr.size < int(world):                    # (the library reads `world` entries; it refuses every other mismatch itself)
            raise ValueError("rank_rows must hold one row count per rank")
        self.check(self.lib.sse_train_backward_inbatch_global(self._h, C.c_void_p(gathered.data_ptr()), int(world), int(cap),
                                                              int(rank), _ptr(rr)))

    # ---- forward-only loss / accuracy / cosines of held-out pairs (sse_eval_loss*): no update, inference kernels
    def _eval_call(self, by_rows, src, tgt, labels, want_cos):
        if by_rows:
            s, t, z = self._rows_batch(src, tgt, labels)
        else:
            s, t, z = self._train_batch(src, tgt, labels)
            self._check_tgt_kind(t)
        B = s.shape[0]
        sums = (C.c_double * 3)()
        cos = np.empty(B, np.float32) if want_cos else None
        if by_rows:
            self.check(self.lib.sse_eval_loss_rows(self._h, _ptr(s), _ptr(t), _ptr(z), B, sums, _ptr(cos) if want_cos else None))
        else:
            self.check(self.lib.sse_eval_loss(self._h, _ptr(s), _ptr(t), _ptr(z), B, s.shape[1], sums, _ptr(cos) if want_cos else None))
        return (float(sums[0]), float(sums[1]), float(sums[2])), cos

    @staticmethod
    def _eval_result(sums, cos, return_cos):
        n = sums[2] if sums[2] else 1.0
        loss, acc = np.float32(sums[0] / n), np.float32(sums[1] / n)
        return (loss, acc, cos) if return_cos else (loss, acc)

    def eval_loss_sums(self, src_ids, tgt_ids, labels):
        """(sum of the row losses, sum of the row accuracies, rows) as float64: what ranks or slices of a held-out set add."""
        return self._eval_call(False, src_ids, tgt_ids, labels, False)[0]

    def eval_loss_rows_sums(self, src_rows, tgt_rows, labels):
        return self._eval_call(True, src_rows, tgt_rows, labels, False)[0]

    def eval_loss(self, src_ids, tgt_ids, labels, return_cos=False):
        """Loss and binary accuracy of a batch of pairs as the train step reports them, WITHOUT the step: (np.float32 loss,
        np.float32 acc), with return_cos also the cosine of every pair row (float32 [B]; the logit is 64 cos)."""
        sums, cos = self._eval_call(False, src_ids, tgt_ids, labels, return_cos)
        return self._eval_result(sums, cos, return_cos)

    def eval_loss_rows(self, src_rows, tgt_rows, labels, return_cos=False):
        """eval_loss by row numbers into the corpora of corpus_upload (tgt: rows of the free target matrix in the modes
        that have one)."""
        sums, cos = self._eval_call(True, src_rows, tgt_rows, labels, return_cos)
        return self._eval_result(sums, cos, return_cos)

    # ---- (row id, gradient row) exchange of the word-embedding gradient (data_parallel.py)
    def dp_packed_floats(self, cap):
        return int(self.lib.sse_train_packed_embedding_floats(self._h, int(cap)))

    def dp_pack_embedding(self, cap, packed):
        """packed: contiguous float32 CUDA tensor of dp_packed_floats(cap) elements."""
        self.check(self.lib.sse_train_pack_embedding_grad(self._h, int(cap), C.c_void_p(packed.data_ptr())))

    def dp_unpack_embedding(self, gathered, world, cap):
        """gathered: the `world` packed buffers back to back (all_gather_into_tensor), float32 CUDA."""
        self.check(self.lib.sse_train_unpack_embedding_grad(self._h, C.c_void_p(gathered.data_ptr()), int(world), int(cap)))

    @property
    def learning_rate(self):
        v = C.c_float()
        self.check(self.lib.sse_get_learning_rate(self._h, C.byref(v)))
        return float(v.value)

    @learning_rate.setter
    def learning_rate(self, lr):
        self.check(self.lib.sse_set_learning_rate(self._h, float(lr)))

    def decay_learning_rate(self):
        self.check(self.lib.sse_decay_learning_rate(self._h))

    @property
    def global_step(self):
        v = C.c_int64()
        self.check(self.lib.sse_get_global_step(self._h, C.byref(v)))
        return int(v.value)

    @global_step.setter
    def global_step(self, step):
        self.check(self.lib.sse_set_global_step(self._h, int(step)))

    # -- timing --------------------------------------------------------------
    def timer_record(self, slot, stream=0):
        self.check(self.lib.sse_timer_record(self._h, slot, stream))

    def timer_elapsed_ms(self, a, b):
        v = C.c_float()
        self.check(self.lib.sse_timer_elapsed_ms(self._h, a, b, C.byref(v)))
        return float(v.value)

    def synchronize(self):
        self.check(self.lib.sse_synchronize(self._h))
