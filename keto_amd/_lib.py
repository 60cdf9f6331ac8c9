"""ctypes binding of libketogpu.so (include/ketogpu.h).  Fails loudly when the HIP library is
missing -- there is no CPU fallback on the product path."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# KG_LIB_PATH: another build of the same library (A/B runs of bench.py on one box)
LIB_PATH = os.environ.get("KG_LIB_PATH") or os.path.join(HERE, "lib", "libketogpu.so")

KG_SUBJECT_ID = 0xFFFFFFFF
KG_NOT_MEMBER, KG_IS_MEMBER, KG_ERROR = 0, 1, 2
KG_FREC_HIT = 0xFFFFFFFF
KG_FREC_ERR = 0xFFFFFFFE
KG_SHARD_MAX_RANKS = 64
KG_ERR_NONE, KG_ERR_RELATION_NOT_FOUND, KG_ERR_NOT_IMPLEMENTED, KG_ERR_REWRITE_CYCLE, KG_ERR_RESOURCE = 0, 1, 2, 3, 4


KG_PACK_ID_MAX = 4094
KG_PACK_SUBJECT_ID = 4095


def pack_queries(q: "np.ndarray") -> "np.ndarray":
    """kg_pack_query (include/ketogpu.h) over an (n, 7) uint32 kg_query array: (n, 4) uint32 kg_query_packed
    rows.  Raises ValueError when an id does not fit (namespace / relation ids <= KG_PACK_ID_MAX)."""
    import numpy as np
    q = np.ascontiguousarray(q, dtype=np.uint32).reshape(-1, 7)
    sid = q[:, 3] == 0xFFFFFFFF
    sns = np.where(sid, KG_PACK_SUBJECT_ID, q[:, 3]).astype(np.uint64)
    srel = np.where(sid, 0, q[:, 5]).astype(np.uint64)
    d = q[:, 6].view(np.int32).astype(np.int64)
    d = np.clip(d, 0, 65535).astype(np.uint64)
    if (q[:, 0] > KG_PACK_ID_MAX).any() or (q[:, 2] > KG_PACK_ID_MAX).any() or \
            ((sns > KG_PACK_ID_MAX) & ~sid).any() or (srel > KG_PACK_ID_MAX).any():
        raise ValueError("an id does not fit kg_query_packed (use kg_check_batch)")
    out = np.empty((len(q), 4), np.uint32)
    out[:, 0] = q[:, 1]
    out[:, 1] = q[:, 4]
    out[:, 2] = (q[:, 0].astype(np.uint64) | (q[:, 2].astype(np.uint64) << 12) | ((sns & 0xFF) << 24)).astype(np.uint32)
    out[:, 3] = ((sns >> 8) | (srel << 4) | (d << 16)).astype(np.uint32)
    return out


class kg_tuple(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("ns", "obj", "rel", "sns", "sobj", "srel")]


class kg_query(C.Structure):
    _fields_ = [("t", kg_tuple), ("max_depth", C.c_int32)]


class kg_set(C.Structure):
    _fields_ = [("sns", C.c_uint32), ("sobj", C.c_uint32), ("srel", C.c_uint32), ("max_depth", C.c_int32)]


class kg_dict(C.Structure):
    _fields_ = [("n_namespaces", C.c_uint32), ("n_relations", C.c_uint32), ("wildcard_rel", C.c_uint32)]


class kg_rw_node(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "rel", "crel", "first", "count")]


class kg_rewrite_prog(C.Structure):
    _fields_ = [("n_ns", C.c_uint32), ("ns_has_rel", C.c_void_p), ("n_rel", C.c_uint32), ("rel_ns", C.c_void_p),
                ("rel_rel", C.c_void_p), ("rel_root", C.c_void_p), ("n_rw", C.c_uint32), ("rw", C.c_void_p),
                ("n_child", C.c_uint32), ("child", C.c_void_p)]


class kg_stats(C.Structure):
    _fields_ = [("rows_opened", C.c_uint64), ("edges_read", C.c_uint64), ("direct_probes", C.c_uint64),
                ("frontier_hbm", C.c_uint64), ("n_light", C.c_uint64), ("n_heavy", C.c_uint64),
                ("n_general", C.c_uint64), ("n_medium", C.c_uint64), ("light_rows_opened", C.c_uint64), ("light_edges_read", C.c_uint64),
                ("light_probes", C.c_uint64), ("kernel_ms", C.c_double), ("light_ms", C.c_double),
                ("n_wide", C.c_uint64), ("n_grid", C.c_uint64),
                ("n_back", C.c_uint64), ("n_no_holder", C.c_uint64), ("back_rows", C.c_uint64),
                ("back_edges", C.c_uint64), ("light_steps", C.c_uint64), ("light_waves", C.c_uint64),
                ("light_wave_ticks", C.c_uint64),
                ("light_span_ticks", C.c_uint64), ("light_wave_max_ticks", C.c_uint64),
                ("tail_ms", C.c_double), ("tail_launches", C.c_uint64), ("tail_kind", C.c_uint64),
                ("tail_rows", C.c_uint64), ("tail_edges", C.c_uint64), ("tail_probes", C.c_uint64),
                ("tail_logged", C.c_uint64), ("ms_edges_loaded", C.c_uint64), ("ms_words_active", C.c_uint64),
                ("split_ms", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class kg_tree_node(C.Structure):
    _fields_ = [("type", C.c_uint8), ("is_set", C.c_uint8), ("pad", C.c_uint16), ("ns", C.c_uint32),
                ("obj", C.c_uint32), ("rel", C.c_uint32), ("n_children", C.c_uint32)]


class kg_tree_buf(C.Structure):
    _fields_ = [("nodes", C.POINTER(kg_tree_node)), ("n_nodes", C.c_uint64), ("root_off", C.POINTER(C.c_uint64)),
                ("n_roots", C.c_uint64), ("kernel_ms", C.c_double), ("pinned", C.c_uint64)]


class kg_lookup_buf(C.Structure):
    _fields_ = [("req_off", C.POINTER(C.c_uint64)), ("objs", C.POINTER(C.c_uint32)),
                ("err_code", C.POINTER(C.c_uint32)), ("n_errors", C.POINTER(C.c_uint64)),
                ("n_reqs", C.c_uint64), ("n_objs", C.c_uint64), ("exact", C.c_uint64), ("candidates", C.c_uint64),
                ("confirmed", C.c_uint64), ("reverse_edges", C.c_uint64), ("levels", C.c_uint64),
                ("kernel_ms", C.c_double), ("pinned", C.c_uint64)]


KG_LOOKUP_END = 0xFFFFFFFF


class kg_lookup_page(C.Structure):
    _fields_ = [("from_", C.c_uint32), ("limit", C.c_uint32)]


class kg_lookup_pages(C.Structure):
    _fields_ = [("list", kg_lookup_buf), ("next", C.POINTER(C.c_uint32)), ("rounds", C.c_uint64),
                ("pinned", C.c_uint64)]


class kg_lookup_subj_set(C.Structure):
    """A kg_lookup_subject_sets request: list the subject sets sns:*#srel (sns = KG_SUBJECT_ID: subject ids)."""
    _fields_ = [("ns", C.c_uint32), ("obj", C.c_uint32), ("rel", C.c_uint32), ("sns", C.c_uint32),
                ("srel", C.c_uint32), ("max_depth", C.c_int32)]


class kg_lookup_mask_buf(C.Structure):
    """What a mask call returns on the host: per-request counts and error words, the unpaged call's counters."""
    _fields_ = [("n_set", C.POINTER(C.c_uint64)), ("n_errors", C.POINTER(C.c_uint64)),
                ("err_code", C.POINTER(C.c_uint32)), ("n_reqs", C.c_uint64), ("exact", C.c_uint64),
                ("candidates", C.c_uint64), ("confirmed", C.c_uint64), ("reverse_edges", C.c_uint64),
                ("levels", C.c_uint64), ("kernel_ms", C.c_double), ("pinned", C.c_uint64)]


KG_Q_NS, KG_Q_OBJ, KG_Q_REL, KG_Q_SUBJECT = 1, 2, 4, 8


class kg_row_query(C.Structure):
    _fields_ = [("mask", C.c_uint32), ("t", kg_tuple), ("after", C.c_uint64), ("limit", C.c_uint32)]


class kg_query_buf(C.Structure):
    _fields_ = [("req_off", C.POINTER(C.c_uint64)), ("rows", C.POINTER(kg_tuple)), ("keys", C.POINTER(C.c_uint64)),
                ("next", C.POINTER(C.c_uint64)), ("matched", C.POINTER(C.c_uint64)),
                ("n_reqs", C.c_uint64), ("n_rows", C.c_uint64), ("rows_scanned", C.c_uint64), ("passes", C.c_uint64),
                ("kernel_ms", C.c_double), ("pinned", C.c_uint64)]


KG_DELETE_MAX_QUERIES = 64
KG_DELETE_KEYS = 1


class kg_delete_buf(C.Structure):
    _fields_ = [("matched", C.POINTER(C.c_uint64)), ("keys", C.POINTER(C.c_uint64)), ("n_queries", C.c_uint64),
                ("n_deleted", C.c_uint64), ("rows_scanned", C.c_uint64), ("kernel_ms", C.c_double),
                ("pinned", C.c_uint64)]


# kg_row_query as a numpy record (48 B: the u64 is 8-aligned)
ROW_QUERY_DTYPE = np.dtype({"names": ["mask", "t", "after", "limit"],
                            "formats": ["<u4", ("<u4", (6,)), "<u8", "<u4"],
                            "offsets": [0, 4, 32, 40], "itemsize": 48})


class kg_synth_params(C.Structure):
    _fields_ = [("n_tuples_target", C.c_uint64), ("seed", C.c_uint64), ("n_layers", C.c_uint32),
                ("max_degree", C.c_uint32), ("set_fraction", C.c_float), ("doc_set_fraction", C.c_float),
                ("preset", C.c_uint32), ("doc_alpha", C.c_float), ("group_alpha", C.c_float)]


KG_SHARD_UNIQUE_ID_BYTES = 128
# kg_shard_transport callbacks (include/ketogpu.h): collective over the ranks, 0 = success
ALLTOALL2_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                           C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.c_void_p)


class kg_check_node(C.Structure):
    _fields_ = [("type", C.c_uint8), ("has_tuple", C.c_uint8), ("pad", C.c_uint16), ("n_children", C.c_uint32),
                ("t", kg_tuple)]


KG_CTREE = {1: "leaf", 2: "union", 3: "intersection", 4: "computed_subject_set", 5: "tuple_to_subject_set", 6: "not"}


class kg_shard_transport(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int32), ("world", C.c_int32), ("host_memory", C.c_int32),
                ("alltoall2", ALLTOALL2_FN), ("allgather", ALLGATHER_FN), ("allreduce_max_u64", ALLREDUCE_FN)]


class kg_batcher_stats_t(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("checks", C.c_uint64), ("batch_p50_ms", C.c_double),
                ("batch_p99_ms", C.c_double), ("call_p50_ms", C.c_double), ("call_p99_ms", C.c_double)]


def _bindings() -> dict:
    vp, sz, i32, u32, u64, i, P = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_uint64, C.c_int, C.POINTER
    return {
        "kg_version": (C.c_char_p, []),
        "kg_last_error": (sz, [C.c_char_p, sz]),
        "kg_snapshot_create": (i, [vp, sz, P(kg_dict), P(kg_rewrite_prog), i, P(vp)]),
        "kg_snapshot_create_on": (i, [vp, sz, P(kg_dict), P(kg_rewrite_prog), vp, i, P(vp)]),
        "kg_snapshot_create_ordered": (i, [vp, vp, sz, vp, vp, vp, i, vp]),
        "kg_snapshot_apply": (i, [vp, vp, vp, sz, vp, sz, vp, vp, vp]),
        "kg_snapshot_delete_matching": (i, [vp, vp, sz, u32, vp, vp, P(vp), P(kg_delete_buf)]),
        "kg_delete_free": (None, [P(kg_delete_buf)]),
        "kg_snapshot_synthetic": (i, [P(kg_synth_params), P(kg_rewrite_prog), i, P(vp)]),
        "kg_snapshot_synthetic_on": (i, [P(kg_synth_params), P(kg_rewrite_prog), vp, i, P(vp)]),
        "kg_snapshot_replicas": (i, [vp, vp, i]),
        "kg_snapshot_destroy": (None, [vp]),
        "kg_snapshot_info": (i, [vp, vp]),
        "kg_snapshot_materialized": (i, [vp, vp]),
        "kg_snapshot_tune": (i, [vp, C.c_char_p, C.c_int64]),
        "kg_snapshot_holder_sig": (i, [vp]),
        "kg_synth_ids": (i, [vp, vp]),
        "kg_snapshot_export": (C.c_int64, [vp, vp, u64]),
        "kg_snapshot_rows": (C.c_int64, [vp, vp, sz, vp, vp, u64]),
        "kg_snapshot_export_csr": (i, [vp, vp, vp, vp, vp, vp]),
        "kg_check_batch": (i, [vp, vp, sz, i32, vp, vp, P(kg_stats)]),
        "kg_check_batch_packed": (i, [vp, vp, sz, i32, vp, vp, vp, sz, P(sz), P(kg_stats)]),
        "kg_check_batch_device": (i, [vp, vp, sz, i32, vp, vp, P(kg_stats), vp]),
        "kg_check_batch_packed_device": (i, [vp, vp, sz, i32, vp, vp, P(kg_stats), vp]),
        "kg_pack_queries_device": (i, [vp, vp, sz, vp, vp]),
        "kg_synth_queries": (i, [vp, u64, sz, vp]),
        "kg_check_tree": (i, [vp, vp, i32, vp, sz, vp, sz, P(sz), P(C.c_uint8), P(u32)]),
        "kg_expand_batch": (i, [vp, vp, sz, i32, P(kg_tree_buf)]),
        "kg_expand_batch_device": (i, [vp, vp, sz, i32, P(kg_tree_buf), vp]),
        "kg_tree_free": (None, [P(kg_tree_buf)]),
        "kg_lookup_objects": (i, [vp, vp, sz, i32, P(kg_lookup_buf)]),
        "kg_lookup_subjects": (i, [vp, vp, sz, i32, P(kg_lookup_buf)]),
        "kg_lookup_subject_sets": (i, [vp, vp, sz, i32, P(kg_lookup_buf)]),
        "kg_lookup_free": (None, [P(kg_lookup_buf)]),
        "kg_lookup_objects_page": (i, [vp, vp, vp, sz, i32, P(kg_lookup_pages)]),
        "kg_lookup_subjects_page": (i, [vp, vp, vp, sz, i32, P(kg_lookup_pages)]),
        "kg_lookup_subject_sets_page": (i, [vp, vp, vp, sz, i32, P(kg_lookup_pages)]),
        "kg_lookup_pages_free": (None, [P(kg_lookup_pages)]),
        "kg_lookup_objects_mask_device": (i, [vp, vp, sz, i32, u32, u32, vp, sz, P(kg_lookup_mask_buf), vp]),
        "kg_lookup_subject_sets_mask_device": (i, [vp, vp, sz, i32, u32, u32, vp, sz, P(kg_lookup_mask_buf), vp]),
        "kg_lookup_mask_free": (None, [P(kg_lookup_mask_buf)]),
        "kg_mask_select_device": (i, [vp, vp, sz, u32, u32, vp, sz, u32, u32, vp, vp, vp]),
        "kg_snapshot_query": (i, [vp, vp, sz, P(kg_query_buf)]),
        "kg_query_free": (None, [P(kg_query_buf)]),
        "kg_batcher_create": (i, [vp, i32, sz, u32, i, P(vp)]),
        "kg_batcher_check": (i, [vp, vp, sz, vp, vp]),
        "kg_batcher_stats": (i, [vp, P(kg_batcher_stats_t)]),
        "kg_batcher_reset_stats": (None, [vp]),
        "kg_batcher_destroy": (None, [vp]),
        "kg_shard_owner": (u32, [u32, u32, u32]),
        "kg_snapshot_create_shard": (i, [vp, sz, P(kg_dict), P(kg_rewrite_prog), i, u32, u32, P(vp)]),
        "kg_snapshot_synthetic_shard": (i, [P(kg_synth_params), P(kg_rewrite_prog), i, u32, u32, P(vp)]),
        "kg_shard_seed": (i, [vp, vp, sz, i32, vp, sz, vp, vp, vp, vp]),
        "kg_shard_level": (i, [vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, u32, vp]),
        "kg_shard_level_seg": (i, [vp, vp, u32, sz, vp, vp, sz, vp, vp, vp, vp, u32, vp]),
        "kg_shard_levels": (i, [vp, i32, vp, vp, sz, vp, vp, i32, vp, vp, sz, i32, P(i32), vp]),
        "kg_shard_done": (i, [vp, sz, vp, vp, i, vp, u32, vp]),
        "kg_shard_back_list": (i, [vp, sz, vp, vp, vp, sz, vp, vp]),
        "kg_shard_back_seed": (i, [vp, vp, sz, vp, vp, sz, vp, vp]),
        "kg_shard_back_level": (i, [vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, u32, vp]),
        "kg_shard_refwd_seed": (i, [vp, sz, vp, vp, vp, sz, vp, vp]),
        "kg_shard_held_words": (i, [vp, vp]),
        "kg_shard_held": (i, [vp, vp, sz, i, vp]),
        "kg_shard_finish": (i, [vp, sz, vp, vp, vp]),
        "kg_shard_result_slots": (sz, [vp, sz]),
        "kg_shard_bad_nodes": (i, [vp, vp]),
        "kg_shard_unique_id": (i, [vp]),
        "kg_shard_comm_init": (i, [vp, vp, i, i, vp]),
        "kg_shard_transport_attach": (i, [vp, P(kg_shard_transport), vp]),
        "kg_shard_comm_release": (i, [vp, vp]),
        "kg_shard_comm_stats": (i, [vp, vp, vp]),
        "kg_shard_comm_stats_ex": (i, [vp, vp, vp, sz]),
        "kg_shard_comm_levels": (C.c_int64, [vp, vp, vp, sz]),
    }


# every symbol include/ketogpu.h declares: name -> (restype, argtypes)
BINDINGS = _bindings()
EXPORTS = list(BINDINGS)


class KetoGPUError(RuntimeError):
    pass


_lib = None


def load(path: str = LIB_PATH):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise KetoGPUError(f"libketogpu.so not found at {path}: build it with `python -m keto_amd.build` "
                           "(there is no CPU fallback)")
    L = C.CDLL(path)
    own = path == os.path.join(HERE, "lib", "libketogpu.so")
    for name, (restype, argtypes) in BINDINGS.items():
        if not hasattr(L, name):
            if own:
                raise KetoGPUError(f"{path} does not export {name}: rebuild it with `python -m keto_amd.build --force`")
            continue  # an older A/B build loaded through KG_LIB_PATH goes without the calls added since
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


_hip = None


def device_to_host(dst: np.ndarray, src, nbytes: int) -> None:
    """hipMemcpy of nbytes from a device pointer the library returned (kg_expand_batch_device trees)
    into a host array: test and bench plumbing."""
    global _hip
    if nbytes == 0:
        return
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    assert dst.nbytes >= nbytes
    rc = _hip.hipMemcpy(dst.ctypes.data_as(C.c_void_p), C.cast(src, C.c_void_p), nbytes, 2)  # hipMemcpyDeviceToHost
    if rc != 0:
        raise KetoGPUError(f"hipMemcpy device->host failed ({rc})")


def last_error() -> str:
    buf = C.create_string_buffer(2048)
    load().kg_last_error(buf, 2048)
    return buf.value.decode(errors="replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise KetoGPUError(f"{what} failed ({rc}): {last_error()}")
