"""ctypes binding of the C ABI in include/rdst_hip.h.

The shared library is built in-tree (``rdst_amd/librdst_hip.so``) by
``__graft_entry__.build()`` / ``make -C rdst_amd/csrc``.  There is no CPU fallback: if the
library is missing or a call fails, the caller gets an exception.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RDST_HIP_LIB: another build of the same library (tools/ A/B runs only; tests and bench use the in-tree one)
LIB_PATH = os.environ.get("RDST_HIP_LIB") or os.path.join(_HERE, "librdst_hip.so")

RDST_KEY_UNSIGNED, RDST_KEY_SIGNED, RDST_KEY_FLOAT, RDST_KEY_BYTES_BE = 0, 1, 2, 3
RDST_OK = 0
RDST_BYTES_MAX_N = 4096  # longest [u8; N] key the device route takes (include/rdst_hip.h)
RDST_BYTES_NOWAIT_MAX_N = 128  # longest key the nowait [u8; N] and described-key entries take
RDST_FIELD_DESCENDING = 1  # rdst_key_field.flags: complement the field's mapped bytes
RDST_KEY_FIELDS_MAX = 16   # fields in one key description
RDST_STAGE_SEGMENTS = 13   # rdst_stage: the batched launches of the segmented sort
RDST_STAGE_SEGMENTS_TILED = 14   # rdst_stage: the tiled route of the nowait entries (segments beyond block_max)
RDST_STAGE_TOPK = 15       # rdst_stage: one select level of the partial sort (level in bits 8..15; 0xFF: the collection pass)
RDST_STAGE_SELECT = 16     # rdst_stage: one level of one round of the order statistics (level in bits 8..15; 0xFF: the collection pass)
RDST_TOPK_LARGEST = 1      # rdst_hip_topk_device flags: the k largest, in descending order
RDST_RUNS_PAD_STARTS = 1   # rdst_hip_runs_device flags: fill the starts behind slot R with m, up to the capacity
RDST_RANK_LOWER, RDST_RANK_HIGHER, RDST_RANK_NEAREST = 0, 1, 2   # rdst_rank_spec.mode: how a quantile's virtual index is rounded


class TuningParamsC(ctypes.Structure):
    _fields_ = [
        ("threads", ctypes.c_uint64),
        ("level", ctypes.c_uint64),
        ("total_levels", ctypes.c_uint64),
        ("input_len", ctypes.c_uint64),
        ("parent_len", ctypes.c_int64),
    ]


class HipOptsC(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("low_memory", ctypes.c_int32), ("reserved1", ctypes.c_uint64)]


class KeyFieldC(ctypes.Structure):
    """rdst_key_field: one field of a described key (offset, bytes, kind, flags)."""
    _fields_ = [("offset", ctypes.c_uint32), ("bytes", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class SegmentItemC(ctypes.Structure):
    """rdst_segment_item: one entry of the segmented sort's work list (start, len, segment index)."""
    _fields_ = [("start", ctypes.c_uint64), ("len", ctypes.c_uint32), ("seg", ctypes.c_uint32)]


class RankSpecC(ctypes.Structure):
    """rdst_rank_spec: an absolute rank (den == 0) or the quantile num / den rounded by mode, resolved per segment"""
    _fields_ = [("num", ctypes.c_uint32), ("den", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class RdstHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rdst_hip call failed with status {code}: {msg}")
        self.code = code


def _signatures():
    vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    u64p, u32p, u8p, f32p = ctypes.POINTER(u64), ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_float)
    opts, kfp, items, specs = ctypes.POINTER(HipOptsC), ctypes.POINTER(KeyFieldC), ctypes.POINTER(SegmentItemC), ctypes.POINTER(RankSpecC)
    return {
        "rdst_hip_sort": (ci, [vp, u64, u32, ci, u32, opts]),
        "rdst_hip_sort_device": (ci, [vp, vp, u64, u32, ci, u32, vp]),
        "rdst_hip_sort_device_lowmem": (ci, [vp, u64, u32, ci, u32, vp, u64, vp]),
        "rdst_hip_partition_device": (ci, [vp, u64, u32, ci, u32, u32, vp, u64, u64p, vp]),
        "rdst_regions_plan": (ci, None),
        "rdst_hip_host_timing": (ci, [f32p, f32p, f32p]),
        "rdst_hip_sort_pairs_device": (ci, [vp, vp, vp, vp, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_sort_device_devlen": (ci, [vp, vp, u64, vp, u32, u32, ci, u32, vp]),
        "rdst_hip_sort_pairs_device_devlen": (ci, [vp, vp, vp, vp, u64, vp, u32, u32, ci, u32, u32, vp]),
        "rdst_hip_topk_device": (ci, [vp, u64, u64, vp, vp, u32, vp, u64, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_topk_scratch_bytes": (u64, [u64, u64, u32, u32, u64]),
        "rdst_hip_topk_limits": (ci, [u32, u32, u32p]),
        "rdst_hip_debug_topk_state": (ci, [vp, vp, u64p]),
        "rdst_hip_select_device": (ci, [vp, u64, u64p, u64, vp, vp, u32, vp, u64, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_select_scratch_bytes": (u64, [u64, u64, u32, u32, u64]),
        "rdst_hip_select_limits": (ci, [u32, u32, u32p]),
        "rdst_hip_debug_select_state": (ci, [vp, vp, u64p]),
        "rdst_hip_topk_segments_device": (ci, [vp, u64, u64p, u64, u64, vp, vp, u32, vp, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_topk_segments_scratch_bytes": (u64, [u64, u64, u64, u32, u32]),
        "rdst_hip_topk_segments_limits": (ci, [u32, u32, u32p]),
        "rdst_topk_segments_plan": (ci, [u64p, u64, u64, u64, u32, u32, items, u64, u64p, u64p]),
        "rdst_hip_set_topk_segments_stream_max": (ci, [u32]),
        "rdst_rank_for_length": (ci, [specs, u64, u64p]),
        "rdst_hip_select_segments_device": (ci, [vp, u64, u64p, u64, specs, u64, vp, vp, u32, vp, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_select_segments_scratch_bytes": (u64, [u64, u64, u64, u32, u32]),
        "rdst_hip_select_segments_limits": (ci, [u32, u32, u32p]),
        "rdst_hip_topk_segments_device_offsets": (ci, [vp, u64, vp, u32, u64, u64, vp, vp, u32, vp, u64, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_topk_segments_device_offsets_scratch_bytes": (u64, [u64, u64, u64, u32, u32]),
        "rdst_hip_debug_topk_segments_plan_device": (ci, [vp, u32, u64, u64, u64, u32, u32, u32, vp, u64, items, u64, u64p, u64p, u32p, vp]),
        "rdst_hip_select_segments_device_offsets": (ci, [vp, u64, vp, u32, u64, specs, u64, vp, vp, u32, vp, u64, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_select_segments_device_offsets_scratch_bytes": (u64, [u64, u64, u64, u32, u32]),
        "rdst_hip_runs_device": (ci, [vp, u64, vp, u32, vp, vp, vp, u32, u64, vp, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_runs_scratch_bytes": (u64, [u64, u32]),
        "rdst_hip_runs_limits": (ci, [u32, u32p]),
        "rdst_hip_search_device": (ci, [vp, u64, vp, u32, vp, u64, vp, vp, u32, vp, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_search_scratch_bytes": (u64, [u64, u64, u32]),
        "rdst_hip_search_limits": (ci, [u32, u32p]),
        "rdst_hip_debug_search_state": (ci, [vp, vp, u64p]),
        "rdst_hip_sort_segments_device": (ci, [vp, vp, u64, u64, u64p, u64, u32, ci, u32, vp]),
        "rdst_hip_sort_segments_pairs_device": (ci, [vp, vp, vp, vp, u64, u64, u64p, u64, u32, ci, u32, u32, vp]),
        "rdst_hip_sort_segments_limits": (ci, [u32, u32, u32p]),
        "rdst_segments_plan": (ci, [u64p, u64, u64, u32, u32, items, u64, u64p, u64p]),
        "rdst_hip_sort_segments_device_offsets": (ci, [vp, vp, u64, u64, vp, u32, u64, u32, ci, u32, vp, u64, vp]),
        "rdst_hip_sort_segments_pairs_device_offsets": (ci, [vp, vp, vp, vp, u64, u64, vp, u32, u64, u32, ci, u32, u32, vp, u64, vp]),
        "rdst_hip_sort_segments_device_offsets_scratch_bytes": (u64, [u64]),
        "rdst_hip_sort_segments_device_offsets_nowait": (ci, [vp, vp, u64, vp, u32, u64, u32, ci, u32, vp, u64, vp]),
        "rdst_hip_sort_segments_pairs_device_offsets_nowait": (ci, [vp, vp, vp, vp, u64, vp, u32, u64, u32, ci, u32, u32, vp, u64, vp]),
        "rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes": (u64, [u64, u64, u32, u32]),
        "rdst_hip_debug_segments_plan_device": (ci, [vp, u32, u64, u64, u32, u32, vp, u64, items, u64, u64p, u64p, u32p, vp]),
        "rdst_hip_sort_records": (ci, [vp, u64, u32, u32, u32, ci, opts]),
        "rdst_hip_sort_bytes_device": (ci, [vp, u64, u32, vp, u64, vp]),
        "rdst_hip_sort_bytes_scratch_bytes": (u64, [u64, u32]),
        "rdst_hip_sort_bytes_device_nowait": (ci, [vp, u64, u32, vp, u64, vp]),
        "rdst_hip_sort_records_by_fields": (ci, [vp, u64, u32, kfp, u32, opts]),
        "rdst_hip_sort_records_by_fields_device": (ci, [vp, u64, u32, kfp, u32, vp, u64, vp]),
        "rdst_hip_sort_records_by_fields_scratch_bytes": (u64, [u64, u32, kfp, u32]),
        "rdst_hip_sort_records_by_fields_device_nowait": (ci, [vp, u64, u32, kfp, u32, vp, u64, vp]),
        "rdst_hip_pack_fields_device": (ci, [vp, u64, u32, kfp, u32, vp, vp, vp]),
        "rdst_hip_device_status": (ci, [vp]),
        "rdst_hip_level_counts": (ci, [vp, u64, u32, ci, u32, u64p, u8p, u8p, u8p, vp]),
        "rdst_hip_all_level_counts": (ci, [vp, u64, u32, ci, u32, u64p, vp]),
        "rdst_hip_scatter_level": (ci, [vp, vp, u64, u32, ci, u32, u64p, vp]),
        "rdst_hip_split_top_level_device": (ci, [vp, vp, u64, u32, ci, vp, vp]),
        "rdst_hip_split_top16_device": (ci, [vp, vp, u64, u32, ci, vp, vp]),
        "rdst_pick_algorithm": (ci, [ci, ctypes.POINTER(TuningParamsC), u64p, u64]),
        "rdst_hip_workspace_bytes": (u64, [u64, u32]),
        "rdst_hip_release_workspace": (ci, []),
        "rdst_hip_set_tuning": (ci, [ci, ci]),
        "rdst_hip_set_chain_split": (ci, [ci]),
        "rdst_hip_set_fast_rank": (ci, [ci]),
        "rdst_hip_set_small_sort": (ci, [ci]),
        "rdst_hip_set_profiling": (ci, [ci]),
        "rdst_hip_profile_runs": (ci, None),
        "rdst_hip_profile_run": (ci, [ci, f32p, u32, u32p]),
        "rdst_hip_profile_run_stages": (ci, [ci, u32p, u32, u32p]),
        "rdst_hip_set_hybrid": (ci, [ci, u64]),
        "rdst_hip_last_route": (ci, [vp, u32p]),
        "rdst_hip_debug_raise_device_error": (ci, [u32, vp]),
        "rdst_hip_debug_last_sample": (ci, [vp, u32p]),
        "rdst_hip_stream_copy": (ci, [vp, vp, u64, vp]),
        "rdst_hip_stream_read": (ci, [vp, u64, vp]),
        "rdst_hip_stream_fill": (ci, [vp, u64, vp]),
        "rdst_hip_last_error": (ctypes.c_char_p, None),
        "rdst_hip_abi_version": (ci, None),
    }


# every symbol include/rdst_hip.h declares -> (restype, argtypes; None: not declared to ctypes, the caller converts); tests
# check that the library exports all of them
SIGNATURES = _signatures()
SYMBOLS = tuple(SIGNATURES)

_lib = None


def load():
    """Load librdst_hip.so once.  Importing torch first makes the loader resolve
    libamdhip64.so.7 to the copy torch already mapped, so device pointers and streams
    handed over from torch belong to the same HIP runtime."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RdstHipError(-100, f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    try:
        import torch  # noqa: F401  (runtime unification, see docstring)
    except Exception:  # pragma: no cover - torch is optional for host-only use
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc):
    if rc != RDST_OK:
        raise RdstHipError(rc, load().rdst_hip_last_error().decode("utf-8", "replace"))
