"""rdst_amd — MI355X (gfx950) device route for rdst's radix sort, behind rdst's own surface.

    import rdst_amd
    rdst_amd.radix_sort_unstable(x)                       # numpy array or HIP torch tensor, in place
    rdst_amd.radix_sort_builder(x).with_tuner(t).sort()

The compute is hand-written HIP (rdst_amd/csrc) behind the C ABI of include/rdst_hip.h;
this package is the thin host mirror of src/radix_sort.rs, src/radix_sort_builder.rs and
src/tuner.rs of the reference.
"""
from . import tuner  # noqa: F401
from .radix_sort import (  # noqa: F401
    RadixSortBuilder,
    all_level_counts,
    device_status,
    key_info,
    level_counts,
    radix_sort_builder,
    radix_sort_unstable,
    scatter_level,
    set_tuning,
    set_profiling,
    set_hybrid,
    last_route,
    last_sample,
    release_workspace,
    last_profile,
    profile_run,
    profile_runs,
    sort_bytes_device_tensor,
    sort_bytes_device_nowait_tensor,
    sort_device_tensor,
    sort_device_tensor_lowmem,
    partition_device,
    sort_host_array,
    sort_host_records,
    segments_limits,
    segments_plan,
    segments_plan_device,
    segments_device_offsets_scratch_bytes,
    sort_pairs_device_tensor,
    sort_device_devlen_tensor,
    sort_pairs_device_devlen_tensor,
    topk_device_tensor,
    topk_scratch_bytes,
    topk_limits,
    topk_state,
    select_device_tensor,
    select_scratch_bytes,
    select_limits,
    select_state,
    quantile_ranks,
    topk_segments_device_tensor,
    topk_segments_device_offsets_tensor,
    topk_segments_device_offsets_scratch_bytes,
    topk_segments_plan_device,
    topk_rows_tensor,
    topk_segments_scratch_bytes,
    topk_segments_limits,
    topk_segments_plan,
    set_topk_segments_stream_max,
    sort_segments_device_tensor,
    sort_segments_device_offsets_tensor,
    sort_segments_device_offsets_nowait_tensor,
    segments_nowait_scratch_bytes,
    sort_records_by_key,
    sort_records_device_tensor,
    sort_records_device_nowait_tensor,
    KeyField,
    key_fields_of,
)
from ._lib import RdstHipError  # noqa: F401

__all__ = [
    "radix_sort_unstable", "radix_sort_builder", "RadixSortBuilder", "tuner", "RdstHipError",
    "sort_device_tensor", "sort_bytes_device_tensor", "sort_device_tensor_lowmem", "partition_device", "sort_host_array", "sort_host_records", "sort_pairs_device_tensor", "sort_segments_device_tensor", "segments_limits", "segments_plan",
    "sort_segments_device_offsets_tensor", "sort_segments_device_offsets_nowait_tensor", "segments_nowait_scratch_bytes", "segments_device_offsets_scratch_bytes", "segments_plan_device", "sort_records_by_key", "level_counts", "all_level_counts", "scatter_level",
    "device_status", "set_tuning", "set_profiling", "set_hybrid", "last_route", "last_sample", "release_workspace", "last_profile", "key_info",
    "KeyField", "key_fields_of", "sort_records_device_tensor", "sort_bytes_device_nowait_tensor", "sort_records_device_nowait_tensor",
    "sort_device_devlen_tensor", "sort_pairs_device_devlen_tensor",
    "topk_device_tensor", "topk_scratch_bytes", "topk_limits", "topk_state",
    "select_device_tensor", "select_scratch_bytes", "select_limits", "select_state", "quantile_ranks",
    "topk_segments_device_tensor", "topk_rows_tensor", "topk_segments_scratch_bytes", "topk_segments_limits", "topk_segments_plan",
    "set_topk_segments_stream_max", "topk_segments_device_offsets_tensor", "topk_segments_device_offsets_scratch_bytes", "topk_segments_plan_device",
]
