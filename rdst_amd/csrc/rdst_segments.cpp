// rdst_segments.cpp — host side of the segmented sort (rdst_hip_sort_segments_device): the class limits and the work list.
//
// A caller with many independent slices — the reference's own recursion over the 256 buckets of a chunk
// (src/sorter.rs:131-138), a `chunks_mut(..).par_for_each(|c| c.radix_sort_unstable())`, a ragged batch — hands over one
// array and a table of segment borders.  Every segment of at least two keys becomes one work item in one of three
// classes, chosen by its length alone:
//   wave   2 <= len <= wave_max          one wave sorts it in registers; several segments share a workgroup
//   block  wave_max < len <= block_max   one workgroup sorts it (the one-workgroup LDS sort)
//   long   len > block_max               the whole-slice route, one segment after another
// Items are written wave class first (segment order), then block class (longest first, ties in segment order: the
// grid's tail is short work), then long class (segment order).
//
// The limits follow from what the kernels of rdst_segments.hip keep per lane and per workgroup; rdst_segments_layout.h
// states them, and the scratch layouts, once for both files.
//
// The segmented partial sort (rdst_hip_topk_segments_device, rdst_topk_segments.hip) has its limits, its border setter and its
// plan here too: four classes, and a segment of one key is work.  The segmented select (rdst_hip_select_segments_device,
// rdst_select_segments.hip) runs that plan with k = 1; its rank rule (rdst_rank_for_length) and its limits are here.
//
// Host only: no HIP here (bound by tests/test_segments_plan.py without a device, and compiled into a stand-alone
// program under the address sanitizer by the same test).
#include <stdint.h>
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "rdst_hip.h"
#include "rdst_args.h"
#include "rdst_rank_rule.h"
#include "rdst_segments_layout.h"

namespace rdst_internal {
// Records `what` for rdst_hip_last_error and returns `code` (rdst_kernels.hip; a stand-alone program brings its own).
int note_error(int code, const char* what);
}  // namespace rdst_internal

using rdst_internal::note_error;
namespace L = rdst_segments_layout;

extern "C" int rdst_hip_sort_segments_limits(uint32_t elem_bytes, uint32_t val_bytes, uint32_t out[2]) {
    if (!out) return note_error(RDST_ERR_ARG, "segments_limits: null output");
    if (!L::key_width_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "device path is built for 1-, 2-, 4-, 8- and 16-byte keys");
    if (val_bytes != 0) {
        if (!L::pair_width_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "key-value sorts take 4- or 8-byte keys");
        if (!L::pair_width_ok(val_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "key-value sorts carry 4- or 8-byte values");
    }
    out[0] = L::wave_max(elem_bytes);
    out[1] = L::block_max(elem_bytes, val_bytes);
    return RDST_OK;
}

// The scratch of the device-offsets entries: the plan's layout.
extern "C" uint64_t rdst_hip_sort_segments_device_offsets_scratch_bytes(uint64_t n_segments) {
    if (n_segments == 0 || n_segments > L::MAX_SEGMENTS) return 0;
    return L::plan_layout(n_segments).total;
}

// The scratch of the nowait entries (rdst_hip_sort_segments_device_offsets_nowait / _pairs_): the plan's layout, then the
// tiled route's.
extern "C" uint64_t rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(uint64_t n_segments, uint64_t len, uint32_t elem_bytes,
                                                                               uint32_t val_bytes) {
    if (n_segments == 0 || n_segments > L::MAX_SEGMENTS || len >= (1ull << 32)) return 0;
    if (!L::key_width_ok(elem_bytes) || (val_bytes != 0 && !(L::pair_width_ok(elem_bytes) && L::pair_width_ok(val_bytes)))) return 0;
    return L::tile_layout(n_segments, len, L::block_max(elem_bytes, val_bytes)).total;
}

extern "C" int rdst_segments_plan(const uint64_t* offsets, uint64_t n_segments, uint64_t len, uint32_t elem_bytes, uint32_t val_bytes,
                                  rdst_segment_item* items_out, uint64_t capacity, uint64_t class_counts_out[3],
                                  uint64_t* tmp_elems_out) {
    uint32_t lim[2];
    if (int rc = rdst_hip_sort_segments_limits(elem_bytes, val_bytes, lim)) return rc;
    if (!class_counts_out || !tmp_elems_out) return note_error(RDST_ERR_ARG, "segments_plan: null output");
    class_counts_out[0] = class_counts_out[1] = class_counts_out[2] = 0;
    *tmp_elems_out = 0;
    if (n_segments == 0) return RDST_OK;
    if (!offsets) return note_error(RDST_ERR_ARG, "segments: null offsets");
    if (n_segments >= (1ull << 32)) return note_error(RDST_ERR_ARG, "segments: n_segments must be below 2^32");
    for (uint64_t s = 0; s < n_segments; ++s)
        if (offsets[s + 1] < offsets[s]) return note_error(RDST_ERR_ARG, "segments: offsets must be non-decreasing");
    if (offsets[n_segments] > len) return note_error(RDST_ERR_ARG, "segments: the last offset lies past len");
    const uint64_t wave_max = lim[0], block_max = lim[1];
    uint64_t counts[3] = {0, 0, 0}, longest = 0;
    for (uint64_t s = 0; s < n_segments; ++s) {
        const uint64_t n = offsets[s + 1] - offsets[s];
        if (n < 2) continue;
        ++counts[n <= wave_max ? 0 : (n <= block_max ? 1 : 2)];
        if (n > block_max && n > longest) longest = n;
    }
    class_counts_out[0] = counts[0];
    class_counts_out[1] = counts[1];
    class_counts_out[2] = counts[2];
    *tmp_elems_out = longest;
    const uint64_t total = counts[0] + counts[1] + counts[2];
    if (total > capacity) return note_error(RDST_ERR_ARG, "segments_plan: capacity too small for the work list");
    if (total == 0) return RDST_OK;
    if (!items_out) return note_error(RDST_ERR_ARG, "segments_plan: null item table");
    uint64_t at[3] = {0, counts[0], counts[0] + counts[1]};
    for (uint64_t s = 0; s < n_segments; ++s) {
        const uint64_t n = offsets[s + 1] - offsets[s];
        if (n < 2) continue;
        const int c = n <= wave_max ? 0 : (n <= block_max ? 1 : 2);
        // a batched segment is at most block_max keys long; a long one's `len` saturates (its length is offsets[seg + 1] - offsets[seg])
        items_out[at[c]++] = {offsets[s], (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull), (uint32_t)s};
    }
    rdst_segment_item* block = items_out + counts[0];
    std::stable_sort(block, block + counts[1], [](const rdst_segment_item& a, const rdst_segment_item& b) { return a.len > b.len; });
    return RDST_OK;
}

// ---- the segmented partial sort: limits and plan (the kernels and the entry: rdst_topk_segments.hip) ----------------------

namespace {
uint32_t g_topk_stream_max = 0;  // 0: the default
// keys only: every width; with an index: 4- and 8-byte keys and a 4- or 8-byte index (rdst_hip_topk_limits' codes)
int topk_segments_widths(uint32_t elem_bytes, uint32_t index_bytes) {
    if (!L::key_width_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "device path is built for 1-, 2-, 4-, 8- and 16-byte keys");
    if (index_bytes != 0 && !rdst_args::index_bytes_ok(index_bytes)) return note_error(RDST_ERR_ARG, "topk: index_bytes must be 4 or 8");
    if (index_bytes != 0 && !rdst_args::index_keys_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "topk: an index output takes 4- or 8-byte keys");
    return RDST_OK;
}
}  // namespace

extern "C" int rdst_hip_set_topk_segments_stream_max(uint32_t stream_max) {
    g_topk_stream_max = stream_max;
    return RDST_OK;
}

extern "C" int rdst_hip_topk_segments_limits(uint32_t elem_bytes, uint32_t index_bytes, uint32_t out[4]) {
    if (!out) return note_error(RDST_ERR_ARG, "topk_segments_limits: null output");
    if (int rc = topk_segments_widths(elem_bytes, index_bytes)) return rc;
    const uint32_t bm = L::block_max(elem_bytes, index_bytes ? 4 : 0);  // the position travels as a u32 beside the key
    out[0] = L::wave_max(elem_bytes);
    out[1] = bm;
    out[2] = std::max(bm, g_topk_stream_max ? g_topk_stream_max : L::TOPK_STREAM_MAX_DEFAULT);  // (a border below bm: no stream class)
    out[3] = bm;
    return RDST_OK;
}

extern "C" int rdst_topk_segments_plan(const uint64_t* offsets, uint64_t n_segments, uint64_t len, uint64_t k, uint32_t elem_bytes,
                                       uint32_t index_bytes, rdst_segment_item* items_out, uint64_t capacity, uint64_t class_counts_out[4],
                                       uint64_t* longest_far_out) {
    uint32_t lim[4];
    if (int rc = rdst_hip_topk_segments_limits(elem_bytes, index_bytes, lim)) return rc;
    if (!class_counts_out || !longest_far_out) return note_error(RDST_ERR_ARG, "topk_segments_plan: null output");
    class_counts_out[0] = class_counts_out[1] = class_counts_out[2] = class_counts_out[3] = 0;
    *longest_far_out = 0;
    if (n_segments == 0 || k == 0) return RDST_OK;
    if (!offsets) return note_error(RDST_ERR_ARG, "segments: null offsets");
    if (n_segments >= (1ull << 32)) return note_error(RDST_ERR_ARG, "segments: n_segments must be below 2^32");
    for (uint64_t s = 0; s < n_segments; ++s)
        if (offsets[s + 1] < offsets[s]) return note_error(RDST_ERR_ARG, "segments: offsets must be non-decreasing");
    if (offsets[n_segments] > len) return note_error(RDST_ERR_ARG, "segments: the last offset lies past len");
    const uint64_t wave_max = lim[0], block_max = lim[1], stream_max = lim[2], k_stream_max = lim[3];
    const auto class_of = [&](uint64_t n) { return n <= wave_max ? 0 : (n <= block_max ? 1 : (n <= stream_max && k <= k_stream_max ? 2 : 3)); };
    uint64_t counts[4] = {0, 0, 0, 0}, longest = 0;
    for (uint64_t s = 0; s < n_segments; ++s) {
        const uint64_t n = offsets[s + 1] - offsets[s];
        if (n == 0) continue;
        const int c = class_of(n);
        ++counts[c];
        if (c == 3 && n > longest) longest = n;
    }
    uint64_t total = 0;
    for (int c = 0; c < 4; ++c) total += class_counts_out[c] = counts[c];
    *longest_far_out = longest;
    if (total > capacity) return note_error(RDST_ERR_ARG, "topk_segments_plan: capacity too small for the work list");
    if (total == 0) return RDST_OK;
    if (!items_out) return note_error(RDST_ERR_ARG, "topk_segments_plan: null item table");
    uint64_t at[4] = {0, counts[0], counts[0] + counts[1], counts[0] + counts[1] + counts[2]};
    for (uint64_t s = 0; s < n_segments; ++s) {
        const uint64_t n = offsets[s + 1] - offsets[s];
        if (n == 0) continue;
        items_out[at[class_of(n)]++] = {offsets[s], (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull), (uint32_t)s};
    }
    const auto longer = [](const rdst_segment_item& a, const rdst_segment_item& b) { return a.len > b.len; };
    rdst_segment_item* block = items_out + counts[0];
    std::stable_sort(block, block + counts[1], longer);
    std::stable_sort(block + counts[1], block + counts[1] + counts[2], longer);
    return RDST_OK;
}

// ---- the segmented select: the rank rule and the limits (the kernels and the entry: rdst_select_segments.hip) ---------------

extern "C" int rdst_rank_for_length(const rdst_rank_spec* spec, uint64_t n, uint64_t* rank_out) {
    if (!spec || !rank_out) return note_error(RDST_ERR_ARG, "rank_for_length: null argument");
    if (!rdst_rank_rule::spec_ok(*spec))
        return note_error(RDST_ERR_ARG, "rank spec: num <= den for a quantile, mode 0 .. 2 (0 for an absolute rank), reserved 0");
    if (spec->den != 0 && n > (1ull << 32)) return note_error(RDST_ERR_ARG, "rank_for_length: a quantile takes n <= 2^32");
    uint64_t rank = 0;
    if (!rdst_rank_rule::resolve(*spec, n, &rank)) return 0;
    *rank_out = rank;
    return 1;
}

extern "C" int rdst_hip_select_segments_limits(uint32_t elem_bytes, uint32_t index_bytes, uint32_t out[4]) {
    if (!out) return note_error(RDST_ERR_ARG, "select_segments_limits: null output");
    if (int rc = rdst_hip_topk_segments_limits(elem_bytes, index_bytes, out)) return rc;  // the classes of the plan with k = 1
    out[3] = L::SELECT_SEGMENTS_MAX_RANKS;
    return RDST_OK;
}
