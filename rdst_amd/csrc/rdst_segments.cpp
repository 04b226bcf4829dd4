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
// The limits follow from what the kernels of rdst_segments.hip keep per lane and per workgroup; both files take them
// from rdst_hip_sort_segments_limits, below.
//
// Host only: no HIP here (bound by tests/test_segments_plan.py without a device, and compiled into a stand-alone
// program under the address sanitizer by the same test).
#include <stdint.h>
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "rdst_hip.h"

namespace rdst_internal {
// Records `what` for rdst_hip_last_error and returns `code` (rdst_kernels.hip; a stand-alone program brings its own).
int note_error(int code, const char* what);
}  // namespace rdst_internal

using rdst_internal::note_error;

// Keys per lane: the wave class holds WAVE_KPT keys per lane of its one wave, the block class BLOCK_KPT per thread of
// its 1024.  Keys only, the block class is the one-workgroup sort's tile (64 KiB of keys; 16 384 one- and two-byte
// keys); with values, key and value tiles share the 160 KiB of LDS beside the 16 KiB of count tables.
extern "C" int rdst_hip_sort_segments_limits(uint32_t elem_bytes, uint32_t val_bytes, uint32_t out[2]) {
    if (!out) return note_error(RDST_ERR_ARG, "segments_limits: null output");
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16)
        return note_error(RDST_ERR_UNSUPPORTED, "device path is built for 1-, 2-, 4-, 8- and 16-byte keys");
    if (val_bytes != 0) {
        if (elem_bytes != 4 && elem_bytes != 8) return note_error(RDST_ERR_UNSUPPORTED, "key-value sorts take 4- or 8-byte keys");
        if (val_bytes != 4 && val_bytes != 8) return note_error(RDST_ERR_UNSUPPORTED, "key-value sorts carry 4- or 8-byte values");
    }
    const uint32_t wave_kpt = elem_bytes == 16 ? 4u : 8u;
    uint32_t block_kpt = elem_bytes <= 4 ? 16u : (elem_bytes == 8 ? 8u : 4u);
    if (val_bytes != 0 && elem_bytes + val_bytes > 8) block_kpt = 8u;
    out[0] = 64u * wave_kpt;
    out[1] = 1024u * block_kpt;
    return RDST_OK;
}

// Device-resident offsets: what the plan keeps in the caller's scratch.  A 256-byte header; four u32 arrays of n_segments
// (the class keys and segment indices of the plan's pair sort, and that sort's two tmps), each rounded up to 256 bytes; the
// item table (16 bytes per segment), rounded up likewise: 32 bytes per segment and at most 1 536 bytes besides.
extern "C" uint64_t rdst_hip_sort_segments_device_offsets_scratch_bytes(uint64_t n_segments) {
    if (n_segments == 0 || n_segments > (1ull << 30)) return 0;
    const uint64_t arr = (n_segments * sizeof(uint32_t) + 255) / 256 * 256;
    const uint64_t table = (n_segments * sizeof(rdst_segment_item) + 255) / 256 * 256;
    return 256 + 4 * arr + table;
}

// The nowait entries (rdst_hip_sort_segments_device_offsets_nowait / _pairs_): the plan's layout above, then what the tiled
// route keeps for the long class.  What the host knows bounds that class: a long segment holds more than block_max keys, so
// there are at most n_long_bound = min(n_segments, len / (block_max + 1)) of them, and with tiles of T = block_max keys item i
// has ceil(len_i / T) tiles: at most tiles_bound = len / T + n_long_bound in all.  Behind the plan: tile_base
// (n_long_bound + 1 u32), digit_base (256 u32 per possible long item), tile_counts (256 u32 per possible tile), each rounded
// up to 256 bytes.  This is the one statement of the layout (rdst_segments.hip checks its own against it).
extern "C" uint64_t rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(uint64_t n_segments, uint64_t len, uint32_t elem_bytes,
                                                                               uint32_t val_bytes) {
    const uint64_t plan = rdst_hip_sort_segments_device_offsets_scratch_bytes(n_segments);
    if (plan == 0 || len >= (1ull << 32)) return 0;
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16) return 0;
    if (val_bytes != 0 && ((elem_bytes != 4 && elem_bytes != 8) || (val_bytes != 4 && val_bytes != 8))) return 0;
    uint32_t block_kpt = elem_bytes <= 4 ? 16u : (elem_bytes == 8 ? 8u : 4u);  // (rdst_hip_sort_segments_limits, without its error notes)
    if (val_bytes != 0 && elem_bytes + val_bytes > 8) block_kpt = 8u;
    const uint64_t tile = 1024ull * block_kpt;
    const uint64_t n_long_bound = std::min<uint64_t>(n_segments, len / (tile + 1));
    const uint64_t tiles_bound = len / tile + n_long_bound;
    const auto up = [](uint64_t bytes) { return (bytes + 255) / 256 * 256; };
    return plan + up((n_long_bound + 1) * sizeof(uint32_t)) + up(n_long_bound * 256 * sizeof(uint32_t)) + up(tiles_bound * 256 * sizeof(uint32_t));
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
