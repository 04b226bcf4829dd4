// rdst_segments_layout.h — the segmented sort's shapes and scratch layouts, stated once for the kernels and their launches
// (rdst_segments.hip) and for the host-only half (rdst_segments.cpp: rdst_hip_sort_segments_limits and the two
// ..._scratch_bytes functions).  No HIP here, and constexpr throughout: the kernels take the shapes as template arguments.
#ifndef RDST_SEGMENTS_LAYOUT_H
#define RDST_SEGMENTS_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "rdst_hip.h"
#include "rdst_args.h"

namespace rdst_segments_layout {

// ---- widths ----------------------------------------------------------------------------------------------------------
using rdst_args::key_width_ok;
constexpr bool pair_width_ok(uint32_t b) { return b == 4 || b == 8; }  // the keys and the values of a key-value sort

// ---- shapes ----------------------------------------------------------------------------------------------------------
// Keys per lane: the wave class holds wave_kpt keys per lane of its one wave, the block class block_kpt per thread of its
// 1024.  Keys only, the block class is the one-workgroup sort's tile (64 KiB of keys; 16 384 one- and two-byte keys); with
// values, key and value tiles share the 160 KiB of LDS beside the 16 KiB of count tables.
constexpr int BLOCK_THREADS = 1024;
constexpr int wave_kpt(size_t key_bytes) { return key_bytes == 16 ? 4 : 8; }
constexpr int block_kpt(size_t key_bytes, size_t val_bytes) {
    return val_bytes != 0 && key_bytes + val_bytes > 8 ? 8 : (key_bytes <= 4 ? 16 : (key_bytes == 8 ? 8 : 4));
}
constexpr uint32_t wave_max(size_t key_bytes) { return 64u * (uint32_t)wave_kpt(key_bytes); }  // the longest segment of the wave class
constexpr uint32_t block_max(size_t key_bytes, size_t val_bytes) {                                // ... of the block class; the tiled route's tile
    return (uint32_t)BLOCK_THREADS * (uint32_t)block_kpt(key_bytes, val_bytes);
}

// The segmented partial sort (rdst_topk_segments.hip): the longest segment its one-workgroup radix select streams from global
// memory.  Measured with one segment per call (DESIGN.md §2i has the sweep): at 2^17 keys the one workgroup still beats the
// whole-array route's per-call floor, at 2^18 the route's every-CU reads win, for 4- and 8-byte keys alike.
constexpr uint32_t TOPK_STREAM_MAX_DEFAULT = 1u << 17;

// The segmented select (rdst_select_segments.hip): rank specs per round, a kernel argument of 16 bytes each; one lane of a
// 32-lane step resolves each against the segment's length.
constexpr uint32_t SELECT_SEGMENTS_MAX_RANKS = 32;

// ---- scratch (byte offsets from its 256-byte aligned base; every array is rounded up to 256 bytes) ----------------------
constexpr uint64_t MAX_SEGMENTS = 1ull << 30;  // of a table in device memory
constexpr uint64_t up256(uint64_t bytes) { return (bytes + 255) / 256 * 256; }
// the segmented partial sort and select, borders on the host: the item table; a far segment's own scratch lies behind it
constexpr uint64_t table_bytes(uint64_t n_segments) { return up256(n_segments * sizeof(rdst_segment_item)); }

// Device-resident offsets: what the plan keeps.  A 256-byte header; four u32 arrays of n_segments (the class keys and
// segment indices of the plan's pair sort, and that sort's two tmps); the item table (16 bytes per segment): 32 bytes per
// segment and at most 1 536 bytes besides.
constexpr uint64_t PLAN_HEADER_BYTES = 256;
struct PlanLayout {
    uint64_t keys, segs, tmp_keys, tmp_segs, items, total;
};
constexpr PlanLayout plan_layout(uint64_t n_segments) {
    const uint64_t arr = up256(n_segments * sizeof(uint32_t)), at = PLAN_HEADER_BYTES;
    return {at, at + arr, at + 2 * arr, at + 3 * arr, at + 4 * arr, at + 4 * arr + up256(n_segments * sizeof(rdst_segment_item))};
}

// ---- the segmented partial sort with device-resident offsets (rdst_topk_segments_offsets.hip) ------------------------------
// Its plan keeps plan_layout's arrays.  The header words (u32) its kernels and the counted top-k kernels
// (rdst_topk_segments.hip) index:
enum TopkPlanHeader : int {
    HDR_TOPK_N_WAVE = 0,       // items of the wave class
    HDR_TOPK_N_BLOCK = 1,      // items of the block class (they follow the wave class in the item table)
    HDR_TOPK_N_STREAM = 2,     // items of the stream class (they follow the block class)
    HDR_TOPK_N_FAR = 3,        // items of the far class (they follow the stream class, in segment order)
    HDR_TOPK_FLAGS = 4,        // TOPK_PLAN_* bits: what the plan found wrong
    HDR_TOPK_LONGEST_FAR = 6,  // u64 in the words 6 and 7: the longest far segment
    HDR_TOPK_RUN_WAVE = 8,     // the counts the counted kernels run: the three N_ words, or 0, 0, 0 when nothing may be written
    HDR_TOPK_RUN_BLOCK = 9,
    HDR_TOPK_RUN_STREAM = 10,
    HDR_TOPK_WORDS = 64,
};
static_assert(HDR_TOPK_WORDS * sizeof(uint32_t) == PLAN_HEADER_BYTES, "the header the kernels index is the header of the layout");
constexpr uint32_t TOPK_PLAN_DECREASING = 1;  // offsets[s + 1] < offsets[s] somewhere
constexpr uint32_t TOPK_PLAN_PAST_LEN = 2;    // offsets[n_segments] > len
constexpr uint32_t TOPK_PLAN_FAR = 4;         // asynchronous mode only: a far segment, which only the host can enqueue
// The header as a host reads it back: the first TOPK_PLAN_READ_WORDS words, decoded in one place for every entry that waits.
constexpr int TOPK_PLAN_READ_WORDS = 8;
struct TopkPlanResult {
    uint64_t counts[4], longest_far;
    uint32_t flags;
};
constexpr TopkPlanResult topk_plan_result(const uint32_t (&h)[TOPK_PLAN_READ_WORDS]) {
    static_assert(HDR_TOPK_LONGEST_FAR + 1 < TOPK_PLAN_READ_WORDS && HDR_TOPK_N_FAR < TOPK_PLAN_READ_WORDS, "the words read cover what is decoded");
    TopkPlanResult r{};
    for (int c = 0; c < 4; ++c) r.counts[c] = h[HDR_TOPK_N_WAVE + c];
    r.flags = h[HDR_TOPK_FLAGS];
    r.longest_far = (uint64_t)h[HDR_TOPK_LONGEST_FAR] | ((uint64_t)h[HDR_TOPK_LONGEST_FAR + 1] << 32);
    return r;
}
// What the host answers for a plan that raised TOPK_PLAN_DECREASING or TOPK_PLAN_PAST_LEN.
constexpr const char* topk_plan_flags_message(uint32_t flags) {
    return flags & TOPK_PLAN_DECREASING ? "segments: offsets must be non-decreasing" : "segments: the last offset lies past len";
}

// The class key of a segment of n keys (n < 2^32): the plan sorts (key, segment) pairs by the library's stable 4-level pair
// sort, and the sorted pairs are the work list.  `stream_limit`: the longest segment of the stream class (block_max: none).
//   0                                       wave class: stays in segment order
//   1 + (block_max - n)                     block class, wave_max < n <= block_max: 1 .. block_max - wave_max, longest first
//   TOPK_KEY_STREAM_LAST - (n - block_max - 1)
//                                           stream class, block_max < n <= 2^32 - 1: block_max - 1 .. TOPK_KEY_STREAM_LAST,
//                                           longest first (the sort is stable: ties in segment order)
//   TOPK_KEY_FAR                            far class: in segment order
//   TOPK_KEY_NONE                           no key: no item
constexpr uint32_t TOPK_KEY_STREAM_LAST = 0xFFFFFFFDu, TOPK_KEY_FAR = 0xFFFFFFFEu, TOPK_KEY_NONE = 0xFFFFFFFFu;
constexpr uint32_t topk_class(uint64_t n, uint32_t wave_max, uint32_t block_max, uint32_t stream_limit) {  // 0 .. 3, or 4: no item
    return n == 0 ? 4u : (n <= wave_max ? 0u : (n <= block_max ? 1u : (n <= stream_limit ? 2u : 3u)));
}
constexpr uint32_t topk_class_key(uint64_t n, uint32_t wave_max, uint32_t block_max, uint32_t stream_limit) {
    const uint32_t c = topk_class(n, wave_max, block_max, stream_limit);
    return c == 0 ? 0u
                  : (c == 1 ? 1u + (block_max - (uint32_t)n)
                            : (c == 2 ? TOPK_KEY_STREAM_LAST - ((uint32_t)n - block_max - 1u) : (c == 3 ? TOPK_KEY_FAR : TOPK_KEY_NONE)));
}
// wave < block < stream < far < none for every width: the block keys end at block_max - wave_max, the stream keys start at
// block_max - 1 (n = 2^32 - 1)
constexpr bool topk_class_keys_disjoint() {
    for (uint32_t kb : {1u, 2u, 4u, 8u, 16u})
        for (uint32_t vb : {0u, 4u}) {
            const uint32_t wm = wave_max(kb), bm = block_max(kb, vb);
            if (!(wm >= 2 && wm < bm)) return false;
            if (!(topk_class_key(wm + 1, wm, bm, 0xFFFFFFFFu) == bm - wm && topk_class_key(bm, wm, bm, 0xFFFFFFFFu) == 1)) return false;
            if (!(topk_class_key(0xFFFFFFFFull, wm, bm, 0xFFFFFFFFu) == bm - 1 && bm - wm < bm - 1)) return false;
            if (!(topk_class_key((uint64_t)bm + 1, wm, bm, 0xFFFFFFFFu) == TOPK_KEY_STREAM_LAST && TOPK_KEY_STREAM_LAST < TOPK_KEY_FAR)) return false;
        }
    return TOPK_KEY_FAR < TOPK_KEY_NONE;
}
static_assert(topk_class_keys_disjoint(), "the class keys of the four classes lie in disjoint, ascending ranges");

// The nowait entries: the plan's layout, then what the tiled route keeps for the long class.  What the host knows bounds
// that class: a long segment holds more than block_max keys, so there are at most n_long_bound = min(n_segments,
// len / (block_max + 1)) of them, and with tiles of `tile` = block_max keys item i has ceil(len_i / tile) tiles: at most
// tiles_bound = len / tile + n_long_bound in all.  Behind the plan: tile_base (n_long_bound + 1 u32), digit_base (256 u32
// per possible long item), tile_counts (256 u32 per possible tile).  len < 2^32.
struct TileLayout {
    uint32_t n_long_bound, tiles_bound;
    uint64_t tile_base, digit_base, tile_counts, total;
};
constexpr TileLayout tile_layout(uint64_t n_segments, uint64_t len, uint32_t tile) {
    const uint64_t longs = len / ((uint64_t)tile + 1) < n_segments ? len / ((uint64_t)tile + 1) : n_segments;
    const uint64_t tiles = len / tile + longs;
    const uint64_t tile_base = plan_layout(n_segments).total;
    const uint64_t digit_base = tile_base + up256((longs + 1) * sizeof(uint32_t));
    const uint64_t tile_counts = digit_base + up256(longs * 256 * sizeof(uint32_t));
    return {(uint32_t)longs, (uint32_t)tiles, tile_base, digit_base, tile_counts, tile_counts + up256(tiles * 256 * sizeof(uint32_t))};
}

}  // namespace rdst_segments_layout

#endif  // RDST_SEGMENTS_LAYOUT_H
