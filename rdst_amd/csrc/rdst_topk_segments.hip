// rdst_topk_segments.hip — the segmented partial sort: the k first (RDST_TOPK_LARGEST: last) keys of every segment of one
// array, in order, with their segment-local positions if asked for (rdst_hip_topk_segments_device; include/rdst_hip.h,
// DESIGN.md §2i).  Row s of the outputs holds what rdst_hip_topk_device gives for segment s, bit for bit.
//
// The host plan (rdst_topk_segments_plan, rdst_segments.cpp) puts every segment of at least one key into one of four classes:
//
//   topk_segment_wave_kernel     one WAVE per segment of up to wave_max keys, four segments per workgroup: segment_wave_body's
//   topk_segment_block_kernel    level loop (rdst_segments.hip), and one WORKGROUP per segment of up to block_max keys:
//                                segment_block_body's.  Both restated here with what differs: the source is const, the value
//                                beside a key is its position in the segment, generated, and the first k_s ranks go to row
//                                `seg` of the outputs as original key bits.  The LSD loops are stable and positions start in
//                                ascending order, so equal keys come out in ascending position.
//   topk_segment_stream_kernel   one workgroup of 1 024 threads per segment of up to stream_max keys, for k <= block_max: a radix
//                                select on the mapped key out of global memory (L2 after the first read), 12-bit digits, most
//                                significant first, into 4 096 LDS counters; pick_bucket (rdst_device.h: rdst_topk.hip's scan)
//                                extends the prefix.  It stops when c_below + m <= TILE (keys before the prefix + keys on it) or
//                                the digits are exhausted.  One more read collects, IN POSITION ORDER, every key before the
//                                prefix and the first TILE - c_below keys on it into the LDS stage (an ordered compaction: a
//                                shuffle scan inside the wave, 16 wave totals per group of loads); the block class's level loop
//                                orders the stage and the first k are stored.  Digits exhausted: the keys on the prefix are
//                                equal, and the first of them in position order are the ties that win.
//   far                          everything else, one segment after another through rdst_hip_topk_device's own route
//                                (rdst_internal::topk_slice_locked), in the part of the scratch behind the item table.
//
// Each of the three kernels is one body (topk_segment_*_body) under two entries: the kernel the host entry launches with the
// counts it knows, and a ..._counted_kernel that reads its item range from the plan header in device memory
// (rdst_hip_topk_segments_device_offsets, rdst_topk_segments_offsets.hip, through rdst_internal::topk_segments_launch_locked).
//
// The level loops (wave_order, block_order), the select's counting read (count_digits) and the ordered compaction (collect_trip,
// collect_segment) live in rdst_segments_device.h: the segmented select (rdst_select_segments.hip) runs on them too.
//
// Slots past a segment's end hold the largest mapped key; they start behind every real key and stay there (rdst_segments.hip).
// With RDST_TOPK_LARGEST both xor masks are complemented, as run_topk does; the kernels always map.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_device.h"
#include "rdst_segments_layout.h"
#include "rdst_segments_device.h"

namespace {

using rdst_internal::launch;
using rdst_internal::set_error;

// ---- wave class --------------------------------------------------------------------------------------------------------------

template <typename K, bool IDX>
__device__ __forceinline__ void topk_segment_wave_body(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items, uint32_t n_items,
                                                       const Rows<K> o) {
    constexpr int KPT = L::wave_kpt(sizeof(K));
    constexpr int CAP = 64 * KPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t item = blockIdx.x * SEG_WAVES + (uint32_t)wave;
    if (item >= n_items) return;  // wave-uniform; no workgroup barrier follows
    uint32_t* tbl = reinterpret_cast<uint32_t*>(smem) + wave * RADIX;
    K* stage = reinterpret_cast<K*>(smem + SEG_WAVES * RADIX * sizeof(uint32_t)) + wave * CAP;
    uint32_t* vstage = reinterpret_cast<uint32_t*>(smem + SEG_WAVES * (RADIX * sizeof(uint32_t) + CAP * sizeof(K))) + (IDX ? wave * CAP : 0);
    const rdst_segment_item it = items[item];
    const uint32_t n = it.len < (uint32_t)CAP ? it.len : (uint32_t)CAP;  // (the plan never hands this class a longer one)
    const uint32_t k_s = o.k < n ? (uint32_t)o.k : n;
    const K* seg = keys + it.start;
    const int rounds = (int)((n + 63) / 64);
    K mk[KPT];
    uint32_t mv[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = (uint32_t)i * 64u + (uint32_t)lane;
        K v = (K) ~(K)0;
        if (i < rounds && idx < n) v = map_key<K>(seg[idx], o.neg, o.pos);
        mk[i] = v;
        mv[i] = idx;
    }
    wave_order<K, IDX, KPT>(mk, mv, rounds, tbl, stage, vstage);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t rank = (uint32_t)i * 64u + (uint32_t)lane;
        if (i < rounds && rank < k_s) store_rank<K, IDX>(o, it.seg, rank, mk[i], mv[i]);
    }
}

template <typename K, bool IDX>
__global__ __launch_bounds__(SEG_WAVES * 64) void topk_segment_wave_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                            uint32_t n_items, const Rows<K> o) {
    topk_segment_wave_body<K, IDX>(keys, items, n_items, o);
}

// ---- block class (the level loop, shared with the stream class: rdst_segments_device.h) -----------------------------------------

template <typename K, bool IDX, int KPT>
__device__ __forceinline__ void store_first(const K (&mk)[KPT], const uint32_t (&mv)[KPT], int rounds, uint32_t k_s, uint32_t seg, const Rows<K>& o) {
    const uint32_t wbase = (threadIdx.x >> 6) * 64u * (uint32_t)rounds + (threadIdx.x & 63u);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t rank = wbase + i * 64;
        if (i < rounds && rank < k_s) store_rank<K, IDX>(o, seg, rank, mk[i], mv[i]);
    }
}

template <typename K, bool IDX>
__device__ __forceinline__ void topk_segment_block_body(const K* __restrict__ keys, const rdst_segment_item it, const Rows<K> o) {
    constexpr int KPT = BlockLds<K, IDX>::KPT;
    constexpr uint32_t TILE = BlockLds<K, IDX>::TILE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const BlockLds<K, IDX> lds(smem);
    const uint32_t n = it.len < TILE ? it.len : TILE;  // (the plan never hands this class a longer one)
    const uint32_t k_s = o.k < n ? (uint32_t)o.k : n;
    const K* seg = keys + it.start;
    const int rounds = (int)((n + BLOCK_THREADS - 1) / BLOCK_THREADS);
    const uint32_t wbase = (threadIdx.x >> 6) * 64u * (uint32_t)rounds + (threadIdx.x & 63u);
    K mk[KPT];
    uint32_t mv[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = wbase + i * 64;
        K v = (K) ~(K)0;
        if (i < rounds && idx < n) v = map_key<K>(seg[idx], o.neg, o.pos);
        mk[i] = v;
        mv[i] = idx;
    }
    block_order<K, IDX, KPT>(mk, mv, rounds, lds);
    store_first<K, IDX, KPT>(mk, mv, rounds, k_s, it.seg, o);
}

template <typename K, bool IDX>
__global__ __launch_bounds__(BLOCK_THREADS) void topk_segment_block_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                           const Rows<K> o) {
    topk_segment_block_body<K, IDX>(keys, items[blockIdx.x], o);  // the grid is exactly this class's items
}

// ---- stream class ------------------------------------------------------------------------------------------------------------

template <typename K, bool IDX>
__device__ __forceinline__ void topk_segment_stream_body(const K* __restrict__ keys, const rdst_segment_item it, const Rows<K> o) {
    constexpr int KPT = BlockLds<K, IDX>::KPT;
    constexpr uint32_t TILE = BlockLds<K, IDX>::TILE;
    constexpr uint32_t BITS = 8 * sizeof(K), DIGIT = sizeof(K) == 1 ? 8 : 12;  // rdst_topk.hip's digits
    constexpr uint32_t SELECT_LEVELS = (BITS + DIGIT - 1) / DIGIT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_wave[2][STREAM_UNROLL][BLOCK_WAVES];
    __shared__ SelectState<K> s_state;
    static_assert(sizeof(s_wave) + sizeof(SelectState<K>) + 16 <= STREAM_STATIC_LDS, "the static LDS stays within what the launch accounts for");
    const BlockLds<K, IDX> lds(smem);
    uint32_t* cnt = lds.wave_hist;
    const uint32_t tid = threadIdx.x;
    const uint32_t n = it.len;
    uint32_t k = o.k < n ? (uint32_t)o.k : n;
    if (k > TILE) k = TILE;  // (the plan hands this class k <= TILE only)
    const SegmentCut<K> cut(keys + it.start, n);

    // ---- select: the prefix of the k-th key, a digit per read
    K pref = 0, pmask = 0;
    uint32_t c_below = 0, m = n;
    for (uint32_t level = 0; level < SELECT_LEVELS && c_below + m > TILE; ++level) {  // block-uniform
        const uint32_t hi = BITS - level * DIGIT, lo = hi > DIGIT ? hi - DIGIT : 0u;
        const int shift = (int)lo;
        const uint32_t dmask = (1u << (hi - lo)) - 1u;
        count_digits<K>(cut, o.neg, o.pos, pref, pmask, shift, dmask, cnt);
        uint32_t c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = cnt[4 * tid + j];
        uint32_t run;
        int j;
        if (pick_bucket(c, k - c_below, &s_wave[0][0][0], &run, &j)) {  // exactly one thread
            const uint32_t bucket = 4 * tid + (uint32_t)j;
            s_state.pref = (K)(pref | (K)((K)bucket << shift));
            s_state.pmask = (K)(pmask | (K)((K)dmask << shift));
            s_state.c_below = c_below + run;
            s_state.m = c[j];
        }
        __syncthreads();
        pref = s_state.pref;
        pmask = s_state.pmask;
        c_below = s_state.c_below;
        m = s_state.m;
    }

    // ---- collect, in position order: head, vectors, tail
    const uint32_t lim = TILE - (c_below < TILE ? c_below : TILE);
    uint32_t tot_b = 0, tot_o = 0;
    __syncthreads();  // (pick_bucket's wave sums lie in s_wave)
    collect_segment<K, IDX, true>(cut, o.neg, o.pos, pref, pmask, lim, 0u, TILE, lds.stage, lds.vstage, s_wave, tot_b, tot_o);

    // ---- order the stage, store the first k
    const uint32_t kept_on = tot_o < lim ? tot_o : lim;
    const uint32_t filled = tot_b + kept_on < TILE ? tot_b + kept_on : TILE;
    const int rounds = (int)((filled + BLOCK_THREADS - 1) / BLOCK_THREADS);
    __syncthreads();  // the stage is complete
    K rk[KPT];
    uint32_t rv[KPT];
    order_stage<K, IDX, KPT>(rk, rv, filled, rounds, lds);
    store_first<K, IDX, KPT>(rk, rv, rounds, k < filled ? k : filled, it.seg, o);
}

template <typename K, bool IDX>
__global__ __launch_bounds__(BLOCK_THREADS) void topk_segment_stream_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                            const Rows<K> o) {
    topk_segment_stream_body<K, IDX>(keys, items[blockIdx.x], o);  // the grid is exactly this class's items
}

// ---- the same three bodies with their item range read from the plan header in device memory (device-resident offsets) ----------
//
// rdst_topk_segments_offsets.hip writes the header (rdst_segments_layout.h: TopkPlanHeader) and the item table.  The grids are
// bounds the host can state without the counts; waves and workgroups past the count return before any barrier.
template <typename K, bool IDX>
__global__ __launch_bounds__(SEG_WAVES * 64) void topk_segment_wave_counted_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                                    const uint32_t* __restrict__ hdr, const Rows<K> o) {
    topk_segment_wave_body<K, IDX>(keys, items, hdr[L::HDR_TOPK_RUN_WAVE], o);
}

template <typename K, bool IDX>
__global__ __launch_bounds__(BLOCK_THREADS) void topk_segment_block_counted_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                                   const uint32_t* __restrict__ hdr, const Rows<K> o) {
    if (blockIdx.x >= hdr[L::HDR_TOPK_RUN_BLOCK]) return;  // block-uniform
    topk_segment_block_body<K, IDX>(keys, items[hdr[L::HDR_TOPK_N_WAVE] + blockIdx.x], o);
}

template <typename K, bool IDX>
__global__ __launch_bounds__(BLOCK_THREADS) void topk_segment_stream_counted_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                                    const uint32_t* __restrict__ hdr, const Rows<K> o) {
    if (blockIdx.x >= hdr[L::HDR_TOPK_RUN_STREAM]) return;  // block-uniform
    topk_segment_stream_body<K, IDX>(keys, items[hdr[L::HDR_TOPK_N_WAVE] + hdr[L::HDR_TOPK_N_BLOCK] + blockIdx.x], o);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

using SegTopkCall = rdst_internal::TopkSegmentsCall;

// The three batched launches over the item table in device memory: wave class first, then block class, then stream class.
// `hdr` == nullptr: the host knows the counts, counts[0 .. 2], and the classes follow one another in `items`.  With `hdr`, the
// plan header in device memory: the counts stand there, and counts[0 .. 2] are the host's bounds on them, for the grids alone.
template <typename K, bool IDX>
int launch_classes_t(const SegTopkCall& c, const rdst_segment_item* items, const uint32_t* hdr, const uint64_t counts[3]) {
    constexpr size_t wave_lds = wave_lds_bytes(sizeof(K), IDX), block_lds = block_lds_bytes(sizeof(K), IDX);
    static_assert(wave_lds <= LDS_LIMIT && block_lds + STREAM_STATIC_LDS <= LDS_LIMIT, "a workgroup's LDS stays within 160 KiB");
    unsigned __int128 neg, pos;
    rdst_internal::key_xor_masks(c.kind, (uint32_t)sizeof(K), &neg, &pos);
    Rows<K> o{static_cast<K*>(c.out_keys), c.out_index, c.index_bytes, c.k, (K)neg, (K)pos};
    if (c.largest) {  // the complement of the mapped key: both masks complemented
        o.neg = (K)~o.neg;
        o.pos = (K)~o.pos;
    }
    const K* keys = static_cast<const K*>(c.keys);
    const dim3 wave_grid((uint32_t)((counts[0] + SEG_WAVES - 1) / SEG_WAVES)), block_grid((uint32_t)counts[1]), stream_grid((uint32_t)counts[2]);
    int rc;
    if (counts[0]) {
        rc = hdr ? launch("topk_segment_wave_counted_kernel", topk_segment_wave_counted_kernel<K, IDX>, wave_grid, dim3(SEG_WAVES * 64), wave_lds, c.s, keys,
                          items, hdr, o)
                 : launch("topk_segment_wave_kernel", topk_segment_wave_kernel<K, IDX>, wave_grid, dim3(SEG_WAVES * 64), wave_lds, c.s, keys, items,
                          (uint32_t)counts[0], o);
        if (rc) return rc;
        if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_SEGMENTS))) return rc;
    }
    if (counts[1]) {
        rc = hdr ? launch("topk_segment_block_counted_kernel", topk_segment_block_counted_kernel<K, IDX>, block_grid, dim3(BLOCK_THREADS), block_lds, c.s, keys,
                          items, hdr, o)
                 : launch("topk_segment_block_kernel", topk_segment_block_kernel<K, IDX>, block_grid, dim3(BLOCK_THREADS), block_lds, c.s, keys,
                          items + counts[0], o);
        if (rc) return rc;
        if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_SEGMENTS | (1u << 8)))) return rc;
    }
    if (counts[2]) {
        rc = hdr ? launch("topk_segment_stream_counted_kernel", topk_segment_stream_counted_kernel<K, IDX>, stream_grid, dim3(BLOCK_THREADS), block_lds, c.s,
                          keys, items, hdr, o)
                 : launch("topk_segment_stream_kernel", topk_segment_stream_kernel<K, IDX>, stream_grid, dim3(BLOCK_THREADS), block_lds, c.s, keys,
                          items + counts[0] + counts[1], o);
        if (rc) return rc;
        if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_SEGMENTS | (2u << 8)))) return rc;
    }
    return RDST_OK;
}

int launch_classes(const SegTopkCall& c, const rdst_segment_item* items, const uint32_t* hdr, const uint64_t counts[3]) {
    if (c.index_bytes != 0)
        return c.elem_bytes == 4 ? launch_classes_t<uint32_t, true>(c, items, hdr, counts) : launch_classes_t<uint64_t, true>(c, items, hdr, counts);
    switch (c.elem_bytes) {
        case 1: return launch_classes_t<uint8_t, false>(c, items, hdr, counts);
        case 2: return launch_classes_t<uint16_t, false>(c, items, hdr, counts);
        case 4: return launch_classes_t<uint32_t, false>(c, items, hdr, counts);
        case 8: return launch_classes_t<uint64_t, false>(c, items, hdr, counts);
        default: return launch_classes_t<u128, false>(c, items, hdr, counts);
    }
}

}  // namespace

int rdst_internal::topk_segments_launch_locked(const TopkSegmentsCall& c, const rdst_segment_item* items, const uint32_t* hdr, const uint64_t counts[3]) {
    if (counts[0] >= (1ull << 33) || counts[1] >= (1ull << 31) || counts[2] >= (1ull << 31))
        return set_error(RDST_ERR_ARG, "segments: too many segments of one class for one launch");
    return launch_classes(c, items, hdr, counts);
}

extern "C" int rdst_hip_topk_segments_device(const void* dev_keys, uint64_t len, const uint64_t* offsets, uint64_t n_segments, uint64_t k,
                                             void* dev_out_keys, void* dev_out_index, uint32_t index_bytes, void* dev_scratch, uint64_t scratch_bytes,
                                             uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, uint32_t flags, void* stream) {
    if (int rc = rdst_internal::rank_check_head("topk", dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (flags & ~RDST_TOPK_LARGEST) return set_error(RDST_ERR_ARG, "topk: unknown flag bits");
    if (k == 0 || n_segments == 0) return RDST_OK;
    // the table: its own errors, and the counts (a work list that does not fit capacity 0 is the expected answer)
    if (dev_out_index == nullptr) index_bytes = 0;
    const bool index_ok = rdst_args::index_widths_ok(elem_bytes, index_bytes);
    uint64_t counts[4] = {0, 0, 0, 0}, longest_far = 0;
    int rc = rdst_topk_segments_plan(offsets, n_segments, len, k, elem_bytes, index_ok ? index_bytes : 0, nullptr, 0, counts, &longest_far);
    const uint64_t total = counts[0] + counts[1] + counts[2] + counts[3];
    if (rc != RDST_OK && !(rc == RDST_ERR_ARG && total > 0)) return rc;
    if ((rc = rdst_internal::rank_check_outputs("topk", dev_out_keys, dev_out_index, &index_bytes, dev_scratch, elem_bytes))) return rc;
    uint64_t longest = 0;
    for (uint64_t s = 0; s < n_segments; ++s) longest = std::max(longest, offsets[s + 1] - offsets[s]);
    if (scratch_bytes < rdst_hip_topk_segments_scratch_bytes(n_segments, longest, k, elem_bytes, index_bytes))
        return set_error(RDST_ERR_ARG, "topk: scratch_bytes is below rdst_hip_topk_segments_scratch_bytes(n_segments, longest segment, k, elem_bytes, index_bytes)");
    if (total == 0) return RDST_OK;  // every segment is empty
    std::vector<rdst_segment_item> items((size_t)total);
    if ((rc = rdst_topk_segments_plan(offsets, n_segments, len, k, elem_bytes, index_bytes, items.data(), total, counts, &longest_far))) return rc;
    if (counts[1] >= (1ull << 31) || counts[2] >= (1ull << 31)) return set_error(RDST_ERR_ARG, "segments: too many block-class segments for one launch");
    const SegTopkCall c{dev_keys, k, dev_out_keys, dev_out_index, index_bytes, elem_bytes, kind, (flags & RDST_TOPK_LARGEST) != 0, static_cast<hipStream_t>(stream)};
    int cus = 0, dev = 0;
    if ((rc = rdst_internal::device_cus(&cus))) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    const uint64_t batched = counts[0] + counts[1] + counts[2];
    if (batched) {
        RDST_HIP_TRY(hipGetDevice(&dev));
        if ((rc = rdst_internal::profile_open_run(c.s))) return rc;
        if ((rc = rdst_internal::stage_segment_items(dev, items.data(), (size_t)batched, dev_scratch, c.s))) return rc;
        if ((rc = launch_classes(c, static_cast<const rdst_segment_item*>(dev_scratch), nullptr, counts))) return rc;
    }
    // far segments one after another, each by the whole-array route (no copy to the host, no wait), in the scratch behind the table
    char* far_scratch = static_cast<char*>(dev_scratch) + L::table_bytes(n_segments);
    for (uint64_t i = batched; i < total; ++i) {
        const uint32_t sg = items[i].seg;
        const uint64_t start = offsets[sg], n = offsets[sg + 1] - start, row = (uint64_t)sg * k;
        rc = rdst_internal::topk_slice_locked(static_cast<const char*>(dev_keys) + start * elem_bytes, n, std::min(k, n),
                                              static_cast<char*>(dev_out_keys) + row * elem_bytes,
                                              dev_out_index ? static_cast<char*>(dev_out_index) + row * index_bytes : nullptr, index_bytes, far_scratch,
                                              elem_bytes, kind, c.largest, cus, c.s);
        if (rc) return rc;
    }
    return RDST_OK;
}
