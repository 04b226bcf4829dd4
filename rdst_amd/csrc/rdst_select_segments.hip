// rdst_select_segments.hip — the segmented select: the keys at given ranks of every segment of one array, with their
// segment-local positions if asked for, without sorting the array (rdst_hip_select_segments_device; include/rdst_hip.h,
// DESIGN.md §2k).  Slot i of row s of the outputs holds what rdst_hip_select_device gives for segment s at the rank that
// ranks[i] stands for in a segment of that length (rdst_rank_rule.h), bit for bit.
//
// The work list is the segmented partial sort's with k = 1 (rdst_topk_segments_plan, rdst_segments.cpp): the class of a segment
// follows from its length alone.  The rank specs travel as a kernel argument, MAX_RANKS per round; a longer list is served in
// rounds over the same items.
//
//   select_segment_wave_kernel     one WAVE per segment of up to wave_max keys, four segments per workgroup, and one WORKGROUP
//   select_segment_block_kernel    per segment of up to block_max keys: the level loops of the segmented partial sort
//                                  (rdst_segments_device.h) order the whole segment, the position generated beside each key
//                                  only when an index is asked for.  A 32-lane step resolves the specs against n_s; the
//                                  thread that holds sorted rank r stores it to every slot whose resolved rank is r.
//   select_segment_stream_kernel   one workgroup of 1 024 threads per segment of up to stream_max keys.  The specs are resolved
//                                  and ordered ascending (a 32-lane rank-by-counting, ties by slot) and served in that order.
//                                  A rank outside [lo, lo + filled), what the LDS stage holds, runs the partial sort's 12-bit
//                                  radix select on the mapped key from the root, a digit per read (L2 after the first), until
//                                  m <= TILE keys lie on its prefix or the digits are exhausted: the keys BEFORE the prefix
//                                  are only counted, never staged.  One more read collects, in position order, the keys on
//                                  the prefix into the stage; the block class's level loop orders them; lo = c_below,
//                                  filled = m, and every rank inside is answered without another read.  Digits exhausted
//                                  with m > TILE: the keys on the prefix are equal, the key is the prefix itself, and the
//                                  position of rank r is that of the (r - c_below)-th of them in position order: the read
//                                  collects the window of TILE ordinals that holds it, unsorted, and ranks in the same
//                                  window share it.
//   far                            everything longer, one segment after another through rdst_hip_select_device's own route
//                                  (rdst_internal::select_slice_locked) with the ranks the host resolved, in the part of the
//                                  scratch behind the item table.
//
// Each of the three kernels is one body (select_segment_*_body) under two entries: the kernel the host-table entry launches
// with the counts it knows, and a ..._counted_kernel that reads its item range from the plan header in device memory
// (rdst_hip_select_segments_device_offsets, rdst_select_segments_offsets.hip).  Both entries go through
// rdst_internal::select_segments_launch_locked, which serves the rounds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <exception>
#include <mutex>
#include <vector>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_device.h"
#include "rdst_rank_rule.h"
#include "rdst_segments_layout.h"
#include "rdst_segments_device.h"

namespace {

using rdst_internal::launch;
using rdst_internal::set_error;

constexpr uint32_t MAX_RANKS = L::SELECT_SEGMENTS_MAX_RANKS;
constexpr uint32_t NO_RANK = 0xFFFFFFFFu;  // a spec the segment has no element for (no batched segment is that long)
static_assert(MAX_RANKS == 32, "one lane of a 32-lane step per spec");

struct RankSpecs {  // one round's specs: a kernel argument.  Spec i of the round belongs to slot slot0 + i of every row.
    uint32_t n, slot0;
    rdst_rank_spec spec[MAX_RANKS];
};

// the rank spec `i` of the round stands for in a segment of n keys, or NO_RANK
__device__ __forceinline__ uint32_t resolved_rank(const RankSpecs& rs, uint32_t i, uint32_t n) {
    uint64_t r = 0;
    return i < rs.n && rdst_rank_rule::resolve(rs.spec[i], n, &r) ? (uint32_t)r : NO_RANK;
}

// ---- wave class --------------------------------------------------------------------------------------------------------------

template <typename K, bool IDX>
__device__ __forceinline__ void select_segment_wave_body(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items, uint32_t n_items,
                                                         const Rows<K>& o, const RankSpecs& rs) {
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
    const uint32_t mine = resolved_rank(rs, (uint32_t)lane, n);  // lanes 0 .. 31 resolve a spec each (below n, or none)
    for (uint32_t j = 0; j < rs.n; ++j) {                        // wave-uniform
        const uint32_t r = (uint32_t)__shfl((int)mine, (int)j);
        if (r != NO_RANK && (r & 63u) == (uint32_t)lane) {  // this lane holds the ranks lane, 64 + lane, ...: one lane goes on
#pragma unroll
            for (int i = 0; i < KPT; ++i)
                if ((uint32_t)i == r >> 6) store_rank<K, IDX>(o, it.seg, rs.slot0 + j, mk[i], mv[i]);
        }
    }
}

template <typename K, bool IDX>
__global__ __launch_bounds__(SEG_WAVES * 64) void select_segment_wave_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                              uint32_t n_items, const Rows<K> o, const RankSpecs rs) {
    select_segment_wave_body<K, IDX>(keys, items, n_items, o, rs);
}

// ---- block class -------------------------------------------------------------------------------------------------------------

template <typename K, bool IDX>
__device__ __forceinline__ void select_segment_block_body(const K* __restrict__ keys, const rdst_segment_item it, const Rows<K> o, const RankSpecs rs) {
    constexpr int KPT = BlockLds<K, IDX>::KPT;
    constexpr uint32_t TILE = BlockLds<K, IDX>::TILE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_rank[MAX_RANKS];
    const BlockLds<K, IDX> lds(smem);
    const uint32_t n = it.len < TILE ? it.len : TILE;  // (the plan never hands this class a longer one)
    const K* seg = keys + it.start;
    const int rounds = (int)((n + BLOCK_THREADS - 1) / BLOCK_THREADS);
    const uint32_t wbase = (threadIdx.x >> 6) * 64u * (uint32_t)rounds + (threadIdx.x & 63u);
    if (threadIdx.x < MAX_RANKS) s_rank[threadIdx.x] = resolved_rank(rs, threadIdx.x, n);  // (block_order's barriers stand before the reads)
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
    for (uint32_t j = 0; j < rs.n; ++j) {  // block-uniform
        const uint32_t at = s_rank[j] - wbase;  // this thread holds the ranks wbase, wbase + 64, ...: one thread of the workgroup goes on
        if (s_rank[j] != NO_RANK && (at & 63u) == 0 && (at >> 6) < (uint32_t)rounds) {
#pragma unroll
            for (int i = 0; i < KPT; ++i)
                if ((uint32_t)i == at >> 6) store_rank<K, IDX>(o, it.seg, rs.slot0 + j, mk[i], mv[i]);
        }
    }
}

template <typename K, bool IDX>
__global__ __launch_bounds__(BLOCK_THREADS) void select_segment_block_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                             const Rows<K> o, const RankSpecs rs) {
    select_segment_block_body<K, IDX>(keys, items[blockIdx.x], o, rs);  // the grid is exactly this class's items
}

// ---- stream class ------------------------------------------------------------------------------------------------------------

// Nothing below assumes n <= stream_max: n, m, c_below, the ordinals and every counter are u32 and n < 2^32;
// the asynchronous device-offsets entry hands it segments of any length.
template <typename K, bool IDX>
__device__ __forceinline__ void select_segment_stream_body(const K* __restrict__ keys, const rdst_segment_item it, const Rows<K> o, const RankSpecs rs) {
    constexpr int KPT = BlockLds<K, IDX>::KPT;
    constexpr uint32_t TILE = BlockLds<K, IDX>::TILE;
    constexpr uint32_t BITS = 8 * sizeof(K), DIGIT = sizeof(K) == 1 ? 8 : 12;  // rdst_topk.hip's digits
    constexpr uint32_t SELECT_LEVELS = (BITS + DIGIT - 1) / DIGIT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_wave[2][STREAM_UNROLL][BLOCK_WAVES];
    __shared__ SelectState<K> s_state;
    __shared__ uint32_t s_res[MAX_RANKS];   // the resolved rank of spec i
    __shared__ uint32_t s_rank[MAX_RANKS];  // the resolved ranks, ascending (NO_RANK last)
    __shared__ uint32_t s_slot[MAX_RANKS];  // the spec of each
    static_assert(sizeof(s_wave) + sizeof(SelectState<K>) + 3 * sizeof(s_res) + 16 + SYNC_OR_LDS <= STREAM_STATIC_LDS,
                  "the static LDS stays within what the launch accounts for");
    const BlockLds<K, IDX> lds(smem);
    uint32_t* cnt = lds.wave_hist;
    const uint32_t tid = threadIdx.x;
    const uint32_t n = it.len;
    const SegmentCut<K> cut(keys + it.start, n);

    // ---- the specs against n, then in ascending rank order, ties by slot
    if (tid < MAX_RANKS) s_res[tid] = resolved_rank(rs, tid, n);
    __syncthreads();
    if (tid < MAX_RANKS) {
        const uint32_t mine = s_res[tid];
        uint32_t at = 0;
        for (uint32_t j = 0; j < MAX_RANKS; ++j) {
            const uint32_t other = s_res[j];
            at += other < mine || (other == mine && j < tid) ? 1u : 0u;
        }
        s_rank[at] = mine;
        s_slot[at] = tid;
    }
    __syncthreads();
    uint32_t n_valid = 0;  // block-uniform, like everything the loop below decides on
    while (n_valid < rs.n && s_rank[n_valid] != NO_RANK) ++n_valid;

    uint32_t q = 0;
    while (q < n_valid) {
        const uint32_t r = s_rank[q];  // the lowest rank not answered yet: beyond what the stage holds
        // ---- select: the prefix of the key at rank r, a digit per read
        K pref = 0, pmask = 0;
        uint32_t c_below = 0, m = n;
        for (uint32_t level = 0; level < SELECT_LEVELS && m > TILE; ++level) {  // block-uniform
            const uint32_t hi = BITS - level * DIGIT, lo = hi > DIGIT ? hi - DIGIT : 0u;
            const int shift = (int)lo;
            const uint32_t dmask = (1u << (hi - lo)) - 1u;
            count_digits<K>(cut, o.neg, o.pos, pref, pmask, shift, dmask, cnt);
            uint32_t c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = cnt[4 * tid + j];
            uint32_t run;
            int j;
            if (pick_bucket(c, r + 1 - c_below, &s_wave[0][0][0], &run, &j)) {  // exactly one thread
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
        // ---- what the stage holds next: the ranks [lo, lo + filled)
        const bool equal = m > TILE;  // digits exhausted: every key on the prefix is the prefix
        uint32_t lo = c_below, filled = m;
        if (!equal || IDX) {
            // m <= TILE: all keys on the prefix.  Equal keys, with an index: the window of TILE ordinals that holds rank r.
            const uint32_t first = equal ? (r - c_below) / TILE * TILE : 0u;
            lo = c_below + first;
            filled = m - first < TILE ? m - first : TILE;
            uint32_t tot_b, tot_o;
            __syncthreads();  // (pick_bucket's wave sums lie in s_wave; the answers of the stage before have been read)
            collect_segment<K, IDX, false>(cut, o.neg, o.pos, pref, pmask, 0u, first, TILE, lds.stage, lds.vstage, s_wave, tot_b, tot_o);
            __syncthreads();  // the stage is complete
            if (!equal) {
                const int rounds = (int)((filled + BLOCK_THREADS - 1) / BLOCK_THREADS);
                const uint32_t wbase = (tid >> 6) * 64u * (uint32_t)rounds + (tid & 63u);
                K rk[KPT];
                uint32_t rv[KPT];
                order_stage<K, IDX, KPT>(rk, rv, filled, rounds, lds);
#pragma unroll
                for (int i = 0; i < KPT; ++i) {  // back to the stage, in order (a level that found one digit left it as it was)
                    const uint32_t idx = wbase + i * 64;
                    if (i < rounds && idx < filled) {
                        lds.stage[idx] = rk[i];
                        if constexpr (IDX) lds.vstage[idx] = rv[i];
                    }
                }
                __syncthreads();
            }
        }
        // ---- every rank inside is answered from the stage (keys only, equal keys: from the prefix)
        if (tid >= q && tid < n_valid) {
            const uint32_t at = s_rank[tid] - lo;  // ranks ascend from r >= lo
            if (at < filled) {
                const bool staged = !equal || IDX;
                uint32_t position = 0;
                if constexpr (IDX) position = lds.vstage[at];
                store_rank<K, IDX>(o, it.seg, rs.slot0 + s_slot[tid], staged ? lds.stage[at] : pref, position);
            }
        }
        while (q < n_valid && s_rank[q] - lo < filled) ++q;  // (at least r itself)
    }
}

template <typename K, bool IDX>
__global__ __launch_bounds__(BLOCK_THREADS) void select_segment_stream_kernel(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items,
                                                                              const Rows<K> o, const RankSpecs rs) {
    select_segment_stream_body<K, IDX>(keys, items[blockIdx.x], o, rs);  // the grid is exactly this class's items
}

// ---- the same three bodies with their item range read from the plan header in device memory (device-resident offsets) ----------
//
// rdst_topk_segments_offsets.hip writes the header (rdst_segments_layout.h: TopkPlanHeader) and the item table: the plan of
// the segmented partial sort with k = 1.  The grids are bounds the host can state without the counts; waves and workgroups
// past the count return before any barrier.  With a flag up the RUN counts are zero and nothing runs.
template <typename K, bool IDX>
__global__ __launch_bounds__(SEG_WAVES * 64) void select_segment_wave_counted_kernel(const K* __restrict__ keys,
                                                                                      const rdst_segment_item* __restrict__ items,
                                                                                      const uint32_t* __restrict__ hdr, const Rows<K> o, const RankSpecs rs) {
    select_segment_wave_body<K, IDX>(keys, items, hdr[L::HDR_TOPK_RUN_WAVE], o, rs);
}

template <typename K, bool IDX>
__global__ __launch_bounds__(BLOCK_THREADS) void select_segment_block_counted_kernel(const K* __restrict__ keys,
                                                                                     const rdst_segment_item* __restrict__ items,
                                                                                     const uint32_t* __restrict__ hdr, const Rows<K> o, const RankSpecs rs) {
    if (blockIdx.x >= hdr[L::HDR_TOPK_RUN_BLOCK]) return;  // block-uniform
    select_segment_block_body<K, IDX>(keys, items[hdr[L::HDR_TOPK_N_WAVE] + blockIdx.x], o, rs);
}

template <typename K, bool IDX>
__global__ __launch_bounds__(BLOCK_THREADS) void select_segment_stream_counted_kernel(const K* __restrict__ keys,
                                                                                      const rdst_segment_item* __restrict__ items,
                                                                                      const uint32_t* __restrict__ hdr, const Rows<K> o, const RankSpecs rs) {
    if (blockIdx.x >= hdr[L::HDR_TOPK_RUN_STREAM]) return;  // block-uniform
    select_segment_stream_body<K, IDX>(keys, items[hdr[L::HDR_TOPK_N_WAVE] + hdr[L::HDR_TOPK_N_BLOCK] + blockIdx.x], o, rs);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

using SegSelectCall = rdst_internal::SelectSegmentsCall;

// One round over the item table in device memory: wave class first, then block class, then stream class.  `hdr` == nullptr:
// the host knows the counts, counts[0 .. 2], and the classes follow one another in `items`.  With `hdr`, the plan header in
// device memory: the counts stand there, and counts[0 .. 2] are the host's bounds on them, for the grids alone.
template <typename K, bool IDX>
int launch_round_t(const SegSelectCall& c, const rdst_segment_item* items, const uint32_t* hdr, const uint64_t counts[3], const RankSpecs& rs) {
    constexpr size_t wave_lds = wave_lds_bytes(sizeof(K), IDX), block_lds = block_lds_bytes(sizeof(K), IDX);
    static_assert(wave_lds <= LDS_LIMIT && block_lds + STREAM_STATIC_LDS <= LDS_LIMIT, "a workgroup's LDS stays within 160 KiB");
    unsigned __int128 neg, pos;
    rdst_internal::key_xor_masks(c.kind, (uint32_t)sizeof(K), &neg, &pos);
    Rows<K> o{static_cast<K*>(c.out_keys), c.out_index, c.index_bytes, c.n_ranks, (K)neg, (K)pos};
    if (c.largest) {  // the complement of the mapped key: both masks complemented
        o.neg = (K)~o.neg;
        o.pos = (K)~o.pos;
    }
    const K* keys = static_cast<const K*>(c.keys);
    const dim3 wave_grid((uint32_t)((counts[0] + SEG_WAVES - 1) / SEG_WAVES)), block_grid((uint32_t)counts[1]), stream_grid((uint32_t)counts[2]);
    int rc;
    if (counts[0]) {
        rc = hdr ? launch("select_segment_wave_counted_kernel", select_segment_wave_counted_kernel<K, IDX>, wave_grid, dim3(SEG_WAVES * 64), wave_lds, c.s,
                          keys, items, hdr, o, rs)
                 : launch("select_segment_wave_kernel", select_segment_wave_kernel<K, IDX>, wave_grid, dim3(SEG_WAVES * 64), wave_lds, c.s, keys, items,
                          (uint32_t)counts[0], o, rs);
        if (rc) return rc;
        if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_SEGMENTS))) return rc;
    }
    if (counts[1]) {
        rc = hdr ? launch("select_segment_block_counted_kernel", select_segment_block_counted_kernel<K, IDX>, block_grid, dim3(BLOCK_THREADS), block_lds,
                          c.s, keys, items, hdr, o, rs)
                 : launch("select_segment_block_kernel", select_segment_block_kernel<K, IDX>, block_grid, dim3(BLOCK_THREADS), block_lds, c.s, keys,
                          items + counts[0], o, rs);
        if (rc) return rc;
        if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_SEGMENTS | (1u << 8)))) return rc;
    }
    if (counts[2]) {
        rc = hdr ? launch("select_segment_stream_counted_kernel", select_segment_stream_counted_kernel<K, IDX>, stream_grid, dim3(BLOCK_THREADS), block_lds,
                          c.s, keys, items, hdr, o, rs)
                 : launch("select_segment_stream_kernel", select_segment_stream_kernel<K, IDX>, stream_grid, dim3(BLOCK_THREADS), block_lds, c.s, keys,
                          items + counts[0] + counts[1], o, rs);
        if (rc) return rc;
        if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_SEGMENTS | (2u << 8)))) return rc;
    }
    return RDST_OK;
}

int launch_round(const SegSelectCall& c, const rdst_segment_item* items, const uint32_t* hdr, const uint64_t counts[3], const RankSpecs& rs) {
    if (c.index_bytes != 0)
        return c.elem_bytes == 4 ? launch_round_t<uint32_t, true>(c, items, hdr, counts, rs) : launch_round_t<uint64_t, true>(c, items, hdr, counts, rs);
    switch (c.elem_bytes) {
        case 1: return launch_round_t<uint8_t, false>(c, items, hdr, counts, rs);
        case 2: return launch_round_t<uint16_t, false>(c, items, hdr, counts, rs);
        case 4: return launch_round_t<uint32_t, false>(c, items, hdr, counts, rs);
        case 8: return launch_round_t<uint64_t, false>(c, items, hdr, counts, rs);
        default: return launch_round_t<u128, false>(c, items, hdr, counts, rs);
    }
}

}  // namespace

// Every round of c.n_ranks specs, MAX_RANKS a round, over the same items: slot i keeps its place in the row.
int rdst_internal::select_segments_launch_locked(const SelectSegmentsCall& c, const rdst_segment_item* items, const uint32_t* hdr,
                                                 const uint64_t counts[3], const rdst_rank_spec* ranks) {
    if (counts[0] >= (1ull << 33) || counts[1] >= (1ull << 31) || counts[2] >= (1ull << 31))
        return set_error(RDST_ERR_ARG, "segments: too many segments of one class for one launch");
    for (uint64_t start = 0; start < c.n_ranks; start += MAX_RANKS) {
        RankSpecs rs{};
        rs.n = (uint32_t)std::min<uint64_t>(MAX_RANKS, c.n_ranks - start);
        rs.slot0 = (uint32_t)start;
        for (uint32_t i = 0; i < rs.n; ++i) rs.spec[i] = ranks[start + i];
        if (int rc = launch_round(c, items, hdr, counts, rs)) return rc;
    }
    return RDST_OK;
}

extern "C" int rdst_hip_select_segments_device(const void* dev_keys, uint64_t len, const uint64_t* offsets, uint64_t n_segments,
                                               const rdst_rank_spec* ranks, uint64_t n_ranks, void* dev_out_keys, void* dev_out_index,
                                               uint32_t index_bytes, void* dev_scratch, uint64_t scratch_bytes, uint32_t elem_bytes, rdst_key_kind kind,
                                               uint32_t levels, uint32_t flags, void* stream) {
    if (int rc = rdst_internal::rank_check_head("select", dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (flags & ~RDST_TOPK_LARGEST) return set_error(RDST_ERR_ARG, "select: unknown flag bits");
    if (n_ranks == 0 || n_segments == 0) return RDST_OK;
    // the table: its own errors, and the counts (a work list that does not fit capacity 0 is the expected answer)
    if (dev_out_index == nullptr) index_bytes = 0;
    const bool index_ok = rdst_args::index_widths_ok(elem_bytes, index_bytes);
    uint64_t counts[4] = {0, 0, 0, 0}, longest_far = 0;
    int rc = rdst_topk_segments_plan(offsets, n_segments, len, 1, elem_bytes, index_ok ? index_bytes : 0, nullptr, 0, counts, &longest_far);
    const uint64_t total = counts[0] + counts[1] + counts[2] + counts[3];
    if (rc != RDST_OK && !(rc == RDST_ERR_ARG && total > 0)) return rc;
    if (ranks == nullptr) return set_error(RDST_ERR_ARG, "select: null ranks");
    for (uint64_t i = 0; i < n_ranks; ++i)
        if (!rdst_rank_rule::spec_ok(ranks[i])) {
            char msg[160];
            snprintf(msg, sizeof msg, "select: ranks[%llu] is not a rank spec (num <= den for a quantile, mode 0 .. 2, 0 for an absolute rank, reserved 0)",
                     (unsigned long long)i);
            return set_error(RDST_ERR_ARG, msg);
        }
    if ((rc = rdst_internal::rank_check_outputs("select", dev_out_keys, dev_out_index, &index_bytes, dev_scratch, elem_bytes))) return rc;
    uint64_t longest = 0;
    for (uint64_t s = 0; s < n_segments; ++s) longest = std::max(longest, offsets[s + 1] - offsets[s]);
    if (scratch_bytes < rdst_hip_select_segments_scratch_bytes(n_segments, longest, n_ranks, elem_bytes, index_bytes))
        return set_error(RDST_ERR_ARG,
                         "select: scratch_bytes is below rdst_hip_select_segments_scratch_bytes(n_segments, longest segment, n_ranks, elem_bytes, index_bytes)");
    if (total == 0) return RDST_OK;  // every segment is empty
    // nothing may be thrown through the C ABI
    // per far segment, n_ranks places each: the ranks it has, their slots, their ascending order; far_have: how many it has
    std::vector<rdst_segment_item> items;
    std::vector<uint64_t> far_ranks, far_slots, far_order, far_have;
    try {
        items.resize((size_t)total);
        if (counts[3]) {
            far_ranks.resize((size_t)(counts[3] * n_ranks));
            far_slots.resize((size_t)(counts[3] * n_ranks));
            far_order.resize((size_t)(counts[3] * n_ranks));
            far_have.resize((size_t)counts[3]);
        }
    } catch (const std::exception&) {
        return set_error(RDST_ERR_ARG, "select: no host memory for the work list (16 bytes per segment) and the far segments' ranks (24 bytes per rank each)");
    }
    if ((rc = rdst_topk_segments_plan(offsets, n_segments, len, 1, elem_bytes, index_bytes, items.data(), total, counts, &longest_far))) return rc;
    // the far segments' ranks, resolved and ordered here, before the mutex is taken; a spec the segment has no element for is left out
    const uint64_t batched = counts[0] + counts[1] + counts[2];
    for (uint64_t f = 0; f < counts[3]; ++f) {
        const uint32_t sg = items[batched + f].seg;
        const uint64_t n = offsets[sg + 1] - offsets[sg];
        uint64_t* fr = far_ranks.data() + f * n_ranks;
        uint64_t* fs = far_slots.data() + f * n_ranks;
        uint64_t have = 0;
        for (uint64_t j = 0; j < n_ranks; ++j)
            if (rdst_rank_rule::resolve(ranks[j], n, &fr[have])) fs[have++] = j;
        far_have[f] = have;
        if ((rc = rdst_internal::order_ranks(fr, have, far_order.data() + f * n_ranks))) return rc;
    }
    const SegSelectCall c{dev_keys, n_ranks, dev_out_keys, dev_out_index, index_bytes, elem_bytes, kind, (flags & RDST_TOPK_LARGEST) != 0,
                          static_cast<hipStream_t>(stream)};
    int cus = 0, dev = 0;
    if ((rc = rdst_internal::device_cus(&cus))) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    if (batched) {
        RDST_HIP_TRY(hipGetDevice(&dev));
        if ((rc = rdst_internal::profile_open_run(c.s))) return rc;
        if ((rc = rdst_internal::stage_segment_items(dev, items.data(), (size_t)batched, dev_scratch, c.s))) return rc;
        if ((rc = rdst_internal::select_segments_launch_locked(c, static_cast<const rdst_segment_item*>(dev_scratch), nullptr, counts, ranks))) return rc;
    }
    // far segments one after another, each by the whole-array select (no copy to the host, no wait), in the scratch behind the
    // table
    char* far_scratch = static_cast<char*>(dev_scratch) + L::table_bytes(n_segments);
    for (uint64_t f = 0; f < counts[3]; ++f) {
        const uint32_t sg = items[batched + f].seg;
        const uint64_t start = offsets[sg], n = offsets[sg + 1] - start, row = (uint64_t)sg * n_ranks, have = far_have[f];
        if (have == 0) continue;
        rc = rdst_internal::select_slice_locked(static_cast<const char*>(dev_keys) + start * elem_bytes, n, far_ranks.data() + f * n_ranks,
                                                far_slots.data() + f * n_ranks, far_order.data() + f * n_ranks, have,
                                                static_cast<char*>(dev_out_keys) + row * elem_bytes,
                                                dev_out_index ? static_cast<char*>(dev_out_index) + row * index_bytes : nullptr, index_bytes, far_scratch, 0,
                                                elem_bytes, kind, c.largest, cus, c.s);
        if (rc) return rc;
    }
    return RDST_OK;
}
