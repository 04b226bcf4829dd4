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

namespace {

namespace L = rdst_segments_layout;
using rdst_internal::launch;
using rdst_internal::set_error;

constexpr int RADIX = 256;
constexpr int SEG_WAVES = 4;  // segments per workgroup of the wave class
constexpr int BLOCK_THREADS = L::BLOCK_THREADS;
constexpr int BLOCK_WAVES = BLOCK_THREADS / 64;
constexpr uint32_t COUNTERS = 4096;  // the select's count table: it lies over the level loop's per-wave digit tables
static_assert(COUNTERS == BLOCK_WAVES * RADIX && COUNTERS == 4 * BLOCK_THREADS, "one table in the place of the other, four counters per thread");
constexpr int STREAM_UNROLL = 4;  // 16-byte loads in flight per thread
constexpr size_t LDS_LIMIT = 160 << 10;
constexpr size_t STREAM_STATIC_LDS = 1024;  // bound on the stream kernel's static LDS (wave totals, select state)

constexpr size_t val_bytes(bool idx) { return idx ? sizeof(uint32_t) : 0; }
constexpr size_t wave_lds_bytes(size_t key_bytes, bool idx) {  // per workgroup: tables, then key stages, then position stages
    return (size_t)SEG_WAVES * (RADIX * sizeof(uint32_t) + 64 * L::wave_kpt(key_bytes) * (key_bytes + val_bytes(idx)));
}
constexpr size_t block_lds_bytes(size_t key_bytes, bool idx) {
    return (size_t)BLOCK_WAVES * 1024 + 16 + (key_bytes + val_bytes(idx)) * BLOCK_THREADS * L::block_kpt(key_bytes, val_bytes(idx));
}

// orders this wave's LDS accesses: nothing moves across it, in the compiler or in the wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Where the results go: row `seg` of both outputs starts at element seg * k.
template <typename K>
struct Rows {
    K* keys;
    void* index;           // unused without an index
    uint32_t index_bytes;  // 4 or 8: a position is widened at the store
    uint64_t k;
    K neg, pos;            // the xor masks of the key map (complemented for RDST_TOPK_LARGEST)
};

template <typename K, bool IDX>
__device__ __forceinline__ void store_rank(const Rows<K>& o, uint32_t seg, uint32_t rank, K mapped, uint32_t position) {
    const uint64_t at = (uint64_t)seg * o.k + rank;
    o.keys[at] = unmap_any<K>(mapped, o.neg, o.pos);
    if constexpr (IDX) {
        if (o.index_bytes == 8) static_cast<uint64_t*>(o.index)[at] = position;
        else static_cast<uint32_t*>(o.index)[at] = position;
    }
}

// ---- wave class --------------------------------------------------------------------------------------------------------------

template <typename K, bool IDX>
__device__ __forceinline__ void topk_segment_wave_body(const K* __restrict__ keys, const rdst_segment_item* __restrict__ items, uint32_t n_items,
                                                       const Rows<K> o) {
    constexpr int LEVELS = (int)sizeof(K);
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
    const uint32_t live = (uint32_t)rounds * 64u;
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
    for (int level = 0; level < LEVELS; ++level) {
        const int shift = level * 8, bit0 = shift & 31;
#pragma unroll
        for (int j = 0; j < 4; ++j) tbl[lane + 64 * j] = 0;
        wave_sync();
#pragma unroll
        for (int i = 0; i < KPT; ++i)
            if (i < rounds) atomicAdd(&tbl[digit_of(mk[i], shift)], 1u);
        wave_sync();
        // lane l owns the bins 4 l .. 4 l + 3
        uint32_t c[4], sum = 0;
        bool all_one = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = tbl[4 * lane + j];
            sum += c[j];
            all_one |= c[j] == live;
        }
        if (__builtin_amdgcn_ballot_w64(all_one) != 0) {  // one digit holds everything: wave-uniform; the table is re-zeroed at the top
            wave_sync();
            continue;
        }
        uint32_t incl = sum;
#pragma unroll
        for (int o2 = 1; o2 < 64; o2 <<= 1) {
            const uint32_t y = __shfl_up(incl, o2);
            if (lane >= o2) incl += y;
        }
        uint32_t run = incl - sum;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tbl[4 * lane + j] = run;
            run += c[j];
        }
        wave_sync();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if (i < rounds) {  // wave-uniform: all 64 lanes rank (peers_below needs them)
                uint32_t* slot = &tbl[digit_of(mk[i], shift)];
                const uint32_t b = *slot;
                const uint32_t below = peers_below(digit_word<K>(mk[i], shift), bit0);
                wave_sync();
                atomicAdd(slot, 1u);
                stage[b + below] = mk[i];
                if constexpr (IDX) vstage[b + below] = mv[i];
                wave_sync();
            }
        }
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if (i < rounds) {
                mk[i] = stage[i * 64 + lane];
                if constexpr (IDX) mv[i] = vstage[i * 64 + lane];
            }
        }
        wave_sync();
    }
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

// ---- block class: the level loop, shared with the stream class ------------------------------------------------------------------

// What a workgroup's dynamic LDS holds (segment_block_body's layout).
template <typename K, bool IDX>
struct BlockLds {
    static constexpr int KPT = L::block_kpt(sizeof(K), val_bytes(IDX));
    static constexpr uint32_t TILE = (uint32_t)BLOCK_THREADS * KPT;
    uint32_t* wave_hist;  // [BLOCK_WAVES][256]; the stream class's select counts in it first
    uint32_t* s_sum;      // [4]
    K* stage;             // [TILE]
    uint32_t* vstage;     // [TILE] with an index
    __device__ explicit BlockLds(unsigned char* smem)
        : wave_hist(reinterpret_cast<uint32_t*>(smem)),
          s_sum(reinterpret_cast<uint32_t*>(smem + BLOCK_WAVES * 1024)),
          stage(reinterpret_cast<K*>(smem + BLOCK_WAVES * 1024 + 16)),
          vstage(reinterpret_cast<uint32_t*>(smem + BLOCK_WAVES * 1024 + 16 + sizeof(K) * TILE)) {}
};

// Orders the workgroup's keys (and positions): key index = wave * 64 * rounds + round * 64 + lane, before and after.
// `rounds` is block-uniform; the stage may hold anything (every thread has what it needs of it in registers).
template <typename K, bool IDX, int KPT>
__device__ __forceinline__ void block_order(K (&mk)[KPT], uint32_t (&mv)[KPT], int rounds, const BlockLds<K, IDX>& lds) {
    constexpr int LEVELS = (int)sizeof(K);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t live = (uint32_t)rounds * BLOCK_THREADS;
    const uint32_t wbase = (uint32_t)wave * 64u * (uint32_t)rounds + (uint32_t)lane;
    uint32_t* wave_hist = lds.wave_hist;
    uint32_t* wh = wave_hist + wave * RADIX;
    for (int level = 0; level < LEVELS; ++level) {
        const int shift = level * 8, bit0 = shift & 31;
#pragma unroll
        for (int j = 0; j < 4; ++j) wh[lane + 64 * j] = 0;
#pragma unroll
        for (int i = 0; i < KPT; ++i)
            if (i < rounds) atomicAdd(&wh[digit_of(mk[i], shift)], 1u);
        __syncthreads();
        uint32_t cw[BLOCK_WAVES], count_d = 0;
        if (tid < RADIX) {
#pragma unroll
            for (int w = 0; w < BLOCK_WAVES; ++w) { cw[w] = wave_hist[w * RADIX + tid]; count_d += cw[w]; }
        }
        const bool trivial = __syncthreads_or(tid < RADIX && count_d == live) != 0;  // one digit holds everything
        if (trivial) continue;  // block-uniform; the tables are re-zeroed at the top
        uint32_t incl = count_d;
#pragma unroll
        for (int o2 = 1; o2 < 64; o2 <<= 1) {
            const uint32_t y = __shfl_up(incl, o2);
            if (lane >= o2) incl += y;
        }
        if (tid < RADIX && lane == 63) lds.s_sum[wave] = incl;
        __syncthreads();
        if (tid < RADIX) {
            uint32_t run = incl - count_d;
            for (int w = 0; w < wave; ++w) run += lds.s_sum[w];
#pragma unroll
            for (int w = 0; w < BLOCK_WAVES; ++w) { wave_hist[w * RADIX + tid] = run; run += cw[w]; }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if (i < rounds) {  // block-uniform
                uint32_t* slot = &wh[digit_of(mk[i], shift)];
                const uint32_t b = *slot;
                const uint32_t below = peers_below(digit_word<K>(mk[i], shift), bit0);
                __builtin_amdgcn_wave_barrier();
                atomicAdd(slot, 1u);
                lds.stage[b + below] = mk[i];
                if constexpr (IDX) lds.vstage[b + below] = mv[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if (i < rounds) {
                mk[i] = lds.stage[wbase + i * 64];
                if constexpr (IDX) mv[i] = lds.vstage[wbase + i * 64];
            }
        }
        __syncthreads();
    }
}

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

template <typename K>
struct alignas(16) KeyVec {
    static constexpr int N = 16 / (int)sizeof(K);
    K e[N];
};

// A plain 16-byte load: the segment is read two to four times by this one workgroup, and the later reads should find it in L2.
template <typename K>
__device__ __forceinline__ KeyVec<K> load_vec(const K* p) {  // p is 16-byte aligned
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 raw = *reinterpret_cast<const u32x4*>(p);
    KeyVec<K> v;
    __builtin_memcpy(&v, &raw, 16);
    return v;
}

template <typename K>
struct SelectState {  // block-uniform, in LDS between two barriers
    K pref, pmask;
    uint32_t c_below, m;
};

// One trip of the ordered compaction: G groups of E elements per thread, position order = (group, thread, element).  Keeps
// every key before the prefix and the keys on it while fewer than `lim` of those were kept; a kept element's slot is the
// number of kept elements before it.  tot_b / tot_o: the keys before / on the prefix seen so far (block-uniform).  Every
// thread of the workgroup calls it; one barrier, and `wave_tot` alternates between two buffers from trip to trip.
template <typename K, bool IDX, int G, int E>
__device__ __forceinline__ void collect_trip(const K (&m)[G][E], const bool (&ok)[G], const uint32_t (&pos0)[G], K pref, K pmask, uint32_t lim,
                                             uint32_t tile, K* stage, uint32_t* vstage, uint32_t (*wave_tot)[BLOCK_WAVES], uint32_t& tot_b,
                                             uint32_t& tot_o) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t excl[G];  // (before << 16 | on) over the lower lanes of this wave: at most 64 * 16 each
#pragma unroll
    for (int g = 0; g < G; ++g) {
        uint32_t p = 0;
        if (ok[g]) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const K km = (K)(m[g][e] & pmask);
                p += km < pref ? 0x10000u : (km == pref ? 1u : 0u);
            }
        }
        uint32_t incl = p;
#pragma unroll
        for (int o2 = 1; o2 < 64; o2 <<= 1) {
            const uint32_t y = __shfl_up(incl, o2);
            if (lane >= (uint32_t)o2) incl += y;
        }
        excl[g] = incl - p;
        if (lane == 63) wave_tot[g][wave] = incl;
    }
    __syncthreads();
    uint32_t run_b = tot_b, run_o = tot_o;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        uint32_t gb = 0, go = 0, wb = 0, wo = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)BLOCK_WAVES; ++w) {
            const uint32_t t = wave_tot[g][w];
            gb += t >> 16;
            go += t & 0xFFFFu;
            if (w < wave) {
                wb += t >> 16;
                wo += t & 0xFFFFu;
            }
        }
        uint32_t b = run_b + wb + (excl[g] >> 16), on = run_o + wo + (excl[g] & 0xFFFFu);
        if (ok[g]) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const K km = (K)(m[g][e] & pmask);
                const bool before = km < pref, is_on = km == pref;
                if (before || (is_on && on < lim)) {
                    const uint32_t slot = b + (on < lim ? on : lim);
                    if (slot < tile) {  // (it is: b <= c_below and on <= lim; a store outside the stage is never made)
                        stage[slot] = m[g][e];
                        if constexpr (IDX) vstage[slot] = pos0[g] + (uint32_t)e;
                    }
                }
                b += before ? 1u : 0u;
                on += is_on ? 1u : 0u;
            }
        }
        run_b += gb;
        run_o += go;
    }
    tot_b = run_b;
    tot_o = run_o;
}

template <typename K, bool IDX>
__device__ __forceinline__ void topk_segment_stream_body(const K* __restrict__ keys, const rdst_segment_item it, const Rows<K> o) {
    constexpr int KPT = BlockLds<K, IDX>::KPT;
    constexpr uint32_t TILE = BlockLds<K, IDX>::TILE;
    constexpr uint32_t VEC = KeyVec<K>::N;
    constexpr uint32_t BITS = 8 * sizeof(K), DIGIT = sizeof(K) == 1 ? 8 : 12;  // rdst_topk.hip's digits
    constexpr uint32_t SELECT_LEVELS = (BITS + DIGIT - 1) / DIGIT;
    constexpr uint32_t TRIP = (uint32_t)BLOCK_THREADS * STREAM_UNROLL;  // vectors per trip of the workgroup
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_wave[2][STREAM_UNROLL][BLOCK_WAVES];
    __shared__ SelectState<K> s_state;
    static_assert(sizeof(s_wave) + sizeof(SelectState<K>) + 16 <= STREAM_STATIC_LDS, "the static LDS stays within what the launch accounts for");
    const BlockLds<K, IDX> lds(smem);
    uint32_t* cnt = lds.wave_hist;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t n = it.len;
    const K* seg = keys + it.start;
    uint32_t k = o.k < n ? (uint32_t)o.k : n;
    if (k > TILE) k = TILE;  // (the plan hands this class k <= TILE only)
    // a scalar head up to the first 16-byte boundary, whole 16-byte vectors, a scalar tail
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(seg) & 15u);
    const uint32_t head_want = mis ? (16u - mis) / (uint32_t)sizeof(K) : 0u;
    const uint32_t head = head_want < n ? head_want : n;
    const uint32_t nvec = (n - head) / VEC;
    const uint32_t tail_start = head + nvec * VEC, tail_n = n - tail_start;
    const K* body = seg + head;

    // ---- select: the prefix of the k-th key, a digit per read
    K pref = 0, pmask = 0;
    uint32_t c_below = 0, m = n;
    for (uint32_t level = 0; level < SELECT_LEVELS && c_below + m > TILE; ++level) {  // block-uniform
        const uint32_t hi = BITS - level * DIGIT, lo = hi > DIGIT ? hi - DIGIT : 0u;
        const int shift = (int)lo;
        const uint32_t dmask = (1u << (hi - lo)) - 1u;
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt[tid + (uint32_t)BLOCK_THREADS * j] = 0;
        __syncthreads();
        // One 16-byte vector per lane, all 64 lanes of the wave in every call.  Every key of the wave on one counter (equal keys,
        // a shared digit): ONE add for the wave; otherwise an add per key on the prefix.  The test costs one ballot per vector.
        const auto count_vec = [&](const KeyVec<K>& v, bool ok) {
            uint32_t d[VEC];
            bool hit[VEC], same = ok;
#pragma unroll
            for (uint32_t j = 0; j < VEC; ++j) {
                const K mk = map_key<K>(v.e[j], o.neg, o.pos);
                hit[j] = ok && (K)(mk & pmask) == pref;
                d[j] = (uint32_t)(mk >> shift) & dmask;
                same = same && hit[j] && d[j] == d[0];
            }
            const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[0]);
            if (__builtin_amdgcn_ballot_w64(same && d[0] == d0) == ~0ull) {  // wave-uniform
                if (lane == 0) atomicAdd(&cnt[d0], 64u * VEC);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < VEC; ++j)
                    if (hit[j]) atomicAdd(&cnt[d[j]], 1u);
            }
        };
        for (uint64_t base = 0; base < nvec; base += TRIP) {  // block-uniform
            KeyVec<K> vec[STREAM_UNROLL];
            bool ok[STREAM_UNROLL];
#pragma unroll
            for (int u = 0; u < STREAM_UNROLL; ++u) {
                const uint64_t vi = base + (uint64_t)u * BLOCK_THREADS + tid;
                ok[u] = vi < nvec;
                if (ok[u]) vec[u] = load_vec<K>(body + vi * VEC);
                else
                    for (uint32_t j = 0; j < VEC; ++j) vec[u].e[j] = 0;
            }
#pragma unroll
            for (int u = 0; u < STREAM_UNROLL; ++u) count_vec(vec[u], ok[u]);
        }
        if (tid < head + tail_n) {  // head and tail: fewer than 2 * 16 / sizeof(K) <= 32 elements
            const K mk = map_key<K>(seg[tid < head ? tid : tail_start + (tid - head)], o.neg, o.pos);
            if ((K)(mk & pmask) == pref) atomicAdd(&cnt[(uint32_t)(mk >> shift) & dmask], 1u);
        }
        __syncthreads();
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
    uint32_t tot_b = 0, tot_o = 0, parity = 0;
    const auto scalar_trip = [&](uint32_t first, uint32_t count) {  // block-uniform arguments; count <= 16
        const bool ok[1] = {tid < count};
        const K one[1][1] = {{ok[0] ? map_key<K>(seg[first + tid], o.neg, o.pos) : (K)0}};
        const uint32_t pos0[1] = {first + tid};
        collect_trip<K, IDX, 1, 1>(one, ok, pos0, pref, pmask, lim, TILE, lds.stage, lds.vstage, s_wave[parity], tot_b, tot_o);
        parity ^= 1u;
    };
    __syncthreads();  // (pick_bucket's wave sums lie in s_wave)
    if (head) scalar_trip(0, head);
    for (uint64_t base = 0; base < nvec; base += TRIP) {  // block-uniform
        K mk[STREAM_UNROLL][VEC];
        bool ok[STREAM_UNROLL];
        uint32_t pos0[STREAM_UNROLL];
#pragma unroll
        for (int u = 0; u < STREAM_UNROLL; ++u) {
            const uint64_t vi = base + (uint64_t)u * BLOCK_THREADS + tid;
            ok[u] = vi < nvec;
            pos0[u] = head + (uint32_t)vi * VEC;
            KeyVec<K> v;
            if (ok[u]) v = load_vec<K>(body + vi * VEC);
            else
                for (uint32_t j = 0; j < VEC; ++j) v.e[j] = 0;
#pragma unroll
            for (uint32_t j = 0; j < VEC; ++j) mk[u][j] = map_key<K>(v.e[j], o.neg, o.pos);
        }
        collect_trip<K, IDX, STREAM_UNROLL, (int)VEC>(mk, ok, pos0, pref, pmask, lim, TILE, lds.stage, lds.vstage, s_wave[parity], tot_b, tot_o);
        parity ^= 1u;
    }
    if (tail_n) scalar_trip(tail_start, tail_n);

    // ---- order the stage, store the first k
    const uint32_t kept_on = tot_o < lim ? tot_o : lim;
    const uint32_t filled = tot_b + kept_on < TILE ? tot_b + kept_on : TILE;
    const int rounds = (int)((filled + BLOCK_THREADS - 1) / BLOCK_THREADS);
    const uint32_t wbase = (tid >> 6) * 64u * (uint32_t)rounds + lane;
    __syncthreads();  // the stage is complete
    K rk[KPT];
    uint32_t rv[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = wbase + i * 64;
        const bool real = i < rounds && idx < filled;
        rk[i] = real ? lds.stage[idx] : (K) ~(K)0;
        rv[i] = 0;
        if constexpr (IDX)
            if (real) rv[i] = lds.vstage[idx];
    }
    __syncthreads();  // every thread holds its part of the stage before the level loop writes to it
    block_order<K, IDX, KPT>(rk, rv, rounds, lds);
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

bool misaligned(const void* p, uint64_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }

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

uint64_t table_bytes(uint64_t n_segments) { return L::up256(n_segments * sizeof(rdst_segment_item)); }

}  // namespace

int rdst_internal::topk_segments_launch_locked(const TopkSegmentsCall& c, const rdst_segment_item* items, const uint32_t* hdr, const uint64_t counts[3]) {
    if (counts[0] >= (1ull << 33) || counts[1] >= (1ull << 31) || counts[2] >= (1ull << 31))
        return set_error(RDST_ERR_ARG, "segments: too many segments of one class for one launch");
    return launch_classes(c, items, hdr, counts);
}

extern "C" uint64_t rdst_hip_topk_segments_scratch_bytes(uint64_t n_segments, uint64_t longest_segment, uint64_t k, uint32_t elem_bytes,
                                                         uint32_t index_bytes) {
    uint32_t lim[4];
    if (n_segments == 0 || n_segments >= (1ull << 32) || longest_segment >= (1ull << 32)) return 0;
    if (rdst_hip_topk_segments_limits(elem_bytes, index_bytes, lim)) return 0;
    uint64_t total = table_bytes(n_segments);
    if (longest_segment > lim[2] || (longest_segment > lim[1] && k > lim[3]))  // a far segment is possible
        total += rdst_hip_topk_scratch_bytes(longest_segment, std::min(k, longest_segment), elem_bytes, index_bytes, 0);
    return total;
}

extern "C" int rdst_hip_topk_segments_device(const void* dev_keys, uint64_t len, const uint64_t* offsets, uint64_t n_segments, uint64_t k,
                                             void* dev_out_keys, void* dev_out_index, uint32_t index_bytes, void* dev_scratch, uint64_t scratch_bytes,
                                             uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, uint32_t flags, void* stream) {
    if (int rc = rdst_internal::check_key_args(dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (kind == RDST_KEY_BYTES_BE) return set_error(RDST_ERR_UNSUPPORTED, "topk: [u8; N] keys are not built");
    if (len >= (1ull << 32)) return set_error(RDST_ERR_UNSUPPORTED, "topk: len must be below 2^32");
    if (flags & ~RDST_TOPK_LARGEST) return set_error(RDST_ERR_ARG, "topk: unknown flag bits");
    if (k == 0 || n_segments == 0) return RDST_OK;
    // the table: its own errors, and the counts (a work list that does not fit capacity 0 is the expected answer)
    if (dev_out_index == nullptr) index_bytes = 0;
    const bool index_ok = index_bytes == 0 || ((index_bytes == 4 || index_bytes == 8) && (elem_bytes == 4 || elem_bytes == 8));
    uint64_t counts[4] = {0, 0, 0, 0}, longest_far = 0;
    int rc = rdst_topk_segments_plan(offsets, n_segments, len, k, elem_bytes, index_ok ? index_bytes : 0, nullptr, 0, counts, &longest_far);
    const uint64_t total = counts[0] + counts[1] + counts[2] + counts[3];
    if (rc != RDST_OK && !(rc == RDST_ERR_ARG && total > 0)) return rc;
    if (dev_out_keys == nullptr) return set_error(RDST_ERR_ARG, "topk: null key output");
    if (misaligned(dev_out_keys, elem_bytes)) return set_error(RDST_ERR_ALIGN, "topk: key output not aligned to the element size");
    if (dev_out_index != nullptr) {
        if (index_bytes != 4 && index_bytes != 8) return set_error(RDST_ERR_ARG, "topk: index_bytes must be 4 or 8");
        if (elem_bytes != 4 && elem_bytes != 8) return set_error(RDST_ERR_UNSUPPORTED, "topk: an index output takes 4- or 8-byte keys");
        if (misaligned(dev_out_index, index_bytes)) return set_error(RDST_ERR_ALIGN, "topk: index output not aligned to index_bytes");
    }
    if (dev_scratch == nullptr) return set_error(RDST_ERR_ARG, "topk: null scratch");
    if (misaligned(dev_scratch, 256)) return set_error(RDST_ERR_ALIGN, "topk: scratch not aligned to 256 bytes");
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
    char* far_scratch = static_cast<char*>(dev_scratch) + table_bytes(n_segments);
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
