// rdst_segments.hip — the segmented sort: many independent slices of one array in one call
// (rdst_hip_sort_segments_device, rdst_hip_sort_segments_pairs_device; include/rdst_hip.h).
//
// The reference sorts the 256 buckets of a chunk as slices of their own, in parallel (src/sorter.rs:131-138), each small
// one with Sorter::lsb_sort_adapter (src/sorts/lsb_sort.rs:39-127).  A loop over rdst_hip_sort_device gives every short
// slice one workgroup of a 256-CU device and one launch.  Here the host turns the table of segment borders into a work
// list (rdst_segments.cpp) and two launches serve every segment up to block_max keys:
//
//   segment_wave_kernel   one WAVE per segment of up to 64 * WAVE_KPT keys, SEG_WAVES segments per workgroup.  The keys
//                         (and values) sit in registers, index = round * 64 + lane; per level the wave counts its digits
//                         into its own 256-bin LDS table, scans it (four bins per lane), ranks every round with the
//                         ballot ranking of the scatter passes (peers_below) and re-orders through its own LDS stage.
//                         After the item is read there is NO workgroup barrier: the waves of a workgroup hold segments
//                         of different lengths, skip different levels, and the waves past the last item have returned.
//                         wave_sync() — a wavefront-scope fence and __builtin_amdgcn_wave_barrier — is the only ordering,
//                         and every branch around it is wave-uniform (a barrier under divergence is undefined).
//   segment_block_kernel  one WORKGROUP per segment of up to 1024 * BLOCK_KPT keys: small_sort_kernel's algorithm
//                         (rdst_kernels.hip) with the segment taken from the work list and a value array beside the keys.
//                         `rounds` and the trivial-level skip are block-uniform: the whole workgroup serves one segment.
//
// Slots past a segment's end hold the largest mapped key.  They start behind every real key and the passes are stable,
// so they stay behind every real key — also behind real keys with the same bits — and are never stored; neither are
// their value slots.  Both kernels load and store element by element: a segment start has the element's alignment only.
//
// Longer segments take the whole-slice route one after another (the way run_split_sort runs its parts).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_device.h"
#include "rdst_segments_layout.h"

namespace {

namespace L = rdst_segments_layout;
using rdst_internal::by_uint;
using rdst_internal::launch;
using rdst_internal::set_error;
using rdst_internal::with_bools;

constexpr int RADIX = 256;
struct NoVal {};  // keys only
template <typename V> struct ValBytes { static constexpr int value = (int)sizeof(V); };
template <> struct ValBytes<NoVal> { static constexpr int value = 0; };

// Shapes: rdst_segments_layout.h states them for this file and for rdst_hip_sort_segments_limits (rdst_segments.cpp).
using L::BLOCK_THREADS;
using L::block_kpt;
using L::wave_kpt;
constexpr int SEG_WAVES = 4;  // segments per workgroup of the wave class
constexpr int BLOCK_WAVES = BLOCK_THREADS / 64;
constexpr size_t wave_lds_bytes(size_t key_bytes, size_t val_bytes) {  // per workgroup: tables, then key stages, then value stages
    return (size_t)SEG_WAVES * (RADIX * sizeof(uint32_t) + 64 * wave_kpt(key_bytes) * (key_bytes + val_bytes));
}
constexpr size_t block_lds_bytes(size_t key_bytes, size_t val_bytes) {
    return (size_t)BLOCK_WAVES * 1024 + 16 + (key_bytes + val_bytes) * BLOCK_THREADS * block_kpt(key_bytes, val_bytes);
}
constexpr size_t LDS_LIMIT = 160 << 10;

// orders this wave's LDS accesses: nothing moves across it, in the compiler or in the wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <typename K, typename V, int LEVELS, bool MAPPED>
__device__ __forceinline__ void segment_wave_body(K* __restrict__ keys, V* __restrict__ vals, const rdst_segment_item* __restrict__ items,
                                                  uint32_t n_items, K neg, K pos) {
    constexpr bool HAS_V = ValBytes<V>::value != 0;
    constexpr int KPT = wave_kpt(sizeof(K));
    constexpr int CAP = 64 * KPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t item = blockIdx.x * SEG_WAVES + (uint32_t)wave;
    if (item >= n_items) return;  // wave-uniform; no workgroup barrier follows
    uint32_t* tbl = reinterpret_cast<uint32_t*>(smem) + wave * RADIX;
    K* stage = reinterpret_cast<K*>(smem + SEG_WAVES * RADIX * sizeof(uint32_t)) + wave * CAP;
    V* vstage = reinterpret_cast<V*>(smem + SEG_WAVES * (RADIX * sizeof(uint32_t) + CAP * sizeof(K))) + (HAS_V ? wave * CAP : 0);
    const rdst_segment_item it = items[item];
    const uint32_t n = it.len < (uint32_t)CAP ? it.len : (uint32_t)CAP;  // (the plan never hands this class a longer one)
    K* seg = keys + it.start;
    V* vseg = HAS_V ? vals + it.start : vals;
    const int rounds = (int)((n + 63) / 64);
    const uint32_t live = (uint32_t)rounds * 64u;
    K mk[KPT];
    V mv[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = (uint32_t)i * 64u + (uint32_t)lane;
        K v = (K) ~(K)0;
        if (i < rounds && idx < n) {
            v = seg[idx];
            if constexpr (MAPPED) v = map_key<K>(v, neg, pos);
            if constexpr (HAS_V) mv[i] = vseg[idx];
        }
        mk[i] = v;
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
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
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
                if constexpr (HAS_V) vstage[b + below] = mv[i];
                wave_sync();
            }
        }
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if (i < rounds) {
                mk[i] = stage[i * 64 + lane];
                if constexpr (HAS_V) mv[i] = vstage[i * 64 + lane];
            }
        }
        wave_sync();
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = (uint32_t)i * 64u + (uint32_t)lane;
        if (i < rounds && idx < n) {
            seg[idx] = MAPPED ? unmap_key<K>(mk[i], neg, pos) : mk[i];
            if constexpr (HAS_V) vseg[idx] = mv[i];
        }
    }
}

template <typename K, typename V, int LEVELS, bool MAPPED>
__global__ __launch_bounds__(SEG_WAVES * 64) void segment_wave_kernel(K* __restrict__ keys, V* __restrict__ vals,
                                                                       const rdst_segment_item* __restrict__ items, uint32_t n_items, K neg, K pos) {
    segment_wave_body<K, V, LEVELS, MAPPED>(keys, vals, items, n_items, neg, pos);
}

template <typename K, typename V, int LEVELS, bool MAPPED>
__device__ __forceinline__ void segment_block_body(K* __restrict__ keys, V* __restrict__ vals, const rdst_segment_item it, K neg, K pos) {
    constexpr bool HAS_V = ValBytes<V>::value != 0;
    constexpr int KPT = block_kpt(sizeof(K), ValBytes<V>::value);
    constexpr int TILE = BLOCK_THREADS * KPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* wave_hist = reinterpret_cast<uint32_t*>(smem);                              // [BLOCK_WAVES][256]
    uint32_t* s_sum = reinterpret_cast<uint32_t*>(smem + BLOCK_WAVES * 1024);             // [4]
    K* stage = reinterpret_cast<K*>(smem + BLOCK_WAVES * 1024 + 16);                      // [TILE]
    V* vstage = reinterpret_cast<V*>(smem + BLOCK_WAVES * 1024 + 16 + sizeof(K) * TILE);  // [TILE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = it.len < (uint32_t)TILE ? it.len : (uint32_t)TILE;  // (the plan never hands this class a longer one)
    K* seg = keys + it.start;
    V* vseg = HAS_V ? vals + it.start : vals;
    // only as many rounds as the segment needs: key index = wave * 64 * rounds + round * 64 + lane
    const int rounds = (int)((n + BLOCK_THREADS - 1) / BLOCK_THREADS);
    const uint32_t live = (uint32_t)rounds * BLOCK_THREADS;
    const uint32_t wbase = (uint32_t)wave * 64u * (uint32_t)rounds + (uint32_t)lane;
    K mk[KPT];
    V mv[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = wbase + i * 64;
        K v = (K) ~(K)0;
        if (i < rounds && idx < n) {
            v = seg[idx];
            if constexpr (MAPPED) v = map_key<K>(v, neg, pos);
            if constexpr (HAS_V) mv[i] = vseg[idx];
        }
        mk[i] = v;
    }
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
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (tid < RADIX && lane == 63) s_sum[wave] = incl;
        __syncthreads();
        if (tid < RADIX) {
            uint32_t run = incl - count_d;
            for (int w = 0; w < wave; ++w) run += s_sum[w];
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
                stage[b + below] = mk[i];
                if constexpr (HAS_V) vstage[b + below] = mv[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if (i < rounds) {
                mk[i] = stage[wbase + i * 64];
                if constexpr (HAS_V) mv[i] = vstage[wbase + i * 64];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = wbase + i * 64;
        if (i < rounds && idx < n) {
            seg[idx] = MAPPED ? unmap_key<K>(mk[i], neg, pos) : mk[i];
            if constexpr (HAS_V) vseg[idx] = mv[i];
        }
    }
}

template <typename K, typename V, int LEVELS, bool MAPPED>
__global__ __launch_bounds__(BLOCK_THREADS) void segment_block_kernel(K* __restrict__ keys, V* __restrict__ vals,
                                                                      const rdst_segment_item* __restrict__ items, K neg, K pos) {
    segment_block_body<K, V, LEVELS, MAPPED>(keys, vals, items[blockIdx.x], neg, pos);  // the grid is exactly this class's items
}

// ---- the same two bodies with their item range read from a plan header in device memory (device-resident offsets) -------
//
// The header is the first 256 bytes of the caller's scratch (rdst_hip_sort_segments_device_offsets_scratch_bytes):
enum PlanHeader : int {
    HDR_N_WAVE = 0,      // items of the wave class
    HDR_N_BLOCK = 1,     // items of the block class (they follow the wave class in the item table)
    HDR_N_LONG = 2,      // items of the long class
    HDR_FLAGS = 3,       // PLAN_* bits: what the plan found wrong
    HDR_LONGEST = 4,     // u64 in the words 4 and 5: the longest long segment
    HDR_RUN_WAVE = 6,    // the counts the batched kernels run: HDR_N_WAVE and HDR_N_BLOCK, or 0 and 0 when nothing may be sorted
    HDR_RUN_BLOCK = 7,
    HDR_RUN_LONG = 8,    // the tiled route (nowait entries): the long items it serves, or 0 when nothing may be sorted
    HDR_TILES = 9,       //   their tiles in all
    HDR_LONG_AT = 10,    //   where they start in the item table: HDR_N_WAVE + HDR_N_BLOCK
    HDR_WORDS = 64,
};
constexpr uint32_t PLAN_DECREASING = 1;  // offsets[s + 1] < offsets[s] somewhere
constexpr uint32_t PLAN_PAST_LEN = 2;    // offsets[n_segments] > len
constexpr uint32_t PLAN_LONG_NO_TMP = 4; // asynchronous mode only: a segment beyond block_max, and no tmp to sort it with
constexpr uint32_t ERR_SEGMENTS_TABLE = 16;  // the device error word's bit for all three (1, 2, 4, 8 and the bits from 8 up are taken)

// The grids are bounds the host can state without the counts; workgroups (waves) past the count return before any barrier.
template <typename K, typename V, int LEVELS, bool MAPPED>
__global__ __launch_bounds__(SEG_WAVES * 64) void segment_wave_counted_kernel(K* __restrict__ keys, V* __restrict__ vals,
                                                                               const rdst_segment_item* __restrict__ items,
                                                                               const uint32_t* __restrict__ hdr, K neg, K pos) {
    segment_wave_body<K, V, LEVELS, MAPPED>(keys, vals, items, hdr[HDR_RUN_WAVE], neg, pos);
}

template <typename K, typename V, int LEVELS, bool MAPPED>
__global__ __launch_bounds__(BLOCK_THREADS) void segment_block_counted_kernel(K* __restrict__ keys, V* __restrict__ vals,
                                                                              const rdst_segment_item* __restrict__ items,
                                                                              const uint32_t* __restrict__ hdr, K neg, K pos) {
    if (blockIdx.x >= hdr[HDR_RUN_BLOCK]) return;  // block-uniform
    segment_block_body<K, V, LEVELS, MAPPED>(keys, vals, items[hdr[HDR_N_WAVE] + blockIdx.x], neg, pos);
}

// ---- the plan on the device ------------------------------------------------------------------------------------------------
//
// rdst_segments_plan's work list, item for item, from a table of borders in device memory: a class key per segment, one
// stable (u32 key, u32 segment) pair sort by the library's own route, and the items written from the sorted pairs.
//   key 0                        wave class: stays in segment order
//   key 1 + (block_max - n)      block class: longest first, ties in segment order
//   key block_max + 2            long class: in segment order
//   key block_max + 3            fewer than two keys: no item
// block_max is at most 16 384, so every key lies below 2^16 and the sort's two upper levels hold one digit.
constexpr int PLAN_THREADS = 256;

template <typename Off>
__global__ __launch_bounds__(PLAN_THREADS) void segments_keygen_kernel(const Off* __restrict__ offsets, uint32_t n_segments, uint64_t len,
                                                                       uint32_t wave_max, uint32_t block_max, uint32_t* __restrict__ keys,
                                                                       uint32_t* __restrict__ segs, uint32_t* __restrict__ hdr) {
    __shared__ uint32_t s_count[4];  // wave, block, long, flags
    __shared__ unsigned long long s_longest;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 4) s_count[tid] = 0;
    if (tid == 0) s_longest = 0;
    __syncthreads();
    const uint32_t s = blockIdx.x * PLAN_THREADS + (uint32_t)tid;  // n_segments <= 2^30
    uint32_t cls = 3, flags = 0;
    uint64_t n = 0;
    if (s < n_segments) {
        const uint64_t lo = offsets[s], hi = offsets[s + 1];
        if (hi < lo) flags |= PLAN_DECREASING;
        else n = hi - lo;
        if (s == n_segments - 1 && hi > len) flags |= PLAN_PAST_LEN;
        cls = n < 2 ? 3u : (n <= wave_max ? 0u : (n <= block_max ? 1u : 2u));
        keys[s] = cls == 0 ? 0u : (cls == 1 ? 1u + (block_max - (uint32_t)n) : block_max + cls);
        segs[s] = s;
    }
    // per wave one LDS atomic per count, per workgroup one global atomic per count
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        const uint32_t hits = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == c));
        if (lane == 0 && hits) atomicAdd(&s_count[c], hits);
    }
    if (flags) atomicOr(&s_count[3], flags);             // (an invalid table: nothing is sorted, time does not matter)
    if (cls == 2) atomicMax(&s_longest, (unsigned long long)n);  // (long segments are few)
    __syncthreads();
    if (tid < 3 && s_count[tid]) atomicAdd(&hdr[tid], s_count[tid]);
    if (tid == 3 && s_count[3]) atomicOr(&hdr[HDR_FLAGS], s_count[3]);
    if (tid == 4 && s_longest) atomicMax(reinterpret_cast<unsigned long long*>(hdr + HDR_LONGEST), s_longest);
}

// One thread per sorted pair: position i of the sorted pairs is position i of the work list.  `long_lens`: the unsaturated
// lengths of the long items, in their order (for the host, which enqueues them).  Thread 0 closes the header: with a flag
// up — or, with `no_long` == 1, a long segment — the batched kernels get zero counts and `err` (if given) the table bit.
// `no_long` == 2 (the nowait entries): long items are no error, the tiled route sorts them; a flag still zeroes the counts.
template <typename Off>
__global__ __launch_bounds__(PLAN_THREADS) void segments_items_kernel(const Off* __restrict__ offsets, uint32_t n_segments, uint32_t block_max,
                                                                      const uint32_t* __restrict__ keys, const uint32_t* __restrict__ segs,
                                                                      rdst_segment_item* __restrict__ items, uint64_t* __restrict__ long_lens,
                                                                      uint32_t* hdr, uint32_t no_long, uint32_t* err) {
    const uint32_t i = blockIdx.x * PLAN_THREADS + threadIdx.x;
    const uint32_t n_wave = hdr[HDR_N_WAVE], n_block = hdr[HDR_N_BLOCK];
    if (i == 0) {
        uint32_t flags = hdr[HDR_FLAGS];
        if (no_long == 1 && hdr[HDR_N_LONG] != 0) {
            flags |= PLAN_LONG_NO_TMP;
            hdr[HDR_FLAGS] = flags;
        }
        hdr[HDR_RUN_WAVE] = flags ? 0u : n_wave;
        hdr[HDR_RUN_BLOCK] = flags ? 0u : n_block;
        if (flags && err) atomicOr(err, ERR_SEGMENTS_TABLE);
    }
    if (i >= n_segments) return;
    const uint32_t key = keys[i], seg = segs[i];
    if (key > block_max + 2 || seg >= n_segments) return;  // no item (and a segment index is never trusted beyond the table)
    const uint64_t lo = offsets[seg], n = (uint64_t)offsets[seg + 1] - lo;  // (an item's class says offsets[seg + 1] >= lo)
    items[i] = {lo, (uint32_t)(n < 0xFFFFFFFFull ? n : 0xFFFFFFFFull), seg};
    if (key == block_max + 2) {
        const uint32_t j = i - n_wave - n_block;
        if (j < n_segments) long_lens[j] = n;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// The work list's way to the device: a pinned buffer per device and an event behind the copy that reads it.  Callers hold
// the library's mutex.
struct Staging {
    void* host = nullptr;
    size_t bytes = 0;
    hipEvent_t copied = nullptr;
    bool in_flight = false;
};
Staging g_staging[16];

int stage_items(Staging& st, const rdst_segment_item* items, size_t count, void* dev_dst, hipStream_t s) {
    const size_t bytes = count * sizeof(rdst_segment_item);
    if (st.in_flight) {  // the previous call's copy still reads the buffer
        RDST_HIP_TRY(hipEventSynchronize(st.copied));
        st.in_flight = false;
    }
    if (!st.copied) RDST_HIP_TRY(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    if (st.bytes < bytes) {
        if (st.host) RDST_HIP_TRY(hipHostFree(st.host));
        st.host = nullptr;
        st.bytes = 0;
        const size_t want = (bytes + bytes / 4 + 4095) / 4096 * 4096;
        RDST_HIP_TRY(hipHostMalloc(&st.host, want, hipHostMallocDefault));
        st.bytes = want;
    }
    memcpy(st.host, items, bytes);
    RDST_HIP_TRY(hipMemcpyAsync(dev_dst, st.host, bytes, hipMemcpyHostToDevice, s));
    RDST_HIP_TRY(hipEventRecord(st.copied, s));
    st.in_flight = true;
    return RDST_OK;
}

// f(K{}, V{}) for the nine (key, value) widths the entries take — NoVal{}: keys only.  The widths were checked (check_call).
template <typename F>
int with_key_value_types(uint32_t key_bytes, uint32_t val_bytes, F&& f) {
    if (val_bytes == 0) {
        switch (key_bytes) {
            case 1: return f(uint8_t{}, NoVal{});
            case 2: return f(uint16_t{}, NoVal{});
            case 4: return f(uint32_t{}, NoVal{});
            case 8: return f(uint64_t{}, NoVal{});
            default: return f(u128{}, NoVal{});
        }
    }
    return by_uint(key_bytes, [&](auto k) { return by_uint(val_bytes, [&](auto v) { return f(k, v); }); });
}

// The order-preserving key map as the kernels take it: the two xor masks, and whether either does anything (MAPPED).
template <typename K>
struct KeyXor {
    K neg, pos;
    bool mapped;
};
template <typename K>
KeyXor<K> key_xor(rdst_key_kind kind) {
    unsigned __int128 neg, pos;
    rdst_internal::key_xor_masks(kind, (uint32_t)sizeof(K), &neg, &pos);
    return {(K)neg, (K)pos, neg != 0 || pos != 0};
}

// One call of any entry, as its worker and the launches see it.  val_bytes == 0: keys only (vals, tmp_vals unused).
struct SegCall {
    void *keys, *vals, *tmp_keys, *tmp_vals;
    uint64_t len;
    uint32_t key_bytes, val_bytes;
    rdst_key_kind kind;
    uint32_t levels;
    hipStream_t s;
    bool pairs() const { return val_bytes != 0; }
};

using rdst_args::misaligned;

// What every entry checks first: the key arguments, then (the pair entries) the widths.
int check_call(const SegCall& c, bool pair_entry, uint64_t n_segments) {
    // with no segment there is nothing the pointers could be used for
    if (int rc = rdst_internal::check_key_args(c.keys, n_segments ? c.len : 0, c.key_bytes, c.kind, c.levels)) return rc;
    if (pair_entry && !L::pair_width_ok(c.key_bytes)) return set_error(RDST_ERR_UNSUPPORTED, "key-value sorts take 4- or 8-byte keys");
    if (pair_entry && !L::pair_width_ok(c.val_bytes)) return set_error(RDST_ERR_UNSUPPORTED, "key-value sorts carry 4- or 8-byte values");
    return RDST_OK;
}

// The value and tmp pointers.  `no_tmp`: the text of an entry that cannot do without a tmp array (nullptr: it can).
int check_pointers(const SegCall& c, const char* no_tmp) {
    if (c.pairs() && c.vals == nullptr && c.len != 0) return set_error(RDST_ERR_ARG, "null value pointer");
    if (c.pairs() && misaligned(c.vals, c.val_bytes)) return set_error(RDST_ERR_ALIGN, "value pointer not aligned to the value size");
    if (no_tmp && (c.tmp_keys == nullptr || (c.pairs() && c.tmp_vals == nullptr))) return set_error(RDST_ERR_ARG, no_tmp);
    if (misaligned(c.tmp_keys, c.key_bytes)) return set_error(RDST_ERR_ALIGN, "tmp pointer not aligned to the element size");
    if (c.pairs() && misaligned(c.tmp_vals, c.val_bytes)) return set_error(RDST_ERR_ALIGN, "tmp value pointer not aligned to the value size");
    return RDST_OK;
}

// The two batched launches: a wave per item of the wave class, a workgroup per item of the block class.  COUNTED == false:
// the host knows the counts, `n_wave` and `n_block`, and the block class follows the wave class in `items`.  COUNTED == true:
// the counts stand in the plan header `hdr`, and `n_wave` and `n_block` are the host's bounds on them, for the grids alone.
template <bool COUNTED, typename K, typename V>
int launch_classes_t(K* keys, V* vals, const rdst_segment_item* items, const uint32_t* hdr, uint64_t n_wave, uint64_t n_block, rdst_key_kind kind,
                     hipStream_t s) {
    constexpr int LEVELS = (int)sizeof(K);
    constexpr size_t VB = ValBytes<V>::value;
    constexpr size_t wave_lds = wave_lds_bytes(sizeof(K), VB), block_lds = block_lds_bytes(sizeof(K), VB);
    static_assert(wave_lds <= LDS_LIMIT && block_lds <= LDS_LIMIT, "a workgroup's LDS stays within 160 KiB");
    const KeyXor<K> x = key_xor<K>(kind);
    const dim3 wave_grid((uint32_t)((n_wave + SEG_WAVES - 1) / SEG_WAVES)), wave_block(SEG_WAVES * 64);
    const dim3 block_grid((uint32_t)n_block), block_block(BLOCK_THREADS);
    int rc = RDST_OK;
    if (n_wave)
        rc = with_bools([&](auto mapped) {
            constexpr bool M = decltype(mapped)::value;
            if constexpr (COUNTED)
                return launch("segment_wave_counted_kernel", segment_wave_counted_kernel<K, V, LEVELS, M>, wave_grid, wave_block, wave_lds, s, keys, vals,
                              items, hdr, x.neg, x.pos);
            else
                return launch("segment_wave_kernel", segment_wave_kernel<K, V, LEVELS, M>, wave_grid, wave_block, wave_lds, s, keys, vals, items,
                              (uint32_t)n_wave, x.neg, x.pos);
        }, x.mapped);
    if (rc || !n_block) return rc;
    return with_bools([&](auto mapped) {
        constexpr bool M = decltype(mapped)::value;
        if constexpr (COUNTED)
            return launch("segment_block_counted_kernel", segment_block_counted_kernel<K, V, LEVELS, M>, block_grid, block_block, block_lds, s, keys, vals,
                          items, hdr, x.neg, x.pos);
        else
            return launch("segment_block_kernel", segment_block_kernel<K, V, LEVELS, M>, block_grid, block_block, block_lds, s, keys, vals,
                          items + n_wave, x.neg, x.pos);
    }, x.mapped);
}

template <bool COUNTED>
int launch_classes(const SegCall& c, const rdst_segment_item* items, const uint32_t* hdr, uint64_t n_wave, uint64_t n_block) {
    return with_key_value_types(c.key_bytes, c.val_bytes, [&](auto k, auto v) {
        return launch_classes_t<COUNTED>(static_cast<decltype(k)*>(c.keys), static_cast<decltype(v)*>(c.vals), items, hdr, n_wave, n_block, c.kind, c.s);
    });
}

// A batched stage between its profiling calls: a run of its own, `enqueue`, the end of RDST_STAGE_SEGMENTS.
template <typename F>
int batched_stage(hipStream_t s, F&& enqueue) {
    if (int rc = rdst_internal::profile_open_run(s)) return rc;
    if (int rc = enqueue()) return rc;
    return rdst_internal::profile_stage_end(s, RDST_STAGE_SEGMENTS);
}

// One long segment, [start, start + n) of the keys (and values), by the whole-slice route.  Callers hold the library's mutex.
int sort_long_slice(const SegCall& c, uint64_t start, uint64_t n) {
    char* k = static_cast<char*>(c.keys) + start * c.key_bytes;
    return c.pairs() ? rdst_internal::sort_pairs_slice_locked(k, static_cast<char*>(c.vals) + start * c.val_bytes, c.tmp_keys, c.tmp_vals, n, c.key_bytes,
                                                              c.kind, c.val_bytes, c.s)
                     : rdst_internal::sort_slice_locked(k, c.tmp_keys, n, c.key_bytes, c.kind, c.s);
}

// Both host-borders entries.
int sort_segments(const SegCall& c, bool pair_entry, uint64_t tmp_elems, const uint64_t* offsets, uint64_t n_segments) {
    int rc = check_call(c, pair_entry, n_segments);
    if (rc || n_segments == 0) return rc;
    std::vector<rdst_segment_item> items;
    uint64_t counts[3] = {0, 0, 0}, longest = 0;
    rc = rdst_segments_plan(offsets, n_segments, c.len, c.key_bytes, c.val_bytes, nullptr, 0, counts, &longest);
    const uint64_t total = counts[0] + counts[1] + counts[2];
    if (rc != RDST_OK && !(rc == RDST_ERR_ARG && total > 0)) return rc;  // (a work list that does not fit capacity 0 is the expected answer)
    if (total == 0) return RDST_OK;
    items.resize(total);
    if ((rc = rdst_segments_plan(offsets, n_segments, c.len, c.key_bytes, c.val_bytes, items.data(), total, counts, &longest))) return rc;
    if ((rc = check_pointers(c, nullptr))) return rc;  // (a work list: len != 0)
    if (counts[2] != 0) {
        if (c.tmp_keys == nullptr || (c.pairs() && c.tmp_vals == nullptr)) return set_error(RDST_ERR_ARG, "segments: a segment beyond block_max needs a tmp array");
        if (tmp_elems < longest) return set_error(RDST_ERR_ARG, "segments: tmp_elems is below the longest segment beyond block_max");
    }
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    const uint64_t batched = counts[0] + counts[1];
    if (counts[1] >= (1ull << 31)) return set_error(RDST_ERR_ARG, "segments: too many block-class segments for one launch");
    // the workspace is sized ONCE, for the work list and for every long segment: a growth between the launches would free
    // memory the batched kernels were handed
    const size_t table_bytes = (size_t)batched * sizeof(rdst_segment_item);
    size_t ws_bytes = table_bytes;
    for (uint64_t i = batched; i < total; ++i) {
        const uint32_t sg = items[i].seg;
        ws_bytes = std::max(ws_bytes, rdst_internal::slice_workspace_bytes(offsets[sg + 1] - offsets[sg], c.key_bytes, c.kind, c.val_bytes));
    }
    void* ws = nullptr;
    int dev = 0;
    rc = rdst_internal::workspace_take(ws_bytes, c.s, &ws, &dev);
    if (rc && ws_bytes > table_bytes) rc = rdst_internal::workspace_take(std::max<size_t>(table_bytes, 256), c.s, &ws, &dev);  // no room: a long segment then picks its lean layout itself
    if (rc) return rc;
    if (batched) {
        rc = batched_stage(c.s, [&] {
            if (int e = stage_items(g_staging[dev], items.data(), (size_t)batched, ws, c.s)) return e;
            return launch_classes<false>(c, static_cast<const rdst_segment_item*>(ws), nullptr, counts[0], counts[1]);
        });
        if (rc) return rc;
        if ((rc = rdst_internal::workspace_handback(c.s))) return rc;
    }
    // long segments one after another; each uses the workspace (the work list is dead by then, in stream order)
    for (uint64_t i = batched; i < total; ++i) {
        const uint32_t sg = items[i].seg;
        if ((rc = sort_long_slice(c, offsets[sg], offsets[sg + 1] - offsets[sg]))) return rc;
    }
    return RDST_OK;
}

// ---- device-resident offsets -------------------------------------------------------------------------------------------------

// The caller's scratch: header, the plan's pair arrays and their tmps, the item table, where rdst_segments_layout.h puts them.
struct PlanScratch {
    uint32_t* hdr;
    uint32_t *keys, *segs, *tmp_keys, *tmp_segs;
    rdst_segment_item* items;
    uint64_t* long_lens;  // over the two tmps, which are dead once the pairs are sorted
};

PlanScratch plan_scratch(void* scratch, uint64_t n_segments) {
    static_assert(HDR_WORDS * sizeof(uint32_t) == L::PLAN_HEADER_BYTES, "the header the kernels index is the header of the layout");
    static_assert(sizeof(uint64_t) == 2 * sizeof(uint32_t), "the long lengths fit the two tmps");
    const L::PlanLayout at = L::plan_layout(n_segments);
    char* base = static_cast<char*>(scratch);
    const auto u32 = [base](uint64_t offset) { return reinterpret_cast<uint32_t*>(base + offset); };
    return {u32(0), u32(at.keys), u32(at.segs), u32(at.tmp_keys), u32(at.tmp_segs), reinterpret_cast<rdst_segment_item*>(base + at.items),
            reinterpret_cast<uint64_t*>(base + at.tmp_keys)};
}

// What the device-offsets entries and the plan hook check alike, before any device work.
int check_offsets_table(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len) {
    if (n_segments > L::MAX_SEGMENTS) return set_error(RDST_ERR_UNSUPPORTED, "segments: device-resident offsets take at most 2^30 segments");
    if (offset_bytes != 4 && offset_bytes != 8) return set_error(RDST_ERR_ARG, "segments: offset_bytes must be 4 or 8");
    if (dev_offsets == nullptr) return set_error(RDST_ERR_ARG, "segments: null offsets");
    if (misaligned(dev_offsets, offset_bytes)) return set_error(RDST_ERR_ALIGN, "segments: offsets pointer not aligned to offset_bytes");
    if (offset_bytes == 4 && len >= (1ull << 32)) return set_error(RDST_ERR_ARG, "segments: 4-byte offsets need len below 2^32");
    return RDST_OK;
}

// `need`: the bytes this entry's ..._scratch_bytes function asks for; `below_need`: the text that names the function.
int check_scratch(const void* scratch, uint64_t scratch_bytes, uint64_t need, const char* below_need) {
    if (scratch == nullptr) return set_error(RDST_ERR_ARG, "segments: null scratch");
    if (misaligned(scratch, 256)) return set_error(RDST_ERR_ALIGN, "segments: scratch not aligned to 256 bytes");
    if (scratch_bytes < need) return set_error(RDST_ERR_ARG, below_need);
    return RDST_OK;
}

int check_offsets_args(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len, const void* scratch, uint64_t scratch_bytes) {
    if (int rc = check_offsets_table(dev_offsets, offset_bytes, n_segments, len)) return rc;
    return check_scratch(scratch, scratch_bytes, L::plan_layout(n_segments).total,
                         "segments: scratch_bytes is below rdst_hip_sort_segments_device_offsets_scratch_bytes(n_segments)");
}

// The class keys of the plan (segments_keygen_kernel) reach block_max + 3.
constexpr bool class_keys_fit_16_bits() {
    for (uint32_t kb : {1u, 2u, 4u, 8u, 16u})
        for (uint32_t vb : {0u, 4u, 8u})
            if (L::block_max(kb, vb) + 3 >= (1u << 16)) return false;
    return true;
}

// Enqueues the plan: header cleared, class keys, the pair sort (it takes and hands back the workspace itself), items.
// Callers hold the library's mutex.  Nothing here waits for the device.
template <typename Off>
int enqueue_plan_t(const void* dev_offsets, uint64_t n_segments, uint64_t len, uint32_t wave_max, uint32_t block_max, const PlanScratch& P,
                   uint32_t no_long, uint32_t* err, hipStream_t s) {
    const Off* off = static_cast<const Off*>(dev_offsets);
    const uint32_t nseg = (uint32_t)n_segments;
    const dim3 grid((uint32_t)((n_segments + PLAN_THREADS - 1) / PLAN_THREADS));
    RDST_HIP_TRY(hipMemsetAsync(P.hdr, 0, HDR_WORDS * sizeof(uint32_t), s));
    int rc = launch("segments_keygen_kernel", segments_keygen_kernel<Off>, grid, dim3(PLAN_THREADS), 0, s, off, nseg, len, wave_max, block_max, P.keys, P.segs, P.hdr);
    if (rc) return rc;
    if (n_segments > 1 && (rc = rdst_internal::sort_pairs_slice_locked(P.keys, P.segs, P.tmp_keys, P.tmp_segs, n_segments, 4, RDST_KEY_UNSIGNED, 4, s))) return rc;
    return launch("segments_items_kernel", segments_items_kernel<Off>, grid, dim3(PLAN_THREADS), 0, s, off, nseg, block_max,
                  static_cast<const uint32_t*>(P.keys), static_cast<const uint32_t*>(P.segs), P.items, P.long_lens, P.hdr, no_long, err);
}

int enqueue_plan(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len, uint32_t key_bytes, uint32_t val_bytes,
                 const PlanScratch& P, uint32_t no_long, uint32_t* err, hipStream_t s) {
    static_assert(class_keys_fit_16_bits(), "the plan's pair sort relies on class keys below 2^16");
    const uint32_t wave_max = L::wave_max(key_bytes), block_max = L::block_max(key_bytes, val_bytes);
    return offset_bytes == 4 ? enqueue_plan_t<uint32_t>(dev_offsets, n_segments, len, wave_max, block_max, P, no_long, err, s)
                             : enqueue_plan_t<uint64_t>(dev_offsets, n_segments, len, wave_max, block_max, P, no_long, err, s);
}

// The batched launches of the asynchronous mode: grids from what the host knows, counts from the header.  A wave-class
// segment holds at least two keys, a block-class one more than wave_max.
int launch_counted(const SegCall& c, const PlanScratch& P, uint64_t n_segments) {
    return launch_classes<true>(c, P.items, P.hdr, std::min<uint64_t>(n_segments, c.len / 2),
                                std::min<uint64_t>(n_segments, c.len / (L::wave_max(c.key_bytes) + 1)));
}

// The header as the host reads it (tmp mode and the plan hook): one copy and one wait for `s`.
struct PlanResult {
    uint64_t counts[3], longest;
    uint32_t flags;
};
int read_plan(const PlanScratch& P, PlanResult* r, hipStream_t s) {
    uint32_t h[8] = {};
    RDST_HIP_TRY(hipMemcpyAsync(h, P.hdr, sizeof h, hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    r->counts[0] = h[HDR_N_WAVE];
    r->counts[1] = h[HDR_N_BLOCK];
    r->counts[2] = h[HDR_N_LONG];
    r->flags = h[HDR_FLAGS];
    r->longest = (uint64_t)h[HDR_LONGEST] | ((uint64_t)h[HDR_LONGEST + 1] << 32);
    return RDST_OK;
}

int flags_error(uint32_t flags) {
    if (flags & PLAN_DECREASING) return set_error(RDST_ERR_ARG, "segments: offsets must be non-decreasing");
    return set_error(RDST_ERR_ARG, "segments: the last offset lies past len");
}

// Both device-offsets entries.
int sort_segments_offsets(const SegCall& c, bool pair_entry, uint64_t tmp_elems, const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments,
                          void* scratch, uint64_t scratch_bytes) {
    int rc = check_call(c, pair_entry, n_segments);
    if (rc || n_segments == 0) return rc;
    if ((rc = check_offsets_args(dev_offsets, offset_bytes, n_segments, c.len, scratch, scratch_bytes))) return rc;
    if ((rc = check_pointers(c, tmp_elems != 0 ? "segments: tmp_elems > 0 needs a tmp array" : nullptr))) return rc;
    const PlanScratch P = plan_scratch(scratch, n_segments);
    const bool async = tmp_elems == 0;
    uint32_t* err = nullptr;
    if (async && (rc = rdst_internal::device_error_word(&err))) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    if ((rc = enqueue_plan(dev_offsets, offset_bytes, n_segments, c.len, c.key_bytes, c.val_bytes, P, async ? 1u : 0u, err, c.s))) return rc;
    if (async) return batched_stage(c.s, [&] { return launch_counted(c, P, n_segments); });  // the counts stay on the device
    PlanResult r;
    if ((rc = read_plan(P, &r, c.s))) return rc;  // the one wait of this mode (and one more below, if there are long segments)
    if (r.flags) return flags_error(r.flags);
    if (r.counts[2] != 0 && tmp_elems < r.longest) return set_error(RDST_ERR_ARG, "segments: tmp_elems is below the longest segment beyond block_max");
    const uint64_t batched = r.counts[0] + r.counts[1];
    if (batched && (rc = batched_stage(c.s, [&] { return launch_classes<false>(c, P.items, nullptr, r.counts[0], r.counts[1]); }))) return rc;
    if (r.counts[2] == 0) return RDST_OK;
    std::vector<rdst_segment_item> long_items((size_t)r.counts[2]);
    std::vector<uint64_t> long_lens((size_t)r.counts[2]);
    RDST_HIP_TRY(hipMemcpyAsync(long_items.data(), P.items + batched, long_items.size() * sizeof(rdst_segment_item), hipMemcpyDeviceToHost, c.s));
    RDST_HIP_TRY(hipMemcpyAsync(long_lens.data(), P.long_lens, long_lens.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c.s));
    RDST_HIP_TRY(hipStreamSynchronize(c.s));
    for (size_t i = 0; i < long_items.size(); ++i) {
        const uint64_t start = long_items[i].start, n = long_lens[i];
        if (n > tmp_elems || start > c.len || n > c.len - start) return set_error(RDST_ERR_DEVICE, "segments: a long item of the device plan lies outside the array");
        if ((rc = sort_long_slice(c, start, n))) return rc;
    }
    return RDST_OK;
}

// ---- the tiled route: long segments on the device (the nowait entries) -----------------------------------------------------------
//
// The plan leaves the long items behind the batched ones in the item table, in segment order.  A long item is cut into tiles
// of T = BLOCK_THREADS * block_kpt keys — segment_block_body's tile — and sorted by LEVELS stable counting passes between the
// keys and tmp (values: vals and tmp_vals), every item over its own range of both arrays:
//   segments_tiles_kernel        one workgroup: exclusive scan of the items' tile counts into tile_base, the total into the header
//   per level  segment_tile_count_kernel    a workgroup per tile (grid-stride): 256 digit counts into tile_counts[tile]
//              segment_tile_offsets_kernel  a workgroup per item: per digit, exclusive prefixes over the item's tiles in place;
//                                           the 256 totals become the exclusive digit bases digit_base[item]
//              segment_tile_scatter_kernel  a workgroup per tile: segment_block_body's wave-major layout and ranking, slots
//                                           starting at digit_base + the tile's prefix + the earlier waves' counts
//   segment_tile_copy_kernel     one-byte keys only (an odd level count leaves the result in tmp)
// No kernel waits for another workgroup: every dependency is a kernel boundary.  Every count read from memory is bounded
// against what the host passed (TileBounds) before it is used, and every store is checked against the item's own length.
struct TileBounds {
    uint32_t n_segments;    // the item table's size
    uint32_t n_long_bound;  // min(n_segments, len / (T + 1))
    uint32_t tiles_bound;   // len / T + n_long_bound
    uint32_t tile;          // T
    uint64_t len;           // below 2^32
};
struct TileScratch {
    uint32_t* tile_base;    // [n_long_bound + 1]
    uint32_t* digit_base;   // [n_long_bound][256]
    uint32_t* tile_counts;  // [tiles_bound][256]
};
constexpr int TILE_GRID_PER_CU = 4;  // the tile kernels' grids: min(tiles_bound, this * CU count), grid-stride beyond

__global__ __launch_bounds__(BLOCK_THREADS) void segments_tiles_kernel(const rdst_segment_item* __restrict__ items, uint32_t* hdr,
                                                                       uint32_t* __restrict__ tile_base, TileBounds B, uint32_t* err) {
    __shared__ uint32_t s_wave[BLOCK_WAVES];
    __shared__ uint32_t s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t flags = hdr[HDR_FLAGS], n_long = hdr[HDR_N_LONG];
    const uint64_t at = (uint64_t)hdr[HDR_N_WAVE] + hdr[HDR_N_BLOCK];
    const bool off_limits = n_long > B.n_long_bound || at + n_long > B.n_segments;
    if (flags || off_limits) {  // block-uniform: the header words stay zero (the plan cleared them), nothing later runs
        if (tid == 0 && !flags && err) atomicOr(err, ERR_SEGMENTS_TABLE);
        return;
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();
    uint32_t carry = 0;  // block-uniform: the tiles of the chunks before this one
    bool bad = false;
    for (uint32_t base = 0; base < n_long && carry <= B.tiles_bound; base += BLOCK_THREADS) {  // n_long <= n_long_bound
        const uint32_t i = base + (uint32_t)tid;
        uint32_t mine = 0;
        if (i < n_long) {
            const rdst_segment_item it = items[at + i];
            if (it.len == 0 || it.start > B.len || it.len > B.len - it.start) bad = true;
            else mine = (it.len - 1) / B.tile + 1;
        }
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if (lane >= o) incl += y;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;  // a chunk holds at most 1024 * (2^32 / 4096 + 1) tiles: below 2^31
#pragma unroll
        for (int w = 0; w < BLOCK_WAVES; ++w) {
            const uint32_t c = s_wave[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        if (i < n_long) tile_base[i] = carry + before + incl - mine;
        carry += total;
        __syncthreads();
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (tid == 0) {
        const bool ok = s_bad == 0 && carry <= B.tiles_bound;
        tile_base[n_long] = ok ? carry : 0u;
        hdr[HDR_LONG_AT] = (uint32_t)at;
        hdr[HDR_TILES] = ok ? carry : 0u;
        hdr[HDR_RUN_LONG] = ok ? n_long : 0u;
        if (!ok && err) atomicOr(err, ERR_SEGMENTS_TABLE);
    }
}

// What the tile kernels read from the header, bounded.
struct TileRun {
    uint32_t n_long, tiles, at;
};
__device__ __forceinline__ TileRun tile_run(const uint32_t* __restrict__ hdr, const TileBounds& B) {
    TileRun r;
    r.n_long = hdr[HDR_RUN_LONG];
    r.tiles = hdr[HDR_TILES];
    r.at = hdr[HDR_LONG_AT];
    if (r.n_long == 0 || r.n_long > B.n_long_bound || r.tiles > B.tiles_bound || (uint64_t)r.at + r.n_long > B.n_segments) r.n_long = r.tiles = 0;
    return r;
}

// Tile t of the route: its item (a bounded binary search in tile_base: the last i with tile_base[i] <= t), the item's range
// and the tile's range inside it.  `n` == 0: the tables do not agree with each other, the tile is left alone.
struct TileRef {
    uint64_t start;  // the item's first element
    uint32_t ilen;   // the item's length
    uint32_t first;  // the tile's first position inside the item
    uint32_t n;      // the tile's keys: T, or fewer in an item's last tile
    uint32_t item;
};
__device__ __forceinline__ TileRef tile_ref(const rdst_segment_item* __restrict__ items, const uint32_t* __restrict__ tile_base, const TileRun& R,
                                            const TileBounds& B, uint32_t t) {
    uint32_t lo = 0, hi = R.n_long;
    for (int step = 0; step < 32 && hi - lo > 1; ++step) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tile_base[mid] <= t) lo = mid;
        else hi = mid;
    }
    const rdst_segment_item it = items[R.at + lo];
    TileRef r;
    r.item = lo;
    r.start = it.start;
    r.ilen = it.len;
    const uint32_t tb = tile_base[lo];
    const uint64_t first = (uint64_t)(t - tb) * B.tile;
    const bool ok = tb <= t && first < it.len && it.start <= B.len && it.len <= B.len - it.start;
    r.first = ok ? (uint32_t)first : 0u;
    r.n = ok ? (it.len - r.first < B.tile ? it.len - r.first : B.tile) : 0u;
    return r;
}

template <typename K, typename V, bool MAPPED>
__global__ __launch_bounds__(BLOCK_THREADS) void segment_tile_count_kernel(const K* __restrict__ src, const rdst_segment_item* __restrict__ items,
                                                                           const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ tile_base,
                                                                           uint32_t* __restrict__ tile_counts, TileBounds B, int shift, K neg, K pos) {
    constexpr int KPT = block_kpt(sizeof(K), ValBytes<V>::value);
    __shared__ uint32_t wave_hist[BLOCK_WAVES * RADIX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* wh = wave_hist + wave * RADIX;
    const TileRun R = tile_run(hdr, B);
    for (uint32_t t = blockIdx.x; t < R.tiles; t += gridDim.x) {  // block-uniform; tiles <= tiles_bound
        const TileRef T = tile_ref(items, tile_base, R, B, t);
        const K* seg = src + T.start + T.first;
#pragma unroll
        for (int j = 0; j < 4; ++j) wh[lane + 64 * j] = 0;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t idx = (uint32_t)tid + (uint32_t)i * BLOCK_THREADS;
            if (idx < T.n) {
                K v = seg[idx];
                if constexpr (MAPPED) v = map_key<K>(v, neg, pos);
                atomicAdd(&wh[digit_of(v, shift)], 1u);
            }
        }
        __syncthreads();
        if (tid < RADIX) {
            uint32_t count_d = 0;
#pragma unroll
            for (int w = 0; w < BLOCK_WAVES; ++w) count_d += wave_hist[w * RADIX + tid];
            tile_counts[(size_t)t * RADIX + tid] = count_d;
        }
        __syncthreads();  // the tables are zeroed again at the top
    }
}

// One workgroup per long item, four groups of 256 threads: thread d of group g walks the g-th quarter of the item's tiles.
// First the quarters' sums, then every quarter's exclusive prefixes from the sum of the quarters before it: a single walk of
// an item of 2^32 - 1 four-byte keys (2^18 tiles) is split in four, and the loads of a walk do not depend on each other.
constexpr int OFFSET_GROUPS = BLOCK_THREADS / RADIX;
__global__ __launch_bounds__(BLOCK_THREADS) void segment_tile_offsets_kernel(const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ tile_base,
                                                                             uint32_t* __restrict__ tile_counts, uint32_t* __restrict__ digit_base,
                                                                             TileBounds B) {
    __shared__ uint32_t s_part[OFFSET_GROUPS][RADIX];
    __shared__ uint32_t s_sum[RADIX / 64];
    const TileRun R = tile_run(hdr, B);
    const uint32_t item = blockIdx.x;
    if (item >= R.n_long) return;  // block-uniform
    const uint32_t t0 = tile_base[item], t1 = tile_base[item + 1];
    if (t0 > t1 || t1 > R.tiles) return;  // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, g = tid >> 8, d = tid & (RADIX - 1);
    const uint32_t nt = t1 - t0, per = (nt + OFFSET_GROUPS - 1) / OFFSET_GROUPS;
    const uint32_t a = (uint32_t)g * per < nt ? (uint32_t)g * per : nt, b = nt - a < per ? nt : a + per;
    uint32_t* col = tile_counts + (size_t)t0 * RADIX + d;
    uint32_t sum = 0;
    for (uint32_t j = a; j < b; ++j) sum += col[(size_t)j * RADIX];  // nt <= tiles_bound
    s_part[g][d] = sum;
    __syncthreads();
    uint32_t run = 0, total = 0;
#pragma unroll
    for (int q = 0; q < OFFSET_GROUPS; ++q) {
        const uint32_t c = s_part[q][d];
        run += q < g ? c : 0u;
        total += c;
    }
    for (uint32_t j = a; j < b; ++j) {
        const uint32_t c = col[(size_t)j * RADIX];
        col[(size_t)j * RADIX] = run;
        run += c;
    }
    // group 0 (the waves 0 .. 3): the exclusive scan of the 256 totals
    uint32_t incl = total;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (g == 0 && lane == 63) s_sum[tid >> 6] = incl;
    __syncthreads();
    if (g == 0) {
        uint32_t base = incl - total;
        for (int w = 0; w < (tid >> 6); ++w) base += s_sum[w];
        digit_base[(size_t)item * RADIX + d] = base;
    }
}

template <typename K, typename V, bool MAPPED>
__global__ __launch_bounds__(BLOCK_THREADS) void segment_tile_scatter_kernel(const K* __restrict__ src, K* __restrict__ dst, const V* __restrict__ vsrc,
                                                                             V* __restrict__ vdst, const rdst_segment_item* __restrict__ items,
                                                                             const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ tile_base,
                                                                             const uint32_t* __restrict__ tile_counts,
                                                                             const uint32_t* __restrict__ digit_base, TileBounds B, int shift, K neg,
                                                                             K pos) {
    constexpr bool HAS_V = ValBytes<V>::value != 0;
    constexpr int KPT = block_kpt(sizeof(K), ValBytes<V>::value);
    __shared__ uint32_t wave_hist[BLOCK_WAVES * RADIX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bit0 = shift & 31;
    uint32_t* wh = wave_hist + wave * RADIX;
    const TileRun R = tile_run(hdr, B);
    for (uint32_t t = blockIdx.x; t < R.tiles; t += gridDim.x) {  // block-uniform; tiles <= tiles_bound
        const TileRef T = tile_ref(items, tile_base, R, B, t);
        const K* seg = src + T.start + T.first;
        const V* vseg = HAS_V ? vsrc + T.start + T.first : vsrc;
        K* out = dst + T.start;
        V* vout = HAS_V ? vdst + T.start : vdst;
        // segment_block_body's layout: key index = wave * 64 * rounds + round * 64 + lane, only as many rounds as the tile needs
        const int rounds = (int)((T.n + BLOCK_THREADS - 1) / BLOCK_THREADS);
        const uint32_t wbase = (uint32_t)wave * 64u * (uint32_t)rounds + (uint32_t)lane;
        K mk[KPT];
        V mv[KPT];
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t idx = wbase + i * 64;
            K v = (K) ~(K)0;
            if (i < rounds && idx < T.n) {
                v = seg[idx];
                if constexpr (MAPPED) v = map_key<K>(v, neg, pos);
                if constexpr (HAS_V) mv[i] = vseg[idx];
            }
            mk[i] = v;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) wh[lane + 64 * j] = 0;
#pragma unroll
        for (int i = 0; i < KPT; ++i)
            if (i < rounds && wbase + i * 64 < T.n) atomicAdd(&wh[digit_of(mk[i], shift)], 1u);  // slots past the tile's end are not counted
        __syncthreads();
        if (tid < RADIX) {
            uint32_t run = digit_base[(size_t)T.item * RADIX + tid] + tile_counts[(size_t)t * RADIX + tid];
#pragma unroll
            for (int w = 0; w < BLOCK_WAVES; ++w) {
                const uint32_t c = wave_hist[w * RADIX + tid];
                wave_hist[w * RADIX + tid] = run;
                run += c;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            if (i < rounds) {  // block-uniform: all 64 lanes rank (peers_below needs them)
                uint32_t* slot = &wh[digit_of(mk[i], shift)];
                const uint32_t b = *slot;
                // the slots past the tile's end sit in the lanes above every real key of their round: they change no real key's rank
                const uint32_t below = peers_below(digit_word<K>(mk[i], shift), bit0);
                __builtin_amdgcn_wave_barrier();
                const uint32_t to = b + below;
                if (wbase + i * 64 < T.n) {
                    atomicAdd(slot, 1u);
                    if (to < T.ilen) {  // (always, when the counts are those of these keys)
                        out[to] = MAPPED ? unmap_key<K>(mk[i], neg, pos) : mk[i];
                        if constexpr (HAS_V) vout[to] = mv[i];
                    }
                }
            }
        }
        __syncthreads();  // the tables are zeroed again at the top
    }
}

// One-byte keys: their one level leaves the sorted items in tmp.
template <typename K, typename V>
__global__ __launch_bounds__(BLOCK_THREADS) void segment_tile_copy_kernel(const K* __restrict__ src, K* __restrict__ dst, const V* __restrict__ vsrc,
                                                                          V* __restrict__ vdst, const rdst_segment_item* __restrict__ items,
                                                                          const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ tile_base,
                                                                          TileBounds B) {
    constexpr bool HAS_V = ValBytes<V>::value != 0;
    constexpr int KPT = block_kpt(sizeof(K), ValBytes<V>::value);
    const TileRun R = tile_run(hdr, B);
    for (uint32_t t = blockIdx.x; t < R.tiles; t += gridDim.x) {
        const TileRef T = tile_ref(items, tile_base, R, B, t);
        const uint64_t at = T.start + T.first;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t idx = (uint32_t)threadIdx.x + (uint32_t)i * BLOCK_THREADS;
            if (idx < T.n) {
                dst[at + idx] = src[at + idx];
                if constexpr (HAS_V) vdst[at + idx] = vsrc[at + idx];
            }
        }
    }
}

// The tiled route's bounds and its arrays behind the plan's, where rdst_segments_layout.h puts them.
void tile_scratch(void* scratch, uint64_t n_segments, uint64_t len, uint32_t tile, TileBounds* B, TileScratch* out) {
    const L::TileLayout at = L::tile_layout(n_segments, len, tile);
    *B = {(uint32_t)n_segments, at.n_long_bound, at.tiles_bound, tile, len};
    char* base = static_cast<char*>(scratch);
    *out = {reinterpret_cast<uint32_t*>(base + at.tile_base), reinterpret_cast<uint32_t*>(base + at.digit_base),
            reinterpret_cast<uint32_t*>(base + at.tile_counts)};
}

template <typename K, typename V>
int launch_tiled_t(K* keys, V* vals, K* tmp_keys, V* tmp_vals, const PlanScratch& P, const TileScratch& S, const TileBounds& B, int cus, uint32_t* err,
                   rdst_key_kind kind, hipStream_t s) {
    constexpr int LEVELS = (int)sizeof(K);
    static_assert(BLOCK_WAVES * RADIX * sizeof(uint32_t) <= LDS_LIMIT, "a workgroup's LDS stays within 160 KiB");  // the per-wave count tables: 16 KiB
    const KeyXor<K> x = key_xor<K>(kind);
    const rdst_segment_item* items = P.items;
    const uint32_t *hdr = P.hdr, *tile_base = S.tile_base, *counts = S.tile_counts, *bases = S.digit_base;
    const dim3 block(BLOCK_THREADS);
    const dim3 tile_grid(std::min<uint32_t>(B.tiles_bound, (uint32_t)(TILE_GRID_PER_CU * cus)));
    const dim3 item_grid(B.n_long_bound);
    int rc = launch("segments_tiles_kernel", segments_tiles_kernel, dim3(1), block, 0, s, items, P.hdr, S.tile_base, B, err);
    if (rc) return rc;
    for (int level = 0; level < LEVELS; ++level) {
        const int shift = level * 8;
        const K* src = level & 1 ? tmp_keys : keys;
        K* dst = level & 1 ? keys : tmp_keys;
        const V* vsrc = level & 1 ? tmp_vals : vals;
        V* vdst = level & 1 ? vals : tmp_vals;
        rc = with_bools([&](auto mapped) {
            return launch("segment_tile_count_kernel", segment_tile_count_kernel<K, V, decltype(mapped)::value>, tile_grid, block, 0, s, src, items, hdr,
                          tile_base, S.tile_counts, B, shift, x.neg, x.pos);
        }, x.mapped);
        if (rc) return rc;
        if ((rc = launch("segment_tile_offsets_kernel", segment_tile_offsets_kernel, item_grid, block, 0, s, hdr, tile_base, S.tile_counts, S.digit_base, B)))
            return rc;
        rc = with_bools([&](auto mapped) {
            return launch("segment_tile_scatter_kernel", segment_tile_scatter_kernel<K, V, decltype(mapped)::value>, tile_grid, block, 0, s, src, dst, vsrc,
                          vdst, items, hdr, tile_base, counts, bases, B, shift, x.neg, x.pos);
        }, x.mapped);
        if (rc) return rc;
    }
    if constexpr (LEVELS & 1) {
        const K* src = tmp_keys;
        const V* vsrc = tmp_vals;
        rc = launch("segment_tile_copy_kernel", segment_tile_copy_kernel<K, V>, tile_grid, block, 0, s, src, keys, vsrc, vals, items, hdr, tile_base, B);
    }
    return rc;
}

int launch_tiled(const SegCall& c, const PlanScratch& P, const TileScratch& S, const TileBounds& B, int cus, uint32_t* err) {
    return with_key_value_types(c.key_bytes, c.val_bytes, [&](auto k, auto v) {
        using K = decltype(k);
        using V = decltype(v);
        return launch_tiled_t(static_cast<K*>(c.keys), static_cast<V*>(c.vals), static_cast<K*>(c.tmp_keys), static_cast<V*>(c.tmp_vals), P, S, B, cus, err,
                              c.kind, c.s);
    });
}

// Both nowait entries.  Nothing between here and the return waits for the device or copies to the host: the plan, the two
// counted launches and the tiled launches are enqueued and the call returns.
int sort_segments_nowait(const SegCall& c, bool pair_entry, const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, void* scratch,
                         uint64_t scratch_bytes) {
    int rc = check_call(c, pair_entry, n_segments);
    if (rc || n_segments == 0) return rc;
    if ((rc = check_offsets_table(dev_offsets, offset_bytes, n_segments, c.len))) return rc;
    if (c.len >= (1ull << 32)) return set_error(RDST_ERR_UNSUPPORTED, "segments: the nowait entries take len below 2^32 (tile indices and positions inside an item are u32)");
    const uint32_t tile = L::block_max(c.key_bytes, c.val_bytes);
    if ((rc = check_scratch(scratch, scratch_bytes, L::tile_layout(n_segments, c.len, tile).total,
                            "segments: scratch_bytes is below rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(n_segments, len, ...)")))
        return rc;
    if ((rc = check_pointers(c, c.len != 0 ? "segments: the nowait entries need a tmp array of len elements" : nullptr))) return rc;
    const PlanScratch P = plan_scratch(scratch, n_segments);
    TileBounds B;
    TileScratch S;
    tile_scratch(scratch, n_segments, c.len, tile, &B, &S);
    uint32_t* err = nullptr;
    int cus = 0;
    if ((rc = rdst_internal::device_error_word(&err, &cus))) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    if ((rc = enqueue_plan(dev_offsets, offset_bytes, n_segments, c.len, c.key_bytes, c.val_bytes, P, 2u, err, c.s))) return rc;
    if ((rc = batched_stage(c.s, [&] { return launch_counted(c, P, n_segments); }))) return rc;
    if (B.n_long_bound == 0) return RDST_OK;  // no segment of this table can be longer than block_max
    if ((rc = launch_tiled(c, P, S, B, cus, err))) return rc;
    return rdst_internal::profile_stage_end(c.s, RDST_STAGE_SEGMENTS_TILED);
}

}  // namespace

int rdst_internal::stage_segment_items(int device, const rdst_segment_item* items, size_t count, void* dev_dst, hipStream_t s) {
    if (device < 0 || device >= (int)(sizeof g_staging / sizeof g_staging[0])) return set_error(RDST_ERR_ARG, "segments: device index beyond the staging buffers");
    return stage_items(g_staging[device], items, count, dev_dst, s);
}

int rdst_internal::check_offsets_table(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len) {
    return ::check_offsets_table(dev_offsets, offset_bytes, n_segments, len);
}

extern "C" int rdst_hip_sort_segments_device_offsets(void* dev_keys, void* dev_tmp, uint64_t tmp_elems, uint64_t len, const void* dev_offsets,
                                                     uint32_t offset_bytes, uint64_t n_segments, uint32_t elem_bytes, rdst_key_kind kind,
                                                     uint32_t levels, void* dev_scratch, uint64_t scratch_bytes, void* stream) {
    return sort_segments_offsets({dev_keys, nullptr, dev_tmp, nullptr, len, elem_bytes, 0, kind, levels, static_cast<hipStream_t>(stream)}, false, tmp_elems,
                                 dev_offsets, offset_bytes, n_segments, dev_scratch, scratch_bytes);
}

extern "C" int rdst_hip_sort_segments_pairs_device_offsets(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals, uint64_t tmp_elems,
                                                           uint64_t len, const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments,
                                                           uint32_t key_bytes, rdst_key_kind kind, uint32_t levels, uint32_t val_bytes,
                                                           void* dev_scratch, uint64_t scratch_bytes, void* stream) {
    return sort_segments_offsets({dev_keys, dev_vals, dev_tmp_keys, dev_tmp_vals, len, key_bytes, val_bytes, kind, levels, static_cast<hipStream_t>(stream)},
                                 true, tmp_elems, dev_offsets, offset_bytes, n_segments, dev_scratch, scratch_bytes);
}

extern "C" int rdst_hip_sort_segments_device_offsets_nowait(void* dev_keys, void* dev_tmp, uint64_t len, const void* dev_offsets, uint32_t offset_bytes,
                                                            uint64_t n_segments, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                                            void* dev_scratch, uint64_t scratch_bytes, void* stream) {
    return sort_segments_nowait({dev_keys, nullptr, dev_tmp, nullptr, len, elem_bytes, 0, kind, levels, static_cast<hipStream_t>(stream)}, false, dev_offsets,
                                offset_bytes, n_segments, dev_scratch, scratch_bytes);
}

extern "C" int rdst_hip_sort_segments_pairs_device_offsets_nowait(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals, uint64_t len,
                                                                  const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments,
                                                                  uint32_t key_bytes, rdst_key_kind kind, uint32_t levels, uint32_t val_bytes,
                                                                  void* dev_scratch, uint64_t scratch_bytes, void* stream) {
    return sort_segments_nowait({dev_keys, dev_vals, dev_tmp_keys, dev_tmp_vals, len, key_bytes, val_bytes, kind, levels, static_cast<hipStream_t>(stream)},
                                true, dev_offsets, offset_bytes, n_segments, dev_scratch, scratch_bytes);
}

extern "C" int rdst_hip_debug_segments_plan_device(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len,
                                                   uint32_t elem_bytes, uint32_t val_bytes, void* dev_scratch, uint64_t scratch_bytes,
                                                   rdst_segment_item* items_out, uint64_t capacity, uint64_t class_counts_out[3],
                                                   uint64_t* tmp_elems_out, uint32_t* flags_out, void* stream) {
    uint32_t lim[2];
    int rc = rdst_hip_sort_segments_limits(elem_bytes, val_bytes, lim);
    if (rc) return rc;
    if (!class_counts_out || !tmp_elems_out || !flags_out) return set_error(RDST_ERR_ARG, "segments_plan_device: null output");
    class_counts_out[0] = class_counts_out[1] = class_counts_out[2] = 0;
    *tmp_elems_out = 0;
    *flags_out = 0;
    if (n_segments == 0) return RDST_OK;
    if ((rc = check_offsets_args(dev_offsets, offset_bytes, n_segments, len, dev_scratch, scratch_bytes))) return rc;
    const PlanScratch P = plan_scratch(dev_scratch, n_segments);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    if ((rc = enqueue_plan(dev_offsets, offset_bytes, n_segments, len, elem_bytes, val_bytes, P, 0u, nullptr, s))) return rc;
    PlanResult r;
    if ((rc = read_plan(P, &r, s))) return rc;
    for (int c = 0; c < 3; ++c) class_counts_out[c] = r.counts[c];
    *tmp_elems_out = r.longest;
    *flags_out = r.flags;
    const uint64_t total = r.counts[0] + r.counts[1] + r.counts[2];
    if (r.flags || total == 0) return RDST_OK;  // (an invalid table: the flags are the answer, the items mean nothing)
    if (total > capacity) return set_error(RDST_ERR_ARG, "segments_plan_device: capacity too small for the work list");
    if (!items_out) return set_error(RDST_ERR_ARG, "segments_plan_device: null item table");
    RDST_HIP_TRY(hipMemcpyAsync(items_out, P.items, (size_t)total * sizeof(rdst_segment_item), hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    return RDST_OK;
}

extern "C" int rdst_hip_sort_segments_device(void* dev_keys, void* dev_tmp, uint64_t tmp_elems, uint64_t len, const uint64_t* offsets,
                                             uint64_t n_segments, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, void* stream) {
    return sort_segments({dev_keys, nullptr, dev_tmp, nullptr, len, elem_bytes, 0, kind, levels, static_cast<hipStream_t>(stream)}, false, tmp_elems, offsets,
                         n_segments);
}

extern "C" int rdst_hip_sort_segments_pairs_device(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals, uint64_t tmp_elems,
                                                   uint64_t len, const uint64_t* offsets, uint64_t n_segments, uint32_t key_bytes, rdst_key_kind kind,
                                                   uint32_t levels, uint32_t val_bytes, void* stream) {
    return sort_segments({dev_keys, dev_vals, dev_tmp_keys, dev_tmp_vals, len, key_bytes, val_bytes, kind, levels, static_cast<hipStream_t>(stream)}, true,
                         tmp_elems, offsets, n_segments);
}
