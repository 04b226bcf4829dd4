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

namespace {

using rdst_internal::launch;
using rdst_internal::set_error;

constexpr int RADIX = 256;
struct NoVal {};  // keys only
template <typename V> struct ValBytes { static constexpr int value = (int)sizeof(V); };
template <> struct ValBytes<NoVal> { static constexpr int value = 0; };

// Shapes.  rdst_hip_sort_segments_limits (rdst_segments.cpp) states the same numbers; limits_match() below checks them
// against each other before the first launch.
constexpr int SEG_WAVES = 4;  // segments per workgroup of the wave class
constexpr int wave_kpt(size_t key_bytes) { return key_bytes == 16 ? 4 : 8; }
constexpr int BLOCK_WAVES = 16;
constexpr int BLOCK_THREADS = BLOCK_WAVES * 64;
constexpr int block_kpt(size_t key_bytes, size_t val_bytes) {
    return val_bytes != 0 && key_bytes + val_bytes > 8 ? 8 : (key_bytes <= 4 ? 16 : (key_bytes == 8 ? 8 : 4));
}
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
__global__ __launch_bounds__(SEG_WAVES * 64) void segment_wave_kernel(K* __restrict__ keys, V* __restrict__ vals,
                                                                       const rdst_segment_item* __restrict__ items, uint32_t n_items, K neg, K pos) {
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
__global__ __launch_bounds__(BLOCK_THREADS) void segment_block_kernel(K* __restrict__ keys, V* __restrict__ vals,
                                                                      const rdst_segment_item* __restrict__ items, K neg, K pos) {
    constexpr bool HAS_V = ValBytes<V>::value != 0;
    constexpr int KPT = block_kpt(sizeof(K), ValBytes<V>::value);
    constexpr int TILE = BLOCK_THREADS * KPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* wave_hist = reinterpret_cast<uint32_t*>(smem);                              // [BLOCK_WAVES][256]
    uint32_t* s_sum = reinterpret_cast<uint32_t*>(smem + BLOCK_WAVES * 1024);             // [4]
    K* stage = reinterpret_cast<K*>(smem + BLOCK_WAVES * 1024 + 16);                      // [TILE]
    V* vstage = reinterpret_cast<V*>(smem + BLOCK_WAVES * 1024 + 16 + sizeof(K) * TILE);  // [TILE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const rdst_segment_item it = items[blockIdx.x];  // the grid is exactly this class's items
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

#define SEG_HIP_TRY(expr)                                                   \
    do {                                                                    \
        hipError_t e__ = (expr);                                            \
        if (e__ != hipSuccess) return set_error(RDST_ERR_HIP, #expr, e__);  \
    } while (0)

int stage_items(Staging& st, const rdst_segment_item* items, size_t count, void* dev_dst, hipStream_t s) {
    const size_t bytes = count * sizeof(rdst_segment_item);
    if (st.in_flight) {  // the previous call's copy still reads the buffer
        SEG_HIP_TRY(hipEventSynchronize(st.copied));
        st.in_flight = false;
    }
    if (!st.copied) SEG_HIP_TRY(hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    if (st.bytes < bytes) {
        if (st.host) SEG_HIP_TRY(hipHostFree(st.host));
        st.host = nullptr;
        st.bytes = 0;
        const size_t want = (bytes + bytes / 4 + 4095) / 4096 * 4096;
        SEG_HIP_TRY(hipHostMalloc(&st.host, want, hipHostMallocDefault));
        st.bytes = want;
    }
    memcpy(st.host, items, bytes);
    SEG_HIP_TRY(hipMemcpyAsync(dev_dst, st.host, bytes, hipMemcpyHostToDevice, s));
    SEG_HIP_TRY(hipEventRecord(st.copied, s));
    st.in_flight = true;
    return RDST_OK;
}

template <typename K, typename V>
bool limits_match() {
    uint32_t lim[2] = {0, 0};
    return rdst_hip_sort_segments_limits((uint32_t)sizeof(K), (uint32_t)ValBytes<V>::value, lim) == RDST_OK &&
           lim[0] == 64u * wave_kpt(sizeof(K)) && lim[1] == (uint32_t)BLOCK_THREADS * block_kpt(sizeof(K), ValBytes<V>::value);
}

template <typename K, typename V>
int launch_batched(K* keys, V* vals, const rdst_segment_item* dev_items, uint64_t n_wave, uint64_t n_block, rdst_key_kind kind, hipStream_t s) {
    constexpr int LEVELS = (int)sizeof(K);
    constexpr size_t VB = ValBytes<V>::value;
    static_assert(wave_lds_bytes(sizeof(K), VB) <= LDS_LIMIT && block_lds_bytes(sizeof(K), VB) <= LDS_LIMIT, "a workgroup's LDS stays within 160 KiB");
    if (!limits_match<K, V>()) return set_error(RDST_ERR_ARG, "segments: the kernels' shapes and rdst_hip_sort_segments_limits disagree");
    unsigned __int128 neg128, pos128;
    rdst_internal::key_xor_masks(kind, (uint32_t)sizeof(K), &neg128, &pos128);
    const K neg = (K)neg128, pos = (K)pos128;
    const bool mapped = neg128 != 0 || pos128 != 0;
    int rc = RDST_OK;
    if (n_wave) {
        const dim3 grid((uint32_t)((n_wave + SEG_WAVES - 1) / SEG_WAVES));
        rc = mapped ? launch("segment_wave_kernel", segment_wave_kernel<K, V, LEVELS, true>, grid, dim3(SEG_WAVES * 64), wave_lds_bytes(sizeof(K), VB), s, keys,
                             vals, dev_items, (uint32_t)n_wave, neg, pos)
                    : launch("segment_wave_kernel", segment_wave_kernel<K, V, LEVELS, false>, grid, dim3(SEG_WAVES * 64), wave_lds_bytes(sizeof(K), VB), s, keys,
                             vals, dev_items, (uint32_t)n_wave, neg, pos);
        if (rc) return rc;
    }
    if (n_block) {
        const dim3 grid((uint32_t)n_block);
        const rdst_segment_item* block_items = dev_items + n_wave;
        rc = mapped ? launch("segment_block_kernel", segment_block_kernel<K, V, LEVELS, true>, grid, dim3(BLOCK_THREADS), block_lds_bytes(sizeof(K), VB), s, keys,
                             vals, block_items, neg, pos)
                    : launch("segment_block_kernel", segment_block_kernel<K, V, LEVELS, false>, grid, dim3(BLOCK_THREADS), block_lds_bytes(sizeof(K), VB), s, keys,
                             vals, block_items, neg, pos);
    }
    return rc;
}

int dispatch_batched(void* keys, void* vals, uint32_t key_bytes, uint32_t val_bytes, const rdst_segment_item* dev_items, uint64_t n_wave,
                     uint64_t n_block, rdst_key_kind kind, hipStream_t s) {
    NoVal* const none = nullptr;
    if (val_bytes == 0) {
        switch (key_bytes) {
            case 1: return launch_batched(static_cast<uint8_t*>(keys), none, dev_items, n_wave, n_block, kind, s);
            case 2: return launch_batched(static_cast<uint16_t*>(keys), none, dev_items, n_wave, n_block, kind, s);
            case 4: return launch_batched(static_cast<uint32_t*>(keys), none, dev_items, n_wave, n_block, kind, s);
            case 8: return launch_batched(static_cast<uint64_t*>(keys), none, dev_items, n_wave, n_block, kind, s);
            default: return launch_batched(static_cast<u128*>(keys), none, dev_items, n_wave, n_block, kind, s);
        }
    }
    if (key_bytes == 4)
        return val_bytes == 4 ? launch_batched(static_cast<uint32_t*>(keys), static_cast<uint32_t*>(vals), dev_items, n_wave, n_block, kind, s)
                              : launch_batched(static_cast<uint32_t*>(keys), static_cast<uint64_t*>(vals), dev_items, n_wave, n_block, kind, s);
    return val_bytes == 4 ? launch_batched(static_cast<uint64_t*>(keys), static_cast<uint32_t*>(vals), dev_items, n_wave, n_block, kind, s)
                          : launch_batched(static_cast<uint64_t*>(keys), static_cast<uint64_t*>(vals), dev_items, n_wave, n_block, kind, s);
}

// Both entries.  val_bytes == 0: keys only (vals, tmp_vals unused).
int sort_segments(void* keys, void* vals, void* tmp_keys, void* tmp_vals, uint64_t tmp_elems, uint64_t len, const uint64_t* offsets,
                  uint64_t n_segments, uint32_t key_bytes, rdst_key_kind kind, uint32_t levels, uint32_t val_bytes, void* stream) {
    const bool pairs = val_bytes != 0;
    // with no segment there is nothing the pointers could be used for
    int rc = rdst_internal::check_key_args(keys, n_segments ? len : 0, key_bytes, kind, levels);
    if (rc) return rc;
    if (n_segments == 0) return RDST_OK;
    std::vector<rdst_segment_item> items;
    uint64_t counts[3] = {0, 0, 0}, longest = 0;
    rc = rdst_segments_plan(offsets, n_segments, len, key_bytes, val_bytes, nullptr, 0, counts, &longest);
    const uint64_t total = counts[0] + counts[1] + counts[2];
    if (rc != RDST_OK && !(rc == RDST_ERR_ARG && total > 0)) return rc;  // (a work list that does not fit capacity 0 is the expected answer)
    if (total == 0) return RDST_OK;
    items.resize(total);
    if ((rc = rdst_segments_plan(offsets, n_segments, len, key_bytes, val_bytes, items.data(), total, counts, &longest))) return rc;
    if (pairs && vals == nullptr) return set_error(RDST_ERR_ARG, "null value pointer");
    if (pairs && reinterpret_cast<uintptr_t>(vals) % val_bytes) return set_error(RDST_ERR_ALIGN, "value pointer not aligned to the value size");
    if (reinterpret_cast<uintptr_t>(tmp_keys) % key_bytes) return set_error(RDST_ERR_ALIGN, "tmp pointer not aligned to the element size");
    if (pairs && reinterpret_cast<uintptr_t>(tmp_vals) % val_bytes) return set_error(RDST_ERR_ALIGN, "tmp value pointer not aligned to the value size");
    if (counts[2] != 0) {
        if (tmp_keys == nullptr || (pairs && tmp_vals == nullptr)) return set_error(RDST_ERR_ARG, "segments: a segment beyond block_max needs a tmp array");
        if (tmp_elems < longest) return set_error(RDST_ERR_ARG, "segments: tmp_elems is below the longest segment beyond block_max");
    }
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t batched = counts[0] + counts[1];
    if (counts[1] >= (1ull << 31)) return set_error(RDST_ERR_ARG, "segments: too many block-class segments for one launch");
    // the workspace is sized ONCE, for the work list and for every long segment: a growth between the launches would free
    // memory the batched kernels were handed
    const size_t table_bytes = (size_t)batched * sizeof(rdst_segment_item);
    size_t ws_bytes = table_bytes;
    for (uint64_t i = batched; i < total; ++i) {
        const uint32_t sg = items[i].seg;
        ws_bytes = std::max(ws_bytes, rdst_internal::slice_workspace_bytes(offsets[sg + 1] - offsets[sg], key_bytes, kind, val_bytes));
    }
    void* ws = nullptr;
    int dev = 0;
    rc = rdst_internal::workspace_take(ws_bytes, s, &ws, &dev);
    if (rc && ws_bytes > table_bytes) rc = rdst_internal::workspace_take(std::max<size_t>(table_bytes, 256), s, &ws, &dev);  // no room: a long segment then picks its lean layout itself
    if (rc) return rc;
    if (batched) {
        if ((rc = rdst_internal::profile_open_run(s))) return rc;
        if ((rc = stage_items(g_staging[dev], items.data(), (size_t)batched, ws, s))) return rc;
        if ((rc = dispatch_batched(keys, vals, key_bytes, val_bytes, static_cast<const rdst_segment_item*>(ws), counts[0], counts[1], kind, s))) return rc;
        if ((rc = rdst_internal::profile_stage_end(s, RDST_STAGE_SEGMENTS))) return rc;
        if ((rc = rdst_internal::workspace_handback(s))) return rc;
    }
    // long segments one after another; each uses the workspace (the work list is dead by then, in stream order)
    for (uint64_t i = batched; i < total; ++i) {
        const uint32_t sg = items[i].seg;
        const uint64_t start = offsets[sg], n = offsets[sg + 1] - offsets[sg];
        char* k = static_cast<char*>(keys) + start * key_bytes;
        rc = pairs ? rdst_internal::sort_pairs_slice_locked(k, static_cast<char*>(vals) + start * val_bytes, tmp_keys, tmp_vals, n, key_bytes, kind, val_bytes, s)
                   : rdst_internal::sort_slice_locked(k, tmp_keys, n, key_bytes, kind, s);
        if (rc) return rc;
    }
    return RDST_OK;
}

}  // namespace

extern "C" int rdst_hip_sort_segments_device(void* dev_keys, void* dev_tmp, uint64_t tmp_elems, uint64_t len, const uint64_t* offsets,
                                             uint64_t n_segments, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, void* stream) {
    return sort_segments(dev_keys, nullptr, dev_tmp, nullptr, tmp_elems, len, offsets, n_segments, elem_bytes, kind, levels, 0, stream);
}

extern "C" int rdst_hip_sort_segments_pairs_device(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals, uint64_t tmp_elems,
                                                   uint64_t len, const uint64_t* offsets, uint64_t n_segments, uint32_t key_bytes, rdst_key_kind kind,
                                                   uint32_t levels, uint32_t val_bytes, void* stream) {
    int rc = rdst_internal::check_key_args(dev_keys, n_segments ? len : 0, key_bytes, kind, levels);
    if (rc) return rc;
    if (key_bytes != 4 && key_bytes != 8) return set_error(RDST_ERR_UNSUPPORTED, "key-value sorts take 4- or 8-byte keys");
    if (val_bytes != 4 && val_bytes != 8) return set_error(RDST_ERR_UNSUPPORTED, "key-value sorts carry 4- or 8-byte values");
    return sort_segments(dev_keys, dev_vals, dev_tmp_keys, dev_tmp_vals, tmp_elems, len, offsets, n_segments, key_bytes, kind, levels, val_bytes, stream);
}
