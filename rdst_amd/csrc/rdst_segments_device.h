// rdst_segments_device.h — what the segmented partial sort (rdst_topk_segments.hip) and the segmented select
// (rdst_select_segments.hip) share on the device: the shapes of their three batched classes, the wave class's and the block
// class's level loops, the 16-byte reader of the stream class, one counting read of its radix select and the ordered
// compaction that fills the LDS stage.  Every TU gets its own copy (anonymous namespace, all of it inlined).
#ifndef RDST_SEGMENTS_DEVICE_H
#define RDST_SEGMENTS_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdst_device.h"
#include "rdst_segments_layout.h"

namespace {

namespace L = rdst_segments_layout;

constexpr int RADIX = 256;
constexpr int SEG_WAVES = 4;  // segments per workgroup of the wave class
constexpr int BLOCK_THREADS = L::BLOCK_THREADS;
constexpr int BLOCK_WAVES = BLOCK_THREADS / 64;
constexpr uint32_t COUNTERS = 4096;  // the select's count table: it lies over the level loop's per-wave digit tables
static_assert(COUNTERS == BLOCK_WAVES * RADIX && COUNTERS == 4 * BLOCK_THREADS, "one table in the place of the other, four counters per thread");
constexpr int STREAM_UNROLL = 4;  // 16-byte loads in flight per thread
constexpr size_t LDS_LIMIT = 160 << 10;
// bound on the stream kernels' static LDS: wave totals, select state, the select's rank lists, and SYNC_OR_LDS
constexpr size_t STREAM_STATIC_LDS = 2048;
// What the compiler keeps for __syncthreads_or (block_order): read from the built kernels' static LDS with ROCm 7.2 (HIP
// 7.2.26015); tools/kernel_resources.py prints static_lds, which must stay below STREAM_STATIC_LDS with any other compiler.
constexpr size_t SYNC_OR_LDS = 256;

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

// ---- wave class: the level loop ----------------------------------------------------------------------------------------------

// Orders one wave's keys (and positions): key index = round * 64 + lane, before and after.  `rounds` is wave-uniform; `tbl`
// (256 words), `stage` and `vstage` (64 * KPT elements each) are this wave's own LDS.
template <typename K, bool IDX, int KPT>
__device__ __forceinline__ void wave_order(K (&mk)[KPT], uint32_t (&mv)[KPT], int rounds, uint32_t* tbl, K* stage, uint32_t* vstage) {
    constexpr int LEVELS = (int)sizeof(K);
    const int lane = threadIdx.x & 63;
    const uint32_t live = (uint32_t)rounds * 64u;
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

// The first `filled` elements of the stage into registers, in block_order's layout, and ordered: slots past `filled` hold the
// largest mapped key.  The stage is complete when the workgroup gets here (a barrier precedes the call).
template <typename K, bool IDX, int KPT>
__device__ __forceinline__ void order_stage(K (&rk)[KPT], uint32_t (&rv)[KPT], uint32_t filled, int rounds, const BlockLds<K, IDX>& lds) {
    const uint32_t wbase = (threadIdx.x >> 6) * 64u * (uint32_t)rounds + (threadIdx.x & 63u);
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

// How one workgroup reads its segment: a scalar head up to the first 16-byte boundary, whole 16-byte vectors, a scalar tail.
template <typename K>
struct SegmentCut {
    static constexpr uint32_t VEC = KeyVec<K>::N;
    static constexpr uint32_t TRIP = (uint32_t)BLOCK_THREADS * STREAM_UNROLL;  // vectors per trip of the workgroup
    const K* seg;
    const K* body;
    uint32_t n, head, nvec, tail_start, tail_n;
    __device__ SegmentCut(const K* s, uint32_t len) : seg(s), n(len) {
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 15u);
        const uint32_t head_want = mis ? (16u - mis) / (uint32_t)sizeof(K) : 0u;
        head = head_want < len ? head_want : len;
        nvec = (len - head) / VEC;
        tail_start = head + nvec * VEC;
        tail_n = len - tail_start;
        body = s + head;
    }
};

// One counting read of the select: the digit (mapped >> shift) & dmask of every key of the segment that lies on the prefix,
// into the 4 096 counters `cnt`.  Every thread of the workgroup calls it; the counters are complete when it returns.
template <typename K>
__device__ __forceinline__ void count_digits(const SegmentCut<K>& cut, K neg, K pos, K pref, K pmask, int shift, uint32_t dmask, uint32_t* cnt) {
    constexpr uint32_t VEC = SegmentCut<K>::VEC, TRIP = SegmentCut<K>::TRIP;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
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
            const K mk = map_key<K>(v.e[j], neg, pos);
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
    for (uint64_t base = 0; base < cut.nvec; base += TRIP) {  // block-uniform
        KeyVec<K> vec[STREAM_UNROLL];
        bool ok[STREAM_UNROLL];
#pragma unroll
        for (int u = 0; u < STREAM_UNROLL; ++u) {
            const uint64_t vi = base + (uint64_t)u * BLOCK_THREADS + tid;
            ok[u] = vi < cut.nvec;
            if (ok[u]) vec[u] = load_vec<K>(cut.body + vi * VEC);
            else
                for (uint32_t j = 0; j < VEC; ++j) vec[u].e[j] = 0;
        }
#pragma unroll
        for (int u = 0; u < STREAM_UNROLL; ++u) count_vec(vec[u], ok[u]);
    }
    if (tid < cut.head + cut.tail_n) {  // head and tail: fewer than 2 * 16 / sizeof(K) <= 32 elements
        const K mk = map_key<K>(cut.seg[tid < cut.head ? tid : cut.tail_start + (tid - cut.head)], neg, pos);
        if ((K)(mk & pmask) == pref) atomicAdd(&cnt[(uint32_t)(mk >> shift) & dmask], 1u);
    }
    __syncthreads();
}

// One trip of the ordered compaction: G groups of E elements per thread, position order = (group, thread, element).
// BEFORE: keeps every key before the prefix and the keys on it while fewer than `lim` of those were kept; a kept element's
// slot is the number of kept elements before it.  Not BEFORE: keeps the keys on the prefix whose ordinal among them, in
// position order, lies in [first, first + tile), at slot ordinal - first; keys before the prefix are only counted.
// tot_b / tot_o: the keys before / on the prefix seen so far (block-uniform).  Every thread of the workgroup calls it; one
// barrier, and `wave_tot` alternates between two buffers from trip to trip.
template <typename K, bool IDX, bool BEFORE, int G, int E>
__device__ __forceinline__ void collect_trip(const K (&m)[G][E], const bool (&ok)[G], const uint32_t (&pos0)[G], K pref, K pmask, uint32_t lim,
                                             uint32_t first, uint32_t tile, K* stage, uint32_t* vstage, uint32_t (*wave_tot)[BLOCK_WAVES],
                                             uint32_t& tot_b, uint32_t& tot_o) {
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
                if constexpr (BEFORE) {
                    if (before || (is_on && on < lim)) {
                        const uint32_t slot = b + (on < lim ? on : lim);
                        if (slot < tile) {  // (it is: b <= c_below and on <= lim; a store outside the stage is never made)
                            stage[slot] = m[g][e];
                            if constexpr (IDX) vstage[slot] = pos0[g] + (uint32_t)e;
                        }
                    }
                } else {
                    const uint32_t slot = on - first;  // (an ordinal before the window wraps beyond the tile)
                    if (is_on && slot < tile) {
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

// The collecting read of a whole segment, in position order: head, vectors, tail; collect_trip says what is kept.  Every
// thread of the workgroup calls it, after a barrier behind the last use of `wave_tot`; the stage is complete after the next
// barrier.  tot_b / tot_o: the keys of the segment before / on the prefix.
template <typename K, bool IDX, bool BEFORE>
__device__ __forceinline__ void collect_segment(const SegmentCut<K>& cut, K neg, K pos, K pref, K pmask, uint32_t lim, uint32_t first, uint32_t tile,
                                                K* stage, uint32_t* vstage, uint32_t (*wave_tot)[STREAM_UNROLL][BLOCK_WAVES], uint32_t& tot_b,
                                                uint32_t& tot_o) {
    constexpr uint32_t VEC = SegmentCut<K>::VEC, TRIP = SegmentCut<K>::TRIP;
    const uint32_t tid = threadIdx.x;
    uint32_t parity = 0;
    tot_b = 0;
    tot_o = 0;
    const auto scalar_trip = [&](uint32_t first_at, uint32_t count) {  // block-uniform arguments; count <= 16
        const bool ok[1] = {tid < count};
        const K one[1][1] = {{ok[0] ? map_key<K>(cut.seg[first_at + tid], neg, pos) : (K)0}};
        const uint32_t pos0[1] = {first_at + tid};
        collect_trip<K, IDX, BEFORE, 1, 1>(one, ok, pos0, pref, pmask, lim, first, tile, stage, vstage, wave_tot[parity], tot_b, tot_o);
        parity ^= 1u;
    };
    if (cut.head) scalar_trip(0, cut.head);
    for (uint64_t base = 0; base < cut.nvec; base += TRIP) {  // block-uniform
        K mk[STREAM_UNROLL][VEC];
        bool ok[STREAM_UNROLL];
        uint32_t pos0[STREAM_UNROLL];
#pragma unroll
        for (int u = 0; u < STREAM_UNROLL; ++u) {
            const uint64_t vi = base + (uint64_t)u * BLOCK_THREADS + tid;
            ok[u] = vi < cut.nvec;
            pos0[u] = cut.head + (uint32_t)vi * VEC;
            KeyVec<K> v;
            if (ok[u]) v = load_vec<K>(cut.body + vi * VEC);
            else
                for (uint32_t j = 0; j < VEC; ++j) v.e[j] = 0;
#pragma unroll
            for (uint32_t j = 0; j < VEC; ++j) mk[u][j] = map_key<K>(v.e[j], neg, pos);
        }
        collect_trip<K, IDX, BEFORE, STREAM_UNROLL, (int)VEC>(mk, ok, pos0, pref, pmask, lim, first, tile, stage, vstage, wave_tot[parity], tot_b, tot_o);
        parity ^= 1u;
    }
    if (cut.tail_n) scalar_trip(cut.tail_start, cut.tail_n);
}

}  // namespace

#endif  // RDST_SEGMENTS_DEVICE_H
