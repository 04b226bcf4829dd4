// rdst_stream.h — what the radix selects (rdst_topk.hip, rdst_select.hip) share: the reader that streams the input exactly at
// every length and alignment, the shape of a select level, the collected element and the per-wave stage of the collection
// pass.  Every TU gets its own copy (anonymous namespace, all of it inlined).
#ifndef RDST_STREAM_H
#define RDST_STREAM_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rdst_device.h"

namespace {

// level l of a field of `bits` bits: its digit is the bits [shift, shift + nbits)
inline void level_shape(uint32_t bits, uint32_t digit, uint32_t l, int* shift, uint32_t* nbits) {
    const uint32_t hi = bits - l * digit;
    const uint32_t lo = hi > digit ? hi - digit : 0;
    *shift = (int)lo;
    *nbits = hi - lo;
}

template <typename K>
__device__ __forceinline__ K header_key(const uint64_t w[2]) {
    if constexpr (sizeof(K) == 16) return (K)w[0] | ((K)w[1] << 64);
    else return (K)w[0];
}

template <typename K>
struct alignas(16) KeyVec {
    static constexpr int N = 16 / (int)sizeof(K);
    K e[N];
};

template <typename K>
__device__ __forceinline__ KeyVec<K> load_vec(const K* p) {  // p is 16-byte aligned
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    KeyVec<K> v;
    __builtin_memcpy(&v, &raw, 16);
    return v;
}

// How a kernel that streams the input cuts it: a scalar head up to the first 16-byte boundary, whole 16-byte vectors, a scalar
// tail.  Exact for any len and any element-aligned pointer.
template <typename K>
struct StreamCut {
    uint32_t head, nvec, tail_start, len;
    __device__ StreamCut(const K* keys, uint32_t n) {
        constexpr uint32_t VEC = KeyVec<K>::N;
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(keys) & 15u);
        uint32_t h = mis ? (16u - mis) / (uint32_t)sizeof(K) : 0u;
        head = h < n ? h : n;
        nvec = (n - head) / VEC;
        tail_start = head + nvec * VEC;
        len = n;
    }
};

// Calls visit(raw_key, position, valid) for every element, with ALL 64 lanes of a wave in every call (visit may ballot):
// lanes without an element pass valid == false.  UNROLL: 16-byte loads in flight per lane.
template <typename K, int UNROLL, typename F>
__device__ __forceinline__ void stream_keys(const K* __restrict__ keys, uint32_t len, F&& visit) {
    constexpr uint32_t VEC = KeyVec<K>::N;
    const StreamCut<K> cut(keys, len);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const K* body = keys + cut.head;
    // wave-uniform loop bound: a wave goes on while its first lane has a vector
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + tid; v - lane < cut.nvec; v += stride * UNROLL) {
        KeyVec<K> vec[UNROLL];
        bool ok[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint64_t vi = v + (uint64_t)u * stride;
            ok[u] = vi < cut.nvec;
            if (ok[u]) vec[u] = load_vec<K>(body + vi * VEC);
            else
                for (uint32_t j = 0; j < VEC; ++j) vec[u].e[j] = 0;
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint64_t vi = v + (uint64_t)u * stride;
            if (__builtin_amdgcn_ballot_w64(ok[u]) == 0) continue;  // wave-uniform
#pragma unroll
            for (uint32_t j = 0; j < VEC; ++j) visit(vec[u].e[j], (uint32_t)(cut.head + vi * VEC + j), ok[u]);
        }
    }
    // head and tail: fewer than 2 * 16 / sizeof(K) <= 32 elements, one wave
    if (blockIdx.x == 0 && tid < 64) {
        const uint32_t tail_n = cut.len - cut.tail_start;
        if (cut.head + tail_n != 0) {
            const bool valid = lane < cut.head + tail_n;
            const uint32_t idx = lane < cut.head ? lane : cut.tail_start + (lane - cut.head);
            const K raw = valid ? keys[idx] : (K)0;
            visit(raw, idx, valid);
        }
    }
}

// One counter more for every `hit` lane (its counter: lds[d]).  A wave whose hits all land on one counter adds once: without
// it an input of equal keys serialises on one address.  `bal`: the ballot of `hit`, not 0.  All 64 lanes call it.
__device__ __forceinline__ void wave_count(uint32_t* lds, uint32_t d, bool hit, uint64_t bal, uint32_t lane) {
    const uint32_t first = (uint32_t)__builtin_ctzll(bal);
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)first);
    if (__builtin_amdgcn_ballot_w64(hit && d == d0) == bal) {  // every hit of the wave on one counter: one add
        if (lane == first) atomicAdd(&lds[d0], (uint32_t)__builtin_popcountll(bal));
    } else if (hit) {
        atomicAdd(&lds[d], 1u);
    }
}

// The element that is collected and sorted: the mapped key, or with an index the composite (mapped key, position).
template <typename K, typename C>
__device__ __forceinline__ C compose(K m, uint32_t idx) {
    if constexpr (sizeof(C) == sizeof(K)) return (C)m;
    else return (C)((C)m << (8 * sizeof(K))) | (C)idx;
}

// orders this wave's LDS accesses: nothing moves across it, in the compiler or in the wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One wave's stage of one class, handed to the output: ONE atomic on the class's cursor claims the range.  `count` is
// wave-uniform.  Claims on a single address serialise (one per element that is kept cost 13 ms per 10^6 kept elements), hence
// the stages: a claim per stage of kept elements and one per wave at the end.
template <typename C>
__device__ __forceinline__ void flush_stage(const C* stage, uint32_t count, uint32_t* cursor, C* __restrict__ dst, uint32_t limit, uint32_t lane) {
    if (count == 0) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(cursor, count);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    wave_sync();
    for (uint32_t i = lane; i < count; i += 64)
        if (base + i < limit) dst[base + i] = stage[i];
    wave_sync();
}

}  // namespace

#endif  // RDST_STREAM_H
