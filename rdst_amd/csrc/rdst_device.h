// rdst_device.h — device helpers shared by the library's HIP translation units (rdst_kernels.hip, rdst_segments.hip, rdst_topk.hip,
// rdst_topk_segments.hip): the
// order-preserving key map, digit extraction and the wave-level digit ranking.  Every TU gets its own copy (anonymous
// namespace, all of it inlined).
#ifndef RDST_DEVICE_H
#define RDST_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef unsigned __int128 u128;  // u128 / i128 keys (src/radix_key_impl.rs:39-46, :123-130)

struct KeyMap {  // order-preserving map as two xor masks (src/radix_key_impl.rs)
    u128 neg;  // xor applied when the sign bit is set
    u128 pos;  // xor applied when it is clear
};

// look-back status word: top two bits state, the rest value (u32 for n < 2^30, u64 above)
constexpr uint32_t ST_EMPTY = 0, ST_AGG = 1, ST_INCL = 2;
template <typename S> struct StatusWord {
    static constexpr int SHIFT = sizeof(S) * 8 - 2;
    static constexpr S MASK = (S(1) << SHIFT) - 1;
};
// bounded spins: s_sleep(2) is ~128 clocks; 1<<22 polls is seconds, never reached in a healthy run
constexpr uint32_t SPIN_LIMIT = 1u << 22;

template <typename S>
__device__ __forceinline__ S ld_relaxed(const S* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename S>
__device__ __forceinline__ void st_relaxed(S* p, S v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename K>
__device__ __forceinline__ K map_key(K k, K neg, K pos) {
    constexpr int W = sizeof(K) * 8;
    return (K)(k ^ ((K)(k >> (W - 1)) ? neg : pos));
}
template <typename K>
__device__ __forceinline__ K unmap_key(K m, K neg, K pos) {
    constexpr int W = sizeof(K) * 8;
    return (K)(m ^ ((K)(m >> (W - 1)) ? pos : neg));
}
template <typename K>
__device__ __forceinline__ uint32_t digit_of(K mapped, int shift) {
    return (uint32_t)(mapped >> shift) & 0xFFu;
}

// lanes of this wave holding the same 8-bit digit (all 64 lanes must be active)
__device__ __forceinline__ uint64_t match_any8(uint32_t d) {
    uint64_t m = ~0ull;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {  // popcount(mask & lanes < me)
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// lanes below me holding my digit, 4 VALU per bit: my bit as a 0 / -1 mask (v_bfe_i32), the
// wave's ballot of that bit (v_cmp), then per 32-lane half ONE v_bitop3_b32 that keeps in `same`
// only the lanes whose bit equals mine:  same &= ~(ballot ^ my_bit)   (truth table 0x90).
__device__ __forceinline__ uint32_t peers_below(uint32_t word, int bit0) {
    // bit by bit (ballot, then the two mask updates that read it): computing the eight ballots first
    // removes the wait states after each ballot but measured 4-6 % slower (64-bit encodings, 16 more SGPRs live)
    uint32_t same_lo = ~0u, same_hi = ~0u;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int m = __builtin_amdgcn_sbfe((int)word, (unsigned)(bit0 + b), 1u);  // 0 or -1
        const uint64_t bal = __builtin_amdgcn_ballot_w64(m != 0);
        same_lo = __builtin_amdgcn_bitop3_b32(same_lo, (uint32_t)bal, (uint32_t)m, 0x90);
        same_hi = __builtin_amdgcn_bitop3_b32(same_hi, (uint32_t)(bal >> 32), (uint32_t)m, 0x90);
    }
    return __builtin_amdgcn_mbcnt_hi(same_hi, __builtin_amdgcn_mbcnt_lo(same_lo, 0u));
}

template <typename K>
__device__ __forceinline__ uint32_t digit_word(K mapped, int shift) {  // 32-bit half that holds the digit
    if constexpr (sizeof(K) > 4) return (uint32_t)(mapped >> (shift & ~31));
    else return (uint32_t)mapped;
}

// The inverse of map_key for ANY pair of masks (the complemented ones of RDST_TOPK_LARGEST too): the preimage whose sign
// bit picks the mask it was mapped with.
template <typename K>
__device__ __forceinline__ K unmap_any(K m, K neg, K pos) {
    const K a = (K)(m ^ neg);
    return (K)(a >> (sizeof(K) * 8 - 1)) ? a : (K)(m ^ pos);
}

// The bucket pick of a radix select, by one workgroup of 1024 threads over 4096 counters: thread t holds the counters
// 4 t .. 4 t + 3 in c.  The ONE thread whose counters hold the `remaining`-th key (1 <= remaining <= the sum of all counters)
// returns true, with *before = the keys in the buckets before the picked one and *j = the picked bucket's place in c.
// `wave_sum`: 16 words of LDS.  Every thread of the workgroup calls it (one barrier inside).
__device__ __forceinline__ bool pick_bucket(const uint32_t (&c)[4], uint32_t remaining, uint32_t* wave_sum, uint32_t* before, int* j) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t sum = c[0] + c[1] + c[2] + c[3];
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t earlier = 0;
    for (uint32_t w = 0; w < wave; ++w) earlier += wave_sum[w];
    incl += earlier;
    uint32_t run = incl - sum;
    if (!(run < remaining && remaining <= incl)) return false;
    int at = 0;
    while (at < 3 && run + c[at] < remaining) run += c[at++];
    *before = run;
    *j = at;
    return true;
}

}  // namespace

#endif  // RDST_DEVICE_H
