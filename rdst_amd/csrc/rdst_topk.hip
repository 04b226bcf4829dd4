// rdst_topk.hip — partial sort: the k keys that come first (RDST_TOPK_LARGEST: last) in mapped-key order, in that order, with
// the input position of each if asked for (rdst_hip_topk_device; include/rdst_hip.h).
//
// A radix select over the mapped key M of rdst_device.h (complemented for "largest"), most significant digit first.  The
// state lives in the header of the caller's scratch: the prefix found so far (a value and a mask), the number of keys strictly
// before it (c_below), the size of its bucket (m) and a ready flag.
//
//   topk_hist_kernel<K>     one read of the input: counts the next digit of the keys that lie on the prefix.  Launched once per
//                           possible level; returns at once when ready is set.
//   topk_pick_kernel        one workgroup: finds the bucket that holds the (k - c_below)-th key, extends the prefix, zeroes the
//                           counters, sets ready when the bucket fits cand_capacity or the digits are exhausted.
//   topk_collect_kernel     one read of the input: elements before the prefix go to the selected buffer (fewer than k), elements
//                           on the prefix to the candidate buffer (at most cand_capacity).  Every wave gathers what it keeps in
//                           an LDS stage of its own per class and claims output space with one atomic per full stage: no spinning,
//                           no waits between workgroups, no workgroup barrier.  The order inside the two buffers is whatever the
//                           claims gave; both are sorted next.
//   topk_append_kernel      the first k - c_below of the sorted candidates behind the selected ones.
//   topk_finish_kernel      the k sorted elements back to original key bits (and positions of index_bytes bytes).
//
// With an index the element that is selected, collected and sorted is the COMPOSITE (M << 32 | position) for 4-byte keys and
// (M << 64 | position) for 8-byte keys: one unsigned integer of twice the key's width.  Sorting composites as plain keys gives
// "ascending M, equal keys in ascending position" in one keys-only sort, and the levels past the last key digit run over the
// position's digits, so the candidate set always ends within cand_capacity.  Keys only, digits exhausted and the bucket still
// over cand_capacity: every candidate is the same key T, and the output gets k - c_below copies of it.
//
// The candidates' count is known to the device only: they are sorted by the device-length pipeline (sort_slice_devlen_locked)
// sized for cand_capacity; the k selected ones by the whole-slice pipeline (sort_slice_nowait_locked: the routes the device
// decides on, never the split of slices beyond the window, which waits for counts — k may be anything below 2^32).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_device.h"
#include "rdst_stream.h"
#include "rdst_topk_layout.h"

namespace {

using namespace rdst_topk_layout;  // the digits, the room of the header, topk_layout: shared with rdst_rank_args.cpp
using namespace rdst_args;          // levels_over, POSITION_BITS
using rdst_internal::launch;
using rdst_internal::set_error;

constexpr int HIST_THREADS = 256;
constexpr int HIST_UNROLL = 4;                // 16-byte loads in flight per lane
constexpr uint32_t STAGE_BYTES = 4096;       // collection: LDS per wave and class between two claims of output space
constexpr int PICK_THREADS = 1024;
constexpr int BLOCKS_PER_CU = 8;

struct TopkHeader {  // the first HEADER_BYTES of the scratch
    uint32_t ready;        // no further level is needed
    uint32_t depth;        // levels used
    uint32_t c_below;      // keys strictly before the prefix
    uint32_t m;            // keys on the prefix
    uint32_t special;      // the keys-only fill or a position digit was reached
    uint32_t fill;         // keys only: digits exhausted with m > cand_capacity
    uint32_t sel_cursor;   // collect: selected so far
    uint32_t cand_cursor;  // collect: candidates so far; afterwards the length of the candidates' sort
    uint32_t pos_pref, pos_mask;  // prefix over the position's bits
    uint32_t pad[6];
    uint64_t pref[2], pmask[2];  // prefix over the key's bits, low word first
};
static_assert(sizeof(TopkHeader) <= HEADER_BYTES, "the header fits its place in the scratch");

// ---- device side -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void topk_init_kernel(TopkHeader* __restrict__ hdr, uint32_t len, uint32_t cap) {
    if (threadIdx.x != 0) return;  // (the header and the counters were cleared just before)
    hdr->m = len;
    hdr->ready = len <= cap ? 1u : 0u;
}

// Counts, over the keys on the prefix, the digit [shift, shift + nbits) of the mapped key (pos_level: of the position).
template <typename K>
__global__ __launch_bounds__(HIST_THREADS) void topk_hist_kernel(const K* __restrict__ keys, uint32_t len, K neg, K pos, int shift, uint32_t dmask,
                                                                uint32_t pos_level, const TopkHeader* __restrict__ hdr, uint32_t* __restrict__ counters) {
    __shared__ uint32_t lds[COUNTERS];
    if (hdr->ready) return;  // uniform over the grid
    for (uint32_t i = threadIdx.x; i < COUNTERS; i += HIST_THREADS) lds[i] = 0;
    const K pref = header_key<K>(hdr->pref), pmask = header_key<K>(hdr->pmask);
    const uint32_t ppref = hdr->pos_pref, ppmask = hdr->pos_mask;
    const uint32_t lane = threadIdx.x & 63u;
    __syncthreads();
    stream_keys<K, HIST_UNROLL>(keys, len, [&](K raw, uint32_t idx, bool valid) {
        const K m = map_key<K>(raw, neg, pos);
        const bool hit = valid && (K)(m & pmask) == pref && (idx & ppmask) == ppref;
        const uint64_t bal = __builtin_amdgcn_ballot_w64(hit);
        if (bal == 0) return;  // wave-uniform
        const uint32_t d = (pos_level ? idx >> shift : (uint32_t)(m >> shift)) & dmask;
        wave_count(lds, d, hit, bal, lane);
    });
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < COUNTERS; i += HIST_THREADS) {
        const uint32_t c = lds[i];
        if (c) atomicAdd(&counters[i], c);
    }
}

// One workgroup: the bucket that holds the (k - c_below)-th key of this level.  `last`: no digit is left after this level.
__global__ __launch_bounds__(PICK_THREADS) void topk_pick_kernel(TopkHeader* __restrict__ hdr, uint32_t* __restrict__ counters, uint32_t k, uint32_t cap,
                                                                 int shift, uint32_t nbits, uint32_t pos_level, uint32_t level, uint32_t last) {
    __shared__ uint32_t wave_sum[PICK_THREADS / 64];
    if (hdr->ready) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t remaining = k - hdr->c_below;
    uint32_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = counters[4 * tid + j];
        counters[4 * tid + j] = 0;
    }
    uint32_t run;
    int j;
    if (!pick_bucket(c, remaining, wave_sum, &run, &j)) return;  // exactly one thread goes on (every thread has read c_below by now)
    const uint32_t bucket = 4 * tid + (uint32_t)j, m = c[j];
    hdr->c_below += run;
    hdr->m = m;
    hdr->depth = level + 1;
    const uint32_t dmask = nbits >= 32 ? ~0u : (1u << nbits) - 1u;
    if (pos_level) {
        hdr->pos_pref |= bucket << shift;
        hdr->pos_mask |= dmask << shift;
        hdr->special = 1;
    } else {
        const u128 p = (u128)bucket << shift, q = (u128)dmask << shift;
        hdr->pref[0] |= (uint64_t)p;
        hdr->pref[1] |= (uint64_t)(p >> 64);
        hdr->pmask[0] |= (uint64_t)q;
        hdr->pmask[1] |= (uint64_t)(q >> 64);
    }
    if (last && m > cap) hdr->fill = hdr->special = 1;  // keys only (composites are unique: m == 1 there)
    if (last || m <= cap) hdr->ready = 1;
}

template <typename K, typename C>
__global__ __launch_bounds__(HIST_THREADS) void topk_collect_kernel(const K* __restrict__ keys, uint32_t len, K neg, K pos, TopkHeader* __restrict__ hdr,
                                                                   C* __restrict__ sel, uint32_t k, C* __restrict__ cand, uint32_t cap) {
    constexpr uint32_t STAGE = STAGE_BYTES / (uint32_t)sizeof(C);  // elements per wave and class; at least one wave's worth
    static_assert(STAGE >= 64, "a stage takes what one ballot can keep");
    __shared__ C stages[HIST_THREADS / 64][2][STAGE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    C* stage_b = stages[wave][0];
    C* stage_o = stages[wave][1];
    uint32_t n_b = 0, n_o = 0;  // wave-uniform
    const K pref = header_key<K>(hdr->pref), pmask = header_key<K>(hdr->pmask);
    const uint32_t ppref = hdr->pos_pref, ppmask = hdr->pos_mask;
    const bool collect_cand = hdr->fill == 0;
    stream_keys<K, HIST_UNROLL>(keys, len, [&](K raw, uint32_t idx, bool valid) {
        const K m = map_key<K>(raw, neg, pos);
        const K km = (K)(m & pmask);
        const uint32_t pm = idx & ppmask;
        const bool before = valid && (km < pref || (km == pref && pm < ppref));
        const bool on = valid && collect_cand && km == pref && pm == ppref;
        const uint64_t bal_b = __builtin_amdgcn_ballot_w64(before), bal_o = __builtin_amdgcn_ballot_w64(on);
        if ((bal_b | bal_o) == 0) return;  // wave-uniform, like every branch below
        const C c = compose<K, C>(m, idx);
        if (bal_b) {
            const uint32_t n = (uint32_t)__builtin_popcountll(bal_b);
            if (n_b + n > STAGE) {
                flush_stage<C>(stage_b, n_b, &hdr->sel_cursor, sel, k, lane);
                n_b = 0;
            }
            if (before) stage_b[n_b + lanes_below(bal_b)] = c;
            n_b += n;
        }
        if (bal_o) {
            const uint32_t n = (uint32_t)__builtin_popcountll(bal_o);
            if (n_o + n > STAGE) {
                flush_stage<C>(stage_o, n_o, &hdr->cand_cursor, cand, cap, lane);
                n_o = 0;
            }
            if (on) stage_o[n_o + lanes_below(bal_o)] = c;
            n_o += n;
        }
    });
    flush_stage<C>(stage_b, n_b, &hdr->sel_cursor, sel, k, lane);
    flush_stage<C>(stage_o, n_o, &hdr->cand_cursor, cand, cap, lane);
}

// sel[c_below + i] = the i-th sorted candidate (fill: the one key every candidate is), i < k - c_below.
template <typename C>
__global__ __launch_bounds__(256) void topk_append_kernel(const TopkHeader* __restrict__ hdr, C* __restrict__ sel, const C* __restrict__ cand, uint32_t k,
                                                          uint32_t cap) {
    const uint32_t below = hdr->c_below;
    if (below >= k) return;
    const uint32_t remaining = k - below;
    const bool fill = hdr->fill != 0;
    const uint32_t have = hdr->cand_cursor < cap ? hdr->cand_cursor : cap;
    const C t = header_key<C>(hdr->pref);  // (fill is keys-only: C is the key type)
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < remaining; i += (uint64_t)gridDim.x * 256) {
        if (fill) sel[below + i] = t;
        else if (i < have) sel[below + i] = cand[i];
    }
}

template <typename K, typename C, typename I>
__global__ __launch_bounds__(256) void topk_finish_kernel(const C* __restrict__ sel, uint32_t k, K neg, K pos, K* __restrict__ out_keys, I* __restrict__ out_index) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < k; i += (uint64_t)gridDim.x * 256) {
        const C c = sel[i];
        K m;
        if constexpr (sizeof(C) == sizeof(K)) m = (K)c;
        else {
            m = (K)(c >> (8 * sizeof(K)));
            out_index[i] = (I)(uint32_t)c;
        }
        out_keys[i] = unmap_any<K>(m, neg, pos);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

struct TopkCall {
    const void* keys;
    uint64_t len, k;
    void *out_keys, *out_index;
    uint32_t index_bytes;
    char* scratch;
    TopkLayout L;
    uint32_t elem_bytes;
    rdst_key_kind kind;
    bool largest;
    int cus;
    hipStream_t s;
};

uint32_t stream_grid(uint64_t len, uint32_t elem_bytes, int cus) {
    const uint64_t vecs = len / (16 / elem_bytes) + 1;
    const uint64_t want = (vecs + HIST_THREADS - 1) / HIST_THREADS;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)cus * BLOCKS_PER_CU));
}
uint32_t small_grid(uint64_t n, int cus) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)cus * BLOCKS_PER_CU)); }

// K: the key type; C: the collected element; I: the index type of the output (unused without an index).  The library's
// mutex is held.
template <typename K, typename C, typename I>
int run_topk(const TopkCall& c) {
    constexpr bool INDEXED = sizeof(C) != sizeof(K);
    unsigned __int128 neg128, pos128;
    rdst_internal::key_xor_masks(c.kind, (uint32_t)sizeof(K), &neg128, &pos128);
    K neg = (K)neg128, pos = (K)pos128;
    if (c.largest) {  // the complement of the mapped key: both masks complemented
        neg = (K)~neg;
        pos = (K)~pos;
    }
    const K* keys = static_cast<const K*>(c.keys);
    const uint32_t len = (uint32_t)c.len, k = (uint32_t)c.k, cap = (uint32_t)c.L.cap;
    TopkHeader* hdr = reinterpret_cast<TopkHeader*>(c.scratch);
    uint32_t* counters = reinterpret_cast<uint32_t*>(c.scratch + c.L.counters);
    C* sel = reinterpret_cast<C*>(c.scratch + c.L.sel);
    C* sel_tmp = reinterpret_cast<C*>(c.scratch + c.L.sel_tmp);
    C* cand = reinterpret_cast<C*>(c.scratch + c.L.cand);
    C* cand_tmp = reinterpret_cast<C*>(c.scratch + c.L.cand_tmp);
    const uint32_t digit = digit_bits_for((uint32_t)sizeof(K));
    const uint32_t key_levels = levels_over(8 * (uint32_t)sizeof(K), digit);
    const uint32_t levels = key_levels + (INDEXED ? levels_over(POSITION_BITS, digit) : 0);
    const dim3 grid(stream_grid(c.len, (uint32_t)sizeof(K), c.cus)), block(HIST_THREADS);
    int rc;
    if ((rc = rdst_internal::profile_open_run(c.s))) return rc;
    RDST_HIP_TRY(hipMemsetAsync(c.scratch, 0, c.L.sel, c.s));  // header and counters: the caller never clears the scratch
    if ((rc = launch("topk_init_kernel", topk_init_kernel, dim3(1), dim3(64), 0, c.s, hdr, len, cap))) return rc;
    for (uint32_t l = 0; l < levels; ++l) {
        const bool pos_level = l >= key_levels;
        int shift;
        uint32_t nbits;
        if (pos_level) level_shape(POSITION_BITS, digit, l - key_levels, &shift, &nbits);
        else level_shape(8 * (uint32_t)sizeof(K), digit, l, &shift, &nbits);
        const uint32_t dmask = (1u << nbits) - 1u;
        if ((rc = launch("topk_hist_kernel", topk_hist_kernel<K>, grid, block, 0, c.s, keys, len, neg, pos, shift, dmask, pos_level ? 1u : 0u,
                         static_cast<const TopkHeader*>(hdr), counters)))
            return rc;
        if ((rc = launch("topk_pick_kernel", topk_pick_kernel, dim3(1), dim3(PICK_THREADS), 0, c.s, hdr, counters, k, cap, shift, nbits, pos_level ? 1u : 0u, l,
                         l + 1 == levels ? 1u : 0u)))
            return rc;
        if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_TOPK | (l << 8)))) return rc;
    }
    if ((rc = launch("topk_collect_kernel", topk_collect_kernel<K, C>, grid, block, 0, c.s, keys, len, neg, pos, hdr, sel, k, cand, cap))) return rc;
    if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_TOPK | (0xFFu << 8)))) return rc;
    // the candidates in order (their count is hdr->cand_cursor, at most cap), the first k - c_below of them behind the selected
    if (cap > 1 && (rc = rdst_internal::sort_slice_devlen_locked(cand, cand_tmp, cap, &hdr->cand_cursor, 4, (uint32_t)sizeof(C), RDST_KEY_UNSIGNED, c.s)))
        return rc;
    if ((rc = launch("topk_append_kernel", topk_append_kernel<C>, dim3(small_grid(k, c.cus)), dim3(256), 0, c.s,
                     static_cast<const TopkHeader*>(hdr), sel, static_cast<const C*>(cand), k, cap)))
        return rc;
    // (not sort_slice_locked: from about 10^9 elements on it splits the slice on counts it reads back, and waits for the stream)
    if (k > 1 && (rc = rdst_internal::sort_slice_nowait_locked(sel, sel_tmp, k, (uint32_t)sizeof(C), RDST_KEY_UNSIGNED, c.s))) return rc;
    return launch("topk_finish_kernel", topk_finish_kernel<K, C, I>, dim3(small_grid(k, c.cus)), dim3(256), 0, c.s, static_cast<const C*>(sel), k, neg, pos,
                  static_cast<K*>(c.out_keys), static_cast<I*>(c.out_index));
}

int dispatch_topk(const TopkCall& c) {
    if (c.index_bytes == 0) {
        switch (c.elem_bytes) {
            case 1: return run_topk<uint8_t, uint8_t, uint32_t>(c);
            case 2: return run_topk<uint16_t, uint16_t, uint32_t>(c);
            case 4: return run_topk<uint32_t, uint32_t, uint32_t>(c);
            case 8: return run_topk<uint64_t, uint64_t, uint32_t>(c);
            default: return run_topk<u128, u128, uint32_t>(c);
        }
    }
    if (c.elem_bytes == 4)
        return c.index_bytes == 4 ? run_topk<uint32_t, uint64_t, uint32_t>(c) : run_topk<uint32_t, uint64_t, uint64_t>(c);
    return c.index_bytes == 4 ? run_topk<uint64_t, u128, uint32_t>(c) : run_topk<uint64_t, u128, uint64_t>(c);
}

}  // namespace

// The call after its checks, for a caller that holds the library's mutex (rdst_topk_segments.hip: one far-class segment):
// the layout is that of rdst_hip_topk_scratch_bytes(len, k, elem_bytes, index_bytes, 0).
int rdst_internal::topk_slice_locked(const void* keys, uint64_t len, uint64_t k, void* out_keys, void* out_index, uint32_t index_bytes, void* scratch,
                                     uint32_t elem_bytes, rdst_key_kind kind, bool largest, int cus, hipStream_t s) {
    TopkCall c{};
    c.L = topk_layout(len, k, elem_bytes, index_bytes, 0);
    c.keys = keys;
    c.len = len;
    c.k = k;
    c.out_keys = out_keys;
    c.out_index = out_index;
    c.index_bytes = index_bytes;
    c.scratch = static_cast<char*>(scratch);
    c.elem_bytes = elem_bytes;
    c.kind = kind;
    c.largest = largest;
    c.cus = cus;
    c.s = s;
    return dispatch_topk(c);
}

extern "C" {

int rdst_hip_topk_device(const void* dev_keys, uint64_t len, uint64_t k, void* dev_out_keys, void* dev_out_index, uint32_t index_bytes,
                         void* dev_scratch, uint64_t scratch_bytes, uint64_t cand_capacity, uint32_t elem_bytes, rdst_key_kind kind,
                         uint32_t levels, uint32_t flags, void* stream) {
    if (int rc = rdst_internal::rank_check_head("topk", dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (k > len) return set_error(RDST_ERR_ARG, "topk: k is larger than len");
    if (flags & ~RDST_TOPK_LARGEST) return set_error(RDST_ERR_ARG, "topk: unknown flag bits");
    if (k == 0) return RDST_OK;
    if (int rc = rdst_internal::rank_check_outputs("topk", dev_out_keys, dev_out_index, &index_bytes, dev_scratch, elem_bytes)) return rc;
    TopkCall c{};
    c.L = topk_layout(len, k, elem_bytes, index_bytes, cand_capacity);
    if (scratch_bytes < c.L.total) return set_error(RDST_ERR_ARG, "topk: scratch_bytes is below rdst_hip_topk_scratch_bytes(len, k, elem_bytes, index_bytes, cand_capacity)");
    c.keys = dev_keys;
    c.len = len;
    c.k = k;
    c.out_keys = dev_out_keys;
    c.out_index = dev_out_index;
    c.index_bytes = index_bytes;
    c.scratch = static_cast<char*>(dev_scratch);
    c.elem_bytes = elem_bytes;
    c.kind = kind;
    c.largest = (flags & RDST_TOPK_LARGEST) != 0;
    c.s = static_cast<hipStream_t>(stream);
    if (int rc = rdst_internal::device_cus(&c.cus)) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    return dispatch_topk(c);
}

int rdst_hip_debug_topk_state(const void* dev_scratch, void* stream, uint64_t out[4]) {
    if (dev_scratch == nullptr || out == nullptr) return set_error(RDST_ERR_ARG, "topk: null scratch or output");
    if (int rc = rdst_internal::rank_check_scratch("topk", dev_scratch)) return rc;
    TopkHeader h;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RDST_HIP_TRY(hipMemcpyAsync(&h, dev_scratch, sizeof h, hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    out[0] = h.depth;
    out[1] = h.c_below;
    out[2] = h.cand_cursor;
    out[3] = h.special;
    return RDST_OK;
}

}  // extern "C"
