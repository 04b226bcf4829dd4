// rdst_select.hip — order statistics: the keys that stand at given ranks of the sort's order, and the input position of each if
// asked for, without sorting the array (rdst_hip_select_device; include/rdst_hip.h).
//
// A radix select over the mapped key M of rdst_device.h (complemented for RDST_TOPK_LARGEST) that follows up to MAX_RANKS ranks
// in the same reads of the input.  The state lives in the caller's scratch: a header and a GROUP TABLE.  A group is a distinct
// prefix that at least one rank of the round lies on; groups are kept in ascending prefix order, all at the same depth, each
// with `below` (elements strictly before its prefix) and `m` (elements on it).  Nothing before a prefix is ever kept: only
// its count.
//
//   select_hist0_kernel<K>   level 0, one read: counts the first digit (12 bits; one-byte keys: all 8) of every key.
//   select_level_kernel<K>   a later level, one read: counts the next 8-bit digit of every key that lies on ANY group's prefix
//                            into that group's row of counters in LDS.  A table over the first digit tells the common key —
//                            on no group — apart with one LDS read; a wave of such keys returns through one ballot.
//   select_pick_kernel       one workgroup per level: per rank the digit whose range holds rank - below; ranks that part ways
//                            split their group, ranks in different groups never merge.  Rewrites the table in prefix order,
//                            zeroes the counters, sets ready when the groups together hold at most cand_capacity elements
//                            or the digits are exhausted.  Launched once per possible level; returns at once when ready.
//   select_collect_kernel    one read: the elements on any group's prefix go to the candidate buffer through per-wave LDS
//                            stages, one claim of output space per stage.
//   select_finish_kernel     groups have disjoint, ordered prefixes, so ONE sort of the candidates orders them all: the answer
//                            for rank r of group g is sorted candidate (sum of m over the groups before g) + (r - below_g),
//                            unmapped into the rank's own slot.  Digits exhausted: the answer is the group's prefix itself.
//
// With an index the element is the composite of rdst_topk.hip (M << 32 | position, M << 64 | position) and the levels past the
// last key digit run over the position's digits: the answer is the element of a STABLE argsort.
//
// The ranks travel as kernel arguments (RankArgs).  More than MAX_RANKS ranks are served in rounds, in ascending rank order,
// all on the same scratch in stream order.  Every launch is enqueued unconditionally and sized on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <exception>
#include <mutex>
#include <numeric>
#include <vector>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_device.h"
#include "rdst_stream.h"
#include "rdst_select_layout.h"

namespace {

using namespace rdst_select_layout;  // the ranks of a round, the digits, the rooms, select_layout: shared with rdst_rank_args.cpp
using rdst_args::POSITION_BITS;
using rdst_internal::launch;
using rdst_internal::set_error;

constexpr int STREAM_THREADS = 256;            // level 0 and the collection
constexpr int LEVEL_THREADS = 512;             // later levels: 74 KiB of LDS per workgroup, two workgroups per CU
constexpr int STREAM_UNROLL = 4;               // 16-byte loads in flight per lane
constexpr uint32_t STAGE_BYTES = 4096;         // collection: LDS per wave between two claims of output space
constexpr int PICK_THREADS = 1024;
constexpr int BLOCKS_PER_CU = 8;
constexpr int LEVEL_BLOCKS_PER_CU = 2;

struct SelectHeader {  // the first HEADER_BYTES of the scratch
    uint32_t ready;        // no further level is needed
    uint32_t depth;        // levels used
    uint32_t groups;       // groups in the table
    uint32_t exhausted;    // the digits ran out: every answer is its group's prefix
    uint32_t cand_cursor;  // collect: candidates so far; afterwards the length of the candidates' sort
    uint32_t total_m;      // sum of m over the groups
    uint32_t pos_mask;     // the position bits the prefixes cover
    uint32_t pad;
    uint64_t pmask[2];     // the key bits the prefixes cover, low word first
};
static_assert(sizeof(SelectHeader) <= HEADER_BYTES, "the header fits its place in the scratch");

struct SelectTable {  // behind the header
    uint64_t pref[MAX_RANKS][2];  // per group: prefix over the key's bits, low word first
    uint32_t ppref[MAX_RANKS];    //            prefix over the position's bits
    uint32_t below[MAX_RANKS];    //            elements strictly before the prefix
    uint32_t m[MAX_RANKS];        //            elements on it
    uint32_t off[MAX_RANKS];      //            sum of m over the groups before it
    uint32_t grp[MAX_RANKS];      // per rank of the round: its group
};
static_assert(sizeof(SelectTable) == TABLE_BYTES, "the table fills the place the layout gives it");

struct RankArgs {  // one round's ranks, ascending, and the caller's slot of each: a kernel argument
    uint32_t n;
    uint32_t rank[MAX_RANKS];
    uint32_t slot[MAX_RANKS];
};

// ---- device side -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void select_init_kernel(SelectHeader* __restrict__ hdr, SelectTable* __restrict__ table, uint32_t len, uint32_t cap) {
    if (threadIdx.x != 0) return;  // (header, table and counters were cleared just before: one group, the empty prefix)
    hdr->groups = 1;
    hdr->total_m = len;
    table->m[0] = len;
    hdr->ready = len <= cap ? 1u : 0u;
}

template <typename K>
__global__ __launch_bounds__(STREAM_THREADS) void select_hist0_kernel(const K* __restrict__ keys, uint32_t len, K neg, K pos, int shift0,
                                                                      const SelectHeader* __restrict__ hdr, uint32_t* __restrict__ counters) {
    __shared__ uint32_t lds[COUNTERS0];
    if (hdr->ready) return;  // uniform over the grid
    for (uint32_t i = threadIdx.x; i < COUNTERS0; i += STREAM_THREADS) lds[i] = 0;
    const uint32_t lane = threadIdx.x & 63u;
    __syncthreads();
    stream_keys<K, STREAM_UNROLL>(keys, len, [&](K raw, uint32_t, bool valid) {
        const uint64_t bal = __builtin_amdgcn_ballot_w64(valid);
        if (bal == 0) return;  // wave-uniform
        const uint32_t d = (uint32_t)(map_key<K>(raw, neg, pos) >> shift0);
        wave_count(lds, d, valid, bal, lane);
    });
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < COUNTERS0; i += STREAM_THREADS) {
        const uint32_t c = lds[i];
        if (c) atomicAdd(&counters[i], c);
    }
}

// Which group a key lies on, for the kernels that stream the input.  `first` holds per value of the first digit the groups
// that start with it, (count << 8 | first group), 0 for none: the one LDS read of the common key.  Among the groups of its
// bucket a key is found by a binary search of `steps`-bounded, wave-uniform length.
template <typename K>
struct GroupLookup {
    K* pref;            // MAX_RANKS
    uint32_t* ppref;    // MAX_RANKS
    uint16_t* first;    // COUNTERS0
    uint32_t* widest;   // one word: the most groups in one bucket
    K pmask;
    uint32_t ppmask, top;
    int shift0;

    // every thread of the workgroup; two barriers inside
    __device__ __forceinline__ void setup(const SelectHeader* __restrict__ hdr, const SelectTable* __restrict__ table, int shift0_) {
        const uint32_t ng = hdr->groups, depth = hdr->depth;
        pmask = header_key<K>(hdr->pmask);
        ppmask = hdr->pos_mask;
        shift0 = shift0_;
        const uint16_t fill = depth == 0 ? (uint16_t)(1u << 8) : (uint16_t)0;  // no level yet: every key is on the one group
        for (uint32_t i = threadIdx.x; i < COUNTERS0; i += blockDim.x) first[i] = fill;
        if (threadIdx.x < ng) {
            pref[threadIdx.x] = header_key<K>(table->pref[threadIdx.x]);
            ppref[threadIdx.x] = table->ppref[threadIdx.x];
        }
        if (threadIdx.x == 0) *widest = 1;
        __syncthreads();
        if (threadIdx.x < ng && depth != 0) {
            const uint32_t g = threadIdx.x, b = (uint32_t)(pref[g] >> shift0);
            if (g == 0 || (uint32_t)(pref[g - 1] >> shift0) != b) {
                uint32_t c = 1;
                while (g + c < ng && (uint32_t)(pref[g + c] >> shift0) == b) ++c;
                first[b] = (uint16_t)(c << 8 | g);
                atomicMax(widest, c);
            }
        }
        __syncthreads();
        const uint32_t w = *widest;
        top = w > 1 ? 1u << (31 - __builtin_clz(w - 1)) : 0u;
    }

    // the bucket's entry: 0 for a key on no group
    __device__ __forceinline__ uint32_t entry(K m) const { return first[(uint32_t)(m >> shift0)]; }

    // for a lane whose entry is not 0: is the key on a group, and which
    __device__ __forceinline__ bool find(K m, uint32_t idx, uint32_t e, uint32_t* g_out) const {
        const K km = (K)(m & pmask);
        const uint32_t pm = idx & ppmask;
        const uint32_t lo = e & 0xFFu, end = lo + (e >> 8);
        uint32_t g = lo;
        for (uint32_t s = top; s; s >>= 1) {  // wave-uniform length
            const uint32_t t = g + s;
            if (t < end) {
                const K p = pref[t];
                if (p < km || (p == km && ppref[t] <= pm)) g = t;
            }
        }
        *g_out = g;
        return pref[g] == km && ppref[g] == pm;
    }
};

// Counts, over the keys on any group's prefix, the digit [shift, shift + bits of dmask) of the mapped key (pos_level: of the
// position) into the group's row.
template <typename K>
__global__ __launch_bounds__(LEVEL_THREADS) void select_level_kernel(const K* __restrict__ keys, uint32_t len, K neg, K pos, int shift, uint32_t dmask,
                                                                     uint32_t pos_level, int shift0, const SelectHeader* __restrict__ hdr,
                                                                     const SelectTable* __restrict__ table, uint32_t* __restrict__ counters) {
    __shared__ uint32_t rows[COUNTER_WORDS];
    __shared__ K s_pref[MAX_RANKS];
    __shared__ uint32_t s_ppref[MAX_RANKS];
    __shared__ uint16_t s_first[COUNTERS0];
    __shared__ uint32_t s_widest;
    if (hdr->ready) return;  // uniform over the grid
    const uint32_t used = hdr->groups * ROW;
    for (uint32_t i = threadIdx.x; i < used; i += LEVEL_THREADS) rows[i] = 0;
    GroupLookup<K> look{s_pref, s_ppref, s_first, &s_widest};
    look.setup(hdr, table, shift0);
    const uint32_t lane = threadIdx.x & 63u;
    stream_keys<K, STREAM_UNROLL>(keys, len, [&](K raw, uint32_t idx, bool valid) {
        const K m = map_key<K>(raw, neg, pos);
        const uint32_t e = valid ? look.entry(m) : 0u;
        if (__builtin_amdgcn_ballot_w64(e != 0) == 0) return;  // wave-uniform: no key of the wave shares a first digit with a group
        uint32_t g = 0;
        const bool hit = e != 0 && look.find(m, idx, e, &g);
        const uint64_t bal = __builtin_amdgcn_ballot_w64(hit);
        if (bal == 0) return;
        const uint32_t d = (pos_level ? idx >> shift : (uint32_t)(m >> shift)) & dmask;
        wave_count(rows, g * ROW + d, hit, bal, lane);
    });
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < used; i += LEVEL_THREADS) {
        const uint32_t c = rows[i];
        if (c) atomicAdd(&counters[i], c);
    }
}

// One workgroup: for every rank the digit of this level whose range holds rank - below, then the table of the next depth.
// `row_len`: counters per group at this level; `last`: no digit is left after this level.
__global__ __launch_bounds__(PICK_THREADS) void select_pick_kernel(SelectHeader* __restrict__ hdr, SelectTable* __restrict__ table,
                                                                   uint32_t* __restrict__ counters, RankArgs ra, uint32_t cap, int shift, uint32_t nbits,
                                                                   uint32_t pos_level, uint32_t level, uint32_t last) {
    __shared__ uint32_t s_d[MAX_RANKS], s_below[MAX_RANKS], s_m[MAX_RANKS], s_flag[MAX_RANKS], s_newm[MAX_RANKS];
    if (hdr->ready) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = ra.n, row_len = 1u << nbits;
    // a wave per rank: scan the group's row, 256 counters at a time
    for (uint32_t i = wave; i < n; i += PICK_THREADS / 64) {
        const uint32_t g = table->grp[i], below = table->below[g];
        const uint32_t r = ra.rank[i] - below;  // the digit with before <= r < before + count
        const uint32_t* row = counters + (level == 0 ? 0u : g * ROW);
        uint32_t run = 0;
        for (uint32_t base = 0; base < row_len; base += 256) {  // wave-uniform
            uint32_t c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t at = base + 4 * lane + (uint32_t)j;
                c[j] = at < row_len ? row[at] : 0u;
            }
            const uint32_t sum = c[0] + c[1] + c[2] + c[3];
            uint32_t incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o);
                if (lane >= (uint32_t)o) incl += y;
            }
            const uint32_t total = __shfl(incl, 63);
            if (r < run + total) {  // wave-uniform: the digit is in this chunk, in exactly one lane's four counters
                uint32_t before = run + incl - sum;
                if (before <= r && r < before + sum) {
                    int at = 0;
                    while (at < 3 && before + c[at] <= r) before += c[at++];
                    s_d[i] = base + 4 * lane + (uint32_t)at;
                    s_below[i] = below + before;
                    s_m[i] = c[at];
                }
                break;
            }
            run += total;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < COUNTER_WORDS; i += PICK_THREADS) counters[i] = 0;  // (every row has been read)
    // ranks ascend, so (group, digit) ascends: a new group starts wherever it changes
    uint32_t g_old = 0, d = 0;
    uint64_t pref0 = 0, pref1 = 0;
    uint32_t ppref = 0;
    if (tid < n) {
        g_old = table->grp[tid];
        d = s_d[tid];
        s_flag[tid] = (tid == 0 || table->grp[tid - 1] != g_old || s_d[tid - 1] != d) ? 1u : 0u;
        pref0 = table->pref[g_old][0];
        pref1 = table->pref[g_old][1];
        ppref = table->ppref[g_old];
    }
    __syncthreads();  // the old table has been read
    if (tid < n) {
        uint32_t g_new = 0;
        for (uint32_t j = 1; j <= tid; ++j) g_new += s_flag[j];
        table->grp[tid] = g_new;
        if (s_flag[tid]) {
            if (pos_level) {
                ppref |= d << shift;
            } else {
                const u128 p = (u128)d << shift;
                pref0 |= (uint64_t)p;
                pref1 |= (uint64_t)(p >> 64);
            }
            table->pref[g_new][0] = pref0;
            table->pref[g_new][1] = pref1;
            table->ppref[g_new] = ppref;
            table->below[g_new] = s_below[tid];
            table->m[g_new] = s_m[tid];
            s_newm[g_new] = s_m[tid];
        }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t ng = 0;
        for (uint32_t j = 0; j < n; ++j) ng += s_flag[j];
        uint32_t acc = 0;
        for (uint32_t g = 0; g < ng; ++g) {
            table->off[g] = acc;
            acc += s_newm[g];
        }
        hdr->groups = ng;
        hdr->total_m = acc;
        hdr->depth = level + 1;
        const uint32_t dmask = nbits >= 32 ? ~0u : (1u << nbits) - 1u;
        if (pos_level) {
            hdr->pos_mask |= dmask << shift;
        } else {
            const u128 q = (u128)dmask << shift;
            hdr->pmask[0] |= (uint64_t)q;
            hdr->pmask[1] |= (uint64_t)(q >> 64);
        }
        if (last) hdr->exhausted = 1;
        if (last || acc <= cap) hdr->ready = 1;
    }
}

template <typename K, typename C>
__global__ __launch_bounds__(STREAM_THREADS) void select_collect_kernel(const K* __restrict__ keys, uint32_t len, K neg, K pos, int shift0,
                                                                        SelectHeader* __restrict__ hdr, const SelectTable* __restrict__ table,
                                                                        C* __restrict__ cand, uint32_t cap) {
    constexpr uint32_t STAGE = STAGE_BYTES / (uint32_t)sizeof(C);  // elements per wave; at least one wave's worth
    static_assert(STAGE >= 64, "a stage takes what one ballot can keep");
    __shared__ C stages[STREAM_THREADS / 64][STAGE];
    __shared__ K s_pref[MAX_RANKS];
    __shared__ uint32_t s_ppref[MAX_RANKS];
    __shared__ uint16_t s_first[COUNTERS0];
    __shared__ uint32_t s_widest;
    if (hdr->exhausted) return;  // uniform over the grid: the answers are the prefixes
    GroupLookup<K> look{s_pref, s_ppref, s_first, &s_widest};
    look.setup(hdr, table, shift0);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    C* stage = stages[wave];
    uint32_t held = 0;  // wave-uniform
    stream_keys<K, STREAM_UNROLL>(keys, len, [&](K raw, uint32_t idx, bool valid) {
        const K m = map_key<K>(raw, neg, pos);
        const uint32_t e = valid ? look.entry(m) : 0u;
        if (__builtin_amdgcn_ballot_w64(e != 0) == 0) return;  // wave-uniform, like every branch below
        uint32_t g = 0;
        const bool on = e != 0 && look.find(m, idx, e, &g);
        const uint64_t bal = __builtin_amdgcn_ballot_w64(on);
        if (bal == 0) return;
        const uint32_t k = (uint32_t)__builtin_popcountll(bal);
        if (held + k > STAGE) {
            flush_stage<C>(stage, held, &hdr->cand_cursor, cand, cap, lane);
            held = 0;
        }
        if (on) stage[held + lanes_below(bal)] = compose<K, C>(m, idx);
        held += k;
    });
    flush_stage<C>(stage, held, &hdr->cand_cursor, cand, cap, lane);
}

// Slot by slot: the sorted candidate the rank points at (digits exhausted: the group's prefix), back to original key bits.
template <typename K, typename C, typename I>
__global__ __launch_bounds__(64) void select_finish_kernel(const SelectHeader* __restrict__ hdr, const SelectTable* __restrict__ table,
                                                           const C* __restrict__ cand, RankArgs ra, uint32_t cap, K neg, K pos, K* __restrict__ out_keys,
                                                           I* __restrict__ out_index) {
    const uint32_t i = threadIdx.x;
    if (i >= ra.n) return;
    const uint32_t g = table->grp[i];
    K m;
    uint32_t position;
    if (hdr->exhausted) {
        m = header_key<K>(table->pref[g]);
        position = table->ppref[g];
    } else {
        const uint32_t at = table->off[g] + (ra.rank[i] - table->below[g]);
        const uint32_t have = hdr->cand_cursor < cap ? hdr->cand_cursor : cap;
        // Invariant: ready without exhaustion means sum(m) <= cap, the collection keeps exactly the sum(m)
        // elements on the prefixes, so have == sum(m) and at < off_g + m_g <= have.  The guard only keeps a read inside `cand`.
        if (at >= have) return;
        const C c = cand[at];
        if constexpr (sizeof(C) == sizeof(K)) {
            m = (K)c;
            position = 0;
        } else {
            m = (K)(c >> (8 * sizeof(K)));
            position = (uint32_t)c;
        }
    }
    out_keys[ra.slot[i]] = unmap_any<K>(m, neg, pos);
    if constexpr (sizeof(C) != sizeof(K)) out_index[ra.slot[i]] = (I)position;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

struct SelectCall {
    const void* keys;
    uint64_t len;
    const uint64_t* ranks;
    const uint64_t* slots;  // the output slot of each rank; nullptr: rank i goes to slot i
    const uint64_t* order;  // the ranks' indices, ascending by rank (equal ranks in slot order)
    uint64_t n_ranks;
    void *out_keys, *out_index;
    char* scratch;
    SelectLayout L;
    uint32_t elem_bytes;
    rdst_key_kind kind;
    bool largest;
    int cus;
    hipStream_t s;
};

uint32_t stream_grid(uint64_t len, uint32_t elem_bytes, int cus, int threads, int per_cu) {
    const uint64_t vecs = len / (16 / elem_bytes) + 1;
    const uint64_t want = (vecs + threads - 1) / threads;
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)cus * per_cu));
}

// K: the key type; C: the collected element; I: the index type of the output (unused without an index).  The library's
// mutex is held.
template <typename K, typename C, typename I>
int run_select(const SelectCall& c) {
    constexpr bool INDEXED = sizeof(C) != sizeof(K);
    constexpr uint32_t KEY_BITS = 8 * (uint32_t)sizeof(K);
    unsigned __int128 neg128, pos128;
    rdst_internal::key_xor_masks(c.kind, (uint32_t)sizeof(K), &neg128, &pos128);
    K neg = (K)neg128, pos = (K)pos128;
    if (c.largest) {  // the complement of the mapped key: both masks complemented
        neg = (K)~neg;
        pos = (K)~pos;
    }
    const K* keys = static_cast<const K*>(c.keys);
    const uint32_t len = (uint32_t)c.len, cap = (uint32_t)c.L.cap;
    SelectHeader* hdr = reinterpret_cast<SelectHeader*>(c.scratch);
    SelectTable* table = reinterpret_cast<SelectTable*>(c.scratch + c.L.table);
    uint32_t* counters = reinterpret_cast<uint32_t*>(c.scratch + c.L.counters);
    C* cand = reinterpret_cast<C*>(c.scratch + c.L.cand);
    C* cand_tmp = reinterpret_cast<C*>(c.scratch + c.L.cand_tmp);
    const uint32_t digit0 = digit0_bits_for((uint32_t)sizeof(K));
    const int shift0 = (int)(KEY_BITS - digit0);
    const uint32_t key_levels = key_levels_for((uint32_t)sizeof(K));
    const uint32_t levels = key_levels + (INDEXED ? levels_over(POSITION_BITS, DIGIT_BITS) : 0);
    const dim3 grid(stream_grid(c.len, (uint32_t)sizeof(K), c.cus, STREAM_THREADS, BLOCKS_PER_CU)), block(STREAM_THREADS);
    const dim3 level_grid(stream_grid(c.len, (uint32_t)sizeof(K), c.cus, LEVEL_THREADS, LEVEL_BLOCKS_PER_CU)), level_block(LEVEL_THREADS);
    const uint64_t* order = c.order;  // ascending rank order: neighbours share prefixes
    int rc;
    if ((rc = rdst_internal::profile_open_run(c.s))) return rc;
    for (uint64_t start = 0; start < c.n_ranks; start += MAX_RANKS) {
        RankArgs ra{};
        ra.n = (uint32_t)std::min<uint64_t>(MAX_RANKS, c.n_ranks - start);
        for (uint32_t i = 0; i < ra.n; ++i) {
            ra.rank[i] = (uint32_t)c.ranks[order[start + i]];
            ra.slot[i] = (uint32_t)(c.slots ? c.slots[order[start + i]] : order[start + i]);
        }
        RDST_HIP_TRY(hipMemsetAsync(c.scratch, 0, c.L.cand, c.s));  // header, table and counters: the caller never clears the scratch
        if ((rc = launch("select_init_kernel", select_init_kernel, dim3(1), dim3(64), 0, c.s, hdr, table, len, cap))) return rc;
        for (uint32_t l = 0; l < levels; ++l) {
            const bool pos_level = l >= key_levels;
            int shift;
            uint32_t nbits;
            if (l == 0) {
                shift = shift0;
                nbits = digit0;
                if ((rc = launch("select_hist0_kernel", select_hist0_kernel<K>, grid, block, 0, c.s, keys, len, neg, pos, shift0,
                                 static_cast<const SelectHeader*>(hdr), counters)))
                    return rc;
            } else {
                if (pos_level) level_shape(POSITION_BITS, DIGIT_BITS, l - key_levels, &shift, &nbits);
                else level_shape(KEY_BITS - digit0, DIGIT_BITS, l - 1, &shift, &nbits);
                if ((rc = launch("select_level_kernel", select_level_kernel<K>, level_grid, level_block, 0, c.s, keys, len, neg, pos, shift,
                                 (1u << nbits) - 1u, pos_level ? 1u : 0u, shift0, static_cast<const SelectHeader*>(hdr),
                                 static_cast<const SelectTable*>(table), counters)))
                    return rc;
            }
            if ((rc = launch("select_pick_kernel", select_pick_kernel, dim3(1), dim3(PICK_THREADS), 0, c.s, hdr, table, counters, ra, cap, shift, nbits,
                             pos_level ? 1u : 0u, l, l + 1 == levels ? 1u : 0u)))
                return rc;
            if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_SELECT | (l << 8)))) return rc;
        }
        if ((rc = launch("select_collect_kernel", select_collect_kernel<K, C>, grid, block, 0, c.s, keys, len, neg, pos, shift0, hdr,
                         static_cast<const SelectTable*>(table), cand, cap)))
            return rc;
        if ((rc = rdst_internal::profile_stage_end(c.s, RDST_STAGE_SELECT | (0xFFu << 8)))) return rc;
        // the candidates in order (their count is hdr->cand_cursor, at most cap)
        if (cap > 1 && (rc = rdst_internal::sort_slice_devlen_locked(cand, cand_tmp, cap, &hdr->cand_cursor, 4, (uint32_t)sizeof(C), RDST_KEY_UNSIGNED, c.s)))
            return rc;
        if ((rc = launch("select_finish_kernel", select_finish_kernel<K, C, I>, dim3(1), dim3(64), 0, c.s, static_cast<const SelectHeader*>(hdr),
                         static_cast<const SelectTable*>(table), static_cast<const C*>(cand), ra, cap, neg, pos, static_cast<K*>(c.out_keys),
                         static_cast<I*>(c.out_index))))
            return rc;
    }
    return RDST_OK;
}

int dispatch_select(const SelectCall& c, uint32_t index_bytes) {
    if (index_bytes == 0) {
        switch (c.elem_bytes) {
            case 1: return run_select<uint8_t, uint8_t, uint32_t>(c);
            case 2: return run_select<uint16_t, uint16_t, uint32_t>(c);
            case 4: return run_select<uint32_t, uint32_t, uint32_t>(c);
            case 8: return run_select<uint64_t, uint64_t, uint32_t>(c);
            default: return run_select<u128, u128, uint32_t>(c);
        }
    }
    if (c.elem_bytes == 4)
        return index_bytes == 4 ? run_select<uint32_t, uint64_t, uint32_t>(c) : run_select<uint32_t, uint64_t, uint64_t>(c);
    return index_bytes == 4 ? run_select<uint64_t, u128, uint32_t>(c) : run_select<uint64_t, u128, uint64_t>(c);
}

}  // namespace

// Ascending rank order (equal ranks in slot order), before the mutex is taken; nothing may be thrown through the C ABI.
int rdst_internal::order_ranks(const uint64_t* ranks, uint64_t n_ranks, uint64_t* order_out) {
    try {
        std::iota(order_out, order_out + n_ranks, 0ull);
        std::stable_sort(order_out, order_out + n_ranks, [&](uint64_t a, uint64_t b) { return ranks[a] < ranks[b]; });
    } catch (const std::exception&) {
        return set_error(RDST_ERR_ARG, "select: no host memory to order n_ranks ranks (16 bytes per rank)");
    }
    return RDST_OK;
}

// rdst_hip_select_device after its checks and the ordering of its ranks (rdst_internal.h); rdst_select_segments.hip runs its
// far class on it.
int rdst_internal::select_slice_locked(const void* keys, uint64_t len, const uint64_t* ranks, const uint64_t* slots, const uint64_t* order,
                                       uint64_t n_ranks, void* out_keys, void* out_index, uint32_t index_bytes, void* scratch, uint64_t cand_capacity,
                                       uint32_t elem_bytes, rdst_key_kind kind, bool largest, int cus, hipStream_t s) {
    SelectCall c{};
    c.L = select_layout(len, elem_bytes, index_bytes, cand_capacity);
    c.keys = keys;
    c.len = len;
    c.ranks = ranks;
    c.slots = slots;
    c.n_ranks = n_ranks;
    c.out_keys = out_keys;
    c.out_index = out_index;
    c.scratch = static_cast<char*>(scratch);
    c.elem_bytes = elem_bytes;
    c.kind = kind;
    c.largest = largest;
    c.cus = cus;
    c.s = s;
    c.order = order;
    return dispatch_select(c, index_bytes);
}

extern "C" {

int rdst_hip_select_device(const void* dev_keys, uint64_t len, const uint64_t* ranks, uint64_t n_ranks, void* dev_out_keys, void* dev_out_index,
                           uint32_t index_bytes, void* dev_scratch, uint64_t scratch_bytes, uint64_t cand_capacity, uint32_t elem_bytes,
                           rdst_key_kind kind, uint32_t levels, uint32_t flags, void* stream) {
    if (int rc = rdst_internal::rank_check_head("select", dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (flags & ~RDST_TOPK_LARGEST) return set_error(RDST_ERR_ARG, "select: unknown flag bits");
    if (n_ranks == 0) return RDST_OK;
    if (ranks == nullptr) return set_error(RDST_ERR_ARG, "select: null ranks");
    for (uint64_t i = 0; i < n_ranks; ++i)
        if (ranks[i] >= len) {
            char msg[96];
            snprintf(msg, sizeof msg, "select: ranks[%llu] is not below len", (unsigned long long)i);
            return set_error(RDST_ERR_ARG, msg);
        }
    if (int rc = rdst_internal::rank_check_outputs("select", dev_out_keys, dev_out_index, &index_bytes, dev_scratch, elem_bytes)) return rc;
    if (scratch_bytes < select_layout(len, elem_bytes, index_bytes, cand_capacity).total)
        return set_error(RDST_ERR_ARG, "select: scratch_bytes is below rdst_hip_select_scratch_bytes(len, n_ranks, elem_bytes, index_bytes, cand_capacity)");
    // ascending rank order (equal ranks in slot order), before the mutex is taken; nothing may be thrown through the C ABI
    std::vector<uint64_t> order;
    try {
        order.resize(n_ranks);
    } catch (const std::exception&) {
        return set_error(RDST_ERR_ARG, "select: no host memory to order n_ranks ranks (16 bytes per rank)");
    }
    if (int rc = rdst_internal::order_ranks(ranks, n_ranks, order.data())) return rc;
    int cus = 0;
    if (int rc = rdst_internal::device_cus(&cus)) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    return rdst_internal::select_slice_locked(dev_keys, len, ranks, nullptr, order.data(), n_ranks, dev_out_keys, dev_out_index, index_bytes, dev_scratch, cand_capacity,
                                              elem_bytes, kind, (flags & RDST_TOPK_LARGEST) != 0, cus, static_cast<hipStream_t>(stream));
}

int rdst_hip_debug_select_state(const void* dev_scratch, void* stream, uint64_t out[4]) {
    if (dev_scratch == nullptr || out == nullptr) return set_error(RDST_ERR_ARG, "select: null scratch or output");
    if (int rc = rdst_internal::rank_check_scratch("select", dev_scratch)) return rc;
    SelectHeader h;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RDST_HIP_TRY(hipMemcpyAsync(&h, dev_scratch, sizeof h, hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    out[0] = h.depth;
    out[1] = h.groups;
    out[2] = h.cand_cursor;
    out[3] = h.exhausted;
    return RDST_OK;
}

}  // extern "C"
