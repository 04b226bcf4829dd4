// rdst_select_layout.h — what rdst_select.hip (kernels, launches) and rdst_rank_args.cpp (the host-only size and limits
// functions) of rdst_hip_select_device share: the ranks of a round, the digits and the layout of the scratch.  No HIP here.
#ifndef RDST_SELECT_LAYOUT_H
#define RDST_SELECT_LAYOUT_H

#include <algorithm>

#include "rdst_args.h"

namespace rdst_select_layout {

using rdst_args::align256;
using rdst_args::levels_over;

constexpr uint32_t MAX_RANKS = 64;             // ranks followed in the same reads: rows of counters in LDS
constexpr uint32_t DIGIT0_BITS_WIDE = 12;      // level 0, keys of two bytes and more
constexpr uint32_t DIGIT0_BITS_BYTE = 8;       // level 0, one-byte keys: the whole key
constexpr uint32_t DIGIT_BITS = 8;             // every later level
constexpr uint32_t COUNTERS0 = 1u << DIGIT0_BITS_WIDE;
constexpr uint32_t ROW = 1u << DIGIT_BITS;     // counters per group
constexpr uint32_t COUNTER_WORDS = MAX_RANKS * ROW;  // 64 KiB: the level kernel's LDS rows and the counters in the scratch
constexpr uint64_t DEFAULT_CAND_CAPACITY = 1ull << 24;  // 64 uniform buckets of 10^9 keys after level 0: 64 x 2.44 x 10^5 = 1.56 x 10^7
constexpr uint64_t HEADER_BYTES = 256;         // the room of SelectHeader (rdst_select.hip, which holds the struct to its place)
// SelectTable (rdst_select.hip, which holds the struct to this size): per group a 16-byte prefix and four words, per rank one
constexpr uint64_t TABLE_BYTES = MAX_RANKS * (2 * sizeof(uint64_t) + 5 * sizeof(uint32_t));
static_assert(COUNTER_WORDS >= COUNTERS0, "level 0 counts into the same counters");
constexpr uint32_t digit0_bits_for(uint32_t elem_bytes) { return elem_bytes == 1 ? DIGIT0_BITS_BYTE : DIGIT0_BITS_WIDE; }
constexpr uint32_t key_levels_for(uint32_t elem_bytes) { return 1 + levels_over(8 * elem_bytes - digit0_bits_for(elem_bytes), DIGIT_BITS); }
// The header, the group table, the counters and two arrays of the candidates' capacity, each rounded up to 256 bytes
struct SelectLayout { uint64_t table, counters, cand, cand_tmp, total, cap; };  // cap: the candidates the buffers are sized for
inline SelectLayout select_layout(uint64_t len, uint32_t elem_bytes, uint32_t index_bytes, uint64_t cand_capacity) {
    const uint64_t c_bytes = index_bytes ? 2ull * elem_bytes : elem_bytes;
    SelectLayout L{};
    L.cap = std::min<uint64_t>(cand_capacity ? cand_capacity : DEFAULT_CAND_CAPACITY, std::max<uint64_t>(len, 1));
    L.table = HEADER_BYTES;
    L.counters = L.table + align256(TABLE_BYTES);
    L.cand = L.counters + COUNTER_WORDS * sizeof(uint32_t);
    L.cand_tmp = L.cand + align256(L.cap * c_bytes);
    L.total = L.cand_tmp + align256(L.cap * c_bytes);
    return L;
}

}  // namespace rdst_select_layout

#endif  // RDST_SELECT_LAYOUT_H
