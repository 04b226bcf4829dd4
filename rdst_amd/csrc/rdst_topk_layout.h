// rdst_topk_layout.h — what rdst_topk.hip (kernels, launches) and rdst_rank_args.cpp (the host-only size and limits functions)
// of rdst_hip_topk_device share: the digits of the radix select and the layout of the caller's scratch.  No HIP here.
#ifndef RDST_TOPK_LAYOUT_H
#define RDST_TOPK_LAYOUT_H

#include <algorithm>

#include "rdst_args.h"

namespace rdst_topk_layout {

using rdst_args::align256;

constexpr uint32_t COUNTERS = 4096;           // one counter per value of the widest digit
constexpr uint32_t DIGIT_BITS_WIDE = 12;      // keys of two bytes and more
constexpr uint32_t DIGIT_BITS_BYTE = 8;       // one-byte keys: the whole key
constexpr uint64_t DEFAULT_CAND_CAPACITY = 1ull << 20;  // a uniform bucket of 10^9 keys after one level: 2.4 x 10^5
constexpr uint64_t HEADER_BYTES = 256;        // the room of TopkHeader (rdst_topk.hip, which holds the struct to its place)

constexpr uint32_t digit_bits_for(uint32_t elem_bytes) { return elem_bytes == 1 ? DIGIT_BITS_BYTE : DIGIT_BITS_WIDE; }
// The header, the counters, two arrays of min(k, len) elements and two of the candidates' capacity, each rounded up to 256 bytes
struct TopkLayout { uint64_t counters, sel, sel_tmp, cand, cand_tmp, total, cap; };  // cap: the candidates the buffers are sized for
inline TopkLayout topk_layout(uint64_t len, uint64_t k, uint32_t elem_bytes, uint32_t index_bytes, uint64_t cand_capacity) {
    const uint64_t c_bytes = index_bytes ? 2ull * elem_bytes : elem_bytes;
    TopkLayout L{};
    L.cap = std::min<uint64_t>(cand_capacity ? cand_capacity : DEFAULT_CAND_CAPACITY, std::max<uint64_t>(len, 1));
    const uint64_t kk = std::min(k, len);
    L.counters = HEADER_BYTES;
    L.sel = L.counters + COUNTERS * sizeof(uint32_t);
    L.sel_tmp = L.sel + align256(kk * c_bytes);
    L.cand = L.sel_tmp + align256(kk * c_bytes);
    L.cand_tmp = L.cand + align256(L.cap * c_bytes);
    L.total = L.cand_tmp + align256(L.cap * c_bytes);
    return L;
}

}  // namespace rdst_topk_layout

#endif  // RDST_TOPK_LAYOUT_H
