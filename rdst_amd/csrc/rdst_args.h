// rdst_args.h — the vocabulary of an argument check, stated once for every entry that looks at caller-supplied pointers and
// sizes before any device work.  No HIP here; no pointer is ever dereferenced.
#ifndef RDST_ARGS_H
#define RDST_ARGS_H

#include <stdint.h>

#include "rdst_hip.h"

namespace rdst_args {

inline bool misaligned(const void* p, uint64_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }
struct Range { uintptr_t lo, hi; };  // [lo, hi) of the address space; an empty one overlaps nothing
// `elems` elements of `bytes_each` (> 0) bytes from `p` on.  The byte count saturates at what the address space has left
// behind `p`: a capacity of 2^64 - 1 elements ends at UINTPTR_MAX and never wraps (hi >= lo always).
inline Range range_of(const void* p, uint64_t elems, uint64_t bytes_each) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    const uint64_t room = UINTPTR_MAX - lo;
    const uint64_t bytes = elems > room / bytes_each ? room : elems * bytes_each;
    return {lo, lo + (uintptr_t)bytes};
}
inline bool overlap(Range a, Range b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

// The key widths that are built.  An index output is 4 or 8 bytes wide and takes 4- or 8-byte keys; 0: none, every key width.
constexpr bool key_width_ok(uint32_t b) { return b == 1 || b == 2 || b == 4 || b == 8 || b == 16; }
constexpr bool index_bytes_ok(uint32_t index_bytes) { return index_bytes == 4 || index_bytes == 8; }
constexpr bool index_keys_ok(uint32_t elem_bytes) { return elem_bytes == 4 || elem_bytes == 8; }
constexpr bool index_widths_ok(uint32_t kb, uint32_t ib) { return ib == 0 || (index_bytes_ok(ib) && index_keys_ok(kb)); }
constexpr uint32_t POSITION_BITS = 32;  // len < 2^32: the position beside a key of an indexed top-k or select
constexpr uint32_t levels_over(uint32_t bits, uint32_t digit) { return (bits + digit - 1) / digit; }
constexpr uint64_t align256(uint64_t x) { return (x + 255) / 256 * 256; }

}  // namespace rdst_args

namespace rdst_internal {
// rdst_rank_args.cpp: the steps the six rank entries share, each in the documented order.  `what`, "topk" or "select", is the
// prefix of every message.  head: the sort's key arguments, no [u8; N] keys, len below 2^32.  outputs: the key output, the
// index output (without one *index_bytes becomes 0), then scratch: null, alignment to 256 bytes.
int rank_check_head(const char* what, const void* dev_keys, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels);
int rank_check_outputs(const char* what, const void* dev_out_keys, const void* dev_out_index, uint32_t* index_bytes, const void* dev_scratch, uint32_t elem_bytes);
int rank_check_scratch(const char* what, const void* dev_scratch);
}  // namespace rdst_internal

#endif  // RDST_ARGS_H
