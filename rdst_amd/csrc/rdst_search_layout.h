// rdst_search_layout.h — what rdst_search.hip (the kernels) and rdst_search.cpp (the host-only checks and the size function) of
// rdst_hip_search_device share: the tile of needles, the splitter table, the window a workgroup stages in LDS and the layout
// of the caller's scratch.  No HIP here.
#ifndef RDST_SEARCH_LAYOUT_H
#define RDST_SEARCH_LAYOUT_H

#include <stdint.h>

#include "rdst_hip.h"
#include "rdst_args.h"

namespace rdst_search_layout {

constexpr uint32_t THREADS = 256;  // one workgroup per tile of needles
// Needles per thread and tile: whole 16-byte loads (16 one-byte keys), and few enough that the needles, their two borders
// and the keys in flight stay in registers while the thread walks all of its searches in lockstep.
constexpr uint32_t needles_per_thread(uint32_t elem_bytes) { return elem_bytes == 1 ? 16 : (elem_bytes == 16 ? 4 : 8); }
constexpr uint32_t needles_per_tile(uint32_t elem_bytes) { return THREADS * needles_per_thread(elem_bytes); }
// Evenly spaced mapped keys of the haystack, the top log2(SPLITTERS) levels of every search: 16 KiB of LDS at the widest key.
constexpr uint32_t SPLITTERS = 1024;
// Keys of the haystack a workgroup stages in LDS: 32 KiB for 4-, 8- and 16-byte keys; 1- and 2-byte keys stay at 8 192 keys.
constexpr uint32_t window(uint32_t elem_bytes) { return elem_bytes == 16 ? 2048 : (elem_bytes == 8 ? 4096 : 8192); }

using rdst_args::key_width_ok;
// the position of splitter j in a haystack of m keys (m > 0): below m, never decreasing in j
constexpr uint32_t splitter_pos(uint32_t j, uint32_t m) { return (uint32_t)((uint64_t)j * m / SPLITTERS); }
// no stretch between two neighbouring splitters (or behind the last one) is longer than this
constexpr uint32_t longest_gap(uint32_t m) { return m / SPLITTERS + 1; }

// The scratch: a 256-byte header of 64-bit words, then the SPLITTERS mapped keys.  The first launch writes all of it.
constexpr uint64_t HEADER_BYTES = 256;
constexpr uint32_t HDR_M = 0, HDR_STAGED = 1, HDR_TABLE = 2, HDR_PAST = 3;  // m, tiles per path, 1 if m > len
constexpr uint64_t up256(uint64_t x) { return (x + 255) / 256 * 256; }
constexpr uint64_t scratch_bytes(uint32_t elem_bytes) { return HEADER_BYTES + up256((uint64_t)SPLITTERS * elem_bytes); }

}  // namespace rdst_search_layout

namespace rdst_internal {
// rdst_search.cpp: every argument check of rdst_hip_search_device, in the documented order, before any device work.
int search_check_args(const void* dev_sorted, uint64_t len, const void* dev_len, uint32_t len_bytes, const void* dev_needles, uint64_t n_needles,
                      const void* dev_out_lower, const void* dev_out_upper, uint32_t offset_bytes, const void* dev_scratch, uint64_t scratch_bytes,
                      uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, uint32_t flags);
}  // namespace rdst_internal

#endif  // RDST_SEARCH_LAYOUT_H
