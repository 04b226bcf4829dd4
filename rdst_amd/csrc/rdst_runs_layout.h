// rdst_runs_layout.h — what rdst_runs.hip (the kernels) and rdst_runs.cpp (the host-only checks and the size function) of
// rdst_hip_runs_device share: the tile, the look-back window and the layout of the caller's scratch.  No HIP here.
#ifndef RDST_RUNS_LAYOUT_H
#define RDST_RUNS_LAYOUT_H

#include <stdint.h>

#include "rdst_hip.h"
#include "rdst_args.h"

namespace rdst_runs_layout {

constexpr uint32_t THREADS = 256;  // one workgroup per tile: four waves, each over a contiguous quarter of the tile
// 16-byte loads per thread and tile.  Every tile costs one ticket, and one word gives out about 88 tickets a microsecond:
// 16 KiB tiles ran at 12.5 ns per tile, 1.2 TB/s, whatever the key width.  Above that the tile's lifetime (ticket, loads,
// look-back, stores, one after the other) against the workgroups a CU holds decides, and was measured per width (DESIGN.md
// §2l): 64 KiB of 8- and 16-byte keys, 32 KiB of 4-byte keys; 2- and 1-byte keys unroll to more keys per load and stay at 32
// and 16 KiB.
constexpr uint32_t rows(uint32_t elem_bytes) { return elem_bytes >= 8 ? 16 : (elem_bytes == 1 ? 4 : 8); }
constexpr uint32_t LOOKBACK_WINDOW = 8;  // predecessor status words fetched per look-back round trip

using rdst_args::key_width_ok;
constexpr uint32_t keys_per_tile(uint32_t elem_bytes) { return THREADS * rows(elem_bytes) * 16 / elem_bytes; }
// tiles the launch is sized for: those of `len` keys, one for an empty array (it writes the outputs of m == 0)
constexpr uint64_t tiles(uint64_t len, uint32_t elem_bytes) {
    const uint64_t t = (len + keys_per_tile(elem_bytes) - 1) / keys_per_tile(elem_bytes);
    return t ? t : 1;
}
constexpr uint64_t up256(uint64_t x) { return (x + 255) / 256 * 256; }

// The scratch: a 256-byte header whose first word is the ticket counter, then one 64-bit status word per tile.
constexpr uint64_t HEADER_BYTES = 256;
constexpr uint64_t scratch_bytes(uint64_t len, uint32_t elem_bytes) { return HEADER_BYTES + up256(8 * tiles(len, elem_bytes)); }

}  // namespace rdst_runs_layout

namespace rdst_internal {
// rdst_runs.cpp: every argument check of rdst_hip_runs_device, in the documented order, before any device work.
int runs_check_args(const void* dev_keys, uint64_t len, const void* dev_len, uint32_t len_bytes, const void* dev_out_keys, const void* dev_out_starts,
                    const void* dev_n_runs, uint32_t offset_bytes, uint64_t out_capacity, const void* dev_scratch, uint64_t scratch_bytes,
                    uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, uint32_t flags);
}  // namespace rdst_internal

#endif  // RDST_RUNS_LAYOUT_H
