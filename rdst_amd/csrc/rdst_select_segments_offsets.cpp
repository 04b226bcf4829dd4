// rdst_select_segments_offsets.cpp — the host-only half of rdst_hip_select_segments_device_offsets
// (rdst_select_segments_offsets.hip): the size of its scratch.  No HIP here: tests/cpp/test_rdst_select_segments_offsets_host.cpp
// compiles this file into a stand-alone program under the address sanitizer.
#include <stdint.h>

#include "rdst_hip.h"
#include "rdst_segments_layout.h"

namespace L = rdst_segments_layout;

// The plan's layout (header, class keys and segment indices with their tmps, item table); with far_capacity > 0, behind it the
// whole-array select's scratch for a far segment of far_capacity keys.
extern "C" uint64_t rdst_hip_select_segments_device_offsets_scratch_bytes(uint64_t n_segments, uint64_t far_capacity, uint64_t n_ranks, uint32_t elem_bytes,
                                                                          uint32_t index_bytes) {
    uint32_t lim[4];
    if (n_segments == 0 || n_segments > L::MAX_SEGMENTS || far_capacity >= (1ull << 32)) return 0;
    if (rdst_hip_select_segments_limits(elem_bytes, index_bytes, lim)) return 0;
    uint64_t total = L::plan_layout(n_segments).total;
    if (far_capacity != 0) total += rdst_hip_select_scratch_bytes(far_capacity, n_ranks, elem_bytes, index_bytes, 0);
    return total;
}
