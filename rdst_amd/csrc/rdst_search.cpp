// rdst_search.cpp — the host-only half of rdst_hip_search_device (rdst_search.hip): its argument checks in the documented order,
// the size of its scratch and its limits.  No HIP here: tests/cpp/test_rdst_search_host.cpp compiles this file into a
// stand-alone program under the address sanitizer.
#include <stdint.h>

#include "rdst_hip.h"
#include "rdst_args.h"
#include "rdst_search_layout.h"

namespace rdst_internal {
// rdst_kernels.hip (a stand-alone program brings its own): records `what` for rdst_hip_last_error and returns `code`; the
// key arguments as rdst_hip_sort_device checks them.
int note_error(int code, const char* what);
int check_key_args(const void* p, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels);
}  // namespace rdst_internal

using namespace rdst_args;
using rdst_internal::note_error;
namespace L = rdst_search_layout;

int rdst_internal::search_check_args(const void* dev_sorted, uint64_t len, const void* dev_len, uint32_t len_bytes, const void* dev_needles,
                                     uint64_t n_needles, const void* dev_out_lower, const void* dev_out_upper, uint32_t offset_bytes,
                                     const void* dev_scratch, uint64_t scratch_bytes, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                     uint32_t flags) {
    // 1 - 4
    if (int rc = check_key_args(dev_sorted, len, elem_bytes, kind, levels)) return rc;
    if (kind == RDST_KEY_BYTES_BE) return note_error(RDST_ERR_UNSUPPORTED, "search: [u8; N] keys are not built");
    if (len >= (1ull << 32) || n_needles >= (1ull << 32)) return note_error(RDST_ERR_UNSUPPORTED, "search: len and n_needles must be below 2^32");
    if (flags != 0) return note_error(RDST_ERR_ARG, "search: unknown flag bits");
    // 5: the length in device memory
    if (dev_len != nullptr) {
        if (len_bytes != 4 && len_bytes != 8) return note_error(RDST_ERR_ARG, "search: the device-resident length is a 4- or 8-byte unsigned integer");
        if (misaligned(dev_len, len_bytes)) return note_error(RDST_ERR_ALIGN, "search: length pointer not aligned to its size");
    }
    // 6: the needles
    if (n_needles > 0 && dev_needles == nullptr) return note_error(RDST_ERR_ARG, "search: null needle pointer");
    if (misaligned(dev_needles, elem_bytes)) return note_error(RDST_ERR_ALIGN, "search: needle pointer not aligned to the element size");
    // 7: the width of the positions
    if (offset_bytes != 4 && offset_bytes != 8) return note_error(RDST_ERR_ARG, "search: offset_bytes must be 4 or 8");
    // 8: the outputs
    if (dev_out_lower == nullptr && dev_out_upper == nullptr) return note_error(RDST_ERR_ARG, "search: both outputs are null");
    if (misaligned(dev_out_lower, offset_bytes)) return note_error(RDST_ERR_ALIGN, "search: lower output not aligned to offset_bytes");
    if (misaligned(dev_out_upper, offset_bytes)) return note_error(RDST_ERR_ALIGN, "search: upper output not aligned to offset_bytes");
    const Range hay = range_of(dev_sorted, len, elem_bytes), needles = range_of(dev_needles, n_needles, elem_bytes);
    const Range length = dev_len ? range_of(dev_len, 1, len_bytes) : Range{0, 0};
    const Range lower = dev_out_lower ? range_of(dev_out_lower, n_needles, offset_bytes) : Range{0, 0};
    const Range upper = dev_out_upper ? range_of(dev_out_upper, n_needles, offset_bytes) : Range{0, 0};
    if (overlap(lower, hay) || overlap(lower, needles) || overlap(lower, length) || overlap(upper, hay) || overlap(upper, needles) || overlap(upper, length))
        return note_error(RDST_ERR_ARG, "search: an output overlaps the haystack, the needles or the length");
    if (overlap(lower, upper)) return note_error(RDST_ERR_ARG, "search: the outputs overlap each other");
    // 9: the scratch
    if (dev_scratch == nullptr) return note_error(RDST_ERR_ARG, "search: null scratch");
    if (misaligned(dev_scratch, 256)) return note_error(RDST_ERR_ALIGN, "search: scratch not aligned to 256 bytes");
    if (scratch_bytes < L::scratch_bytes(elem_bytes))
        return note_error(RDST_ERR_ARG, "search: scratch_bytes is below rdst_hip_search_scratch_bytes(len, n_needles, elem_bytes)");
    const Range work = range_of(dev_scratch, L::scratch_bytes(elem_bytes), 1);
    if (overlap(work, hay) || overlap(work, needles) || overlap(work, length) || overlap(work, lower) || overlap(work, upper))
        return note_error(RDST_ERR_ARG, "search: the scratch overlaps the haystack, the needles, the length or an output");
    return RDST_OK;
}

// A 256-byte header and the splitter table: the same for every length.
extern "C" uint64_t rdst_hip_search_scratch_bytes(uint64_t len, uint64_t n_needles, uint32_t elem_bytes) {
    if (!L::key_width_ok(elem_bytes) || len >= (1ull << 32) || n_needles >= (1ull << 32)) return 0;
    return L::scratch_bytes(elem_bytes);
}

extern "C" int rdst_hip_search_limits(uint32_t elem_bytes, uint32_t out[3]) {
    if (!out) return note_error(RDST_ERR_ARG, "search_limits: null output");
    if (!L::key_width_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "device path is built for 1-, 2-, 4-, 8- and 16-byte keys");
    out[0] = L::needles_per_tile(elem_bytes);
    out[1] = L::SPLITTERS;
    out[2] = L::window(elem_bytes);
    return RDST_OK;
}
