// rdst_runs.cpp — the host-only half of rdst_hip_runs_device (rdst_runs.hip): its argument checks in the documented order, the
// size of its scratch and its limits.  No HIP here: tests/cpp/test_rdst_runs_host.cpp compiles this file into a stand-alone
// program under the address sanitizer.
#include <stdint.h>

#include "rdst_hip.h"
#include "rdst_args.h"
#include "rdst_runs_layout.h"

namespace rdst_internal {
// rdst_kernels.hip (a stand-alone program brings its own): records `what` for rdst_hip_last_error and returns `code`; the
// key arguments as rdst_hip_sort_device checks them.
int note_error(int code, const char* what);
int check_key_args(const void* p, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels);
}  // namespace rdst_internal

using namespace rdst_args;
using rdst_internal::note_error;
namespace L = rdst_runs_layout;

int rdst_internal::runs_check_args(const void* dev_keys, uint64_t len, const void* dev_len, uint32_t len_bytes, const void* dev_out_keys,
                                   const void* dev_out_starts, const void* dev_n_runs, uint32_t offset_bytes, uint64_t out_capacity,
                                   const void* dev_scratch, uint64_t scratch_bytes, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                   uint32_t flags) {
    // 1 - 4
    if (int rc = check_key_args(dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (kind == RDST_KEY_BYTES_BE) return note_error(RDST_ERR_UNSUPPORTED, "runs: [u8; N] keys are not built");
    if (len >= (1ull << 32)) return note_error(RDST_ERR_UNSUPPORTED, "runs: len must be below 2^32");
    if (flags & ~RDST_RUNS_PAD_STARTS) return note_error(RDST_ERR_ARG, "runs: unknown flag bits");
    // 5: the length in device memory
    if (dev_len != nullptr) {
        if (len_bytes != 4 && len_bytes != 8) return note_error(RDST_ERR_ARG, "runs: the device-resident length is a 4- or 8-byte unsigned integer");
        if (misaligned(dev_len, len_bytes)) return note_error(RDST_ERR_ALIGN, "runs: length pointer not aligned to its size");
    }
    // 6, 7: the width of the offsets, the run count
    if (offset_bytes != 4 && offset_bytes != 8) return note_error(RDST_ERR_ARG, "runs: offset_bytes must be 4 or 8");
    if (dev_n_runs == nullptr) return note_error(RDST_ERR_ARG, "runs: null run count pointer");
    if (misaligned(dev_n_runs, offset_bytes)) return note_error(RDST_ERR_ALIGN, "runs: run count pointer not aligned to offset_bytes");
    const Range in = range_of(dev_keys, len, elem_bytes), count = range_of(dev_n_runs, 1, offset_bytes);
    const Range length = dev_len ? range_of(dev_len, 1, len_bytes) : Range{0, 0};
    if (overlap(in, count) || overlap(length, count)) return note_error(RDST_ERR_ARG, "runs: the run count overlaps the input or the length");
    // 8: the outputs
    Range keys = {0, 0}, starts = {0, 0};
    if (out_capacity > 0) {
        if (dev_out_keys && misaligned(dev_out_keys, elem_bytes)) return note_error(RDST_ERR_ALIGN, "runs: key output not aligned to the element size");
        if (dev_out_starts && misaligned(dev_out_starts, offset_bytes)) return note_error(RDST_ERR_ALIGN, "runs: starts output not aligned to offset_bytes");
        if (dev_out_keys) keys = range_of(dev_out_keys, out_capacity, elem_bytes);
        // (capacity + 1 offsets: a capacity of 2^64 - 1 saturates in range_of)
        if (dev_out_starts) starts = range_of(dev_out_starts, out_capacity == ~0ull ? out_capacity : out_capacity + 1, offset_bytes);
        if (overlap(keys, in) || overlap(starts, in) || overlap(keys, length) || overlap(starts, length))
            return note_error(RDST_ERR_ARG, "runs: an output overlaps the input or the length");
        if (overlap(keys, starts) || overlap(keys, count) || overlap(starts, count)) return note_error(RDST_ERR_ARG, "runs: the outputs overlap each other");
        if ((flags & RDST_RUNS_PAD_STARTS) && dev_out_starts == nullptr) return note_error(RDST_ERR_ARG, "runs: RDST_RUNS_PAD_STARTS needs a starts output");
    }
    // 9: the scratch
    if (dev_scratch == nullptr) return note_error(RDST_ERR_ARG, "runs: null scratch");
    if (misaligned(dev_scratch, 256)) return note_error(RDST_ERR_ALIGN, "runs: scratch not aligned to 256 bytes");
    if (scratch_bytes < L::scratch_bytes(len, elem_bytes)) return note_error(RDST_ERR_ARG, "runs: scratch_bytes is below rdst_hip_runs_scratch_bytes(len, elem_bytes)");
    const Range work = range_of(dev_scratch, L::scratch_bytes(len, elem_bytes), 1);
    if (overlap(work, in) || overlap(work, length) || overlap(work, count) || overlap(work, keys) || overlap(work, starts))
        return note_error(RDST_ERR_ARG, "runs: the scratch overlaps the input, the length or an output");
    return RDST_OK;
}

// A 256-byte header and one 64-bit status word per tile of `len` keys (at least one tile).
extern "C" uint64_t rdst_hip_runs_scratch_bytes(uint64_t len, uint32_t elem_bytes) {
    if (!L::key_width_ok(elem_bytes) || len >= (1ull << 32)) return 0;
    return L::scratch_bytes(len, elem_bytes);
}

extern "C" int rdst_hip_runs_limits(uint32_t elem_bytes, uint32_t out[2]) {
    if (!out) return note_error(RDST_ERR_ARG, "runs_limits: null output");
    if (!L::key_width_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "device path is built for 1-, 2-, 4-, 8- and 16-byte keys");
    out[0] = L::keys_per_tile(elem_bytes);
    out[1] = L::LOOKBACK_WINDOW;
    return RDST_OK;
}
