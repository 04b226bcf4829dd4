// rdst_rank_args.cpp — the host-only half of the six rank entries (rdst_hip_topk_device, rdst_hip_select_device, their segmented
// forms with the borders on the host and in device memory): the argument checks they share, the sizes of their scratch and their
// limits.  No HIP here: tests/cpp/test_rdst_rank_args_host.cpp compiles this file into a stand-alone program under the sanitizers.
#include <stdio.h>

#include <algorithm>

#include "rdst_hip.h"
#include "rdst_args.h"
#include "rdst_segments_layout.h"
#include "rdst_select_layout.h"
#include "rdst_topk_layout.h"

namespace rdst_internal {
// rdst_kernels.hip (a stand-alone program brings its own): keeps a copy of `what` for rdst_hip_last_error; the sort's key checks
int note_error(int code, const char* what);
int check_key_args(const void* p, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels);
}  // namespace rdst_internal

using namespace rdst_args;
using rdst_internal::note_error;
namespace S = rdst_segments_layout;
namespace Q = rdst_select_layout;
namespace T = rdst_topk_layout;

namespace {
// "<what>: <text>": note_error keeps a copy, so the buffer may go
int fail(int code, const char* what, const char* text) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s: %s", what, text);
    return note_error(code, msg);
}

// the widths of an index output that is there
int check_index_widths(const char* what, uint32_t elem_bytes, uint32_t index_bytes) {
    if (!index_bytes_ok(index_bytes)) return fail(RDST_ERR_ARG, what, "index_bytes must be 4 or 8");
    if (!index_keys_ok(elem_bytes)) return fail(RDST_ERR_UNSUPPORTED, what, "an index output takes 4- or 8-byte keys");
    return RDST_OK;
}

// what both ..._limits functions check before they answer
int check_limits_args(const char* what, uint32_t elem_bytes, uint32_t index_bytes, const uint32_t* out) {
    if (out == nullptr) return note_error(RDST_ERR_ARG, "null output");
    if (!key_width_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "device path is built for 1-, 2-, 4-, 8- and 16-byte keys");
    return index_bytes != 0 ? check_index_widths(what, elem_bytes, index_bytes) : RDST_OK;
}

// what every segmented size function refuses (it answers 0); `lim`: the classes' limits (the select's plan is the top-k's, k = 1)
bool segments_ok(uint64_t n_segments, uint64_t max_segments, uint64_t longest, uint32_t elem_bytes, uint32_t index_bytes, uint32_t lim[4]) {
    return n_segments != 0 && n_segments <= max_segments && longest < (1ull << 32) && rdst_hip_topk_segments_limits(elem_bytes, index_bytes, lim) == RDST_OK;
}
}  // namespace

int rdst_internal::rank_check_head(const char* what, const void* dev_keys, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels) {
    if (int rc = check_key_args(dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (kind == RDST_KEY_BYTES_BE) return fail(RDST_ERR_UNSUPPORTED, what, "[u8; N] keys are not built");
    if (len >= (1ull << 32)) return fail(RDST_ERR_UNSUPPORTED, what, "len must be below 2^32");
    return RDST_OK;
}

int rdst_internal::rank_check_outputs(const char* what, const void* dev_out_keys, const void* dev_out_index, uint32_t* index_bytes, const void* dev_scratch,
                                      uint32_t elem_bytes) {
    if (dev_out_keys == nullptr) return fail(RDST_ERR_ARG, what, "null key output");
    if (misaligned(dev_out_keys, elem_bytes)) return fail(RDST_ERR_ALIGN, what, "key output not aligned to the element size");
    if (dev_out_index != nullptr) {
        if (int rc = check_index_widths(what, elem_bytes, *index_bytes)) return rc;
        if (misaligned(dev_out_index, *index_bytes)) return fail(RDST_ERR_ALIGN, what, "index output not aligned to index_bytes");
    } else {
        *index_bytes = 0;  // without an index output index_bytes is not looked at
    }
    return rank_check_scratch(what, dev_scratch);
}

int rdst_internal::rank_check_scratch(const char* what, const void* dev_scratch) {
    if (dev_scratch == nullptr) return fail(RDST_ERR_ARG, what, "null scratch");
    if (misaligned(dev_scratch, 256)) return fail(RDST_ERR_ALIGN, what, "scratch not aligned to 256 bytes");
    return RDST_OK;
}

extern "C" {
uint64_t rdst_hip_topk_scratch_bytes(uint64_t len, uint64_t k, uint32_t elem_bytes, uint32_t index_bytes, uint64_t cand_capacity) {
    if (!key_width_ok(elem_bytes) || !index_widths_ok(elem_bytes, index_bytes)) return 0;
    return T::topk_layout(len, k, elem_bytes, index_bytes, cand_capacity).total;
}

int rdst_hip_topk_limits(uint32_t elem_bytes, uint32_t index_bytes, uint32_t out[3]) {
    if (int rc = check_limits_args("topk", elem_bytes, index_bytes, out)) return rc;
    const uint32_t digit = T::digit_bits_for(elem_bytes);
    out[0] = digit;
    out[1] = (uint32_t)T::DEFAULT_CAND_CAPACITY;
    out[2] = levels_over(8 * elem_bytes, digit) + (index_bytes ? levels_over(POSITION_BITS, digit) : 0);
    return RDST_OK;
}

// (n_ranks costs nothing: a longer list is served in rounds on the same scratch)
uint64_t rdst_hip_select_scratch_bytes(uint64_t len, uint64_t, uint32_t elem_bytes, uint32_t index_bytes, uint64_t cand_capacity) {
    if (!key_width_ok(elem_bytes) || !index_widths_ok(elem_bytes, index_bytes)) return 0;
    return Q::select_layout(len, elem_bytes, index_bytes, cand_capacity).total;
}

int rdst_hip_select_limits(uint32_t elem_bytes, uint32_t index_bytes, uint32_t out[5]) {
    if (int rc = check_limits_args("select", elem_bytes, index_bytes, out)) return rc;
    out[0] = Q::MAX_RANKS;
    out[1] = Q::digit0_bits_for(elem_bytes);
    out[2] = Q::DIGIT_BITS;
    out[3] = (uint32_t)Q::DEFAULT_CAND_CAPACITY;
    out[4] = Q::key_levels_for(elem_bytes) + (index_bytes ? levels_over(POSITION_BITS, Q::DIGIT_BITS) : 0);
    return RDST_OK;
}

// Borders on the host: the item table; behind it, if a far segment is possible, the whole-array entry's scratch for the longest.
uint64_t rdst_hip_topk_segments_scratch_bytes(uint64_t n_segments, uint64_t longest_segment, uint64_t k, uint32_t elem_bytes, uint32_t index_bytes) {
    uint32_t lim[4];
    if (!segments_ok(n_segments, (1ull << 32) - 1, longest_segment, elem_bytes, index_bytes, lim)) return 0;
    const bool far = longest_segment > lim[2] || (longest_segment > lim[1] && k > lim[3]);
    return S::table_bytes(n_segments) + (far ? rdst_hip_topk_scratch_bytes(longest_segment, std::min(k, longest_segment), elem_bytes, index_bytes, 0) : 0);
}

uint64_t rdst_hip_select_segments_scratch_bytes(uint64_t n_segments, uint64_t longest_segment, uint64_t n_ranks, uint32_t elem_bytes, uint32_t index_bytes) {
    uint32_t lim[4];
    if (!segments_ok(n_segments, (1ull << 32) - 1, longest_segment, elem_bytes, index_bytes, lim)) return 0;
    return S::table_bytes(n_segments) + (longest_segment > lim[2] ? rdst_hip_select_scratch_bytes(longest_segment, n_ranks, elem_bytes, index_bytes, 0) : 0);
}

// Borders in device memory: the plan's layout; with far_capacity > 0, behind it the whole-array entry's scratch for that many keys.
uint64_t rdst_hip_topk_segments_device_offsets_scratch_bytes(uint64_t n_segments, uint64_t far_capacity, uint64_t k, uint32_t elem_bytes, uint32_t index_bytes) {
    uint32_t lim[4];
    if (!segments_ok(n_segments, S::MAX_SEGMENTS, far_capacity, elem_bytes, index_bytes, lim)) return 0;
    return S::plan_layout(n_segments).total + (far_capacity ? rdst_hip_topk_scratch_bytes(far_capacity, std::min(k, far_capacity), elem_bytes, index_bytes, 0) : 0);
}

uint64_t rdst_hip_select_segments_device_offsets_scratch_bytes(uint64_t n_segments, uint64_t far_capacity, uint64_t n_ranks, uint32_t elem_bytes, uint32_t index_bytes) {
    uint32_t lim[4];
    if (!segments_ok(n_segments, S::MAX_SEGMENTS, far_capacity, elem_bytes, index_bytes, lim)) return 0;
    return S::plan_layout(n_segments).total + (far_capacity ? rdst_hip_select_scratch_bytes(far_capacity, n_ranks, elem_bytes, index_bytes, 0) : 0);
}
}  // extern "C"
