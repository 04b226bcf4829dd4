// rdst_select_segments_offsets.hip — the segmented select with its table of borders in DEVICE memory
// (rdst_hip_select_segments_device_offsets; include/rdst_hip.h).  The work list is the segmented partial
// sort's with k = 1, made on the device by rdst_topk_segments_offsets.hip (rdst_internal::topk_segments_plan_locked: class
// keys, one stable pair sort, the items, the 256-byte header), and the kernels of rdst_select_segments.hip run over it
// (rdst_internal::select_segments_launch_locked).
//
// far_capacity == 0 — the asynchronous mode: select_segments_async enqueues the plan and, per round of MAX_RANKS specs, the
// three counted launches, and returns.  It calls nothing that waits for the device or copies to the host;
// tests/test_select_segments_offsets_abi.py holds that against this text.  Every segment beyond block_max is of the stream
// class then, whatever its length: one workgroup each.  With k = 1 the plan knows no "k > k_stream_max": only an invalid table
// can fail after the argument checks.
// far_capacity > 0 — the wait mode: select_segments_wait reads the header (read_header: one copy, one wait), launches the
// three classes with the counts it read and runs the far segments one after another through
// rdst_internal::select_slice_locked with the ranks resolved here, their items read with one further wait (read_far_items).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <exception>
#include <mutex>
#include <vector>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_rank_rule.h"
#include "rdst_segments_layout.h"

namespace {

namespace L = rdst_segments_layout;
using rdst_internal::set_error;
using Call = rdst_internal::SelectSegmentsCall;
using Plan = rdst_internal::TopkSegmentsPlan;

// The asynchronous mode after the checks: the plan and, per round, three counted launches, grids from what the host knows — a
// segment holds at least one key, a block-class one more than wave_max, a stream-class one more than block_max —, counts
// from the header.  Nothing here waits for the device or copies to the host.  Callers hold the library's mutex.
int select_segments_async(const Call& c, uint64_t len, const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, const rdst_rank_spec* ranks,
                          void* scratch, uint32_t* err) {
    Plan P;
    if (int rc = rdst_internal::topk_segments_plan_locked(dev_offsets, offset_bytes, n_segments, len, 1, c.elem_bytes, c.index_bytes, true, scratch, true,
                                                          err, c.s, &P))
        return rc;
    const uint64_t bounds[3] = {std::min(n_segments, len), std::min(n_segments, len / ((uint64_t)P.wave_max + 1)),
                                std::min(n_segments, len / ((uint64_t)P.block_max + 1))};
    if (int rc = rdst_internal::profile_open_run(c.s)) return rc;
    return rdst_internal::select_segments_launch_locked(c, P.items, P.hdr, bounds, ranks);
}

// The header as the host reads it: one copy and one wait for `s`.
using PlanResult = L::TopkPlanResult;
int read_header(const Plan& P, PlanResult* r, hipStream_t s) {
    uint32_t h[L::TOPK_PLAN_READ_WORDS] = {};
    RDST_HIP_TRY(hipMemcpyAsync(h, P.hdr, sizeof h, hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    *r = L::topk_plan_result(h);
    return RDST_OK;
}

// The far items and their lengths: two copies and one wait for `s`.
int read_far_items(const Plan& P, uint64_t batched, std::vector<rdst_segment_item>* items, std::vector<uint64_t>* lens, hipStream_t s) {
    RDST_HIP_TRY(hipMemcpyAsync(items->data(), P.items + batched, items->size() * sizeof(rdst_segment_item), hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipMemcpyAsync(lens->data(), P.far_lens, lens->size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    return RDST_OK;
}

int flags_error(uint32_t flags) {
    return set_error(RDST_ERR_ARG, L::topk_plan_flags_message(flags));
}

// The far segments one after another, each by the whole-array select (no copy to the host, no wait), with the ranks resolved
// and ordered here as the host-table entry does it; a spec the segment has no element for is left out.
int run_far_segments(const Call& c, uint64_t len, uint64_t n_segments, const rdst_rank_spec* ranks, const std::vector<rdst_segment_item>& items,
                     const std::vector<uint64_t>& lens, void* far_scratch, uint64_t far_capacity, int cus) {
    std::vector<uint64_t> far_ranks, far_slots, far_order;
    try {
        far_ranks.resize((size_t)c.n_ranks);
        far_slots.resize((size_t)c.n_ranks);
        far_order.resize((size_t)c.n_ranks);
    } catch (const std::exception&) {
        return set_error(RDST_ERR_ARG, "select: no host memory for the far segments' ranks (24 bytes per rank)");
    }
    for (size_t f = 0; f < items.size(); ++f) {
        const uint64_t start = items[f].start, n = lens[f], row = (uint64_t)items[f].seg * c.n_ranks;
        if (n == 0 || n > far_capacity || start > len || n > len - start || items[f].seg >= n_segments)
            return set_error(RDST_ERR_DEVICE, "select: a far item of the device plan lies outside the array");
        uint64_t have = 0;
        for (uint64_t j = 0; j < c.n_ranks; ++j)
            if (rdst_rank_rule::resolve(ranks[j], n, &far_ranks[have])) far_slots[have++] = j;
        if (have == 0) continue;
        int rc = rdst_internal::order_ranks(far_ranks.data(), have, far_order.data());
        if (rc) return rc;
        rc = rdst_internal::select_slice_locked(static_cast<const char*>(c.keys) + start * c.elem_bytes, n, far_ranks.data(), far_slots.data(), far_order.data(),
                                                have, static_cast<char*>(c.out_keys) + row * c.elem_bytes,
                                                c.out_index ? static_cast<char*>(c.out_index) + row * c.index_bytes : nullptr, c.index_bytes, far_scratch, 0,
                                                c.elem_bytes, c.kind, c.largest, cus, c.s);
        if (rc) return rc;
    }
    return RDST_OK;
}

// The wait mode after the checks.  Callers hold the library's mutex.
int select_segments_wait(const Call& c, uint64_t len, const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, const rdst_rank_spec* ranks,
                         void* scratch, void* far_scratch, uint64_t far_capacity, int cus) {
    Plan P;
    int rc = rdst_internal::topk_segments_plan_locked(dev_offsets, offset_bytes, n_segments, len, 1, c.elem_bytes, c.index_bytes, false, scratch, false,
                                                      nullptr, c.s, &P);
    if (rc) return rc;
    PlanResult r;
    if ((rc = read_header(P, &r, c.s))) return rc;  // the one wait of this mode (and one more below, if there are far segments)
    if (r.flags) return flags_error(r.flags);
    if (r.counts[3] != 0 && far_capacity < r.longest_far) return set_error(RDST_ERR_ARG, "select: far_capacity is below the longest far segment");
    const uint64_t batched = r.counts[0] + r.counts[1] + r.counts[2];
    if (batched + r.counts[3] > n_segments) return set_error(RDST_ERR_DEVICE, "select: the device plan counts more items than segments");
    if (batched) {
        if ((rc = rdst_internal::profile_open_run(c.s))) return rc;
        if ((rc = rdst_internal::select_segments_launch_locked(c, P.items, nullptr, r.counts, ranks))) return rc;
    }
    if (r.counts[3] == 0) return RDST_OK;
    std::vector<rdst_segment_item> far_items;
    std::vector<uint64_t> far_lens;
    try {
        far_items.resize((size_t)r.counts[3]);
        far_lens.resize((size_t)r.counts[3]);
    } catch (const std::exception&) {
        return set_error(RDST_ERR_ARG, "select: no host memory for the far segments' items (24 bytes per far segment)");
    }
    if ((rc = read_far_items(P, batched, &far_items, &far_lens, c.s))) return rc;
    return run_far_segments(c, len, n_segments, ranks, far_items, far_lens, far_scratch, far_capacity, cus);
}

}  // namespace

extern "C" int rdst_hip_select_segments_device_offsets(const void* dev_keys, uint64_t len, const void* dev_offsets, uint32_t offset_bytes,
                                                       uint64_t n_segments, const rdst_rank_spec* ranks, uint64_t n_ranks, void* dev_out_keys,
                                                       void* dev_out_index, uint32_t index_bytes, void* dev_scratch, uint64_t scratch_bytes,
                                                       uint64_t far_capacity, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, uint32_t flags,
                                                       void* stream) {
    // 1: the key arguments, len and flags, as rdst_hip_select_segments_device checks them
    if (int rc = rdst_internal::rank_check_head("select", dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (flags & ~RDST_TOPK_LARGEST) return set_error(RDST_ERR_ARG, "select: unknown flag bits");
    // 2
    if (n_ranks == 0 || n_segments == 0) return RDST_OK;
    // 3: the table
    int rc = rdst_internal::check_offsets_table(dev_offsets, offset_bytes, n_segments, len);
    if (rc) return rc;
    // 4: the ranks
    if (ranks == nullptr) return set_error(RDST_ERR_ARG, "select: null ranks");
    for (uint64_t i = 0; i < n_ranks; ++i)
        if (!rdst_rank_rule::spec_ok(ranks[i])) {
            char msg[160];
            snprintf(msg, sizeof msg, "select: ranks[%llu] is not a rank spec (num <= den for a quantile, mode 0 .. 2, 0 for an absolute rank, reserved 0)",
                     (unsigned long long)i);
            return set_error(RDST_ERR_ARG, msg);
        }
    // 5, 6: the outputs, the scratch
    if ((rc = rdst_internal::rank_check_outputs("select", dev_out_keys, dev_out_index, &index_bytes, dev_scratch, elem_bytes))) return rc;
    if (far_capacity >= (1ull << 32)) return set_error(RDST_ERR_ARG, "select: far_capacity must be below 2^32 (pass len)");
    if (scratch_bytes < rdst_hip_select_segments_device_offsets_scratch_bytes(n_segments, far_capacity, n_ranks, elem_bytes, index_bytes))
        return set_error(RDST_ERR_ARG, "select: scratch_bytes is below rdst_hip_select_segments_device_offsets_scratch_bytes(n_segments, far_capacity, n_ranks, elem_bytes, index_bytes)");
    const bool async = far_capacity == 0;
    const Call c{dev_keys, n_ranks, dev_out_keys, dev_out_index, index_bytes, elem_bytes, kind, (flags & RDST_TOPK_LARGEST) != 0, static_cast<hipStream_t>(stream)};
    uint32_t* err = nullptr;
    int cus = 0;
    if ((rc = rdst_internal::device_error_word(&err, &cus))) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    if (async) return select_segments_async(c, len, dev_offsets, offset_bytes, n_segments, ranks, dev_scratch, err);
    return select_segments_wait(c, len, dev_offsets, offset_bytes, n_segments, ranks, dev_scratch,
                                static_cast<char*>(dev_scratch) + L::plan_layout(n_segments).total, far_capacity, cus);
}
