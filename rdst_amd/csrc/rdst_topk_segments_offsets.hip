// rdst_topk_segments_offsets.hip — the segmented partial sort with its table of borders in DEVICE memory
// (rdst_hip_topk_segments_device_offsets; include/rdst_hip.h): rdst_topk_segments_plan's work list made on the
// device, the way rdst_segments.hip makes the segmented sort's, and the kernels of rdst_topk_segments.hip run over it.
//
// The plan, in the caller's scratch (rdst_segments_layout.h: plan_layout, TopkPlanHeader, topk_class_key):
//   topk_segments_keygen_kernel   a class key per segment, the four counts, the flags and the longest far segment into the header
//   one stable (u32 key, u32 segment) pair sort by the library's own route: the sorted pairs are the work list
//   topk_segments_items_kernel    the items from the sorted pairs, the far items' lengths for the host, the header closed: with
//                                 a flag up the counted kernels get zero counts
//
// far_capacity == 0 — the asynchronous mode: topk_segments_async enqueues the plan and the three counted launches
// (rdst_internal::topk_segments_launch_locked with the header) and returns.  It calls nothing that waits for the device or
// copies to the host; tests/test_topk_segments_offsets_abi.py holds that against this text.  Every segment beyond block_max is of the
// stream class then, whatever its length: one workgroup each.
// far_capacity > 0 — the wait mode: topk_segments_wait reads the header (read_plan: one copy, one wait), launches the three
// classes with the counts it read and runs the far segments one after another through rdst_internal::topk_slice_locked, their
// items read with one further wait (read_far).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "rdst_hip.h"
#include "rdst_internal.h"
#include "rdst_segments_layout.h"

namespace {

namespace L = rdst_segments_layout;
using rdst_internal::launch;
using rdst_internal::set_error;
using Call = rdst_internal::TopkSegmentsCall;

constexpr int PLAN_THREADS = 256;
constexpr uint32_t ERR_SEGMENTS_TABLE = 16;  // the device error word's bit for a table the device refuses (the segmented sort's)

// ---- the plan on the device --------------------------------------------------------------------------------------------------

template <typename Off>
__global__ __launch_bounds__(PLAN_THREADS) void topk_segments_keygen_kernel(const Off* __restrict__ offsets, uint32_t n_segments, uint64_t len,
                                                                            uint32_t wave_max, uint32_t block_max, uint32_t stream_limit,
                                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ segs,
                                                                            uint32_t* __restrict__ hdr) {
    __shared__ uint32_t s_count[5];  // wave, block, stream, far, flags
    __shared__ unsigned long long s_longest;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 5) s_count[tid] = 0;
    if (tid == 0) s_longest = 0;
    __syncthreads();
    const uint32_t s = blockIdx.x * PLAN_THREADS + (uint32_t)tid;  // n_segments <= 2^30
    uint32_t cls = 4, flags = 0;
    uint64_t n = 0;
    if (s < n_segments) {
        const uint64_t lo = offsets[s], hi = offsets[s + 1];
        if (hi < lo) flags |= L::TOPK_PLAN_DECREASING;
        else n = hi - lo;
        if (s == n_segments - 1 && hi > len) flags |= L::TOPK_PLAN_PAST_LEN;
        cls = L::topk_class(n, wave_max, block_max, stream_limit);
        keys[s] = L::topk_class_key(n, wave_max, block_max, stream_limit);
        segs[s] = s;
    }
    // per wave one LDS atomic per count, per workgroup one global atomic per count
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t hits = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == c));
        if (lane == 0 && hits) atomicAdd(&s_count[c], hits);
    }
    if (flags) atomicOr(&s_count[4], flags);                     // (an invalid table: nothing is written, time does not matter)
    if (cls == 3) atomicMax(&s_longest, (unsigned long long)n);  // (far segments are few)
    __syncthreads();
    if (tid < 4 && s_count[tid]) atomicAdd(&hdr[L::HDR_TOPK_N_WAVE + tid], s_count[tid]);
    if (tid == 4 && s_count[4]) atomicOr(&hdr[L::HDR_TOPK_FLAGS], s_count[4]);
    if (tid == 5 && s_longest) atomicMax(reinterpret_cast<unsigned long long*>(hdr + L::HDR_TOPK_LONGEST_FAR), s_longest);
}

// One thread per sorted pair: position i of the sorted pairs is position i of the work list.  `far_lens`: the unsaturated
// lengths of the far items, in their order (for the host, which enqueues them).  Thread 0 closes the header: with a flag up —
// or, with `no_far`, a far segment — the counted kernels get zero counts and `err` (if given) the table bit.
template <typename Off>
__global__ __launch_bounds__(PLAN_THREADS) void topk_segments_items_kernel(const Off* __restrict__ offsets, uint32_t n_segments,
                                                                           const uint32_t* __restrict__ keys, const uint32_t* __restrict__ segs,
                                                                           rdst_segment_item* __restrict__ items, uint64_t* __restrict__ far_lens,
                                                                           uint32_t* hdr, uint32_t no_far, uint32_t* err) {
    const uint32_t i = blockIdx.x * PLAN_THREADS + threadIdx.x;
    const uint32_t n_wave = hdr[L::HDR_TOPK_N_WAVE], n_block = hdr[L::HDR_TOPK_N_BLOCK], n_stream = hdr[L::HDR_TOPK_N_STREAM];
    if (i == 0) {
        uint32_t flags = hdr[L::HDR_TOPK_FLAGS];
        if (no_far && hdr[L::HDR_TOPK_N_FAR] != 0) {
            flags |= L::TOPK_PLAN_FAR;
            hdr[L::HDR_TOPK_FLAGS] = flags;
        }
        hdr[L::HDR_TOPK_RUN_WAVE] = flags ? 0u : n_wave;
        hdr[L::HDR_TOPK_RUN_BLOCK] = flags ? 0u : n_block;
        hdr[L::HDR_TOPK_RUN_STREAM] = flags ? 0u : n_stream;
        if (flags && err) atomicOr(err, ERR_SEGMENTS_TABLE);
    }
    if (i >= n_segments) return;
    const uint32_t key = keys[i], seg = segs[i];
    if (key == L::TOPK_KEY_NONE || seg >= n_segments) return;  // no item (and a segment index is never trusted beyond the table)
    const uint64_t lo = offsets[seg], n = (uint64_t)offsets[seg + 1] - lo;  // (an item's class says offsets[seg + 1] > lo)
    items[i] = {lo, (uint32_t)(n < 0xFFFFFFFFull ? n : 0xFFFFFFFFull), seg};
    if (key == L::TOPK_KEY_FAR) {
        const uint32_t j = i - n_wave - n_block - n_stream;
        if (j < n_segments) far_lens[j] = n;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// The caller's scratch: header, the plan's pair arrays and their tmps, the item table, where rdst_segments_layout.h puts them.
struct PlanScratch {
    uint32_t* hdr;
    uint32_t *keys, *segs, *tmp_keys, *tmp_segs;
    rdst_segment_item* items;
    uint64_t* far_lens;  // over the two tmps, which are dead once the pairs are sorted
};

PlanScratch plan_scratch(void* scratch, uint64_t n_segments) {
    static_assert(sizeof(uint64_t) == 2 * sizeof(uint32_t), "the far lengths fit the two tmps");
    const L::PlanLayout at = L::plan_layout(n_segments);
    char* base = static_cast<char*>(scratch);
    const auto u32 = [base](uint64_t offset) { return reinterpret_cast<uint32_t*>(base + offset); };
    return {u32(0), u32(at.keys), u32(at.segs), u32(at.tmp_keys), u32(at.tmp_segs), reinterpret_cast<rdst_segment_item*>(base + at.items),
            reinterpret_cast<uint64_t*>(base + at.tmp_keys)};
}

// What the classes are cut by: the limits of rdst_hip_topk_segments_limits, and the longest segment of the stream class for
// this k and mode — block_max (no stream class) for a k beyond k_stream_max, 2^32 - 1 with `unbounded`.
struct Cuts {
    uint32_t wave_max, block_max, stream_limit;
};
int class_cuts(uint64_t k, uint32_t elem_bytes, uint32_t index_bytes, bool unbounded, Cuts* out) {
    uint32_t lim[4];
    if (int rc = rdst_hip_topk_segments_limits(elem_bytes, index_bytes, lim)) return rc;
    *out = {lim[0], lim[1], k > lim[3] ? lim[1] : (unbounded ? 0xFFFFFFFFu : lim[2])};
    return RDST_OK;
}

// Enqueues the plan: header cleared, class keys, the pair sort (it takes and hands back the workspace itself), items.
// Callers hold the library's mutex.  Nothing here waits for the device.
template <typename Off>
int enqueue_plan_t(const void* dev_offsets, uint64_t n_segments, uint64_t len, const Cuts& cuts, const PlanScratch& P, uint32_t no_far, uint32_t* err,
                   hipStream_t s) {
    const Off* off = static_cast<const Off*>(dev_offsets);
    const uint32_t nseg = (uint32_t)n_segments;
    const dim3 grid((uint32_t)((n_segments + PLAN_THREADS - 1) / PLAN_THREADS));
    RDST_HIP_TRY(hipMemsetAsync(P.hdr, 0, L::HDR_TOPK_WORDS * sizeof(uint32_t), s));
    int rc = launch("topk_segments_keygen_kernel", topk_segments_keygen_kernel<Off>, grid, dim3(PLAN_THREADS), 0, s, off, nseg, len, cuts.wave_max,
                    cuts.block_max, cuts.stream_limit, P.keys, P.segs, P.hdr);
    if (rc) return rc;
    if (n_segments > 1 && (rc = rdst_internal::sort_pairs_slice_locked(P.keys, P.segs, P.tmp_keys, P.tmp_segs, n_segments, 4, RDST_KEY_UNSIGNED, 4, s))) return rc;
    return launch("topk_segments_items_kernel", topk_segments_items_kernel<Off>, grid, dim3(PLAN_THREADS), 0, s, off, nseg,
                  static_cast<const uint32_t*>(P.keys), static_cast<const uint32_t*>(P.segs), P.items, P.far_lens, P.hdr, no_far, err);
}

int enqueue_plan(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len, const Cuts& cuts, const PlanScratch& P,
                 uint32_t no_far, uint32_t* err, hipStream_t s) {
    return offset_bytes == 4 ? enqueue_plan_t<uint32_t>(dev_offsets, n_segments, len, cuts, P, no_far, err, s)
                             : enqueue_plan_t<uint64_t>(dev_offsets, n_segments, len, cuts, P, no_far, err, s);
}

// The asynchronous mode after the checks: the plan and three counted launches, grids from what the host knows — a segment
// holds at least one key, a block-class one more than wave_max, a stream-class one more than block_max —, counts from the
// header.  Nothing here waits for the device or copies to the host.  Callers hold the library's mutex.
int topk_segments_async(const Call& c, uint64_t len, const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, const Cuts& cuts,
                        const PlanScratch& P, uint32_t* err) {
    if (int rc = enqueue_plan(dev_offsets, offset_bytes, n_segments, len, cuts, P, 1u, err, c.s)) return rc;
    const uint64_t bounds[3] = {std::min(n_segments, len), std::min(n_segments, len / ((uint64_t)cuts.wave_max + 1)),
                                cuts.stream_limit > cuts.block_max ? std::min(n_segments, len / ((uint64_t)cuts.block_max + 1)) : 0};
    if (int rc = rdst_internal::profile_open_run(c.s)) return rc;
    return rdst_internal::topk_segments_launch_locked(c, P.items, P.hdr, bounds);
}

// The header as the host reads it (the wait mode and the plan hook): one copy and one wait for `s`.
using PlanResult = L::TopkPlanResult;
int read_plan(const PlanScratch& P, PlanResult* r, hipStream_t s) {
    uint32_t h[L::TOPK_PLAN_READ_WORDS] = {};
    RDST_HIP_TRY(hipMemcpyAsync(h, P.hdr, sizeof h, hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    *r = L::topk_plan_result(h);
    return RDST_OK;
}

// The far items and their lengths: two copies and one wait for `s`.
int read_far(const PlanScratch& P, uint64_t batched, std::vector<rdst_segment_item>* items, std::vector<uint64_t>* lens, hipStream_t s) {
    RDST_HIP_TRY(hipMemcpyAsync(items->data(), P.items + batched, items->size() * sizeof(rdst_segment_item), hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipMemcpyAsync(lens->data(), P.far_lens, lens->size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    return RDST_OK;
}

int flags_error(uint32_t flags) {
    return set_error(RDST_ERR_ARG, L::topk_plan_flags_message(flags));
}

// The wait mode after the checks.  Callers hold the library's mutex.
int topk_segments_wait(const Call& c, uint64_t len, const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, const Cuts& cuts,
                       const PlanScratch& P, void* far_scratch, uint64_t far_capacity, int cus) {
    int rc = enqueue_plan(dev_offsets, offset_bytes, n_segments, len, cuts, P, 0u, nullptr, c.s);
    if (rc) return rc;
    PlanResult r;
    if ((rc = read_plan(P, &r, c.s))) return rc;  // the one wait of this mode (and one more below, if there are far segments)
    if (r.flags) return flags_error(r.flags);
    if (r.counts[3] != 0 && far_capacity < r.longest_far) return set_error(RDST_ERR_ARG, "topk: far_capacity is below the longest far segment");
    const uint64_t batched = r.counts[0] + r.counts[1] + r.counts[2];
    if (batched + r.counts[3] > n_segments) return set_error(RDST_ERR_DEVICE, "topk: the device plan counts more items than segments");
    if (batched) {
        if ((rc = rdst_internal::profile_open_run(c.s))) return rc;
        if ((rc = rdst_internal::topk_segments_launch_locked(c, P.items, nullptr, r.counts))) return rc;
    }
    if (r.counts[3] == 0) return RDST_OK;
    std::vector<rdst_segment_item> far_items((size_t)r.counts[3]);
    std::vector<uint64_t> far_lens((size_t)r.counts[3]);
    if ((rc = read_far(P, batched, &far_items, &far_lens, c.s))) return rc;
    for (size_t i = 0; i < far_items.size(); ++i) {
        const uint64_t start = far_items[i].start, n = far_lens[i], row = (uint64_t)far_items[i].seg * c.k;
        if (n == 0 || n > far_capacity || start > len || n > len - start || far_items[i].seg >= n_segments)
            return set_error(RDST_ERR_DEVICE, "topk: a far item of the device plan lies outside the array");
        rc = rdst_internal::topk_slice_locked(static_cast<const char*>(c.keys) + start * c.elem_bytes, n, std::min(c.k, n),
                                              static_cast<char*>(c.out_keys) + row * c.elem_bytes,
                                              c.out_index ? static_cast<char*>(c.out_index) + row * c.index_bytes : nullptr, c.index_bytes, far_scratch,
                                              c.elem_bytes, c.kind, c.largest, cus, c.s);
        if (rc) return rc;
    }
    return RDST_OK;
}

}  // namespace

// The plan for another entry over the same work list (rdst_internal.h; the segmented select's, k = 1).
int rdst_internal::topk_segments_plan_locked(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len, uint64_t k,
                                             uint32_t elem_bytes, uint32_t index_bytes, bool unbounded_stream, void* scratch, bool no_far, uint32_t* err,
                                             hipStream_t s, TopkSegmentsPlan* out) {
    Cuts cuts;
    if (int rc = class_cuts(k, elem_bytes, index_bytes, unbounded_stream, &cuts)) return rc;
    const PlanScratch P = plan_scratch(scratch, n_segments);
    *out = {P.hdr, P.items, P.far_lens, cuts.wave_max, cuts.block_max, cuts.stream_limit};
    return enqueue_plan(dev_offsets, offset_bytes, n_segments, len, cuts, P, no_far ? 1u : 0u, err, s);
}

extern "C" int rdst_hip_topk_segments_device_offsets(const void* dev_keys, uint64_t len, const void* dev_offsets, uint32_t offset_bytes,
                                                     uint64_t n_segments, uint64_t k, void* dev_out_keys, void* dev_out_index, uint32_t index_bytes,
                                                     void* dev_scratch, uint64_t scratch_bytes, uint64_t far_capacity, uint32_t elem_bytes,
                                                     rdst_key_kind kind, uint32_t levels, uint32_t flags, void* stream) {
    // 1: the key arguments, len and flags, as rdst_hip_topk_segments_device checks them
    if (int rc = rdst_internal::rank_check_head("topk", dev_keys, len, elem_bytes, kind, levels)) return rc;
    if (flags & ~RDST_TOPK_LARGEST) return set_error(RDST_ERR_ARG, "topk: unknown flag bits");
    // 2
    if (k == 0 || n_segments == 0) return RDST_OK;
    // 3: the table
    int rc = rdst_internal::check_offsets_table(dev_offsets, offset_bytes, n_segments, len);
    if (rc) return rc;
    // 4, 5: the outputs, the scratch
    if ((rc = rdst_internal::rank_check_outputs("topk", dev_out_keys, dev_out_index, &index_bytes, dev_scratch, elem_bytes))) return rc;
    if (far_capacity >= (1ull << 32)) return set_error(RDST_ERR_ARG, "topk: far_capacity must be below 2^32 (pass len)");
    if (scratch_bytes < rdst_hip_topk_segments_device_offsets_scratch_bytes(n_segments, far_capacity, k, elem_bytes, index_bytes))
        return set_error(RDST_ERR_ARG, "topk: scratch_bytes is below rdst_hip_topk_segments_device_offsets_scratch_bytes(n_segments, far_capacity, k, elem_bytes, index_bytes)");
    const bool async = far_capacity == 0;
    Cuts cuts;
    if ((rc = class_cuts(k, elem_bytes, index_bytes, async, &cuts))) return rc;
    const PlanScratch P = plan_scratch(dev_scratch, n_segments);
    const Call c{dev_keys, k, dev_out_keys, dev_out_index, index_bytes, elem_bytes, kind, (flags & RDST_TOPK_LARGEST) != 0, static_cast<hipStream_t>(stream)};
    uint32_t* err = nullptr;
    int cus = 0;
    if ((rc = rdst_internal::device_error_word(&err, &cus))) return rc;  // (takes the mutex itself)
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    if (async) return topk_segments_async(c, len, dev_offsets, offset_bytes, n_segments, cuts, P, err);
    return topk_segments_wait(c, len, dev_offsets, offset_bytes, n_segments, cuts, P, static_cast<char*>(dev_scratch) + L::plan_layout(n_segments).total,
                              far_capacity, cus);
}

extern "C" int rdst_hip_debug_topk_segments_plan_device(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len, uint64_t k,
                                                        uint32_t elem_bytes, uint32_t index_bytes, uint32_t unbounded_stream, void* dev_scratch,
                                                        uint64_t scratch_bytes, rdst_segment_item* items_out, uint64_t capacity,
                                                        uint64_t class_counts_out[4], uint64_t* longest_far_out, uint32_t* flags_out, void* stream) {
    Cuts cuts;
    int rc = class_cuts(k, elem_bytes, index_bytes, unbounded_stream != 0, &cuts);
    if (rc) return rc;
    if (!class_counts_out || !longest_far_out || !flags_out) return set_error(RDST_ERR_ARG, "topk_segments_plan_device: null output");
    class_counts_out[0] = class_counts_out[1] = class_counts_out[2] = class_counts_out[3] = 0;
    *longest_far_out = 0;
    *flags_out = 0;
    if (n_segments == 0 || k == 0) return RDST_OK;
    if (len >= (1ull << 32)) return set_error(RDST_ERR_UNSUPPORTED, "topk: len must be below 2^32");
    if ((rc = rdst_internal::check_offsets_table(dev_offsets, offset_bytes, n_segments, len))) return rc;
    if ((rc = rdst_internal::rank_check_scratch("topk", dev_scratch))) return rc;
    if (scratch_bytes < L::plan_layout(n_segments).total)
        return set_error(RDST_ERR_ARG, "topk: scratch_bytes is below rdst_hip_topk_segments_device_offsets_scratch_bytes(n_segments, 0, ...)");
    const PlanScratch P = plan_scratch(dev_scratch, n_segments);
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> lock(rdst_internal::library_mutex());
    if ((rc = enqueue_plan(dev_offsets, offset_bytes, n_segments, len, cuts, P, 0u, nullptr, s))) return rc;
    PlanResult r;
    if ((rc = read_plan(P, &r, s))) return rc;
    for (int c = 0; c < 4; ++c) class_counts_out[c] = r.counts[c];
    *longest_far_out = r.longest_far;
    *flags_out = r.flags;
    const uint64_t total = r.counts[0] + r.counts[1] + r.counts[2] + r.counts[3];
    if (r.flags || total == 0) return RDST_OK;  // (an invalid table: the flags are the answer, the items mean nothing)
    if (total > capacity) return set_error(RDST_ERR_ARG, "topk_segments_plan_device: capacity too small for the work list");
    if (!items_out) return set_error(RDST_ERR_ARG, "topk_segments_plan_device: null item table");
    RDST_HIP_TRY(hipMemcpyAsync(items_out, P.items, (size_t)total * sizeof(rdst_segment_item), hipMemcpyDeviceToHost, s));
    RDST_HIP_TRY(hipStreamSynchronize(s));
    return RDST_OK;
}
