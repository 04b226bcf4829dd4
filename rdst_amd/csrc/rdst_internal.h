// rdst_internal.h — hooks between the library's translation units.  Not part of the C ABI (include/rdst_hip.h).
#ifndef RDST_INTERNAL_H
#define RDST_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <type_traits>

#include "rdst_hip.h"

namespace rdst_internal {

// Records `what` (and the HIP error, if any) for rdst_hip_last_error and returns `code`.
int set_error(int code, const char* what, hipError_t e = hipSuccess);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) acts on the CURRENT device's copy of the function: remembers
// (device, kernel) -> bytes.  Callers hold the library's mutex.
int ensure_lds_attr(const void* fn, size_t lds);

// Every kernel launch of the library: sets the dynamic-LDS attribute if the kernel has dynamic LDS, launches, and reports a
// refused launch through set_error, naming the kernel.  Does not wait for the device.
template <typename... P, typename... A>
int launch(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
    if (lds != 0)
        if (int rc = ensure_lds_attr(reinterpret_cast<const void*>(kernel), lds)) return rc;
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RDST_OK : set_error(RDST_ERR_HIP, name, e);
}

// Run-time booleans to compile-time ones: with_bools(f, a, b) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}), so a
// kernel's argument list is written once for all its variants.  Every combination of the booleans is instantiated: a variant
// that is built for some key widths only stays behind an `if constexpr` at the call site.
template <typename F>
int with_bools(F&& f) { return f(); }
template <typename F, typename... B>
int with_bools(F&& f, bool b, B... rest) {
    return b ? with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
             : with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// f(uint32_t{}) or f(uint64_t{}): a 4- or 8-byte key, value or index type picked at run time
template <typename F>
int by_uint(uint32_t bytes, F&& f) { return bytes == 4 ? f(uint32_t{}) : f(uint64_t{}); }

// A failed HIP call inside any function that returns a status: recorded with the expression's text, RDST_ERR_HIP returned.
#define RDST_HIP_TRY(expr)                                                                  \
    do {                                                                                    \
        hipError_t e__ = (expr);                                                            \
        if (e__ != hipSuccess) return ::rdst_internal::set_error(RDST_ERR_HIP, #expr, e__); \
    } while (0)

// The frame of every blocking host-slice entry point: switch to the device the caller named (enter), take a stream and
// device buffers (open + alloc: the job's own; or borrow: a device's cached ones), copy the slice up (upload), run the
// work, and finish: status, then download, then wait.  finish alone writes the caller's memory, and only after the device
// reported success.  On whatever path the entry returns, the work still queued on the stream has finished, what the job
// owns is given back, and the device the caller had selected is selected again.
struct HostJob {
    hipStream_t s = nullptr;
    int enter(const rdst_hip_opts* opts) {
        if (opts && opts->device >= 0) {
            RDST_HIP_TRY(hipGetDevice(&prev_dev));
            RDST_HIP_TRY(hipSetDevice(opts->device));
        }
        return RDST_OK;
    }
    int open() {
        RDST_HIP_TRY(hipStreamCreate(&s));
        own_stream = true;
        return RDST_OK;
    }
    hipError_t alloc(void** p, size_t bytes) {
        if (nbufs == 8) return hipErrorOutOfMemory;
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) bufs[nbufs++] = *p;
        return e;
    }
    // A stream that outlives the job, the lock that guards it and its buffers (held until the job ends), and four events
    // (or none) to record around the upload and around the download.
    void borrow(hipStream_t stream, std::unique_lock<std::mutex>&& guard, hipEvent_t* events) {
        s = stream;
        lock = std::move(guard);
        ev = events;
    }
    int upload(void* dev, const void* host, size_t bytes) {
        if (ev) (void)hipEventRecord(ev[0], s);
        RDST_HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s));
        if (ev) (void)hipEventRecord(ev[1], s);
        return RDST_OK;
    }
    // rdst_hip_device_status, for work that has to know before it goes on.  What it queues afterwards must not be able to
    // raise the error word: finish does not ask a second time.
    int status() {
        if (!status_ok) {
            if (int rc = rdst_hip_device_status(s)) return rc;
            status_ok = true;
        }
        return RDST_OK;
    }
    // `rc`: what the work returned.  `host` is written if and only if the work and the device both reported success.
    int finish(int rc, void* host, const void* dev, size_t bytes) {
        if (rc == RDST_OK) rc = status();
        if (rc != RDST_OK) return rc;
        if (ev) (void)hipEventRecord(ev[2], s);
        RDST_HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
        if (ev) (void)hipEventRecord(ev[3], s);
        RDST_HIP_TRY(hipStreamSynchronize(s));
        idle = true;
        return RDST_OK;
    }
    ~HostJob() {
        if (s && !idle) (void)hipStreamSynchronize(s);
        for (int i = 0; i < nbufs; ++i) (void)hipFree(bufs[i]);
        if (own_stream) (void)hipStreamDestroy(s);
        if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    }

private:
    int prev_dev = -1;
    void* bufs[8] = {};
    int nbufs = 0;
    bool own_stream = false, status_ok = false, idle = false;
    hipEvent_t* ev = nullptr;
    std::unique_lock<std::mutex> lock;  // released last, after the stream has been waited for
};

// The current device's sticky error word (kernels OR bits into it; rdst_hip_device_status reports and clears it).
// `cus_out`, if given: the device's compute-unit count.
int device_error_word(uint32_t** out, int* cus_out = nullptr);
// The current device's compute-unit count alone (takes the library's mutex itself).
int device_cus(int* cus_out);

// [u8; N] rows with N in 1..16, in place on `s`: widened to 4-, 8- or 16-byte integers in `scratch`, sorted by the integer
// route, narrowed back (the path rdst_hip_sort takes for these widths).  Asynchronous.
uint64_t widened_scratch_bytes(uint64_t len, uint32_t nb);
int sort_bytes_widened(void* dev_rows, uint64_t len, uint32_t nb, void* scratch, hipStream_t s);

// The same for host-only translation units (rdst_segments.cpp), which do not see HIP's types.
int note_error(int code, const char* what);

// ---- hooks for rdst_segments.hip, rdst_topk.hip and rdst_topk_segments.hip -------------------------------------------------------------------
// The library's mutex; every hook below this line is called with it held.
std::mutex& library_mutex();
// The argument checks shared by the device entry points (width, kind, levels, pointer, alignment, length); no lock needed.
int check_key_args(const void* p, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels);
// The xor masks of the order-preserving key map (applied when the sign bit is set / clear), in the low elem_bytes bytes.
void key_xor_masks(rdst_key_kind kind, uint32_t elem_bytes, unsigned __int128* neg, unsigned __int128* pos);
// One whole slice (pairs: one pair slice) by the route rdst_hip_sort_device (rdst_hip_sort_pairs_device) takes.
int sort_slice_locked(void* keys, void* tmp, uint64_t n, uint32_t elem_bytes, rdst_key_kind kind, hipStream_t s);
int sort_pairs_slice_locked(void* keys, void* vals, void* tmp_keys, void* tmp_vals, uint64_t n, uint32_t key_bytes, rdst_key_kind kind,
                            uint32_t val_bytes, hipStream_t s);
// sort_slice_locked for entries that promise NO WAIT AT ANY LENGTH: never the split of slices beyond the window, whose 256
// counts come to the host (the one wait rdst_hip_sort_device documents).  The pipeline alone: the routes the device decides
// on, the LSD route beyond the window.  Bit for bit the same result.
int sort_slice_nowait_locked(void* keys, void* tmp, uint64_t n, uint32_t elem_bytes, rdst_key_kind kind, hipStream_t s);
// The same with the length in device memory (rdst_hip_sort_device_devlen / rdst_hip_sort_pairs_device_devlen after their
// checks): `dev_len` is one unsigned integer of `len_bytes` (4 or 8) bytes, read on `s`; launches and workspace are sized
// for `capacity` (> 1).  The LSD route only; no copy to the host, no wait.
int sort_slice_devlen_locked(void* keys, void* tmp, uint64_t capacity, const void* dev_len, uint32_t len_bytes, uint32_t elem_bytes,
                             rdst_key_kind kind, hipStream_t s);
int sort_pairs_slice_devlen_locked(void* keys, void* vals, void* tmp_keys, void* tmp_vals, uint64_t capacity, const void* dev_len, uint32_t len_bytes,
                                   uint32_t key_bytes, rdst_key_kind kind, uint32_t val_bytes, hipStream_t s);
// Bytes of workspace such a slice asks for (an upper bound over its routes).
size_t slice_workspace_bytes(uint64_t n, uint32_t key_bytes, rdst_key_kind kind, uint32_t val_bytes);
// The current device's workspace, grown to `bytes` if need be and handed over to stream `s` (workspace_acquire); every
// slice sorted afterwards that asks for no more than `bytes` leaves it where it is.  workspace_handback records that `s`
// used it (workspace_release).
int workspace_take(size_t bytes, hipStream_t s, void** ws_out, int* device_out);
int workspace_handback(hipStream_t s);
// rdst_segments.hip: `count` work items to `dev_dst` on `s` through device `device`'s pinned staging buffer; waits (on the
// event) only while the previous list that went through it is still on its way.
int stage_segment_items(int device, const rdst_segment_item* items, size_t count, void* dev_dst, hipStream_t s);
// rdst_topk.hip: rdst_hip_topk_device after its checks, with the layout of rdst_hip_topk_scratch_bytes(len, k, elem_bytes,
// index_bytes, 0) in `scratch`; `cus`: the device's compute units.  No copy to the host, no wait.
int topk_slice_locked(const void* keys, uint64_t len, uint64_t k, void* out_keys, void* out_index, uint32_t index_bytes, void* scratch,
                      uint32_t elem_bytes, rdst_key_kind kind, bool largest, int cus, hipStream_t s);
// rdst_select.hip: rdst_hip_select_device after its checks, with the layout of rdst_hip_select_scratch_bytes(len, n_ranks,
// elem_bytes, index_bytes, cand_capacity) in `scratch`.  ranks[i] < len goes to slot slots[i] of the outputs (`slots` ==
// nullptr: to slot i).  `order`: order_ranks' answer for `ranks`, made before the mutex was taken.  No copy to the host, no wait.
int select_slice_locked(const void* keys, uint64_t len, const uint64_t* ranks, const uint64_t* slots, const uint64_t* order, uint64_t n_ranks,
                        void* out_keys, void* out_index, uint32_t index_bytes, void* scratch, uint64_t cand_capacity, uint32_t elem_bytes,
                        rdst_key_kind kind, bool largest, int cus, hipStream_t s);
// rdst_select.hip: the indices of `ranks` in ascending rank order, equal ranks in index order, into order_out[0 .. n_ranks).  No
// lock needed; RDST_ERR_ARG if the sort's host memory cannot be had.
int order_ranks(const uint64_t* ranks, uint64_t n_ranks, uint64_t* order_out);
// rdst_topk_segments.hip: the three batched launches of the segmented partial sort over an item table in device memory,
// for rdst_topk_segments_offsets.hip.  One call as the launches see it:
struct TopkSegmentsCall {
    const void* keys;
    uint64_t k;
    void *out_keys, *out_index;
    uint32_t index_bytes, elem_bytes;
    rdst_key_kind kind;
    bool largest;
    hipStream_t s;
};
// `hdr` == nullptr: counts[0 .. 2] are the wave, block and stream class's item counts and the classes follow one another in
// `items`.  With `hdr` (the plan header, rdst_segments_layout.h: TopkPlanHeader): the counted kernels, which read their item
// range from it; counts[0 .. 2] bound the counts, for the grids alone.  Ends the stages RDST_STAGE_SEGMENTS | (class << 8).
// No copy to the host, no wait.
int topk_segments_launch_locked(const TopkSegmentsCall& c, const rdst_segment_item* items, const uint32_t* hdr, const uint64_t counts[3]);
// rdst_topk_segments_offsets.hip: the plan of the segmented partial sort made on the device, for
// rdst_select_segments_offsets.hip (the select's plan is this one with k = 1).  Where it lies in the caller's scratch
// (rdst_segments_layout.h: plan_layout, TopkPlanHeader) and what the classes were cut by:
struct TopkSegmentsPlan {
    uint32_t* hdr;
    rdst_segment_item* items;
    uint64_t* far_lens;  // the unsaturated lengths of the far items, in their order
    uint32_t wave_max, block_max, stream_limit;
};
// Enqueues the plan for this k and these widths into `scratch` (rdst_hip_sort_segments_device_offsets_scratch_bytes(n_segments)
// bytes of it).  `unbounded_stream`: the classes of the asynchronous mode, whose stream class has no upper length.  `no_far`:
// a far segment raises TOPK_PLAN_FAR; with a flag up the counted kernels get zero counts and `err` (if given) the table bit.
// No copy to the host, no wait.
int topk_segments_plan_locked(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len, uint64_t k, uint32_t elem_bytes,
                              uint32_t index_bytes, bool unbounded_stream, void* scratch, bool no_far, uint32_t* err, hipStream_t s,
                              TopkSegmentsPlan* out);
// rdst_select_segments.hip: the batched launches of the segmented select over an item table in device memory, every round of
// c.n_ranks specs (`ranks`: host array), for both of its entries.  One call as the launches see it:
struct SelectSegmentsCall {
    const void* keys;
    uint64_t n_ranks;
    void *out_keys, *out_index;
    uint32_t index_bytes, elem_bytes;
    rdst_key_kind kind;
    bool largest;
    hipStream_t s;
};
// `hdr` and counts[0 .. 2] as for topk_segments_launch_locked.  No copy to the host, no wait.
int select_segments_launch_locked(const SelectSegmentsCall& c, const rdst_segment_item* items, const uint32_t* hdr, const uint64_t counts[3],
                                  const rdst_rank_spec* ranks);
// rdst_segments.hip: what every entry with a table of borders in device memory checks of it before any device work
// (n_segments, offset_bytes, the pointer and its alignment, 4-byte offsets against len); no lock needed.
int check_offsets_table(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len);
// Profiling (rdst_hip_set_profiling): open a run of its own / close the stage that ends here.  No-ops when profiling is off.
int profile_open_run(hipStream_t s);
int profile_stage_end(hipStream_t s, uint32_t stage);

// rdst_bytes.hip: a host slice of `len` rows of `row_bytes` bytes ordered by the byte string at (key_offset, key_bytes),
// equal keys in input order.  Blocking; the slice is written only after the device reported success.  Arguments are
// checked by the caller.
int sort_bytes_rows_host(void* host_rows, uint64_t len, uint32_t row_bytes, uint32_t key_offset, uint32_t key_bytes,
                         const rdst_hip_opts* opts);

}  // namespace rdst_internal

#endif  // RDST_INTERNAL_H
