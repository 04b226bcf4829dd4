/*
 * rdst_hip.h — C ABI of the MI355X (gfx950) radix-sort hot path that sits behind
 * rdst's RadixSort / RadixKey / Tuner surface.
 *
 * The reference crate (nessex/rdst) has no FFI of its own; every entry point below
 * names the reference interface it stands in for (paths relative to the reference
 * tree, file:line).  A Rust shim binds these with a plain `extern "C"` block
 * (INTEGRATION.md shows it); this repo's own host mirrors (include/rdst.hpp for
 * C++, rdst_amd/ for Python) call exactly the same symbols.
 *
 * Conventions
 *   - every function returns 0 (RDST_OK) or a negative rdst_status; on any non-zero
 *     return the caller's key buffer is unmodified for the host entry point
 *     (rdst_hip_sort), so a shim can fall back to the CPU path and still honour
 *     rdst's infallible `fn sort(self)` contract (src/radix_sort_builder.rs:149-157).
 *   - plain pointers and sizes only; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).
 *   - device pointers must be aligned to the element size; 16-byte alignment gets
 *     the wide-load kernels.
 *   - the library owns its device workspace (histograms, look-back status words,
 *     tickets): one per device, grown on demand, process lifetime, mutex-guarded.
 *     Concurrent calls on one device serialise on that mutex.
 */
#ifndef RDST_HIP_H
#define RDST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDST_HIP_ABI_VERSION 2

/* Which built-in RadixKey mapping the element type uses (src/radix_key_impl.rs). */
typedef enum {
    RDST_KEY_UNSIGNED = 0, /* u8..u64: (self >> level*8) as u8          radix_key_impl.rs:3-76   */
    RDST_KEY_SIGNED   = 1, /* i8..i64: ((self ^ MIN) >> level*8) as u8  radix_key_impl.rs:87-160 */
    RDST_KEY_FLOAT    = 2, /* f32/f64: sign-magnitude flip, then ^ MIN  radix_key_impl.rs:162-185 */
    RDST_KEY_BYTES_BE = 3  /* [u8; N]: self[N - 1 - level], i.e. lexicographic  radix_key_impl.rs:78-85;
                              N = elem_bytes = levels in 1..RDST_BYTES_MAX_N: rdst_hip_sort, rdst_hip_sort_records (a key
                              field) and the device entry rdst_hip_sort_bytes_device */
} rdst_key_kind;

typedef enum {
    RDST_OK              = 0,
    RDST_ERR_ARG         = -1, /* bad pointer / size / kind / levels (LEVELS == 0 panics in rdst: radix_sort_builder.rs:22) */
    RDST_ERR_UNSUPPORTED = -2, /* element width / kind not built for the device path (built: 1-, 2-, 4-, 8-, 16-byte integers, f32, f64, [u8; 1..RDST_BYTES_MAX_N] through rdst_hip_sort) */
    RDST_ERR_HIP         = -3, /* a HIP runtime call failed; see rdst_hip_last_error() */
    RDST_ERR_NO_DEVICE   = -4, /* no usable gfx950 device */
    RDST_ERR_DEVICE      = -5, /* a kernel reported failure through the workspace error word (bounded spin expired) */
    RDST_ERR_ALIGN       = -6  /* pointer not aligned to the element size */
} rdst_status;

/* src/tuner.rs:2-8.  parent_len: -1 encodes None. */
typedef struct {
    uint64_t threads;
    uint64_t level;
    uint64_t total_levels;
    uint64_t input_len;
    int64_t  parent_len;
} rdst_tuning_params;

/* src/tuner.rs:12-22, in declaration order, plus the two device routes a GPU-aware
 * tuner may return (they need a new arm in the `match` at src/sorter.rs:81-102). */
typedef enum {
    RDST_ALGO_MT_OOP = 0,
    RDST_ALGO_MT_LSB = 1,
    RDST_ALGO_SCANNING = 2,
    RDST_ALGO_RECOMBINATING = 3,
    RDST_ALGO_COMPARATIVE = 4,
    RDST_ALGO_LR_LSB = 5,
    RDST_ALGO_LSB = 6,
    RDST_ALGO_REGIONS = 7,
    RDST_ALGO_SKA = 8,
    RDST_ALGO_GPU_LSD = 9,      /* whole slice on one device: rdst_hip_sort / rdst_hip_sort_device */
    RDST_ALGO_GPU_SHARDED = 10  /* slice spread over ranks: MSD split + exchange + local LSD */
} rdst_algorithm;

/* Stock tuners (src/tuners/, one file each) + the device-aware one. */
typedef enum {
    RDST_TUNER_STANDARD = 0,        /* src/tuners/standard_tuner.rs:10-64 */
    RDST_TUNER_LOW_MEMORY = 1,      /* src/tuners/low_memory_tuner.rs:13-43 */
    RDST_TUNER_SINGLE_THREADED = 2, /* src/tuners/single_threaded_tuner.rs:13-43 */
    RDST_TUNER_GPU = 3              /* StandardTuner, except depth-0 chunks >= gpu_min_len go to GPU_LSD */
} rdst_tuner_id;

/* What ran between two profiling marks (rdst_hip_profile_run_stages); a scatter pass carries its
 * level in bits 8..15. */
typedef enum {
    RDST_STAGE_CLEAR = 1,    /* workspace clear */
    RDST_STAGE_HIST = 2,     /* K1: every level's histogram (returns at once on the hybrid route) */
    RDST_STAGE_SCAN = 3,     /* K2 */
    RDST_STAGE_PASS = 4,     /* K3, one level (skipped levels return at once) */
    RDST_STAGE_COPYBACK = 5,
    RDST_STAGE_HIST16 = 6,   /* K1h: counts of the top 16 bits (hybrid route) */
    RDST_STAGE_ROUTE = 7,    /* route decision + bucket starts */
    RDST_STAGE_LOCAL = 8,    /* K4: per-bucket sort of the remaining levels inside LDS (hybrid and atomic routes) */
    RDST_STAGE_MSD_A = 10,   /* atomic route: scatter by the top byte into over-provisioned areas (claims instead of counts) */
    RDST_STAGE_MSD_B = 11,   /* atomic route: scatter of every area by the second byte into the bucket slots (low halves) */
    RDST_STAGE_SAMPLE = 12,  /* the 8 192-key sample (and, if it flags the keys, K1h + the route decision) before the MSD passes */
    RDST_STAGE_SEGMENTS = 13, /* segmented sort: the item table's copy (host offsets) and the batched wave-class and block-class launches */
    RDST_STAGE_SEGMENTS_TILED = 14, /* segmented sort, nowait entries: the tiled route's launches for the segments beyond block_max */
    RDST_STAGE_TOPK = 15,    /* partial sort: one select level (counting read + bucket pick; its number in bits 8..15), or with
                                0xFF there the collection pass */
    RDST_STAGE_SELECT = 16   /* order statistics: one level of one round (counting read + pick; its number in bits 8..15), or with
                                0xFF there the round's collection pass */
} rdst_stage;

/* Device routes (rdst_hip_last_route). */
#define RDST_ROUTE_LSD 0u     /* one scatter pass per level */
#define RDST_ROUTE_HYBRID 1u  /* two scatter passes on the top 16 bits + one in-LDS sort per bucket */
#define RDST_ROUTE_ATOMIC 2u  /* the same without the counting read: MSD passes that claim space with atomics */

/* Options of the host entry point.  NULL = defaults. */
typedef struct {
    int32_t  device;       /* HIP device ordinal, -1 = current device */
    int32_t  low_memory;   /* != 0: the low-memory route (rdst_hip_sort_device_lowmem): the device holds the keys and a scratch of
                              len / 64 elements instead of two arrays — what `with_low_mem_tuner()` asks for
                              (src/radix_sort_builder.rs:74-77) */
    uint64_t reserved1;
} rdst_hip_opts;

/* ---- entry points ------------------------------------------------------------------ */

/* Replaces `RadixSort::radix_sort_unstable` for a host slice of a built-in key type
 * (src/radix_sort.rs:21-45 -> src/radix_sort_builder.rs:149-157 -> src/sorter.rs:106-119).
 * Sorts `len` elements of `elem_bytes` bytes in place, ascending in rdst's mapped-key
 * order.  Blocking.  len <= 1 is a no-op (radix_sort_builder.rs:151).  `levels` must
 * equal elem_bytes (RadixKey::LEVELS of every built-in type).  On failure the buffer
 * is untouched.  The library keeps one stream and one device buffer (keys + tmp, up to 1 GiB; larger ones
 * are released on return) per device for this entry point; concurrent calls on a device serialise. */
int rdst_hip_sort(void* host_data, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind,
                  uint32_t levels, const rdst_hip_opts* opts);

/* Where the time of the most recent rdst_hip_sort on the current device went (HIP events on its stream): the copy
 * to the device, the device sort (incl. its status check), the copy back.  10^9 u32 keys: 2 x 4 GB at the link's
 * ~51 GB/s and 6 ms of sorting; a sort needs its whole input before its first output, so the two copies cannot
 * overlap each other. */
int rdst_hip_host_timing(float* h2d_ms, float* sort_ms, float* d2h_ms);

/* Device-resident form of the same call — the timed path.  `dev_keys` holds the keys and
 * receives the sorted result; `dev_tmp` is a caller-provided scratch of the same size
 * (the `tmp_bucket` of src/sorts/lsb_sort.rs:53).  Asynchronous on `stream`.  The LSD
 * pass loop is the device twin of Sorter::lsb_sort_adapter (src/sorts/lsb_sort.rs:39-127)
 * with mt_lsb_sort's (bucket, tile) offset table (src/sorts/mt_lsb_sort.rs:40-133)
 * replaced by an on-device chained scan.  One exception to "asynchronous": 4- and 8-byte keys beyond the byte-saving routes'
 * window (more than ~1.04e9 8-byte keys, 1.3e9 4-byte keys) are split on their top byte and sorted part by part, as
 * Sorter recurses into a bucket too big for the sort at hand (src/sorter.rs:131-138); the 256 counts of that split come to
 * the host, so the call waits once for `stream` and enqueues the rest. */
int rdst_hip_sort_device(void* dev_keys, void* dev_tmp, uint64_t len, uint32_t elem_bytes,
                         rdst_key_kind kind, uint32_t levels, void* stream);

/* Replaces `radix_sort_unstable` on a host slice of structs whose `RadixKey` reads one built-in
 * field (benches/struct_sort.rs:11-27: `LargeStruct { sort_key: f32, .. }` with
 * `get_level` = the field's; examples/impl_radix_key.rs:32-56).  `record_bytes` = size_of::<T>(),
 * the key is `key_bytes` (4 or 8) at `key_offset`, naturally aligned; rows travel to the device,
 * (key, row index) pairs are sorted there, the rows gathered and copied back.  Rows with equal
 * keys keep their input order (rdst promises none).  Blocking; on failure the slice is untouched.
 * kind == RDST_KEY_BYTES_BE: the key is a [u8; N] field, key_bytes = N in 1..RDST_BYTES_MAX_N, at any
 * offset in rows of any size (no alignment rule), len < 2^32; ordered as rdst_hip_sort_bytes_device orders rows.
 * Keys of several fields, of other widths (u8, u16, i128), of chosen bytes or at unaligned offsets:
 * rdst_hip_sort_records_by_fields below. */
int rdst_hip_sort_records(void* host_records, uint64_t len, uint32_t record_bytes, uint32_t key_offset,
                          uint32_t key_bytes, rdst_key_kind kind, const rdst_hip_opts* opts);

/* Key-value sort, device-resident: sorts `dev_keys` (4- or 8-byte built-in keys) and carries
 * `dev_vals` (4- or 8-byte payloads, e.g. the index of the record a key came from) along.
 * the device route for slices of structs whose `RadixKey` is a built-in key
 * field (benches/struct_sort.rs:11-27, examples/impl_radix_key.rs:32-56) — extract
 * (key, index), sort the pairs here, gather the records.  The passes are stable, so pairs with
 * equal keys keep their input order; rdst itself promises no order among them
 * (src/radix_sort.rs:21-45 "unstable"), so this is one of the outputs rdst may produce.
 * Both tmp arrays have the size of their originals; asynchronous on `stream` like
 * rdst_hip_sort_device, failures are reported by rdst_hip_device_status. */
int rdst_hip_sort_pairs_device(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals,
                               uint64_t len, uint32_t key_bytes, rdst_key_kind kind, uint32_t levels,
                               uint32_t val_bytes, void* stream);

/* The same two sorts over a prefix whose LENGTH LIVES IN DEVICE MEMORY: the count a compaction, a filter or a join left
 * there, sorted without the host ever learning it.  `dev_len` points to one unsigned integer of `len_bytes` (4 or 8) bytes
 * in device memory, aligned to its size; call its value m.  It is read only, and read IN STREAM ORDER: the kernel that
 * writes it may still be running when the call returns.  The host never reads it.
 *   - The first m elements end up bit for bit as rdst_hip_sort_device / rdst_hip_sort_pairs_device would leave a slice of
 *     len = m; pairs with equal keys keep their input order.  Elements [m, capacity) of keys and values are not written.
 *     Of the tmp arrays (both hold `capacity` elements) only [0, m) may be written, their content afterwards is
 *     unspecified.  Nothing outside [0, capacity) of any array is touched.  m <= 1 changes nothing.
 *   - m > capacity: no key, value or tmp element is modified, bit 32 (0x20) of the device error word is set and
 *     rdst_hip_device_status returns RDST_ERR_DEVICE once.
 *   - Key widths, kinds, `levels`, alignment rules, argument errors and their order: those of the known-length twins, with
 *     `capacity` in the place of `len`.  Then, still before any device work: NULL dev_len -> RDST_ERR_ARG, len_bytes not 4
 *     or 8 -> RDST_ERR_ARG, misaligned dev_len -> RDST_ERR_ALIGN.  capacity <= 1 is RDST_OK and does nothing; dev_len is
 *     not looked at.
 *   - ASYNCHRONOUS on `stream` for every capacity: no copy to the host, no stream or event wait (the one exception every
 *     entry shares: a library workspace that has to grow).
 *   - The LSD route only (rdst_hip_last_route reports it): the byte-saving routes and the split beyond the window size their
 *     launches from the length on the host, and the split reads counts back.  A keys-only sort of 4- or 8-byte keys
 *     therefore runs at the LSD rate, not at rdst_hip_sort_device's; key-value sorts take this route in either form.
 *     Every launch is sized for `capacity` and returns early past m, so a short prefix of a large capacity still pays
 *     for the capacity's launches (DESIGN.md §2g has the measured floor).  Level skipping and the whole-slice
 *     already-sorted exit work as in the twins, decided by the first m elements only. */
int rdst_hip_sort_device_devlen(void* dev_keys, void* dev_tmp, uint64_t capacity,
                                const void* dev_len, uint32_t len_bytes,
                                uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, void* stream);
int rdst_hip_sort_pairs_device_devlen(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals,
                                      uint64_t capacity, const void* dev_len, uint32_t len_bytes,
                                      uint32_t key_bytes, rdst_key_kind kind, uint32_t levels,
                                      uint32_t val_bytes, void* stream);

/* ---- partial sort: the k smallest or largest keys, in order ---------------------------------------
 * What `select_nth_unstable` + a sort of the front, or torch.topk, give: the front of the order without sorting the array,
 * copying it or handing over a tmp of its size.  Call M the mapped key of the sort (the order-preserving map of
 * src/radix_key_impl.rs); with RDST_TOPK_LARGEST in `flags`, M is its bitwise complement.
 *   - dev_out_keys[0..k) receives the k keys of dev_keys[0..len) that come first in ascending M, in that order, as their
 *     original bits: without the flag bit for bit the first k elements rdst_hip_sort_device would leave, with it the last k,
 *     reversed.  -0.0 / +0.0 and NaN payloads are distinct keys, as in the sort.
 *   - dev_out_index: NULL for keys only; otherwise it receives k integers of index_bytes (4 or 8) bytes, the input position
 *     of each output key.  Elements with equal keys appear in ascending position, and among the elements tied with the k-th
 *     key the lowest positions are taken: keys and indices are the first k of a STABLE argsort by M (with the flag: by the
 *     complemented M, not a reversed ascending argsort).  Deterministic, bit for bit.  Built for 4- and 8-byte keys, as the
 *     pair sorts are; other widths with an index: RDST_ERR_UNSUPPORTED.  With a NULL dev_out_index, index_bytes is not looked
 *     at: the call is keys only, and its scratch need is rdst_hip_topk_scratch_bytes(..., index_bytes = 0, ...).
 *   - The input is never written.  Of the outputs only [0, k) is written, of the scratch only
 *     [0, rdst_hip_topk_scratch_bytes(len, k, elem_bytes, index_bytes, cand_capacity)); the scratch needs no clearing between
 *     calls, and stream order makes it reusable by the next call on the same stream.
 *   - Keys only: every width and kind of rdst_hip_sort_device (1, 2, 4, 8, 16 bytes; unsigned, signed, f32 / f64).
 *     RDST_KEY_BYTES_BE: RDST_ERR_UNSUPPORTED.
 *   - ASYNCHRONOUS on `stream` for every input: no copy to the host, no stream or event wait (the one exception every entry
 *     shares: a library workspace that has to grow).  Every launch is enqueued unconditionally and sized from len, k and
 *     cand_capacity on the host; there is no data-dependent failure and no error bit: all keys equal, a sorted input, one
 *     heavy bucket are answered exactly.  This holds for every k up to len: the k selected elements are ordered by the sort's
 *     pipeline without the split that rdst_hip_sort_device makes (and waits for) beyond ~10^9 keys; so large a k takes the LSD
 *     route.
 *   - The mechanism is a radix select: per level one counting read of the input over the keys that still
 *     share the k-th key's prefix, digit_bits at a time (rdst_hip_topk_limits), until the keys on the prefix number at most
 *     cand_capacity; then one more read collects the keys before the prefix (fewer than k) and those on it, and only these
 *     are sorted.  With an index the levels go on over the position's digits, so ties beyond cand_capacity cost further
 *     levels, never correctness.  cand_capacity: 0 = the library's default; any value >= 1 is legal and gives the same
 *     result.  It is the most candidates the collection pass may write and the capacity their sort's launches are sized for.
 *   - Arguments, checked in this order before any device work: the key arguments as rdst_hip_sort_device checks them
 *     (its codes and messages; BYTES_BE -> RDST_ERR_UNSUPPORTED); len >= 2^32 -> RDST_ERR_UNSUPPORTED; k > len ->
 *     RDST_ERR_ARG; unknown flag bits -> RDST_ERR_ARG; k == 0 -> RDST_OK, nothing else is looked at; NULL dev_out_keys ->
 *     RDST_ERR_ARG; dev_out_keys misaligned to the element -> RDST_ERR_ALIGN; with an index: index_bytes not 4 or 8 ->
 *     RDST_ERR_ARG, key width not 4 or 8 -> RDST_ERR_UNSUPPORTED, misaligned index pointer -> RDST_ERR_ALIGN; NULL scratch
 *     -> RDST_ERR_ARG; scratch not 256-byte aligned -> RDST_ERR_ALIGN; scratch_bytes below rdst_hip_topk_scratch_bytes(...)
 *     -> RDST_ERR_ARG. */
#define RDST_TOPK_LARGEST 1u
int rdst_hip_topk_device(const void* dev_keys, uint64_t len, uint64_t k,
                         void* dev_out_keys, void* dev_out_index, uint32_t index_bytes,
                         void* dev_scratch, uint64_t scratch_bytes, uint64_t cand_capacity,
                         uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                         uint32_t flags, void* stream);
/* The scratch of the call above.  Pure, monotone in k and in cand_capacity: a 256-byte header, 4 096 counters, two arrays of
 * min(k, len) elements and two of min(cand_capacity or the default, len) elements, each rounded up to 256 bytes; an element
 * is a key, or with an index a (key, position) composite of twice the key's width.  0 for unsupported widths. */
uint64_t rdst_hip_topk_scratch_bytes(uint64_t len, uint64_t k, uint32_t elem_bytes,
                                     uint32_t index_bytes, uint64_t cand_capacity);
/* out = { digit_bits, the default cand_capacity, the most levels a call can take } for this key width (index_bytes 0 = keys
 * only).  Pure.  Unsupported widths: RDST_ERR_UNSUPPORTED. */
int rdst_hip_topk_limits(uint32_t elem_bytes, uint32_t index_bytes, uint32_t out[3]);
/* Test hook, BLOCKING, like rdst_hip_debug_last_sample: what the most recent rdst_hip_topk_device on this scratch decided.
 * out = { levels the device used, keys strictly before the threshold prefix, candidates collected, 1 if the keys-only fill
 * (digits exhausted with more than cand_capacity keys tied) or a position digit was reached }. */
int rdst_hip_debug_topk_state(const void* dev_scratch, void* stream, uint64_t out[4]);

/* ---- order statistics: the keys at given ranks, unsorted -----------------------------------------
 * What `select_nth_unstable`, numpy.partition or torch.kthvalue give — a median, deciles, a p99, a cut-off for pruning — for
 * several ranks at once, without sorting the array, copying it or handing over a tmp of its size.  Call M the mapped key of
 * the sort; with RDST_TOPK_LARGEST in `flags` (the partial sort's flag) M is its bitwise complement, exactly as there.
 *   - ranks: a HOST array of n_ranks ranks, each below len, in any order, repeats allowed.  dev_out_keys[i] is, bit for bit,
 *     the element rdst_hip_sort_device would leave at position ranks[i]; with the flag the element at len - 1 - ranks[i].
 *     Each result goes to its own slot i.  -0.0 / +0.0 and NaN payloads are distinct keys, as in the sort.
 *   - dev_out_index: NULL for keys only.  Otherwise (4- and 8-byte keys, index_bytes 4 or 8) slot i receives the input
 *     position of element ranks[i] of a STABLE argsort by M: equal keys count in ascending position.  With a NULL
 *     dev_out_index, index_bytes is not looked at.  Deterministic, bit for bit.
 *   - Keys only: every width and kind of rdst_hip_topk_device (1, 2, 4, 8, 16 bytes; unsigned, signed, f32 / f64).
 *     RDST_KEY_BYTES_BE: RDST_ERR_UNSUPPORTED.
 *   - The input is never written.  Of the outputs only the slots [0, n_ranks) are written, of the scratch only
 *     [0, rdst_hip_select_scratch_bytes(len, n_ranks, elem_bytes, index_bytes, cand_capacity)).  The scratch needs no
 *     clearing and is reusable in stream order.  It is never len-sized: a header, a group table, counters and two candidate
 *     arrays of min(cand_capacity or the default, len) elements.
 *   - ASYNCHRONOUS on `stream` for every input: no copy to or from the host, no stream or event wait, no staging buffer (the
 *     one exception every entry shares: a library workspace that has to grow).  The ranks travel as kernel arguments: `ranks`
 *     may be reused as soon as the call returns.  Every launch is enqueued unconditionally and sized from len, n_ranks and
 *     cand_capacity on the host; there is no data-dependent failure and no error bit: all keys equal, a sorted input, one
 *     heavy bucket are answered exactly.
 *   - The mechanism is a multi-rank radix select.  Up to max_ranks ranks (rdst_hip_select_limits) are followed
 *     IN THE SAME READS of the input: level 0 counts the first digit of every key, a later level the next digit of every key
 *     that lies on the prefix of some rank (a "group": prefix, count before it, count on it), until the groups together hold
 *     at most cand_capacity elements; then one more read collects the elements on the groups' prefixes, one sort orders
 *     them, and each rank picks its element.  What lies before a prefix is only counted, never kept.  When the digits are
 *     exhausted first — with an index the key's digits and then the position's — every answer is its group's prefix itself
 *     and nothing is collected.  A longer list is served in rounds of max_ranks ranks, taken in ascending rank order so that
 *     neighbours share prefixes; every round has its own reads, all rounds use the same scratch.
 *   - cand_capacity: 0 = the library's default; any value >= 1 is legal and gives the same result.
 *   - n_ranks has no upper limit, but the host orders the ranks before the first launch: O(n_ranks log n_ranks) time and 16
 *     bytes of host memory per rank (std::stable_sort), and one round of reads per max_ranks ranks.  If that memory cannot be
 *     had, the call returns RDST_ERR_ARG after the argument checks and before any device work; nothing is thrown.
 *   - Arguments, checked in this order before any device work: (1) the key arguments as rdst_hip_sort_device checks them (its
 *     codes and messages); (2) BYTES_BE -> RDST_ERR_UNSUPPORTED; (3) len >= 2^32 -> RDST_ERR_UNSUPPORTED; (4) unknown flag
 *     bits -> RDST_ERR_ARG; (5) n_ranks == 0 -> RDST_OK, nothing else is looked at; (6) NULL ranks -> RDST_ERR_ARG; (7) any
 *     ranks[i] >= len -> RDST_ERR_ARG, the message names the first such i; (8) NULL dev_out_keys -> RDST_ERR_ARG, misaligned
 *     to the element -> RDST_ERR_ALIGN; (9) with an index: index_bytes not 4 or 8 -> RDST_ERR_ARG, key width not 4 or 8 ->
 *     RDST_ERR_UNSUPPORTED, misaligned index pointer -> RDST_ERR_ALIGN; (10) NULL scratch -> RDST_ERR_ARG; (11) scratch not
 *     256-byte aligned -> RDST_ERR_ALIGN; (12) scratch_bytes below rdst_hip_select_scratch_bytes(...) -> RDST_ERR_ARG. */
int rdst_hip_select_device(const void* dev_keys, uint64_t len,
                           const uint64_t* ranks, uint64_t n_ranks,
                           void* dev_out_keys, void* dev_out_index, uint32_t index_bytes,
                           void* dev_scratch, uint64_t scratch_bytes, uint64_t cand_capacity,
                           uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                           uint32_t flags, void* stream);
/* The scratch of the call above, sized for one round whatever n_ranks is.  Pure, monotone in cand_capacity: a 256-byte
 * header, the group table (2 304 bytes), 16 384 counters and two arrays of min(cand_capacity or the default, len) elements,
 * each rounded up to 256 bytes; an element is a key, or with an index a (key, position) composite of twice the key's width.
 * 0 for unsupported widths. */
uint64_t rdst_hip_select_scratch_bytes(uint64_t len, uint64_t n_ranks, uint32_t elem_bytes,
                                       uint32_t index_bytes, uint64_t cand_capacity);
/* out = { max_ranks, bits of the first digit, bits of the later digits, the default cand_capacity (sized for max_ranks ranks),
 * the most levels one round can take } for this key width (index_bytes 0 = keys only).  Pure.  Unsupported widths:
 * rdst_hip_topk_limits' codes. */
int rdst_hip_select_limits(uint32_t elem_bytes, uint32_t index_bytes, uint32_t out[5]);
/* Test hook, BLOCKING: what the most recent round of rdst_hip_select_device on this scratch decided.  out = { levels the
 * round used, groups at the end, candidates collected, 1 if the digits were exhausted }. */
int rdst_hip_debug_select_state(const void* dev_scratch, void* stream, uint64_t out[4]);

/* ---- many independent slices in one call ---------------------------------------------------------
 * The reference sorts the 256 buckets of a chunk as slices of their own, in parallel (src/sorter.rs:131-138), and a
 * caller may do the same with `chunks_mut(..).par_for_each(|c| c.radix_sort_unstable())`.  The device form: one array
 * and a table of segment borders.
 *
 * Sorts every segment [offsets[s], offsets[s+1]) of dev_keys on its own; s in [0, n_segments).  offsets: HOST array of
 * n_segments + 1 non-decreasing element indices, offsets[n_segments] <= len; n_segments < 2^32.  Keys before offsets[0]
 * and from offsets[n_segments] on are not touched.  Every segment ends in the order rdst_hip_sort_device would give that
 * slice on its own, bit for bit; pairs with equal keys keep their input order, as rdst_hip_sort_pairs_device keeps them.
 * Key widths, kinds and `levels`: those of rdst_hip_sort_device (pairs: of rdst_hip_sort_pairs_device), with the same
 * error codes; n_segments == 0 is RDST_OK and does nothing.
 *
 * Segments are served by length (rdst_hip_sort_segments_limits gives the borders; length 0 and 1: nothing to do):
 *   2 .. wave_max            one wave per segment, keys in registers, four segments per workgroup — one launch for all;
 *   wave_max+1 .. block_max  one workgroup per segment (the one-workgroup LDS sort, with a value array for pairs),
 *                            longest first — one launch for all;
 *   longer                   the whole-slice route, one segment after another on `stream`, with dev_tmp (pairs:
 *                            dev_tmp_keys, dev_tmp_vals) as scratch: tmp_elems must be at least the longest such segment
 *                            (rdst_segments_plan's *tmp_elems_out).  With no segment over block_max, tmp_elems may be 0
 *                            and the tmp pointers NULL; otherwise RDST_ERR_ARG before any device work.
 * Segment starts need the alignment of the element only.
 *
 * `offsets` is read before the call returns: the caller may free or change it at once.  The work list travels through a
 * pinned staging buffer the library keeps per device: a call WAITS (on an event, not on the stream) only while the list
 * of the previous segmented call on that device has not reached the device yet.  Apart from that, and from what
 * rdst_hip_sort_device documents for slices beyond the window (long segments take that route), the call is asynchronous
 * on `stream`; kernel failures surface in rdst_hip_device_status. */
int rdst_hip_sort_segments_device(void* dev_keys, void* dev_tmp, uint64_t tmp_elems, uint64_t len,
                                  const uint64_t* offsets, uint64_t n_segments,
                                  uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels, void* stream);
int rdst_hip_sort_segments_pairs_device(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals,
                                        uint64_t tmp_elems, uint64_t len, const uint64_t* offsets, uint64_t n_segments,
                                        uint32_t key_bytes, rdst_key_kind kind, uint32_t levels, uint32_t val_bytes, void* stream);
/* out = { wave_max, block_max }: longest segment of the wave class and of the block class, for this key and value width
 * (val_bytes 0 = keys only).  Pure.  Unsupported widths: RDST_ERR_UNSUPPORTED. */
int rdst_hip_sort_segments_limits(uint32_t elem_bytes, uint32_t val_bytes, uint32_t out[2]);
/* Host only, like rdst_regions_plan: the work list the entry runs.  One item per segment of at least two keys: wave
 * class first, in segment order; then block class, longest first, ties in segment order; then long class, in segment
 * order (a long item's `len` saturates at 2^32 - 1: its length is offsets[seg + 1] - offsets[seg]).  class_counts_out:
 * the three counts; *tmp_elems_out: the longest long segment, or 0.  A `capacity` below their sum: RDST_ERR_ARG, with the
 * counts and *tmp_elems_out still written.  Decreasing offsets, a last offset past `len`, NULL offsets with
 * n_segments > 0: RDST_ERR_ARG. */
typedef struct { uint64_t start; uint32_t len; uint32_t seg; } rdst_segment_item;
int rdst_segments_plan(const uint64_t* offsets, uint64_t n_segments, uint64_t len, uint32_t elem_bytes, uint32_t val_bytes,
                       rdst_segment_item* items_out, uint64_t capacity, uint64_t class_counts_out[3],
                       uint64_t* tmp_elems_out);

/* ---- partial sort of every segment in one call ------------------------------------------------------
 * The k first keys of every row of a score matrix, of every query's distances, of every CSR row: rdst_hip_topk_device per
 * segment, in one call.  offsets: HOST table of n_segments + 1 non-decreasing element indices as
 * rdst_hip_sort_segments_device takes it (offsets[n_segments] <= len, n_segments < 2^32), read before the call returns;
 * len < 2^32; segment starts need the element's alignment only.
 *   - Row s of the outputs is dev_out_keys + s * k and dev_out_index + s * k (elements).  With n_s = offsets[s+1] -
 *     offsets[s] and k_s = min(k, n_s), its first k_s slots hold, bit for bit, what rdst_hip_topk_device writes for the slice
 *     dev_keys + offsets[s] of length n_s with k_s and the same kind, flags and index width: ascending mapped key (with
 *     RDST_TOPK_LARGEST: ascending complemented mapped key), positions local to the segment, equal keys in ascending
 *     position, the lowest positions winning a tie at the k-th key, -0.0 / +0.0 and NaN payloads distinct.
 *   - Slots k_s .. k of a row are NOT written (the caller knows the lengths), empty segments write nothing, the input is
 *     never written.  Of the scratch only [0, rdst_hip_topk_segments_scratch_bytes(n_segments, longest segment, k, elem_bytes,
 *     index_bytes)) is written; it needs no clearing, and stream order makes it reusable by the next call.
 *   - Keys only: every width and kind of rdst_hip_topk_device; with an index (4 or 8 bytes): 4- and 8-byte keys.  With a NULL
 *     dev_out_index, index_bytes is not looked at.  RDST_KEY_BYTES_BE: RDST_ERR_UNSUPPORTED.
 *   - There is no limit on k and no data-dependent failure.  Segments are served by length and k
 *     (rdst_hip_topk_segments_limits; bm = block_max for this key width and a 4-byte position beside the key):
 *       1 .. wave_max                       one wave per segment, four segments per workgroup — one launch for all;
 *       .. bm                               one workgroup per segment, longest first — one launch for all;
 *       .. stream_max, and k <= k_stream_max (= bm)
 *                                           one workgroup per segment, longest first — one launch for all: a radix select
 *                                           streamed from global memory, then the workgroup's LDS sort of at most bm keys;
 *       everything else ("far": longer than stream_max, or longer than bm with k > bm)
 *                                           rdst_hip_topk_device's own route, one segment after another on `stream`.
 *   - ASYNCHRONOUS as rdst_hip_sort_segments_device is: the work list travels through the pinned staging buffer the library
 *     keeps per device, and a call WAITS (on an event, not on the stream) only while the list of the previous segmented call
 *     on that device has not reached the device yet.  There is no other copy to the host and no other wait at any k and any
 *     segment length: the far class runs on the hooks rdst_hip_topk_device runs on, which never wait (the one exception every
 *     entry shares: a library workspace that has to grow).  Kernel failures surface in rdst_hip_device_status.
 *   - Profiling: the three batched launches end stages RDST_STAGE_SEGMENTS | (class << 8), class 0 = wave, 1 = block, 2 =
 *     stream; far segments report rdst_hip_topk_device's stages.
 *   - Arguments, checked in this order before any device work: the key arguments as rdst_hip_topk_device checks them (its
 *     codes and messages; BYTES_BE -> RDST_ERR_UNSUPPORTED); len >= 2^32 -> RDST_ERR_UNSUPPORTED; unknown flag bits ->
 *     RDST_ERR_ARG; k == 0 or n_segments == 0 -> RDST_OK, nothing else is looked at; the table: NULL offsets, n_segments >=
 *     2^32, decreasing offsets, a last offset past len -> RDST_ERR_ARG; NULL dev_out_keys -> RDST_ERR_ARG; dev_out_keys
 *     misaligned to the element -> RDST_ERR_ALIGN; with an index: index_bytes not 4 or 8 -> RDST_ERR_ARG, key width not 4 or 8
 *     -> RDST_ERR_UNSUPPORTED, misaligned index pointer -> RDST_ERR_ALIGN; NULL scratch -> RDST_ERR_ARG; scratch not 256-byte
 *     aligned -> RDST_ERR_ALIGN; scratch_bytes below rdst_hip_topk_segments_scratch_bytes(...) for the table's longest segment
 *     -> RDST_ERR_ARG. */
int rdst_hip_topk_segments_device(const void* dev_keys, uint64_t len,
                                  const uint64_t* offsets, uint64_t n_segments, uint64_t k,
                                  void* dev_out_keys, void* dev_out_index, uint32_t index_bytes,
                                  void* dev_scratch, uint64_t scratch_bytes,
                                  uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                  uint32_t flags, void* stream);
/* The scratch of the call above.  Pure, monotone in every argument: the item table, 16 bytes per segment rounded up to 256,
 * and — if a segment of `longest_segment` keys would be of the far class for this k — behind it
 * rdst_hip_topk_scratch_bytes(longest_segment, min(k, longest_segment), elem_bytes, index_bytes, 0).  It moves with
 * rdst_hip_set_topk_segments_stream_max.  0 for no segment, 2^32 segments or keys and more, and unsupported widths. */
uint64_t rdst_hip_topk_segments_scratch_bytes(uint64_t n_segments, uint64_t longest_segment, uint64_t k,
                                              uint32_t elem_bytes, uint32_t index_bytes);
/* out = { wave_max, block_max, stream_max, k_stream_max } for this key width (index_bytes 0 = keys only).  Pure but for the
 * setter below.  Unsupported widths: rdst_hip_topk_limits' codes. */
int rdst_hip_topk_segments_limits(uint32_t elem_bytes, uint32_t index_bytes, uint32_t out[4]);
/* Host only, like rdst_segments_plan: the work list the entry runs.  One item per segment of at least ONE key: wave class
 * first, in segment order; then block class, longest first, ties in segment order; then stream class, the same; then far
 * class, in segment order.  class_counts_out: the four counts; *longest_far_out: the longest far segment, or 0.  A
 * `capacity` below their sum: RDST_ERR_ARG, with the counts and *longest_far_out still written.  k == 0: no items.  The
 * table's errors are rdst_segments_plan's. */
int rdst_topk_segments_plan(const uint64_t* offsets, uint64_t n_segments, uint64_t len, uint64_t k,
                            uint32_t elem_bytes, uint32_t index_bytes,
                            rdst_segment_item* items_out, uint64_t capacity,
                            uint64_t class_counts_out[4], uint64_t* longest_far_out);
/* Test hook, like rdst_hip_set_small_sort: the longest segment of the stream class; 0 = the default (2^17 keys).  A value
 * below block_max leaves the stream class empty. */
int rdst_hip_set_topk_segments_stream_max(uint32_t stream_max);

/* ---- order statistics of every segment in one call ---------------------------------------------------
 * The median of every row, the deciles of every CSR row: rdst_hip_select_device per segment, in one call.  Segments differ
 * in length, so a rank is given as a SPEC that every segment resolves against its own length n_s:
 *   den == 0: the absolute rank `num`; a segment with n_s <= num has no such element: its slot is NOT written.
 *   den  > 0: the quantile num / den (num <= den): the virtual index (n_s - 1) * num / den as an exact rational, rounded by
 *             `mode` as numpy.quantile's methods "lower", "higher" and "nearest" (half to even) round it.  Always a rank
 *             below n_s.  64-bit integer arithmetic only, no floating point: both factors are below 2^32. */
#define RDST_RANK_LOWER   0u   /* floor of the virtual index (numpy method="lower")   */
#define RDST_RANK_HIGHER  1u   /* ceil                                   ("higher")   */
#define RDST_RANK_NEAREST 2u   /* round half to even                     ("nearest")  */
typedef struct { uint32_t num, den, mode, reserved; } rdst_rank_spec;
/* Host only, pure: the rank `spec` stands for in a segment of n keys.  1 = *rank_out is that rank (below n); 0 = none
 * (n == 0, or an absolute rank >= n; *rank_out is not written); RDST_ERR_ARG = a bad spec (den > 0 && num > den; mode > 2;
 * reserved != 0; mode != 0 with den == 0), a NULL argument, or a quantile of n > 2^32 keys. */
int rdst_rank_for_length(const rdst_rank_spec* spec, uint64_t n, uint64_t* rank_out);
/* offsets: HOST table of n_segments + 1 non-decreasing element indices exactly as rdst_hip_topk_segments_device takes it,
 * read before the call returns; ranks: HOST array of n_ranks specs, repeats allowed, any order, read before the call returns
 * too; len < 2^32; segment starts need the element's alignment only.
 *   - Row s of the outputs is dev_out_keys + s * n_ranks and dev_out_index + s * n_ranks (elements).  Slot i of row s holds,
 *     bit for bit, what rdst_hip_select_device returns for the slice dev_keys + offsets[s] of length n_s at the rank
 *     rdst_rank_for_length(&ranks[i], n_s), with the same kind, flags and index width: positions are local to the segment,
 *     equal keys count in ascending position, -0.0 / +0.0 and NaN payloads are distinct keys; with RDST_TOPK_LARGEST the
 *     order is that of the complemented mapped key, as in the select.
 *   - Slots without a rank — every slot of an empty segment, an absolute rank at or past the segment's length — are NOT
 *     written, the input is never written.  Of the scratch only [0, rdst_hip_select_segments_scratch_bytes(n_segments,
 *     longest segment, n_ranks, elem_bytes, index_bytes)) is written; it needs no clearing, and stream order makes it
 *     reusable by the next call.
 *   - Keys only: every width and kind of rdst_hip_select_device (1, 2, 4, 8, 16 bytes); with an index (4 or 8 bytes): 4- and
 *     8-byte keys.  With a NULL dev_out_index, index_bytes is not looked at.  RDST_KEY_BYTES_BE: RDST_ERR_UNSUPPORTED.
 *   - There is no limit on n_ranks and no data-dependent failure.  The work list is rdst_topk_segments_plan's with k = 1, so
 *     the class of a segment follows from its length alone (rdst_hip_select_segments_limits; bm = block_max for this key
 *     width, with a 4-byte position beside the key only when an index is asked for):
 *       1 .. wave_max     one wave per segment, four segments per workgroup: the segment is ordered in registers and LDS
 *                         and the thread that holds a rank stores it;
 *       .. bm             one workgroup per segment, longest first: the same with the workgroup's level loop;
 *       .. stream_max     one workgroup per segment, longest first: the specs are resolved and served in ascending rank
 *                         order; a rank outside what the LDS stage holds runs a radix select on the mapped key from the
 *                         root, streamed from global memory, until at most bm keys lie on its prefix (keys before the
 *                         prefix are only counted), one more read collects those, the level loop orders them, and every
 *                         rank inside them is answered without another read;
 *       longer ("far")    rdst_hip_select_device's own route, one segment after another on `stream`, with the ranks the
 *                         host resolved.
 *     The specs travel as kernel arguments, max_ranks per round; a longer list is served in rounds over the same items,
 *     slot i keeping its place in the row.  stream_max is the border rdst_hip_set_topk_segments_stream_max moves.
 *   - ASYNCHRONOUS exactly as rdst_hip_topk_segments_device is: the work list travels through the pinned staging buffer the
 *     library keeps per device, and the one possible wait is on that buffer's event.  Kernel failures surface in
 *     rdst_hip_device_status.
 *   - Arguments, checked in this order before any device work: the key arguments as rdst_hip_topk_segments_device checks
 *     them (the sort's codes and messages; BYTES_BE -> RDST_ERR_UNSUPPORTED); len >= 2^32 -> RDST_ERR_UNSUPPORTED; unknown
 *     flag bits -> RDST_ERR_ARG; n_ranks == 0 or n_segments == 0 -> RDST_OK, nothing else is looked at; the table: NULL
 *     offsets, n_segments >= 2^32, decreasing offsets, a last offset past len -> RDST_ERR_ARG; NULL ranks, a bad spec ->
 *     RDST_ERR_ARG, the message names the first bad i; NULL dev_out_keys -> RDST_ERR_ARG, misaligned to the element ->
 *     RDST_ERR_ALIGN; with an index: index_bytes not 4 or 8 -> RDST_ERR_ARG, key width not 4 or 8 -> RDST_ERR_UNSUPPORTED,
 *     misaligned index pointer -> RDST_ERR_ALIGN; NULL scratch -> RDST_ERR_ARG; scratch not 256-byte aligned ->
 *     RDST_ERR_ALIGN; scratch_bytes below rdst_hip_select_segments_scratch_bytes(...) for the table's longest segment ->
 *     RDST_ERR_ARG. */
int rdst_hip_select_segments_device(const void* dev_keys, uint64_t len,
                                    const uint64_t* offsets, uint64_t n_segments,
                                    const rdst_rank_spec* ranks, uint64_t n_ranks,
                                    void* dev_out_keys, void* dev_out_index, uint32_t index_bytes,
                                    void* dev_scratch, uint64_t scratch_bytes,
                                    uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                    uint32_t flags, void* stream);
/* The scratch of the call above.  Pure but for the border's setter, monotone in every argument: the item table, 16 bytes per
 * segment rounded up to 256, and — if a segment of `longest_segment` keys would be of the far class — behind it
 * rdst_hip_select_scratch_bytes(longest_segment, n_ranks, elem_bytes, index_bytes, 0).  0 for no segment, 2^32 segments or
 * keys and more, and unsupported widths. */
uint64_t rdst_hip_select_segments_scratch_bytes(uint64_t n_segments, uint64_t longest_segment, uint64_t n_ranks,
                                                uint32_t elem_bytes, uint32_t index_bytes);
/* out = { wave_max, block_max, stream_max, max_ranks per round } for this key width (index_bytes 0 = keys only: the larger
 * keys-only tile).  Pure but for rdst_hip_set_topk_segments_stream_max.  Unsupported widths: rdst_hip_topk_limits' codes. */
int rdst_hip_select_segments_limits(uint32_t elem_bytes, uint32_t index_bytes, uint32_t out[4]);

/* The two segmented sorts (rdst_hip_sort_segments_device, ..._pairs_device) with the table of borders in DEVICE memory (src/sorter.rs:131-138, as above): a CSR row pointer, the
 * cumulative sum of a ragged batch's lengths, the bucket borders rdst_hip_split_top_level_device leaves behind — no copy of
 * the table to the host, no host plan.  dev_offsets: n_segments + 1 unsigned integers of offset_bytes (4 or 8) bytes,
 * aligned to that size, read only, and read in stream order (the kernel that writes the table may still be running when
 * the call returns).  4-byte offsets need len < 2^32; n_segments <= 2^30 (RDST_ERR_UNSUPPORTED beyond: the plan's own
 * sort stays below the lengths rdst_hip_sort_device splits).  Segment semantics, key widths, kinds, `levels`, the classes
 * and their limits, and the error codes for them are those of the host-offsets entries; every segment ends bit for bit as
 * rdst_hip_sort_segments_device leaves it, pairs with equal keys keep their input order, nothing outside
 * [offsets[0], offsets[n_segments]) is written.
 *
 * dev_scratch: caller-provided like rdst_hip_sort_bytes_device's, 256-byte aligned, at least
 * rdst_hip_sort_segments_device_offsets_scratch_bytes(n_segments) bytes.  The plan lives there: a class key and the segment
 * index per segment, one stable (u32, u32) pair sort of them by the library's own pair route (so rdst_hip_last_route, the
 * profile runs and rdst_hip_debug_last_sample see that sort too), and the work list — rdst_segments_plan's, item for item.
 * Stream order makes the scratch reusable by the next call on the same stream.
 *
 * tmp_elems chooses between two modes:
 *   tmp_elems == 0 (tmp pointers may be NULL): FULLY ASYNCHRONOUS.  The call enqueues the plan and the two batched
 *       launches (grids bounded by what the host knows — n_segments and len —, counts read from the scratch) and returns:
 *       no copy to or from the host, no wait on an event or on the stream, no staging buffer.  The one exception is the one
 *       every entry shares: a library workspace that has to grow.  A table the device finds invalid (decreasing, last
 *       offset past len) or a segment longer than block_max cannot be answered by the return code: NO key or value is
 *       modified, the bit of value 16 (0x10) of the sticky device error word is set, and rdst_hip_device_status returns RDST_ERR_DEVICE once.
 *   tmp_elems > 0: for tables that may hold segments beyond block_max, which the host has to enqueue one after another
 *       (dev_tmp — pairs: dev_tmp_keys, dev_tmp_vals — as their scratch, as above).  One exception to "asynchronous", of
 *       the kind rdst_hip_sort_device documents for its split: the call WAITS once for `stream` after the plan and reads
 *       the three counts, the longest long segment and the flags; with long segments it reads their items too (one further
 *       wait), and long segments beyond the window wait as rdst_hip_sort_device does.  Because the host sees the flags, an
 *       invalid table, tmp_elems below the longest long segment, or a NULL tmp is RDST_ERR_ARG with nothing sorted and
 *       nothing left in the error word.
 * Before any device work — RDST_ERR_ARG: NULL dev_offsets with n_segments > 0, offset_bytes not 4 or 8, 4-byte offsets with
 * len >= 2^32, tmp_elems > 0 with a NULL tmp, NULL scratch, scratch_bytes too small; RDST_ERR_ALIGN: a misaligned offsets
 * pointer or scratch; RDST_ERR_UNSUPPORTED: n_segments > 2^30, pair widths other than 4/8 x 4/8.  n_segments == 0 is
 * RDST_OK and needs no pointers. */
int rdst_hip_sort_segments_device_offsets(void* dev_keys, void* dev_tmp, uint64_t tmp_elems, uint64_t len,
                                          const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments,
                                          uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                          void* dev_scratch, uint64_t scratch_bytes, void* stream);
int rdst_hip_sort_segments_pairs_device_offsets(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals,
                                                uint64_t tmp_elems, uint64_t len, const void* dev_offsets, uint32_t offset_bytes,
                                                uint64_t n_segments, uint32_t key_bytes, rdst_key_kind kind, uint32_t levels,
                                                uint32_t val_bytes, void* dev_scratch, uint64_t scratch_bytes, void* stream);
/* The scratch of the two entries above (src/sorter.rs:131-138).  Pure: 32 bytes per segment, rounded up array by array, and a
 * 256-byte header; 0 for n_segments == 0 or > 2^30. */
uint64_t rdst_hip_sort_segments_device_offsets_scratch_bytes(uint64_t n_segments);
/* The device-offsets sorts with NO HOST INVOLVEMENT FOR SEGMENTS OF ANY LENGTH (src/sorter.rs:131-138, as above).  The
 * arguments are those of the two entries above without tmp_elems: dev_tmp (pairs: dev_tmp_keys, dev_tmp_vals) holds `len`
 * elements, as for rdst_hip_sort_device.  Segments up to block_max take the two batched launches of the asynchronous mode;
 * longer ones take a device route of their own ("tiled"): they are cut into tiles of block_max keys and sorted by one
 * stable counting pass per key byte between the keys and tmp — per level a count launch, a prefix launch and a scatter
 * launch over all long segments at once, grids bounded by what the host knows (n_segments and len), counts read from the
 * scratch.  The call enqueues the plan and these launches and returns: no device-to-host copy, no wait on an event or on
 * the stream, no staging buffer (the one exception is the one every entry shares: a library workspace that has to grow for
 * the plan's own pair sort).  Every segment ends bit for bit as rdst_hip_sort_segments_device leaves it, pairs with equal
 * keys keep their input order, nothing outside [offsets[0], offsets[n_segments]) of the keys or values is written, and of
 * tmp only the positions of segments beyond block_max are written (content afterwards unspecified).
 * A table the device finds invalid (decreasing, last offset past len): NO key, value or tmp element is modified, bit 0x10
 * of the device error word is set and rdst_hip_device_status returns RDST_ERR_DEVICE once.  A long segment is no error here.
 * dev_scratch: 256-byte aligned, at least rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(n_segments, len,
 * elem_bytes, val_bytes) bytes.  Before any device work: the errors of the entries above (scratch_bytes against this size
 * function); len >= 2^32: RDST_ERR_UNSUPPORTED (positions inside an item and tile indices are u32, as on the [u8; N > 16]
 * route); a NULL tmp with len > 0 and n_segments > 0: RDST_ERR_ARG.  n_segments == 0 is RDST_OK and needs no pointers. */
int rdst_hip_sort_segments_device_offsets_nowait(void* dev_keys, void* dev_tmp, uint64_t len, const void* dev_offsets,
                                                 uint32_t offset_bytes, uint64_t n_segments, uint32_t elem_bytes,
                                                 rdst_key_kind kind, uint32_t levels, void* dev_scratch, uint64_t scratch_bytes,
                                                 void* stream);
int rdst_hip_sort_segments_pairs_device_offsets_nowait(void* dev_keys, void* dev_vals, void* dev_tmp_keys, void* dev_tmp_vals,
                                                       uint64_t len, const void* dev_offsets, uint32_t offset_bytes,
                                                       uint64_t n_segments, uint32_t key_bytes, rdst_key_kind kind, uint32_t levels,
                                                       uint32_t val_bytes, void* dev_scratch, uint64_t scratch_bytes, void* stream);
/* The scratch of the two nowait entries (src/sorter.rs:131-138).  Pure, monotone in n_segments and in len: the plan's layout
 * (rdst_hip_sort_segments_device_offsets_scratch_bytes) followed by the tiled route's tile_base (n_long_bound + 1 u32),
 * digit_base (256 u32 per possible long segment) and tile_counts (256 u32 per possible tile), each rounded up to 256 bytes,
 * with n_long_bound = min(n_segments, len / (block_max + 1)) and len / block_max + n_long_bound tiles at most: 1 KiB per
 * possible tile, about len / 16 bytes for keys of up to 4 bytes.  0 for n_segments == 0 or > 2^30, len >= 2^32 and unsupported widths. */
uint64_t rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(uint64_t n_segments, uint64_t len, uint32_t elem_bytes,
                                                                    uint32_t val_bytes);
/* Test hook (src/sorter.rs:131-138), BLOCKING: runs the device plan and copies out the work list it produced, in
 * rdst_segments_plan's output form.  *flags_out: 1 = offsets decrease somewhere, 2 = the last offset lies past len (then
 * RDST_OK with the flags as the answer; counts and items mean nothing); the error word is left alone.  A `capacity` below
 * the three counts' sum: RDST_ERR_ARG with the counts, *tmp_elems_out and *flags_out written. */
int rdst_hip_debug_segments_plan_device(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len,
                                        uint32_t elem_bytes, uint32_t val_bytes, void* dev_scratch, uint64_t scratch_bytes,
                                        rdst_segment_item* items_out, uint64_t capacity, uint64_t class_counts_out[3],
                                        uint64_t* tmp_elems_out, uint32_t* flags_out, void* stream);

/* rdst_hip_topk_segments_device with the table of borders in DEVICE memory: a CSR row pointer, the cumulative sum of a ragged
 * batch's lengths, the bucket borders rdst_hip_split_top_level_device leaves behind — no copy of the table to the host, no
 * host plan.  dev_offsets follows the rules of rdst_hip_sort_segments_device_offsets: n_segments + 1 unsigned integers of
 * offset_bytes (4 or 8) bytes, aligned to that size, read only, and read in stream order (the kernel that writes the table may
 * still be running when the call returns); n_segments <= 2^30; len < 2^32 as for every partial sort.  The result is exactly
 * rdst_hip_topk_segments_device's: row s of the outputs starts at element s * k; its first min(k, n_s) slots hold, bit for
 * bit, what rdst_hip_topk_device gives for segment s, positions local to the segment; the slots behind, empty segments and
 * the input are not written.  Keys only: every width and kind; with an index (4 or 8 bytes): 4- and 8-byte keys;
 * RDST_TOPK_LARGEST as there.
 *
 * dev_scratch: 256-byte aligned, at least rdst_hip_topk_segments_device_offsets_scratch_bytes(n_segments, far_capacity, k,
 * elem_bytes, index_bytes) bytes.  The plan lives there: a class key and the segment index per segment, one stable (u32, u32)
 * pair sort of them by the library's own pair route (so rdst_hip_last_route, the profile runs and rdst_hip_debug_last_sample
 * see that sort too), and the work list — rdst_topk_segments_plan's, item for item.  It needs no clearing; stream order makes
 * it reusable by the next call on the same stream.
 *
 * far_capacity chooses between two modes, as tmp_elems does for rdst_hip_sort_segments_device_offsets:
 *   far_capacity == 0: FULLY ASYNCHRONOUS.  The call enqueues the plan and three launches (grids bounded by what the host
 *       knows — n_segments and len —, counts read from the scratch; surplus waves and workgroups return at once) and returns:
 *       no copy to or from the host, no wait on an event or on the stream, no staging buffer.  The one exception is the one
 *       every entry shares: a library workspace that has to grow, here for the plan's pair sort.  In this mode THE STREAM CLASS
 *       HAS NO UPPER LENGTH: with k <= k_stream_max (rdst_hip_topk_segments_limits) every segment beyond block_max is served
 *       by one workgroup's streamed radix select, longest first, whatever rdst_hip_set_topk_segments_stream_max says.  For
 *       such a k the call has no data-dependent failure and never needs the host — and the host knows k before it calls.
 *       One workgroup on a very long segment is a performance cliff (a segment of 2^24 keys is read by 1 of 256 compute
 *       units), never a wrong answer; far_capacity > 0 is the answer to it.  With k > k_stream_max a segment beyond block_max
 *       cannot be served, and neither that nor a table the device finds invalid (decreasing, last offset past len) can be
 *       answered by the return code: NO output element is written, the bit of value 16 (0x10) of the sticky device error word
 *       is set, and rdst_hip_device_status returns RDST_ERR_DEVICE once.
 *   far_capacity > 0: EVERY TABLE, ONE WAIT.  The classes are exactly rdst_hip_topk_segments_device's (they follow
 *       rdst_hip_topk_segments_limits and rdst_hip_set_topk_segments_stream_max).  The call WAITS once for `stream` after the
 *       plan and reads the four counts, the longest far segment and the flags; with far segments it reads their items too
 *       (one further wait).  It launches the three batched classes and runs the far segments one after another by
 *       rdst_hip_topk_device's route, in the scratch behind the plan.  Because the host sees the flags, an invalid table or a
 *       longest far segment above far_capacity is RDST_ERR_ARG with nothing written and nothing left in the error word.  A
 *       caller without a better bound passes len.
 * Profiling: the batched launches end rdst_hip_topk_segments_device's stages, RDST_STAGE_SEGMENTS | (class << 8).
 * Arguments, checked in this order before any device work:
 *   1. the key arguments, len and flags as rdst_hip_topk_segments_device checks them (its codes and messages);
 *   2. k == 0 or n_segments == 0 -> RDST_OK, nothing else is looked at;
 *   3. the table as rdst_hip_sort_segments_device_offsets checks it: n_segments > 2^30 -> RDST_ERR_UNSUPPORTED; offset_bytes
 *      not 4 or 8, NULL dev_offsets -> RDST_ERR_ARG; dev_offsets misaligned to offset_bytes -> RDST_ERR_ALIGN;
 *   4. the outputs as rdst_hip_topk_segments_device checks them: NULL dev_out_keys -> RDST_ERR_ARG; misaligned ->
 *      RDST_ERR_ALIGN; with an index: index_bytes not 4 or 8 -> RDST_ERR_ARG, key width not 4 or 8 -> RDST_ERR_UNSUPPORTED,
 *      misaligned index pointer -> RDST_ERR_ALIGN (with a NULL dev_out_index, index_bytes is not looked at);
 *   5. the scratch: NULL -> RDST_ERR_ARG; not 256-byte aligned -> RDST_ERR_ALIGN; far_capacity >= 2^32 or scratch_bytes below
 *      rdst_hip_topk_segments_device_offsets_scratch_bytes(...) -> RDST_ERR_ARG. */
int rdst_hip_topk_segments_device_offsets(const void* dev_keys, uint64_t len,
                                          const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t k,
                                          void* dev_out_keys, void* dev_out_index, uint32_t index_bytes,
                                          void* dev_scratch, uint64_t scratch_bytes, uint64_t far_capacity,
                                          uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                          uint32_t flags, void* stream);
/* The scratch of the call above.  Pure, monotone in every argument: the plan's layout
 * (rdst_hip_sort_segments_device_offsets_scratch_bytes(n_segments): 32 bytes per segment and a 256-byte header) and, with
 * far_capacity > 0, behind it rdst_hip_topk_scratch_bytes(far_capacity, min(k, far_capacity), elem_bytes, index_bytes, 0).
 * 0 for n_segments == 0 or > 2^30, far_capacity >= 2^32 and unsupported widths. */
uint64_t rdst_hip_topk_segments_device_offsets_scratch_bytes(uint64_t n_segments, uint64_t far_capacity, uint64_t k,
                                                             uint32_t elem_bytes, uint32_t index_bytes);
/* Test hook, BLOCKING, like rdst_hip_debug_segments_plan_device: runs the device plan of the call above for this k and these
 * widths and copies out the work list it produced, in rdst_topk_segments_plan's output form.  unbounded_stream != 0: the
 * classes of the asynchronous mode (no upper length of the stream class); 0: the wait mode's.  *flags_out: 1 = offsets
 * decrease somewhere, 2 = the last offset lies past len (then RDST_OK with the flags as the answer; counts and items mean
 * nothing); the error word is left alone.  dev_scratch: the plan's part of the scratch above.  k == 0: no items.  A
 * `capacity` below the four counts' sum: RDST_ERR_ARG with the counts, *longest_far_out and *flags_out written. */
int rdst_hip_debug_topk_segments_plan_device(const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments, uint64_t len,
                                             uint64_t k, uint32_t elem_bytes, uint32_t index_bytes, uint32_t unbounded_stream,
                                             void* dev_scratch, uint64_t scratch_bytes,
                                             rdst_segment_item* items_out, uint64_t capacity, uint64_t class_counts_out[4],
                                             uint64_t* longest_far_out, uint32_t* flags_out, void* stream);

/* rdst_hip_select_segments_device with the table of borders in DEVICE memory: a CSR row pointer, the cumulative sum of a
 * ragged batch's lengths, the bucket borders rdst_hip_split_top_level_device leaves behind — no copy of the table to the host,
 * no host plan.  dev_offsets follows the rules of rdst_hip_sort_segments_device_offsets: n_segments + 1 unsigned integers of
 * offset_bytes (4 or 8) bytes, aligned to that size, read only, and read in stream order (the kernel that writes the table may
 * still be running when the call returns); n_segments <= 2^30; len < 2^32.  ranks stays a HOST array of n_ranks specs, read
 * before the call returns: the host knows them, and they travel as kernel arguments.  The result is exactly
 * rdst_hip_select_segments_device's, bit for bit: row s of the outputs starts at element s * n_ranks; slot i holds what
 * rdst_hip_select_device gives for the slice at the rank rdst_rank_for_length(&ranks[i], n_s), positions local to the segment;
 * slots without a rank, empty segments and the input are not written.  Keys only: every width and kind; with an index (4 or 8
 * bytes): 4- and 8-byte keys; RDST_TOPK_LARGEST as there.
 *
 * dev_scratch: 256-byte aligned, at least rdst_hip_select_segments_device_offsets_scratch_bytes(n_segments, far_capacity,
 * n_ranks, elem_bytes, index_bytes) bytes; only that range is written, and it needs no clearing.  The plan lives there, made
 * on the device as rdst_hip_topk_segments_device_offsets makes its own: the select's work list is rdst_topk_segments_plan's
 * with k = 1, so rdst_hip_debug_topk_segments_plan_device with k = 1 is the test hook for THIS entry's plan too.  Stream order
 * makes the scratch reusable by the next call on the same stream.
 *
 * far_capacity chooses between two modes, as it does for rdst_hip_topk_segments_device_offsets:
 *   far_capacity == 0: FULLY ASYNCHRONOUS.  The call enqueues the plan — once per call — and three launches per round of
 *       max_ranks specs (rdst_hip_select_segments_limits; every round runs over the same items, slot i keeping its place in
 *       the row; grids bounded by what the host knows — n_segments and len —, counts read from the scratch; surplus waves and
 *       workgroups return at once) and returns: no copy to or from the host, no wait on an event or on the stream, no staging
 *       buffer.  The one exception is the one every entry shares: a library workspace that has to grow, here for the plan's
 *       pair sort.  In this mode THE STREAM CLASS HAS NO UPPER LENGTH: every segment beyond block_max is served by one
 *       workgroup's streamed radix select, longest first, whatever rdst_hip_set_topk_segments_stream_max says.  One workgroup
 *       on a very long segment is a performance cliff, never a wrong answer — and a steeper one than the partial sort's: every
 *       rank that misses what the LDS stage holds counts again from the root, so a segment of 2^24 keys is read by 1 of 256
 *       compute units several times per distinct rank neighbourhood; far_capacity > 0 is the answer to it.  With k = 1 the plan
 *       never meets "k > k_stream_max", so this mode has NO DATA-DEPENDENT FAILURE except an invalid table (decreasing, last
 *       offset past len), which cannot be answered by the return code: NO output element is written, the bit of value 16
 *       (0x10) of the sticky device error word is set, and rdst_hip_device_status returns RDST_ERR_DEVICE once.
 *   far_capacity > 0: EVERY TABLE, ONE WAIT.  The classes are exactly rdst_hip_select_segments_device's (they follow
 *       rdst_hip_select_segments_limits and rdst_hip_set_topk_segments_stream_max).  The call WAITS once for `stream` after the
 *       plan and reads the four counts, the longest far segment and the flags; with far segments it reads their items and
 *       unsaturated lengths too (one further wait), resolves and orders their ranks on the host as the host-table entry does,
 *       and runs them one after another by rdst_hip_select_device's route, in the scratch behind the plan.  Because the host
 *       sees the flags, an invalid table or a longest far segment above far_capacity is RDST_ERR_ARG with nothing written and
 *       nothing left in the error word.  A caller without a better bound passes len.
 * Profiling: the batched launches end rdst_hip_select_segments_device's stages, RDST_STAGE_SEGMENTS | (class << 8).
 * Arguments, checked in this order before any device work:
 *   1. the key arguments, len and flags as rdst_hip_select_segments_device checks them (its codes and messages);
 *   2. n_ranks == 0 or n_segments == 0 -> RDST_OK, nothing else is looked at;
 *   3. the table as rdst_hip_sort_segments_device_offsets checks it: n_segments > 2^30 -> RDST_ERR_UNSUPPORTED; offset_bytes
 *      not 4 or 8, NULL dev_offsets -> RDST_ERR_ARG; dev_offsets misaligned to offset_bytes -> RDST_ERR_ALIGN;
 *   4. NULL ranks, a bad spec -> RDST_ERR_ARG, the message names the first bad i;
 *   5. the outputs as rdst_hip_select_segments_device checks them: NULL dev_out_keys -> RDST_ERR_ARG; misaligned ->
 *      RDST_ERR_ALIGN; with an index: index_bytes not 4 or 8 -> RDST_ERR_ARG, key width not 4 or 8 -> RDST_ERR_UNSUPPORTED,
 *      misaligned index pointer -> RDST_ERR_ALIGN (with a NULL dev_out_index, index_bytes is not looked at);
 *   6. the scratch: NULL -> RDST_ERR_ARG; not 256-byte aligned -> RDST_ERR_ALIGN; far_capacity >= 2^32 or scratch_bytes below
 *      rdst_hip_select_segments_device_offsets_scratch_bytes(...) -> RDST_ERR_ARG. */
int rdst_hip_select_segments_device_offsets(const void* dev_keys, uint64_t len,
                                            const void* dev_offsets, uint32_t offset_bytes, uint64_t n_segments,
                                            const rdst_rank_spec* ranks, uint64_t n_ranks,
                                            void* dev_out_keys, void* dev_out_index, uint32_t index_bytes,
                                            void* dev_scratch, uint64_t scratch_bytes, uint64_t far_capacity,
                                            uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                            uint32_t flags, void* stream);
/* The scratch of the call above.  Pure, monotone in every argument: the plan's layout
 * (rdst_hip_sort_segments_device_offsets_scratch_bytes(n_segments): 32 bytes per segment and a 256-byte header) and, with
 * far_capacity > 0, behind it rdst_hip_select_scratch_bytes(far_capacity, n_ranks, elem_bytes, index_bytes, 0).
 * 0 for n_segments == 0 or > 2^30, far_capacity >= 2^32 and unsupported widths. */
uint64_t rdst_hip_select_segments_device_offsets_scratch_bytes(uint64_t n_segments, uint64_t far_capacity, uint64_t n_ranks,
                                                               uint32_t elem_bytes, uint32_t index_bytes);

/* Runs of equal keys: the device twin of `v.radix_sort_unstable(); v.dedup();` and of "where does each key's group begin".
 * Call m the length: `len`, or, with a non-NULL dev_len, the unsigned integer of len_bytes (4 or 8) bytes it points to, read
 * only and in stream order exactly as rdst_hip_sort_device_devlen reads it.  A run is a maximal stretch of consecutive
 * elements of dev_keys[0 .. m) with BIT-IDENTICAL keys: -0.0 and +0.0, and two NaN payloads, are different keys; identical NaN
 * bits are one key.  The input need not be sorted (Vec::dedup, unique_consecutive); on a sorted input the runs are the
 * distinct keys with their multiplicities.  Call R the number of runs.  Written, bit for bit and deterministic:
 *   - dev_n_runs[0] = R, the true number, whatever out_capacity is (one unsigned integer of offset_bytes bytes);
 *   - for r < min(R, out_capacity): dev_out_keys[r] = the key of run r in its original bits, dev_out_starts[r] = the position
 *     of its first element (offset_bytes bytes each); either pointer may be NULL, which skips that output;
 *   - R <= out_capacity: dev_out_starts[R] = m, so starts[0 .. R] is a CSR table of the groups, valid for every
 *     *_device_offsets entry;
 *   - RDST_RUNS_PAD_STARTS and R <= out_capacity: dev_out_starts[r] = m for every r in (R, out_capacity] as well — a second
 *     launch sized by out_capacity, A WRITE OF out_capacity OFFSETS —, so that a caller passes n_segments = out_capacity to a
 *     segmented entry without ever reading R: the surplus segments are empty.  Without the flag nothing behind slot R is
 *     written;
 *   - R > out_capacity > 0: the first out_capacity runs are complete — keys, starts, and starts[out_capacity] = the end of
 *     the last kept run —, nothing is padded, and the bit of value 64 (0x40) of the device error word is set:
 *     rdst_hip_device_status returns RDST_ERR_DEVICE once;
 *   - out_capacity == 0: the counting call.  Only dev_n_runs is written, the output pointers may be NULL, no error bit;
 *   - m == 0: R = 0 and starts[0] = 0;
 *   - m > len: NOTHING at all is written and bit 0x20 is set, as the _devlen sorts do.
 * The input is never written.  Nothing is touched outside [0, out_capacity) of the keys, [0, out_capacity] of the starts, the
 * one n_runs word and [0, rdst_hip_runs_scratch_bytes(len, elem_bytes)) of the scratch.  Every width of rdst_hip_sort_device
 * (1, 2, 4, 8, 16 bytes) and every kind; 4-byte offsets are legal for every supported len.
 * ASYNCHRONOUS on `stream` for every input: one pass over the keys (a chained scan with decoupled look-back),
 * no copy to or from the host, no wait on an event or on the stream, no library workspace; the caller's scratch (256-byte
 * aligned) holds everything, needs no clearing — the library clears it itself in stream order — and is reusable by the next
 * call on the same stream.  THE ONLY DATA-DEPENDENT OUTCOMES are the two error bits above.
 * Arguments, checked in this order before any device work:
 *   1. the key arguments as rdst_hip_sort_device checks them (its codes and messages);
 *   2. RDST_KEY_BYTES_BE -> RDST_ERR_UNSUPPORTED;   3. len >= 2^32 -> RDST_ERR_UNSUPPORTED (positions are u32 in the kernels);
 *   4. unknown flag bits -> RDST_ERR_ARG;
 *   5. with dev_len: len_bytes not 4 or 8 -> RDST_ERR_ARG, misaligned -> RDST_ERR_ALIGN;
 *   6. offset_bytes not 4 or 8 -> RDST_ERR_ARG;
 *   7. NULL dev_n_runs -> RDST_ERR_ARG, misaligned -> RDST_ERR_ALIGN, inside the input or on the length -> RDST_ERR_ARG;
 *   8. with out_capacity > 0: a misaligned output -> RDST_ERR_ALIGN; outputs that overlap the input, the length or each other
 *      (dev_n_runs included) -> RDST_ERR_ARG; RDST_RUNS_PAD_STARTS with NULL dev_out_starts -> RDST_ERR_ARG;
 *   9. NULL scratch -> RDST_ERR_ARG, not 256-byte aligned -> RDST_ERR_ALIGN, scratch_bytes below
 *      rdst_hip_runs_scratch_bytes(len, elem_bytes) -> RDST_ERR_ARG, those bytes overlapping the input, the length, dev_n_runs
 *      or an output -> RDST_ERR_ARG.
 * len == 0 still does the device writes of m == 0. */
#define RDST_RUNS_PAD_STARTS 1u
int rdst_hip_runs_device(const void* dev_keys, uint64_t len,
                         const void* dev_len, uint32_t len_bytes,
                         void* dev_out_keys, void* dev_out_starts,
                         void* dev_n_runs, uint32_t offset_bytes,
                         uint64_t out_capacity,
                         void* dev_scratch, uint64_t scratch_bytes,
                         uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                         uint32_t flags, void* stream);
/* The scratch of the call above: a 256-byte header and one 64-bit status word per tile of `len` keys (rdst_hip_runs_limits).  Pure, monotone in len.
 * 0 for len >= 2^32 and unsupported widths. */
uint64_t rdst_hip_runs_scratch_bytes(uint64_t len, uint32_t elem_bytes);
/* out[0] = keys per tile, out[1] = status words one look-back round trip fetches (tests place their inputs by them).  Pure.
 * Unsupported widths: RDST_ERR_UNSUPPORTED. */
int rdst_hip_runs_limits(uint32_t elem_bytes, uint32_t out[2]);

/* Binary search: the device twin of `binary_search` / `partition_point` on a sorted slice and of numpy.searchsorted — where
 * each of n_needles keys falls in a sorted array.  Call m the length of the haystack: `len`, or, with a non-NULL dev_len, the
 * unsigned integer of len_bytes (4 or 8) bytes it points to, read only and in stream order exactly as rdst_hip_runs_device
 * reads its length.  THE ORDER IS THE SORT'S: key a comes before key b when map_key(a) < map_key(b) for `kind`; floats go
 * -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, NaNs by their bits, and two keys are equal only when they are
 * BIT-IDENTICAL (the equality of rdst_hip_runs_device).  Precondition: dev_sorted[0 .. m) is in that order, as every sort
 * entry leaves it.  Written for every i < n_needles, bit for bit and deterministic, as unsigned integers of offset_bytes
 * (4 or 8) bytes:
 *   - dev_out_lower[i] = the number of keys of dev_sorted[0 .. m) that order strictly before dev_needles[i]
 *     (partition_point(|x| x < q), side="left");
 *   - dev_out_upper[i] = the number that order before it or equal it (side="right");
 *   either pointer may be NULL, which skips that output.  upper - lower is the multiplicity of the needle in the haystack,
 *   lower == upper means "not present".
 *   - m == 0: every output is 0;
 *   - n_needles == 0: RDST_OK after the argument checks, no device work;
 *   - m > len: NOTHING at all is written and bit 0x20 of the device error word is set, as the _devlen sorts and
 *     rdst_hip_runs_device do.  THE ONLY DATA-DEPENDENT OUTCOME is that bit.
 * AN UNSORTED HAYSTACK costs correctness only, never safety: every output is some value in [0, m], nothing outside the buffers
 * is read or written, and every loop has a bound that does not depend on the data's order.
 * The haystack and the needles are never written and may overlap each other in any way (an array searched for its own keys
 * gives each element's group start and end); the outputs and the scratch may overlap nothing else.  Every width of
 * rdst_hip_sort_device (1, 2, 4, 8, 16 bytes) and every kind except RDST_KEY_BYTES_BE; len and n_needles below 2^32.
 * ASYNCHRONOUS on `stream` for every input: two launches (a splitter table, then one workgroup per tile of needles that
 * searches a staged window in LDS or the table and one gap of the haystack), no copy to or from the host, no
 * wait on an event or on the stream, no library workspace, no allocation; the caller's scratch (256-byte aligned) holds
 * everything, needs no clearing — the library initialises it itself in stream order — and is reusable by the next call on
 * the same stream.
 * Arguments, checked in this order before any device work:
 *   1. the key arguments of the haystack as rdst_hip_sort_device checks them (its codes and messages);
 *   2. RDST_KEY_BYTES_BE -> RDST_ERR_UNSUPPORTED;   3. len or n_needles >= 2^32 -> RDST_ERR_UNSUPPORTED (positions are u32 in
 *      the kernels);
 *   4. any flag bit -> RDST_ERR_ARG (none is defined yet);
 *   5. with dev_len: len_bytes not 4 or 8 -> RDST_ERR_ARG, misaligned -> RDST_ERR_ALIGN;
 *   6. NULL dev_needles with n_needles > 0 -> RDST_ERR_ARG, not aligned to elem_bytes -> RDST_ERR_ALIGN;
 *   7. offset_bytes not 4 or 8 -> RDST_ERR_ARG;
 *   8. both outputs NULL -> RDST_ERR_ARG; a misaligned output -> RDST_ERR_ALIGN; an output that overlaps the haystack, the
 *      needles, the length or the other output -> RDST_ERR_ARG;
 *   9. NULL scratch -> RDST_ERR_ARG, not 256-byte aligned -> RDST_ERR_ALIGN, scratch_bytes below
 *      rdst_hip_search_scratch_bytes(len, n_needles, elem_bytes) -> RDST_ERR_ARG, those bytes overlapping the haystack, the
 *      needles, the length or an output -> RDST_ERR_ARG. */
int rdst_hip_search_device(const void* dev_sorted, uint64_t len,
                           const void* dev_len, uint32_t len_bytes,
                           const void* dev_needles, uint64_t n_needles,
                           void* dev_out_lower, void* dev_out_upper, uint32_t offset_bytes,
                           void* dev_scratch, uint64_t scratch_bytes,
                           uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                           uint32_t flags, void* stream);
/* The scratch of the call above: a 256-byte header and the splitter table (rdst_hip_search_limits), the same for every
 * supported length.  Pure, monotone in every argument.  0 for len or n_needles >= 2^32 and unsupported widths. */
uint64_t rdst_hip_search_scratch_bytes(uint64_t len, uint64_t n_needles, uint32_t elem_bytes);
/* out[0] = needles per workgroup tile, out[1] = splitters, out[2] = the most keys of the haystack a workgroup stages in LDS
 * (tests place their inputs by them).  Pure.  Unsupported widths: RDST_ERR_UNSUPPORTED. */
int rdst_hip_search_limits(uint32_t elem_bytes, uint32_t out[3]);
/* Test hook, BLOCKING on `stream`: the scratch header of the last rdst_hip_search_device call there.  out[0] = m,
 * out[1] = tiles that took the staged path, out[2] = tiles that took the table path, out[3] = 1 if m was past len. */
int rdst_hip_debug_search_state(const void* dev_scratch, void* stream, uint64_t out[4]);

/* [u8; N] rows (N = n_bytes in 1..RDST_BYTES_MAX_N), device-resident, sorted IN PLACE in lexicographic order
 * (src/radix_key_impl.rs:78-85).  No alignment requirement on dev_rows.  dev_scratch: at least
 * rdst_hip_sort_bytes_scratch_bytes(len, n_bytes) bytes, 256-byte aligned.  len <= 1: no-op.
 * N <= 16: the rows are widened to 4-, 8- or 16-byte integers and take the integer route; asynchronous on `stream`.
 * N > 16 (needs len < 2^32, else RDST_ERR_UNSUPPORTED): one stable (u64 prefix, u32 row) pair sort, then rounds over
 * the rows still tied — short runs by a comparison kernel, long ones by another pair sort on (run, next bytes) — and a
 * gather of the rows.  BLOCKING: the tie counts of every round come to the host (one copy and one wait per
 * round; keys that differ in their first 8 bytes take exactly one; rdst_hip_sort_bytes_device_nowait below does without).
 * Equal rows keep their input order.  Kernel failures are reported by rdst_hip_device_status. */
#define RDST_BYTES_MAX_N 4096u
int rdst_hip_sort_bytes_device(void* dev_rows, uint64_t len, uint32_t n_bytes,
                               void* dev_scratch, uint64_t scratch_bytes, void* stream);
uint64_t rdst_hip_sort_bytes_scratch_bytes(uint64_t len, uint32_t n_bytes);   /* 0 for n_bytes outside 1..RDST_BYTES_MAX_N */

/* rdst_hip_sort_bytes_device without the host in the loop (src/radix_key_impl.rs:78-85: the same lexicographic order,
 * bit for bit the blocking entry's result; equal rows keep their input order).  The arguments, the scratch size
 * (rdst_hip_sort_bytes_scratch_bytes), the alignment rules, the argument errors and their order are those of the blocking
 * entry.  N <= 16 forwards to the widened integer route.  N > 16: the prefix pair sort, one kernel that raises a flag word
 * on the device if any two 8-byte prefixes tie, then ceil(N / 8) rounds, last chunk first, each a chunk-key kernel and a
 * stable (u64 chunk, u32 row) pair sort; with the flag down every key of a round is 0 and its pair sort skips all its
 * levels.  The rounds are enqueued whether or not they are needed, so the entry is built for 16 rounds at
 * most: N > RDST_BYTES_NOWAIT_MAX_N -> RDST_ERR_UNSUPPORTED (wider keys take rdst_hip_sort_bytes_device).
 * ASYNCHRONOUS on `stream`: no copy to the host, no stream or event wait; the one exception is the one every entry shares,
 * a library workspace that has to grow.  Kernel failures are reported by rdst_hip_device_status. */
#define RDST_BYTES_NOWAIT_MAX_N 128u
int rdst_hip_sort_bytes_device_nowait(void* dev_rows, uint64_t len, uint32_t n_bytes,
                                      void* dev_scratch, uint64_t scratch_bytes, void* stream);

/* ---- records ordered by a described key ------------------------------------------------------
 * `impl RadixKey for MyStruct` as data (src/radix_key.rs: `const LEVELS` and `get_level`; examples/impl_radix_key.rs:32-56
 * sorts one four-byte struct by all of its bytes, by its even bytes and by its odd bytes).  A key is a table of fields,
 * fields[0] the most significant.  For a record r the mapped key string K(r) is the concatenation, in field order, of every
 * field's mapped value written big-endian: integers are read little-endian from the record at `offset` (no alignment
 * rule), UNSIGNED values are taken as they are, SIGNED values are ^ MIN, FLOAT values get rdst's sign-magnitude flip
 * (src/radix_key_impl.rs:162-185: negative -> every bit flipped, else ^ MIN), BYTES_BE bytes are taken as stored; a
 * descending field has every byte of its mapped value complemented.  Records are ordered by K lexicographically and
 * records with equal K keep their input order.  This is the RadixKey with LEVELS = L = the sum of the fields' widths
 * and get_level(l) = K[L - 1 - l].  A one-byte UNSIGNED field at any offset is the raw level map: the example's "even
 * bytes" key is { {1, 1, RDST_KEY_UNSIGNED, 0}, {3, 1, RDST_KEY_UNSIGNED, 0} }.  Fields may overlap.  L <= RDST_BYTES_MAX_N.
 *
 * Errors, all before any device work: n_fields == 0 -> RDST_ERR_ARG (LEVELS == 0 panics in rdst); n_fields >
 * RDST_KEY_FIELDS_MAX, L > RDST_BYTES_MAX_N or a width not listed for the kind -> RDST_ERR_UNSUPPORTED; an unknown kind, an
 * unknown flag bit, a null table or a field that ends past record_bytes -> RDST_ERR_ARG.  len <= 1 (with a valid
 * description) is a no-op before any pointer check; len >= 2^32 -> RDST_ERR_UNSUPPORTED (row indices are u32). */
#define RDST_FIELD_DESCENDING 1u      /* complement the field's mapped bytes */
#define RDST_KEY_FIELDS_MAX   16u
typedef struct {
    uint32_t offset;  /* byte offset of the field inside the record; no alignment rule */
    uint32_t bytes;   /* UNSIGNED/SIGNED: 1,2,4,8,16   FLOAT: 4,8   BYTES_BE: 1..RDST_BYTES_MAX_N */
    uint32_t kind;    /* rdst_key_kind */
    uint32_t flags;   /* RDST_FIELD_DESCENDING or 0; any other bit: RDST_ERR_ARG */
} rdst_key_field;

/* Host slice of `len` records of `record_bytes` bytes, sorted in place.  Blocking; on failure the slice is untouched.
 * The rows travel to the device, pack_fields_kernel writes K, then: L <= 4 a (u32 key, u32 row) pair sort, L <= 8 a
 * (u64 key, u32 row) pair sort, L > 8 the order core of the [u8; N > 16] route on the packed keys; the rows are gathered
 * by the resulting order and copied back. */
int rdst_hip_sort_records_by_fields(void* host_records, uint64_t len, uint32_t record_bytes,
                                    const rdst_key_field* fields, uint32_t n_fields, const rdst_hip_opts* opts);

/* The same on device-resident records, IN PLACE; the conventions are those of rdst_hip_sort_bytes_device: no alignment
 * rule on dev_records, dev_scratch 256-byte aligned and at least rdst_hip_sort_records_by_fields_scratch_bytes(...) long
 * (the key and index arrays, the packed keys when L > 8, and a staging copy of the rows for the in-place gather), kernel
 * failures are reported by rdst_hip_device_status.  L <= 8: ASYNCHRONOUS on `stream`.  L > 8: BLOCKING, because the tie
 * counts of every refinement round come to the host exactly as on the [u8; N > 16] route. */
int rdst_hip_sort_records_by_fields_device(void* dev_records, uint64_t len, uint32_t record_bytes,
                                           const rdst_key_field* fields, uint32_t n_fields,
                                           void* dev_scratch, uint64_t scratch_bytes, void* stream);
uint64_t rdst_hip_sort_records_by_fields_scratch_bytes(uint64_t len, uint32_t record_bytes,
                                                       const rdst_key_field* fields, uint32_t n_fields);  /* 0 for an invalid description */

/* rdst_hip_sort_records_by_fields_device without the host in the loop (src/radix_key.rs, examples/impl_radix_key.rs:32-56:
 * the same described RadixKey, bit for bit the blocking entry's result; records with equal keys keep their input order).
 * The arguments, the scratch size (rdst_hip_sort_records_by_fields_scratch_bytes), the alignment rules, the argument errors
 * and their order are those of the blocking entry.  L <= 8 forwards to the one pair sort.  L > 8: the packed keys take the
 * rounds of rdst_hip_sort_bytes_device_nowait, which are enqueued whether or not they are needed; hence
 * L > RDST_BYTES_NOWAIT_MAX_N -> RDST_ERR_UNSUPPORTED (longer keys take rdst_hip_sort_records_by_fields_device).
 * ASYNCHRONOUS on `stream` for every L, but for a library workspace that has to grow.  Kernel failures are reported by
 * rdst_hip_device_status. */
int rdst_hip_sort_records_by_fields_device_nowait(void* dev_records, uint64_t len, uint32_t record_bytes,
                                                  const rdst_key_field* fields, uint32_t n_fields,
                                                  void* dev_scratch, uint64_t scratch_bytes, void* stream);

/* Parity and timing hook: pack_fields_kernel alone.  dev_keys receives K for every record in the form the route sorts:
 * L <= 4: len u32 keys, L <= 8: len u64 keys (K left-justified, zero-filled; aligned to their size), L > 8: len dense
 * [u8; L] rows (4-byte aligned).  dev_rows (len x u32; may be NULL when L > 8) receives the row indices 0..len-1.
 * Asynchronous on `stream`. */
int rdst_hip_pack_fields_device(const void* dev_records, uint64_t len, uint32_t record_bytes,
                                const rdst_key_field* fields, uint32_t n_fields,
                                void* dev_keys, uint32_t* dev_rows, void* stream);

/* Blocks until everything queued on `stream` by this library has finished and returns
 * RDST_ERR_DEVICE if any kernel raised the device error word since the last check.  The word is kept
 * outside the per-sort workspace: an error raised by an earlier asynchronous sort is still reported after
 * later sorts were enqueued, once; the check clears it. */
int rdst_hip_device_status(void* stream);

/* Bench yardsticks ("a device copy/triad ceiling on the box", beside the 8 TB/s spec): a
 * 16-bytes-per-lane streaming copy, a read-only sweep and a write-only fill of `bytes` (multiple of 16) on `stream`, in the
 * fastest shape the sweep of profiles/r03_copy_sweep.json found (one contiguous piece per block, non-temporal loads). */
int rdst_hip_stream_copy(void* dev_dst, const void* dev_src, uint64_t bytes, void* stream);
int rdst_hip_stream_read(const void* dev_src, uint64_t bytes, void* stream);
int rdst_hip_stream_fill(void* dev_dst, uint64_t bytes, void* stream);

/* Test hook: ORs `bits` into the device error word from a one-thread kernel on `stream`, exactly as a failing
 * sort kernel would.  The word is sticky: it survives later sorts and workspace growth until
 * rdst_hip_device_status (or a blocking entry point) reports and clears it. */
int rdst_hip_debug_raise_device_error(uint32_t bits, void* stream);

/* Test hook: what the key sample of the most recent pipeline on the current device decided (presample_kernel; it runs from
 * 2^26 keys up, ahead of the byte-saving routes): out = { win_shift, win_top, gross_skew, top_skew, low_dups, predict_lsd },
 * as the sample left them (no later kernel writes these words).  All zero when no pipeline has run, when the sort was too
 * short for a sample or took none (set_hybrid mode 5, the LSD-only setting).  Blocking, like rdst_hip_last_route. */
int rdst_hip_debug_last_sample(void* stream, uint32_t out[6]);

/* Parity hook for get_counts_with_ends (src/sort_utils.rs:109-180) /
 * par_get_counts_with_ends (:35-106): 256-bin histogram of digit `level` over a
 * device-resident slice, plus the `already_sorted` flag (digit sequence non-decreasing)
 * and the first and last digit.  Blocking.  Empty input: counts all zero, sorted = 1,
 * first = last = 0 (sort_utils.rs:116-118). */
int rdst_hip_level_counts(const void* dev_keys, uint64_t len, uint32_t elem_bytes,
                          rdst_key_kind kind, uint32_t level, uint64_t counts[256],
                          uint8_t* already_sorted, uint8_t* first_digit, uint8_t* last_digit,
                          void* stream);

/* Parity hook for the fused multi-level histogram kernel: counts_out[level*256 + digit]
 * for every level in [0, levels).  Same numbers get_counts (sort_utils.rs:183-190)
 * returns level by level.  Blocking. */
int rdst_hip_all_level_counts(const void* dev_keys, uint64_t len, uint32_t elem_bytes,
                              rdst_key_kind kind, uint32_t levels, uint64_t* counts_out,
                              void* stream);

/* Parity hook for one stable counting-sort pass: out_of_place_sort
 * (src/sorts/out_of_place_sort.rs:52-108) / mt_lsb_sort (src/sorts/mt_lsb_sort.rs:40-133)
 * on digit `level`: dev_dst[prefix[d]++] = dev_src[i] in index order.  This is also the
 * MSD split of the sharded route (top level, then contiguous digit ranges per rank).
 * counts_out (nullable) receives the 256 digit counts.  Blocking. */
int rdst_hip_scatter_level(const void* dev_src, void* dev_dst, uint64_t len, uint32_t elem_bytes,
                           rdst_key_kind kind, uint32_t level, uint64_t* counts_out, void* stream);

/* Sharded route (RDST_ALGO_GPU_SHARDED), device-side steps; the collectives between them are the caller's (RCCL through
 * torch.distributed in rdst_amd/sharded.py, or a shim's own ncclAllGather / ncclSend+ncclRecv: INTEGRATION.md).  The
 * reference's analogues are the MSD split of src/sorter.rs:131-138 and the tile -> bucket regrouping of
 * src/sorts/recombinating_sort.rs:68-88.
 *
 * rdst_hip_split_top_level_device: ONE stable pass on the most significant level, dev_src -> dev_dst (dev_src is only
 * read), i.e. the shard grouped by top digit, hence by owner rank (owners are contiguous digit ranges).  The 256 digit
 * counts are left in DEVICE memory (dev_counts, 256 x u64) for the all-gather.  Asynchronous: nothing blocks, the
 * histogram counts that one level only; failures surface in rdst_hip_device_status.
 *
 * rdst_hip_split_top16_device: the fallback when one top digit holds more than a rank's share: two
 * stable passes (levels L-2, L-1; dev_tmp is scratch) leave dev_keys ordered by the top 16 bits of the mapped key, IN
 * PLACE, and dev_counts16 (65 536 x u64, device) receives the bucket lengths — owners are then contiguous ranges of
 * 16-bit prefixes.  Asynchronous.  Keys of at least two bytes. */
int rdst_hip_split_top_level_device(const void* dev_src, void* dev_dst, uint64_t len, uint32_t elem_bytes,
                                    rdst_key_kind kind, uint64_t* dev_counts, void* stream);
int rdst_hip_split_top16_device(void* dev_keys, void* dev_tmp, uint64_t len, uint32_t elem_bytes,
                                rdst_key_kind kind, uint64_t* dev_counts16, void* stream);

/* ---- low-memory route ------------------------------------------------------------------------
 * Device twin of the route `with_low_mem_tuner()` selects (src/radix_sort_builder.rs:74-77; LowMemoryTuner picks Regions
 * above 10^6 elements, Ska below: src/tuners/low_memory_tuner.rs:36-41): sorts `dev_keys` IN PLACE with a scratch of
 * only `tmp_len` elements (`dev_tmp`; len / 64 is a good size, anything from 2^16 elements up works) instead of a second
 * array.  One Regions-sort level (src/sorts/regions_sort.rs:51-286) on the most significant unsorted digit: every tile of
 * tmp_len keys is grouped by digit through the scratch (the per-tile ska_sort of :216-223), the tile x digit counts
 * come to the host, which plans equal-length block swaps in rounds (the reference plans them serially too, :235-239) and
 * a swap kernel runs them; then groups of buckets that fit the scratch are sorted by the ordinary device route, and a
 * bucket that does not fit takes another Regions level on the next digit.  BLOCKING (the plan is made on the host).
 * Same result as rdst_hip_sort_device, bit for bit. */
int rdst_hip_sort_device_lowmem(void* dev_keys, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind, uint32_t levels,
                                void* dev_tmp, uint64_t tmp_len, void* stream);

/* `partition_index` (src/sort_utils.rs:295-331: two-ended in-place partition by a predicate; Ska, Scanning and Regions
 * use it to move the largest bucket aside first) as a device operation: keys whose digit `level` equals `digit` first,
 * the others after, in place, with the same scratch and swap machinery (a two-country Regions level).  Returns the split
 * index in *split_out.  The order inside the two parts is unspecified, as in the reference.  BLOCKING. */
int rdst_hip_partition_device(void* dev_keys, uint64_t len, uint32_t elem_bytes, rdst_key_kind kind, uint32_t level,
                              uint32_t digit, void* dev_tmp, uint64_t tmp_len, uint64_t* split_out, void* stream);

/* The swap plan of one Regions level, host only (what rdst_hip_sort_device_lowmem runs; exposed so that it can be
 * checked without a device).  Every tile consists of `columns` runs, in order; tile_counts[t * columns + c] = length of
 * run c of tile t, col_bucket[c] = the bucket its keys belong to (NULL: column c is bucket c, columns == buckets);
 * tiles = ceil(len / tile_len).  ops_out[round_starts[r] .. round_starts[r + 1]) are the swaps of round r: exchange
 * `len` elements at `a` with those at `b`; the ranges of one round are pairwise disjoint.  starts_out (nullable,
 * buckets + 1 entries) receives the region borders. */
typedef struct { uint64_t a, b, len; } rdst_swap_op;
int rdst_regions_plan(const uint64_t* tile_counts, uint64_t tiles, uint64_t tile_len, uint64_t len, uint32_t columns,
                      const uint32_t* col_bucket, uint32_t buckets, rdst_swap_op* ops_out, uint64_t ops_capacity,
                      uint64_t* nops_out, uint64_t* round_starts, uint32_t max_rounds, uint32_t* nrounds_out,
                      uint64_t* starts_out);

/* Replaces `Tuner::pick_algorithm` (src/tuner.rs:33-35) for the stock tuners: pure
 * integer decision tables, host only.  counts has 256 entries (src/sorter.rs:67-76).
 * gpu_min_len is read only by RDST_TUNER_GPU.  For host slices the device route starts to win at
 * about 7·10^4 elements (pool allocation + PCIe both ways): RDST_GPU_MIN_LEN_HOST_SLICE. */
#define RDST_GPU_MIN_LEN_HOST_SLICE 65536u  /* measured break-even of rdst_hip_sort against the CPU route, see INTEGRATION.md */
int rdst_pick_algorithm(int tuner_id, const rdst_tuning_params* p, const uint64_t counts[256],
                        uint64_t gpu_min_len);

/* Bytes of device memory the workspace needs for a sort of `len` elements. */
uint64_t rdst_hip_workspace_bytes(uint64_t len, uint32_t elem_bytes);

/* The workspace is library-owned, one per device, grown on demand and kept between calls — the device twin of the
 * `tmp_bucket` the reference allocates and drops inside every sort (src/sorts/lsb_sort.rs:53, :126): for 10^9-key slices
 * it is 1.7 x the slice (the byte-saving routes' areas and slots).  This call gives it back (blocking: it waits for every
 * queued sort of the current device); the next sort allocates again.  If the allocation of a large workspace fails, the sort
 * takes the LSD route, whose workspace is an eighth of the slice, instead of failing. */
int rdst_hip_release_workspace(void);

/* Runtime knobs for experiments: pass_config selects the scatter-kernel shape (tile size and
 * LDS staging; negative = built-in default), hist_blocks_per_cu the histogram grid (<= 0 =
 * built-in).  Not part of the reference surface. */
int rdst_hip_set_tuning(int pass_config, int hist_blocks_per_cu);

/* Experiment knob: enabled == 0 makes every scatter pass use ONE look-back chain over all of its
 * tiles instead of splitting its source into segments with a chain each (default: split).
 * Results are identical either way.  Not part of the reference surface. */
int rdst_hip_set_chain_split(int enabled);

/* Experiment knob: enabled == 0 ranks every round of a scatter pass with wave ballots; the default
 * takes the slots a returning LDS add hands out and falls back to the ballots for any round whose
 * result fails the in-kernel order test (rdst_kernels.hip, step 5).  enabled == 2: self-test mode, every
 * round is treated as failed and redone (exercises the fallback).  Results are identical in all modes. */
int rdst_hip_set_fast_rank(int enabled);

/* Experiment knob: enabled == 0 sends slices of at most 64 KiB of keys through the general pipeline too,
 * instead of the one-workgroup LDS sort (the device twin of src/sorts/lsb_sort.rs:39-127).  Same results. */
int rdst_hip_set_small_sort(int enabled);

/* Per-kernel device timing for benchmarks.  While enabled, every pipeline (sort / hook call)
 * records HIP events on its own stream between its launches and appends one "run" to a
 * per-device list; enabling again clears the list.  rdst_hip_profile_run blocks until run
 * `run` (negative = counted from the most recent) has finished and writes the elapsed
 * milliseconds of its stages in launch order: [0] workspace clear, [1] multi-level histogram
 * (K1), [2] scan (K2), then one entry per scatter pass (K3) for the levels the call covered,
 * then the conditional copy-back if the call has one.  *n_out = entries written. */
int rdst_hip_set_profiling(int enabled);
int rdst_hip_profile_runs(void);
int rdst_hip_profile_run(int run, float* out_ms, uint32_t capacity, uint32_t* n_out);
/* The same run's stage codes, entry for entry (rdst_stage, a pass's level in bits 8..15): the hybrid route
 * inserts RDST_STAGE_HIST16 and RDST_STAGE_ROUTE after the clear and RDST_STAGE_LOCAL after the passes. */
int rdst_hip_profile_run_stages(int run, uint32_t* stages_out, uint32_t capacity, uint32_t* n_out);

/* Route choice.  Whole sorts of 4- and 8-byte keys with min_len <= len < 2^30 try routes that move fewer bytes than one
 * scatter pass per level — the device form of rdst's own MSD-then-Lsb route at this size (SURVEY.md §3.1;
 * src/tuners/standard_tuner.rs:46-62 picks by length and counts, too).  The device decides, in this order:
 *   ATOMIC — two MSD passes that claim space in over-provisioned areas with atomics (no counting read at all), then the
 *   in-LDS sort of every bucket; given up if an area or a slot overflows (keys far from uniform);
 *   HYBRID — K1h counts the top 16 bits exactly, two K3 passes, the in-LDS sort; 8-byte keys: if every bucket fits one tile,
 *   4-byte keys: buckets of any size (up to 4 096 of 65 536 keys and more);
 *   LSD — everything else.
 * enabled == 0: LSD route always; 1: the default above; 7: start at the hybrid route; 2 / 3 / 5 / 6 / 9: hybrid route for
 * every width with one detail changed, for A/B runs and tests — 2: ranked in-LDS sort for 4-byte keys as well, 3: pass L-1
 * hands K4 whole keys instead of 16-bit halves, 5: no key sample, 6: 8-byte keys with the one-block-per-CU form of K4, 9: no
 * expanding K4 (4-byte buckets up to one tile only); 8: the atomic route for 4-byte keys only; 10: a failed atomic route
 * falls straight to LSD; 11: no giant kernels; 12: no exact form of the MSD passes; 14: no prediction of the LSD route
 * from the sample; 15: the second form of the 8-byte K4; 16: no split of slices beyond the window; 17: that split at every
 * length, in eight parts.  min_len == 0 keeps the built-in thresholds (atomic route: 3 * 2^26 4-byte keys, 2^26 8-byte keys; K1h hybrid route: 2^28).  Results are identical
 * on every route.  Not part of the reference surface. */
int rdst_hip_set_hybrid(int enabled, uint64_t min_len);

/* Route the most recent sort enqueued by this library on the current device took (RDST_ROUTE_*).  Blocks on `stream`. */
int rdst_hip_last_route(void* stream, uint32_t* route_out);

/* Last error message of the calling thread ("" if none). */
const char* rdst_hip_last_error(void);

/* ABI version of the loaded library (RDST_HIP_ABI_VERSION at build time). */
int rdst_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RDST_HIP_H */
