// rdst.hpp — header-only C++ mirror of rdst's public surface for the device route.
//
// The reference is a Rust crate; where its toolchain is absent the host side above the C ABI
// (include/rdst_hip.h) is C++ with the reference's names, argument meaning and error behaviour:
//
//   rdst::radix_sort_unstable(v)                        RadixSort::radix_sort_unstable     src/radix_sort.rs:21-45
//   rdst::radix_sort_unstable_by_field(v, &T::key)      the same on structs keyed by a field benches/struct_sort.rs:11-27
//   rdst::sort_records_by(v, {RDST_FIELD(T, a, kind), ...})  `impl RadixKey for T` stated as a field table  src/radix_key.rs, examples/impl_radix_key.rs:32-56
//   rdst::sort_bytes_device_nowait<N>(rows, n, ...)     [u8; N] rows in device memory, asynchronous  src/radix_key_impl.rs:78-85
//   rdst::sort_records_by_device_nowait<T>(recs, n, {...}, ...)  the field table on device records, asynchronous  src/radix_key.rs
//   rdst::radix_sort_builder(v).with_*().sort()         RadixSortBuilder                   src/radix_sort_builder.rs:8-158
//   rdst::RadixKey<T>::LEVELS / kind                    RadixKey for the built-in types    src/radix_key_impl.rs:1-185
//   rdst::tuner::{Tuner, TuningParams, Algorithm, ...}  pub mod tuner                      src/tuner.rs:1-40, src/tuners/*.rs
//
// `v` is a std::vector<T> or a (T*, len) slice of a built-in key type.  Sorting is in place and
// blocking, like the reference.  The reference's `sort()` is infallible; this route can fail
// (no device, out of device memory, ...): on failure the slice is untouched and rdst::Error is
// thrown, so a caller can still run the reference's CPU path on the same data.  There is no CPU
// fallback inside this header — the CPU algorithms stay in the reference crate.
#ifndef RDST_HPP
#define RDST_HPP

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <array>
#include <vector>

#include "rdst_hip.h"

namespace rdst {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& what) : std::runtime_error(what), status(s) {}
};

namespace detail {
inline void check(int rc) {  // the status of a library call: anything but RDST_OK throws, with the library's own words
    if (rc != RDST_OK) throw Error(rc, rdst_hip_last_error());
}
}  // namespace detail

// RadixKey (src/radix_key.rs:1-5) for the built-in types whose mapping the device knows.
template <typename T, typename = void> struct RadixKey;  // not defined: no device mapping for T
template <typename T>
struct RadixKey<T, std::enable_if_t<std::is_integral_v<T> && !std::is_same_v<T, bool> && sizeof(T) <= 8>> {
    static constexpr std::size_t LEVELS = sizeof(T);
    static constexpr rdst_key_kind kind = std::is_signed_v<T> ? RDST_KEY_SIGNED : RDST_KEY_UNSIGNED;
};
template <> struct RadixKey<float> { static constexpr std::size_t LEVELS = 4; static constexpr rdst_key_kind kind = RDST_KEY_FLOAT; };
template <> struct RadixKey<double> { static constexpr std::size_t LEVELS = 8; static constexpr rdst_key_kind kind = RDST_KEY_FLOAT; };
template <std::size_t N>
struct RadixKey<std::array<std::uint8_t, N>, std::enable_if_t<(N >= 1 && N <= RDST_BYTES_MAX_N)>> {  // [u8; N], src/radix_key_impl.rs:78-85: lexicographic
    static constexpr std::size_t LEVELS = N;
    static constexpr rdst_key_kind kind = RDST_KEY_BYTES_BE;
};

namespace tuner {

enum class Algorithm : int {  // src/tuner.rs:12-22 + the device routes
    MtOop = RDST_ALGO_MT_OOP, MtLsb = RDST_ALGO_MT_LSB, Scanning = RDST_ALGO_SCANNING,
    Recombinating = RDST_ALGO_RECOMBINATING, Comparative = RDST_ALGO_COMPARATIVE, LrLsb = RDST_ALGO_LR_LSB,
    Lsb = RDST_ALGO_LSB, Regions = RDST_ALGO_REGIONS, Ska = RDST_ALGO_SKA,
    GpuLsd = RDST_ALGO_GPU_LSD, GpuSharded = RDST_ALGO_GPU_SHARDED
};

struct TuningParams {  // src/tuner.rs:2-8; parent_len < 0 encodes None
    std::size_t threads, level, total_levels, input_len;
    std::int64_t parent_len;
};

struct Tuner {  // src/tuner.rs:33-35
    virtual ~Tuner() = default;
    virtual Algorithm pick_algorithm(const TuningParams& p, const std::uint64_t (&counts)[256]) const = 0;
};

namespace detail {
inline Algorithm table(int id, const TuningParams& p, const std::uint64_t (&counts)[256], std::uint64_t gpu_min_len) {
    rdst_tuning_params c{p.threads, p.level, p.total_levels, p.input_len, p.parent_len};
    const int r = rdst_pick_algorithm(id, &c, counts, gpu_min_len);
    if (r < 0) throw Error(r, "rdst_pick_algorithm rejected its arguments");
    return static_cast<Algorithm>(r);
}
}  // namespace detail

struct StandardTuner : Tuner {  // src/tuners/standard_tuner.rs:10-64
    Algorithm pick_algorithm(const TuningParams& p, const std::uint64_t (&c)[256]) const override { return detail::table(RDST_TUNER_STANDARD, p, c, 0); }
};
struct LowMemoryTuner : Tuner {  // src/tuners/low_memory_tuner.rs:13-43
    Algorithm pick_algorithm(const TuningParams& p, const std::uint64_t (&c)[256]) const override { return detail::table(RDST_TUNER_LOW_MEMORY, p, c, 0); }
};
struct SingleThreadedTuner : Tuner {  // src/tuners/single_threaded_tuner.rs:13-43
    Algorithm pick_algorithm(const TuningParams& p, const std::uint64_t (&c)[256]) const override { return detail::table(RDST_TUNER_SINGLE_THREADED, p, c, 0); }
};
constexpr std::uint64_t kGpuMinLenHostSlice = RDST_GPU_MIN_LEN_HOST_SLICE;  // where a host slice is better off on the device
struct GpuTuner : Tuner {  // StandardTuner, except whole top-level slices of >= gpu_min_len elements go to the device
    std::uint64_t gpu_min_len = 0;
    explicit GpuTuner(std::uint64_t min_len = 0) : gpu_min_len(min_len) {}
    Algorithm pick_algorithm(const TuningParams& p, const std::uint64_t (&c)[256]) const override { return detail::table(RDST_TUNER_GPU, p, c, gpu_min_len); }
};

}  // namespace tuner

template <typename T>
class RadixSortBuilder {  // src/radix_sort_builder.rs:8-158
    T* data_;
    std::size_t len_;
    bool multi_threaded_ = true;          // accepted for source compatibility; the device route has no use for it
    bool device_default_ = true;          // no tuner chosen: the slice goes to the device
    bool low_memory_ = false;             // with_low_mem_tuner(): the device's low-memory route
    const tuner::Tuner* tuner_ = nullptr;

   public:
    RadixSortBuilder(T* data, std::size_t len) : data_(data), len_(len) {
        static_assert(RadixKey<T>::LEVELS != 0, "RadixKey must have at least 1 level");  // radix_sort_builder.rs:22
    }
    RadixSortBuilder& with_parallel(bool parallel) { multi_threaded_ = parallel; return *this; }
    RadixSortBuilder& with_tuner(const tuner::Tuner* t) { tuner_ = t; device_default_ = false; low_memory_ = false; return *this; }  // the last with_*tuner call wins (radix_sort_builder.rs:53-147)
    // with_low_mem_tuner (src/radix_sort_builder.rs:74-77) trades speed for memory in the reference (Ska / Regions instead of
    // the out-of-place sorts): so does the device route — the keys and a scratch of len / 64 elements instead of two arrays
    // (rdst_hip_sort_device_lowmem behind rdst_hip_opts::low_memory).  with_single_threaded_tuner selects among the
    // reference's CPU algorithms, which are not shipped here: like a user tuner that answers with a CPU algorithm, sort() throws.
    RadixSortBuilder& with_low_mem_tuner() { low_memory_ = true; tuner_ = nullptr; device_default_ = true; return *this; }
    RadixSortBuilder& with_single_threaded_tuner() { static const tuner::SingleThreadedTuner t; return with_tuner(&t); }

    void sort() {
        if (len_ <= 1) return;  // radix_sort_builder.rs:151
        if (!device_default_) {
            // Sorter::handle_chunk hands the tuner the top-level histogram (src/sorter.rs:67-76);
            // a host-side count of one level is cheap next to the transfer that follows.
            std::uint64_t counts[256] = {};
            const int top = static_cast<int>(RadixKey<T>::LEVELS) - 1;
            for (std::size_t i = 0; i < len_; ++i) ++counts[top_digit(data_[i], top)];
            const tuner::TuningParams p{1, static_cast<std::size_t>(top), RadixKey<T>::LEVELS, len_, -1};
            const auto a = tuner_->pick_algorithm(p, counts);
            if (a != tuner::Algorithm::GpuLsd && a != tuner::Algorithm::GpuSharded)
                throw Error(RDST_ERR_UNSUPPORTED, "tuner picked a CPU algorithm: those stay in the reference crate; this header ships the device route only");
        }
        rdst_hip_opts opts{-1, low_memory_ ? 1 : 0, 0};
        detail::check(rdst_hip_sort(data_, len_, sizeof(T), RadixKey<T>::kind, RadixKey<T>::LEVELS, &opts));
    }

   private:
    static std::uint8_t top_digit(const T& v, int level) {  // RadixKey::get_level (src/radix_key_impl.rs)
        if constexpr (RadixKey<T>::kind == RDST_KEY_BYTES_BE) {
            return reinterpret_cast<const std::uint8_t*>(&v)[RadixKey<T>::LEVELS - 1 - static_cast<std::size_t>(level)];
        } else {
        using U = std::conditional_t<sizeof(T) == 1, std::uint8_t, std::conditional_t<sizeof(T) == 2, std::uint16_t,
                  std::conditional_t<sizeof(T) == 4, std::uint32_t, std::uint64_t>>>;
        U u;
        __builtin_memcpy(&u, &v, sizeof u);
        constexpr U msb = U(U(1) << (sizeof(U) * 8 - 1));
        if (RadixKey<T>::kind == RDST_KEY_SIGNED) u = U(u ^ msb);
        else if (RadixKey<T>::kind == RDST_KEY_FLOAT) u = U(u ^ ((u & msb) ? U(~U(0)) : msb));
        return static_cast<std::uint8_t>(u >> (level * 8));
        }
    }
};

template <typename T> RadixSortBuilder<T> radix_sort_builder(std::vector<T>& v) { return RadixSortBuilder<T>(v.data(), v.size()); }
template <typename T> RadixSortBuilder<T> radix_sort_builder(T* data, std::size_t len) { return RadixSortBuilder<T>(data, len); }
template <typename T> void radix_sort_unstable(std::vector<T>& v) { radix_sort_builder(v).sort(); }
template <typename T> void radix_sort_unstable(T* data, std::size_t len) { radix_sort_builder(data, len).sort(); }

// A slice of structs whose key is one built-in field — what `impl RadixKey for LargeStruct` with
// `get_level` = the field's expresses in the reference (benches/struct_sort.rs:11-27,
// examples/impl_radix_key.rs:32-56).  Rows with equal keys keep their order.  The field is a 4- or 8-byte built-in
// key, or a std::array<std::uint8_t, N> (a [u8; N] key, N up to RDST_BYTES_MAX_N, at any offset).
template <typename T, typename KeyT>
void radix_sort_unstable_by_field(T* data, std::size_t len, KeyT T::*field) {
    static_assert(std::is_trivially_copyable<T>::value, "rows are moved as bytes");
    static_assert(RadixKey<KeyT>::kind == RDST_KEY_BYTES_BE || sizeof(KeyT) == 4 || sizeof(KeyT) == 8,
                  "the device route takes 4- or 8-byte key fields and [u8; N] fields");
    if (len <= 1) return;
    const std::size_t offset = static_cast<std::size_t>(reinterpret_cast<const char*>(&(data[0].*field)) - reinterpret_cast<const char*>(&data[0]));
    detail::check(rdst_hip_sort_records(data, len, sizeof(T), static_cast<std::uint32_t>(offset), sizeof(KeyT), RadixKey<KeyT>::kind, nullptr));
}
template <typename T, typename KeyT>
void radix_sort_unstable_by_field(std::vector<T>& v, KeyT T::*field) { radix_sort_unstable_by_field(v.data(), v.size(), field); }

// A slice of structs ordered by a described key: what `impl RadixKey for T` states with LEVELS and get_level
// (src/radix_key.rs; examples/impl_radix_key.rs:32-56), as a table of fields, most significant first — several fields,
// any built-in width (u8..i128, f32, f64, [u8; N]), any offset (packed structs), descending fields, chosen bytes.  Rows
// with equal keys keep their order (rdst_hip_sort_records_by_fields).
//     struct Event { std::uint16_t tenant; std::int64_t ts; ... };
//     rdst::sort_records_by(v, {RDST_FIELD(Event, tenant, RDST_KEY_UNSIGNED), RDST_FIELD(Event, ts, RDST_KEY_SIGNED)});
#define RDST_FIELD(T, member, kind) \
    rdst_key_field { static_cast<std::uint32_t>(offsetof(T, member)), static_cast<std::uint32_t>(sizeof(static_cast<T*>(nullptr)->member)), static_cast<std::uint32_t>(kind), 0u }
#define RDST_FIELD_DESC(T, member, kind) \
    rdst_key_field { static_cast<std::uint32_t>(offsetof(T, member)), static_cast<std::uint32_t>(sizeof(static_cast<T*>(nullptr)->member)), static_cast<std::uint32_t>(kind), RDST_FIELD_DESCENDING }
template <typename T>
void sort_records_by(T* data, std::size_t n, std::initializer_list<rdst_key_field> fields) {
    static_assert(std::is_trivially_copyable<T>::value, "rows are moved as bytes");
    detail::check(rdst_hip_sort_records_by_fields(data, n, sizeof(T), fields.begin(), static_cast<std::uint32_t>(fields.size()), nullptr));
}
template <typename T>
void sort_records_by(std::vector<T>& v, std::initializer_list<rdst_key_field> fields) { sort_records_by(v.data(), v.size(), fields); }

// Many independent slices of one DEVICE-resident array in one call: segment s is [offsets[s], offsets[s + 1]) (host
// table of n_segments + 1 non-decreasing indices), each sorted as radix_sort_unstable would sort it
// (rdst_hip_sort_segments_device).  dev_tmp / tmp_elems: scratch for segments longer than the block class
// (rdst_hip_sort_segments_limits), at least as long as the longest of them; may be null / 0 when there is none.
// Asynchronous on `stream`; failures of the kernels surface in rdst_hip_device_status.
template <typename T>
void sort_segments(T* dev_keys, std::size_t len, const std::uint64_t* offsets, std::size_t n_segments, T* dev_tmp = nullptr,
                   std::size_t tmp_elems = 0, void* stream = nullptr) {
    detail::check(rdst_hip_sort_segments_device(dev_keys, dev_tmp, tmp_elems, len, offsets, n_segments, sizeof(T), RadixKey<T>::kind,
                                                static_cast<std::uint32_t>(RadixKey<T>::LEVELS), stream));
}

// The same with the table of borders in DEVICE memory (rdst_hip_sort_segments_device_offsets): dev_offsets holds
// n_segments + 1 entries of the unsigned type Off (std::uint32_t or std::uint64_t), read in stream order.  dev_scratch:
// at least segments_device_offsets_scratch_bytes(n_segments) bytes, 256-byte aligned.  tmp_elems == 0: fully asynchronous —
// an invalid table or a segment beyond the block class leaves the keys untouched and surfaces in rdst_hip_device_status;
// tmp_elems > 0: longer segments are sorted too, and the call waits once for `stream` to read the plan's counts.
inline std::size_t segments_device_offsets_scratch_bytes(std::size_t n_segments) {
    return static_cast<std::size_t>(rdst_hip_sort_segments_device_offsets_scratch_bytes(n_segments));
}
template <typename T, typename Off>
void sort_segments_device_offsets(T* dev_keys, std::size_t len, const Off* dev_offsets, std::size_t n_segments, void* dev_scratch,
                                  std::size_t scratch_bytes, T* dev_tmp = nullptr, std::size_t tmp_elems = 0, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "offsets are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_sort_segments_device_offsets(dev_keys, dev_tmp, tmp_elems, len, dev_offsets, sizeof(Off), n_segments, sizeof(T),
                                                        RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS), dev_scratch,
                                                        scratch_bytes, stream));
}
// Key-value form (rdst_hip_sort_segments_pairs_device_offsets): 4- or 8-byte keys and values; equal keys keep their order.
template <typename T, typename V, typename Off>
void sort_segments_pairs_device_offsets(T* dev_keys, V* dev_vals, std::size_t len, const Off* dev_offsets, std::size_t n_segments,
                                        void* dev_scratch, std::size_t scratch_bytes, T* dev_tmp_keys = nullptr, V* dev_tmp_vals = nullptr,
                                        std::size_t tmp_elems = 0, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "offsets are 4- or 8-byte unsigned integers");
    static_assert(std::is_trivially_copyable<V>::value, "values are moved as bytes");
    detail::check(rdst_hip_sort_segments_pairs_device_offsets(dev_keys, dev_vals, dev_tmp_keys, dev_tmp_vals, tmp_elems, len, dev_offsets,
                                                              sizeof(Off), n_segments, sizeof(T), RadixKey<T>::kind,
                                                              static_cast<std::uint32_t>(RadixKey<T>::LEVELS), sizeof(V), dev_scratch,
                                                              scratch_bytes, stream));
}

// Device offsets with no host involvement for segments of ANY length (rdst_hip_sort_segments_device_offsets_nowait): segments
// beyond the block class are sorted on the device too, tile by tile between the keys and dev_tmp, which holds `len` elements
// (only the positions of such segments are written).  Nothing is copied to the host and nothing waited for; an invalid table
// leaves keys, values and tmp untouched and surfaces in rdst_hip_device_status.  dev_scratch: at least
// segments_nowait_scratch_bytes<T>(n_segments, len) bytes (pairs: <T, V>), 256-byte aligned.  len must be below 2^32.
template <typename T>
std::size_t segments_nowait_scratch_bytes(std::size_t n_segments, std::size_t len) {
    return static_cast<std::size_t>(rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(n_segments, len, sizeof(T), 0));
}
template <typename T, typename V>
std::size_t segments_nowait_scratch_bytes(std::size_t n_segments, std::size_t len) {
    return static_cast<std::size_t>(rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(n_segments, len, sizeof(T), sizeof(V)));
}
template <typename T, typename Off>
void sort_segments_device_offsets_nowait(T* dev_keys, T* dev_tmp, std::size_t len, const Off* dev_offsets, std::size_t n_segments,
                                         void* dev_scratch, std::size_t scratch_bytes, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "offsets are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_sort_segments_device_offsets_nowait(dev_keys, dev_tmp, len, dev_offsets, sizeof(Off), n_segments, sizeof(T),
                                                               RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS), dev_scratch,
                                                               scratch_bytes, stream));
}
// Key-value form (rdst_hip_sort_segments_pairs_device_offsets_nowait): 4- or 8-byte keys and values; equal keys keep their order.
template <typename T, typename V, typename Off>
void sort_segments_device_offsets_nowait(T* dev_keys, V* dev_vals, T* dev_tmp_keys, V* dev_tmp_vals, std::size_t len, const Off* dev_offsets,
                                         std::size_t n_segments, void* dev_scratch, std::size_t scratch_bytes, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "offsets are 4- or 8-byte unsigned integers");
    static_assert(std::is_trivially_copyable<V>::value, "values are moved as bytes");
    detail::check(rdst_hip_sort_segments_pairs_device_offsets_nowait(dev_keys, dev_vals, dev_tmp_keys, dev_tmp_vals, len, dev_offsets, sizeof(Off),
                                                                     n_segments, sizeof(T), RadixKey<T>::kind,
                                                                     static_cast<std::uint32_t>(RadixKey<T>::LEVELS), sizeof(V), dev_scratch,
                                                                     scratch_bytes, stream));
}

// One DEVICE-resident slice whose length lives in device memory too (rdst_hip_sort_device_devlen): the first *dev_len of
// `capacity` keys are sorted as radix_sort_unstable would sort them, the rest is not touched.  dev_len: one value of the
// unsigned type Len (std::uint32_t or std::uint64_t), read in stream order — the kernel that counts may still be running —
// and never by the host.  dev_tmp holds `capacity` keys.  Nothing is copied to the host and nothing waited for; a length
// past the capacity changes nothing and surfaces in rdst_hip_device_status (error bit 32).  `stream` is a hipStream_t.
template <typename T, typename Len>
void sort_device_devlen(T* dev_keys, T* dev_tmp, std::size_t capacity, const Len* dev_len, void* stream = nullptr) {
    static_assert(std::is_unsigned<Len>::value && (sizeof(Len) == 4 || sizeof(Len) == 8), "the length is a 4- or 8-byte unsigned integer");
    detail::check(rdst_hip_sort_device_devlen(dev_keys, dev_tmp, capacity, dev_len, sizeof(Len), sizeof(T), RadixKey<T>::kind,
                                              static_cast<std::uint32_t>(RadixKey<T>::LEVELS), stream));
}
// Key-value form (rdst_hip_sort_pairs_device_devlen): 4- or 8-byte keys and values; equal keys keep their order.
template <typename T, typename V, typename Len>
void sort_pairs_device_devlen(T* dev_keys, V* dev_vals, T* dev_tmp_keys, V* dev_tmp_vals, std::size_t capacity, const Len* dev_len,
                              void* stream = nullptr) {
    static_assert(std::is_unsigned<Len>::value && (sizeof(Len) == 4 || sizeof(Len) == 8), "the length is a 4- or 8-byte unsigned integer");
    static_assert(std::is_trivially_copyable<V>::value, "values are moved as bytes");
    detail::check(rdst_hip_sort_pairs_device_devlen(dev_keys, dev_vals, dev_tmp_keys, dev_tmp_vals, capacity, dev_len, sizeof(Len), sizeof(T),
                                                    RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS), sizeof(V), stream));
}

// Partial sort of one DEVICE-resident slice (rdst_hip_topk_device): dev_out_keys[0..k) receives the k keys that
// radix_sort_unstable would put first — `largest`: last, in descending order —, in that order; dev_keys is only read.  The
// second form also writes the input position of every output key to dev_out_index (Idx: std::uint32_t or std::uint64_t;
// 4- and 8-byte keys): equal keys in ascending position, the lowest positions winning a tie at the k-th key.  dev_scratch:
// 256-byte aligned, at least topk_scratch_bytes<T>(len, k) / topk_scratch_bytes<T, Idx>(len, k) bytes.  cand_capacity: 0 =
// the library's default; any value gives the same result.  Nothing is copied to the host and nothing waited for.
template <typename T>
std::size_t topk_scratch_bytes(std::size_t len, std::size_t k, std::size_t cand_capacity = 0) {
    return rdst_hip_topk_scratch_bytes(len, k, sizeof(T), 0, cand_capacity);
}
template <typename T, typename Idx>
std::size_t topk_scratch_bytes(std::size_t len, std::size_t k, std::size_t cand_capacity = 0) {
    return rdst_hip_topk_scratch_bytes(len, k, sizeof(T), sizeof(Idx), cand_capacity);
}
template <typename T>
void topk_device(const T* dev_keys, std::size_t len, std::size_t k, T* dev_out_keys, void* dev_scratch, std::size_t scratch_bytes,
                 bool largest = false, std::size_t cand_capacity = 0, void* stream = nullptr) {
    detail::check(rdst_hip_topk_device(dev_keys, len, k, dev_out_keys, nullptr, 0, dev_scratch, scratch_bytes, cand_capacity, sizeof(T),
                                       RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS), largest ? RDST_TOPK_LARGEST : 0u, stream));
}
template <typename T, typename Idx>
void topk_device(const T* dev_keys, std::size_t len, std::size_t k, T* dev_out_keys, Idx* dev_out_index, void* dev_scratch,
                 std::size_t scratch_bytes, bool largest = false, std::size_t cand_capacity = 0, void* stream = nullptr) {
    static_assert(std::is_unsigned<Idx>::value && (sizeof(Idx) == 4 || sizeof(Idx) == 8), "positions are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_topk_device(dev_keys, len, k, dev_out_keys, dev_out_index, sizeof(Idx), dev_scratch, scratch_bytes, cand_capacity,
                                       sizeof(T), RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS),
                                       largest ? RDST_TOPK_LARGEST : 0u, stream));
}

// Order statistics of one DEVICE-resident slice (rdst_hip_select_device): dev_out_keys[i] receives the key that
// radix_sort_unstable would leave at position ranks[i] — `largest`: at len - 1 - ranks[i] —; dev_keys is only read.  ranks: a
// HOST array, any order, repeats allowed.  The second form also writes the input position of that element of a stable
// argsort to dev_out_index[i] (Idx: std::uint32_t or std::uint64_t; 4- and 8-byte keys).  dev_scratch: 256-byte aligned, at
// least select_scratch_bytes<T>(len, n_ranks) / select_scratch_bytes<T, Idx>(len, n_ranks) bytes, never len-sized.
// cand_capacity: 0 = the library's default; any value gives the same result.  Nothing is copied to the host and nothing
// waited for.
template <typename T>
std::size_t select_scratch_bytes(std::size_t len, std::size_t n_ranks, std::size_t cand_capacity = 0) {
    return rdst_hip_select_scratch_bytes(len, n_ranks, sizeof(T), 0, cand_capacity);
}
template <typename T, typename Idx>
std::size_t select_scratch_bytes(std::size_t len, std::size_t n_ranks, std::size_t cand_capacity = 0) {
    return rdst_hip_select_scratch_bytes(len, n_ranks, sizeof(T), sizeof(Idx), cand_capacity);
}
template <typename T>
void select_device(const T* dev_keys, std::size_t len, const std::uint64_t* ranks, std::size_t n_ranks, T* dev_out_keys, void* dev_scratch,
                   std::size_t scratch_bytes, bool largest = false, std::size_t cand_capacity = 0, void* stream = nullptr) {
    detail::check(rdst_hip_select_device(dev_keys, len, ranks, n_ranks, dev_out_keys, nullptr, 0, dev_scratch, scratch_bytes, cand_capacity, sizeof(T),
                                         RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS), largest ? RDST_TOPK_LARGEST : 0u, stream));
}
template <typename T, typename Idx>
void select_device(const T* dev_keys, std::size_t len, const std::uint64_t* ranks, std::size_t n_ranks, T* dev_out_keys, Idx* dev_out_index,
                   void* dev_scratch, std::size_t scratch_bytes, bool largest = false, std::size_t cand_capacity = 0, void* stream = nullptr) {
    static_assert(std::is_unsigned<Idx>::value && (sizeof(Idx) == 4 || sizeof(Idx) == 8), "positions are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_select_device(dev_keys, len, ranks, n_ranks, dev_out_keys, dev_out_index, sizeof(Idx), dev_scratch, scratch_bytes,
                                         cand_capacity, sizeof(T), RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS),
                                         largest ? RDST_TOPK_LARGEST : 0u, stream));
}

// Partial sort of every segment [offsets[s], offsets[s + 1]) of one DEVICE-resident slice (rdst_hip_topk_segments_device):
// row s of the outputs, dev_out_keys + s * k (and dev_out_index + s * k), receives in its first min(k, n_s) slots what
// topk_device gives for that segment, positions counted inside the segment; the slots behind are not written.  offsets: a
// HOST array of n_segments + 1 non-decreasing element indices, read before the call returns.  dev_scratch: 256-byte aligned,
// at least topk_segments_scratch_bytes<T>(n_segments, longest segment, k) / <T, Idx>(...) bytes.  Asynchronous as
// sort_segments_device is.
template <typename T>
std::size_t topk_segments_scratch_bytes(std::size_t n_segments, std::size_t longest_segment, std::size_t k) {
    return rdst_hip_topk_segments_scratch_bytes(n_segments, longest_segment, k, sizeof(T), 0);
}
template <typename T, typename Idx>
std::size_t topk_segments_scratch_bytes(std::size_t n_segments, std::size_t longest_segment, std::size_t k) {
    return rdst_hip_topk_segments_scratch_bytes(n_segments, longest_segment, k, sizeof(T), sizeof(Idx));
}
template <typename T>
void topk_segments(const T* dev_keys, std::size_t len, const std::uint64_t* offsets, std::size_t n_segments, std::size_t k, T* dev_out_keys,
                   void* dev_scratch, std::size_t scratch_bytes, bool largest = false, void* stream = nullptr) {
    detail::check(rdst_hip_topk_segments_device(dev_keys, len, offsets, n_segments, k, dev_out_keys, nullptr, 0, dev_scratch, scratch_bytes, sizeof(T),
                                                RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS),
                                                largest ? RDST_TOPK_LARGEST : 0u, stream));
}
template <typename T, typename Idx>
void topk_segments(const T* dev_keys, std::size_t len, const std::uint64_t* offsets, std::size_t n_segments, std::size_t k, T* dev_out_keys,
                   Idx* dev_out_index, void* dev_scratch, std::size_t scratch_bytes, bool largest = false, void* stream = nullptr) {
    static_assert(std::is_unsigned<Idx>::value && (sizeof(Idx) == 4 || sizeof(Idx) == 8), "positions are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_topk_segments_device(dev_keys, len, offsets, n_segments, k, dev_out_keys, dev_out_index, sizeof(Idx), dev_scratch,
                                                scratch_bytes, sizeof(T), RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS),
                                                largest ? RDST_TOPK_LARGEST : 0u, stream));
}

// Order statistics of every segment [offsets[s], offsets[s + 1]) of one DEVICE-resident slice
// (rdst_hip_select_segments_device): slot i of row s of the outputs, dev_out_keys + s * n_ranks (and dev_out_index +
// s * n_ranks), receives what select_device gives for that segment at the rank ranks[i] stands for in a segment of its length
// (rank_for_length; rank_at / rank_quantile make a spec), positions counted inside the segment.  A slot whose spec the segment
// has no element for — an empty segment, an absolute rank at or past its length — is not written.  offsets and ranks: HOST
// arrays, read before the call returns.  dev_scratch: 256-byte aligned, at least select_segments_scratch_bytes<T>(n_segments,
// longest segment, n_ranks) / <T, Idx>(...) bytes.  Asynchronous as topk_segments is.
inline rdst_rank_spec rank_at(std::uint32_t rank) { return rdst_rank_spec{rank, 0u, RDST_RANK_LOWER, 0u}; }
inline rdst_rank_spec rank_quantile(std::uint32_t num, std::uint32_t den, std::uint32_t mode = RDST_RANK_LOWER) {
    return rdst_rank_spec{num, den, mode, 0u};
}
// the rank `spec` stands for in a segment of n keys; false: none (an empty segment, an absolute rank >= n)
inline bool rank_for_length(const rdst_rank_spec& spec, std::uint64_t n, std::uint64_t* rank_out) {
    const int rc = rdst_rank_for_length(&spec, n, rank_out);
    if (rc < 0) detail::check(rc);
    return rc == 1;
}
template <typename T>
std::size_t select_segments_scratch_bytes(std::size_t n_segments, std::size_t longest_segment, std::size_t n_ranks) {
    return rdst_hip_select_segments_scratch_bytes(n_segments, longest_segment, n_ranks, sizeof(T), 0);
}
template <typename T, typename Idx>
std::size_t select_segments_scratch_bytes(std::size_t n_segments, std::size_t longest_segment, std::size_t n_ranks) {
    return rdst_hip_select_segments_scratch_bytes(n_segments, longest_segment, n_ranks, sizeof(T), sizeof(Idx));
}
template <typename T>
void select_segments(const T* dev_keys, std::size_t len, const std::uint64_t* offsets, std::size_t n_segments, const rdst_rank_spec* ranks,
                     std::size_t n_ranks, T* dev_out_keys, void* dev_scratch, std::size_t scratch_bytes, bool largest = false, void* stream = nullptr) {
    detail::check(rdst_hip_select_segments_device(dev_keys, len, offsets, n_segments, ranks, n_ranks, dev_out_keys, nullptr, 0, dev_scratch, scratch_bytes,
                                                  sizeof(T), RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS),
                                                  largest ? RDST_TOPK_LARGEST : 0u, stream));
}
template <typename T, typename Idx>
void select_segments(const T* dev_keys, std::size_t len, const std::uint64_t* offsets, std::size_t n_segments, const rdst_rank_spec* ranks,
                     std::size_t n_ranks, T* dev_out_keys, Idx* dev_out_index, void* dev_scratch, std::size_t scratch_bytes, bool largest = false,
                     void* stream = nullptr) {
    static_assert(std::is_unsigned<Idx>::value && (sizeof(Idx) == 4 || sizeof(Idx) == 8), "positions are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_select_segments_device(dev_keys, len, offsets, n_segments, ranks, n_ranks, dev_out_keys, dev_out_index, sizeof(Idx), dev_scratch,
                                                  scratch_bytes, sizeof(T), RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS),
                                                  largest ? RDST_TOPK_LARGEST : 0u, stream));
}

// topk_segments with the table of borders in DEVICE memory (rdst_hip_topk_segments_device_offsets): dev_offsets holds
// n_segments + 1 borders of type Off (a 4- or 8-byte unsigned integer), read in stream order.  far_capacity == 0: fully
// asynchronous — no copy to the host, no wait; every segment beyond block_max is served by ONE workgroup whatever its length (a
// performance cliff for very long rows, never a wrong answer), and a k beyond k_stream_max with such a segment, or an invalid
// table, writes nothing and raises bit 0x10 of the device error word.  far_capacity > 0 (the longest segment the call may
// meet; len if nothing better is known): the classes of topk_segments, one wait for the stream, an invalid table or a longer
// far segment throws.  dev_scratch: 256-byte aligned, at least topk_segments_device_offsets_scratch_bytes<T>(n_segments,
// far_capacity, k) / <T, Idx>(...) bytes.
template <typename T>
std::size_t topk_segments_device_offsets_scratch_bytes(std::size_t n_segments, std::size_t far_capacity, std::size_t k) {
    return rdst_hip_topk_segments_device_offsets_scratch_bytes(n_segments, far_capacity, k, sizeof(T), 0);
}
template <typename T, typename Idx>
std::size_t topk_segments_device_offsets_scratch_bytes(std::size_t n_segments, std::size_t far_capacity, std::size_t k) {
    return rdst_hip_topk_segments_device_offsets_scratch_bytes(n_segments, far_capacity, k, sizeof(T), sizeof(Idx));
}
template <typename T, typename Off>
void topk_segments_device_offsets(const T* dev_keys, std::size_t len, const Off* dev_offsets, std::size_t n_segments, std::size_t k,
                                  T* dev_out_keys, void* dev_scratch, std::size_t scratch_bytes, std::size_t far_capacity = 0,
                                  bool largest = false, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "borders are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_topk_segments_device_offsets(dev_keys, len, dev_offsets, sizeof(Off), n_segments, k, dev_out_keys, nullptr, 0, dev_scratch,
                                                        scratch_bytes, far_capacity, sizeof(T), RadixKey<T>::kind,
                                                        static_cast<std::uint32_t>(RadixKey<T>::LEVELS), largest ? RDST_TOPK_LARGEST : 0u, stream));
}
template <typename T, typename Off, typename Idx>
void topk_segments_device_offsets(const T* dev_keys, std::size_t len, const Off* dev_offsets, std::size_t n_segments, std::size_t k,
                                  T* dev_out_keys, Idx* dev_out_index, void* dev_scratch, std::size_t scratch_bytes, std::size_t far_capacity = 0,
                                  bool largest = false, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "borders are 4- or 8-byte unsigned integers");
    static_assert(std::is_unsigned<Idx>::value && (sizeof(Idx) == 4 || sizeof(Idx) == 8), "positions are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_topk_segments_device_offsets(dev_keys, len, dev_offsets, sizeof(Off), n_segments, k, dev_out_keys, dev_out_index, sizeof(Idx),
                                                        dev_scratch, scratch_bytes, far_capacity, sizeof(T), RadixKey<T>::kind,
                                                        static_cast<std::uint32_t>(RadixKey<T>::LEVELS), largest ? RDST_TOPK_LARGEST : 0u, stream));
}

// select_segments with the table of borders in DEVICE memory (rdst_hip_select_segments_device_offsets): dev_offsets holds
// n_segments + 1 borders of type Off (a 4- or 8-byte unsigned integer), read in stream order; ranks stays a HOST array.
// far_capacity == 0: fully asynchronous — no copy to the host, no wait; every segment beyond block_max is served by ONE
// workgroup whatever its length (a performance cliff for very long rows, steeper than topk's, never a wrong answer), and only
// an invalid table can fail: it writes nothing and raises bit 0x10 of the device error word.  far_capacity > 0 (the longest
// segment the call may meet; len if nothing better is known): the classes of select_segments, one wait for the stream, an
// invalid table or a longer far segment throws.  dev_scratch: 256-byte aligned, at least
// select_segments_device_offsets_scratch_bytes<T>(n_segments, far_capacity, n_ranks) / <T, Idx>(...) bytes.
template <typename T>
std::size_t select_segments_device_offsets_scratch_bytes(std::size_t n_segments, std::size_t far_capacity, std::size_t n_ranks) {
    return rdst_hip_select_segments_device_offsets_scratch_bytes(n_segments, far_capacity, n_ranks, sizeof(T), 0);
}
template <typename T, typename Idx>
std::size_t select_segments_device_offsets_scratch_bytes(std::size_t n_segments, std::size_t far_capacity, std::size_t n_ranks) {
    return rdst_hip_select_segments_device_offsets_scratch_bytes(n_segments, far_capacity, n_ranks, sizeof(T), sizeof(Idx));
}
template <typename T, typename Off>
void select_segments_device_offsets(const T* dev_keys, std::size_t len, const Off* dev_offsets, std::size_t n_segments, const rdst_rank_spec* ranks,
                                    std::size_t n_ranks, T* dev_out_keys, void* dev_scratch, std::size_t scratch_bytes, std::size_t far_capacity = 0,
                                    bool largest = false, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "borders are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_select_segments_device_offsets(dev_keys, len, dev_offsets, sizeof(Off), n_segments, ranks, n_ranks, dev_out_keys, nullptr, 0,
                                                          dev_scratch, scratch_bytes, far_capacity, sizeof(T), RadixKey<T>::kind,
                                                          static_cast<std::uint32_t>(RadixKey<T>::LEVELS), largest ? RDST_TOPK_LARGEST : 0u, stream));
}
template <typename T, typename Off, typename Idx>
void select_segments_device_offsets(const T* dev_keys, std::size_t len, const Off* dev_offsets, std::size_t n_segments, const rdst_rank_spec* ranks,
                                    std::size_t n_ranks, T* dev_out_keys, Idx* dev_out_index, void* dev_scratch, std::size_t scratch_bytes,
                                    std::size_t far_capacity = 0, bool largest = false, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "borders are 4- or 8-byte unsigned integers");
    static_assert(std::is_unsigned<Idx>::value && (sizeof(Idx) == 4 || sizeof(Idx) == 8), "positions are 4- or 8-byte unsigned integers");
    detail::check(rdst_hip_select_segments_device_offsets(dev_keys, len, dev_offsets, sizeof(Off), n_segments, ranks, n_ranks, dev_out_keys, dev_out_index,
                                                          sizeof(Idx), dev_scratch, scratch_bytes, far_capacity, sizeof(T), RadixKey<T>::kind,
                                                          static_cast<std::uint32_t>(RadixKey<T>::LEVELS), largest ? RDST_TOPK_LARGEST : 0u, stream));
}

// Runs of bit-identical keys (rdst_hip_runs_device): `v.dedup()` on the device, and the CSR table of the groups of sorted
// keys.  dev_out_keys: out_capacity keys or nullptr; dev_out_starts: out_capacity + 1 borders of type Off (a 4- or 8-byte
// unsigned integer) or nullptr; dev_n_runs: one Off, the true number of runs R.  starts[0 .. R] is a table every
// *_device_offsets entry takes (starts[R] = the length); with pad_starts the slots behind R hold the length too, so that
// n_segments = out_capacity needs no look at R.  dev_len: nullptr, or the length in device memory (a 4- or 8-byte unsigned
// integer, read in stream order).  More runs than out_capacity (> 0): the first out_capacity are complete and bit 0x40 of the
// device error word is raised; out_capacity == 0 only counts.  Fully asynchronous: no copy to the host, no wait.  dev_scratch:
// 256-byte aligned, at least runs_scratch_bytes<T>(len) bytes.
template <typename T>
std::size_t runs_scratch_bytes(std::size_t len) {
    return rdst_hip_runs_scratch_bytes(len, sizeof(T));
}
template <typename T, typename Off, typename Len = std::uint64_t>
void runs_device(const T* dev_keys, std::size_t len, T* dev_out_keys, Off* dev_out_starts, Off* dev_n_runs, std::size_t out_capacity, void* dev_scratch,
                 std::size_t scratch_bytes, bool pad_starts = false, const Len* dev_len = nullptr, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "borders are 4- or 8-byte unsigned integers");
    static_assert(std::is_unsigned<Len>::value && (sizeof(Len) == 4 || sizeof(Len) == 8), "a device-resident length is a 4- or 8-byte unsigned integer");
    detail::check(rdst_hip_runs_device(dev_keys, len, dev_len, sizeof(Len), dev_out_keys, dev_out_starts, dev_n_runs, sizeof(Off), out_capacity, dev_scratch,
                                       scratch_bytes, sizeof(T), RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS),
                                       pad_starts ? RDST_RUNS_PAD_STARTS : 0u, stream));
}

// Binary search (rdst_hip_search_device): `partition_point` for many needles at once.  For every i < n_needles, lower[i] = the
// number of keys of dev_sorted[0 .. m) that order strictly before dev_needles[i] and upper[i] = the number that order before
// or equal it, in the sort's order (the mapped bits: -0.0 < +0.0, NaNs by their bits); Off is a 4- or 8-byte unsigned
// integer, either output may be nullptr.  m is len, or the value dev_len points to (a 4- or 8-byte unsigned integer in
// device memory, read in stream order; past len: nothing is written and bit 0x20 of the device error word is raised).  The
// haystack and the needles are not written and may overlap.  Fully asynchronous: no copy to the host, no wait.  dev_scratch:
// 256-byte aligned, at least search_scratch_bytes<T>(len, n_needles) bytes.
template <typename T>
std::size_t search_scratch_bytes(std::size_t len, std::size_t n_needles) {
    return rdst_hip_search_scratch_bytes(len, n_needles, sizeof(T));
}
template <typename T, typename Off, typename Len = std::uint64_t>
void search_device(const T* dev_sorted, std::size_t len, const T* dev_needles, std::size_t n_needles, Off* dev_out_lower, Off* dev_out_upper,
                   void* dev_scratch, std::size_t scratch_bytes, const Len* dev_len = nullptr, void* stream = nullptr) {
    static_assert(std::is_unsigned<Off>::value && (sizeof(Off) == 4 || sizeof(Off) == 8), "positions are 4- or 8-byte unsigned integers");
    static_assert(std::is_unsigned<Len>::value && (sizeof(Len) == 4 || sizeof(Len) == 8), "a device-resident length is a 4- or 8-byte unsigned integer");
    detail::check(rdst_hip_search_device(dev_sorted, len, dev_len, sizeof(Len), dev_needles, n_needles, dev_out_lower, dev_out_upper, sizeof(Off), dev_scratch,
                                         scratch_bytes, sizeof(T), RadixKey<T>::kind, static_cast<std::uint32_t>(RadixKey<T>::LEVELS), 0u, stream));
}

// DEVICE-resident [u8; N] rows (src/radix_key_impl.rs:78-85) and DEVICE-resident structs ordered by a described key
// (src/radix_key.rs; examples/impl_radix_key.rs:32-56), in place and with no host involvement
// (rdst_hip_sort_bytes_device_nowait, rdst_hip_sort_records_by_fields_device_nowait): N, or the sum of the fields' widths,
// up to RDST_BYTES_NOWAIT_MAX_N.  Nothing is copied to the host and nothing waited for; failures of the kernels surface in
// rdst_hip_device_status.  Equal keys keep their input order.  dev_scratch: at least rdst_hip_sort_bytes_scratch_bytes(n, N) /
// rdst_hip_sort_records_by_fields_scratch_bytes(n, sizeof(T), fields, n_fields) bytes, 256-byte aligned.
template <std::size_t N>
void sort_bytes_device_nowait(std::array<std::uint8_t, N>* dev_rows, std::size_t n, void* dev_scratch, std::size_t scratch_bytes,
                              void* stream = nullptr) {
    static_assert(N >= 1 && N <= RDST_BYTES_NOWAIT_MAX_N, "the nowait entry takes [u8; N] keys with N in 1..RDST_BYTES_NOWAIT_MAX_N");
    detail::check(rdst_hip_sort_bytes_device_nowait(dev_rows, n, static_cast<std::uint32_t>(N), dev_scratch, scratch_bytes, stream));
}
template <typename T>
void sort_records_by_device_nowait(T* dev_records, std::size_t n, std::initializer_list<rdst_key_field> fields, void* dev_scratch,
                                   std::size_t scratch_bytes, void* stream = nullptr) {
    static_assert(std::is_trivially_copyable<T>::value, "rows are moved as bytes");
    detail::check(rdst_hip_sort_records_by_fields_device_nowait(dev_records, n, sizeof(T), fields.begin(),
                                                                static_cast<std::uint32_t>(fields.size()), dev_scratch, scratch_bytes, stream));
}

}  // namespace rdst
#endif  // RDST_HPP
