// C++ caller of include/rdst.hpp for the segmented select with its borders in device memory
// (rdst::select_segments_device_offsets): a few hundred segments of 0 .. block_max + 1 keys and one of 2^17 + 1 per
// instantiation — keys only and with an index of both widths, borders of both widths, smallest and largest, both modes —
// every slot against std::stable_sort of (key, position) pairs of its segment at the rank rdst::rank_for_length gives; the
// slots without a rank and the input unchanged; argument errors as rdst::Error with the C entry's status.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <type_traits>
#include <utility>
#include <vector>

#include "rdst.hpp"

// the three HIP runtime calls this program needs (no HIP headers: it is built with the host compiler alone)
extern "C" {
int hipMalloc(void** ptr, size_t bytes);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);  // 1: host to device, 2: device to host
}

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

template <typename T>
struct DeviceArray {
    T* p = nullptr;
    size_t n;
    explicit DeviceArray(size_t count) : n(count) { CHECK(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)) == 0); }
    explicit DeviceArray(const std::vector<T>& v) : DeviceArray(v.size()) { CHECK(hipMemcpy(p, v.data(), n * sizeof(T), 1) == 0); }
    ~DeviceArray() { (void)hipFree(p); }
    std::vector<T> host() const {
        std::vector<T> v(n);
        CHECK(hipMemcpy(v.data(), p, n * sizeof(T), 2) == 0);
        return v;
    }
};

// keys with many repeats: positions tell the order of equal keys
template <typename T>
static std::vector<T> make_keys(size_t n, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<T> keys(n);
    for (T& k : keys) {
        const std::int64_t v = static_cast<std::int64_t>(rng() % 4001) - 2000;
        if (std::is_floating_point<T>::value) k = static_cast<T>(static_cast<double>(v) * 0.5);
        else k = static_cast<T>(v);  // (unsigned types: the negative half wraps to the top of the range)
    }
    return keys;
}

// the stable order of one segment by the key (largest: by the key descending, equal keys still in ascending position)
template <typename T>
static std::vector<std::pair<T, size_t>> ordered(const std::vector<T>& keys, size_t lo, size_t hi, bool largest) {
    std::vector<std::pair<T, size_t>> want(hi - lo);
    for (size_t i = lo; i < hi; ++i) want[i - lo] = {keys[i], i - lo};
    std::stable_sort(want.begin(), want.end(), [largest](const std::pair<T, size_t>& a, const std::pair<T, size_t>& b) {
        return largest ? a.first > b.first : a.first < b.first;
    });
    return want;
}

template <typename Off>
static std::vector<Off> make_table(const std::vector<std::uint64_t>& lengths, std::uint64_t first) {
    std::vector<Off> off{static_cast<Off>(first)};
    for (std::uint64_t n : lengths) off.push_back(static_cast<Off>(off.back() + n));
    return off;
}

// a few hundred segments: most short, every tenth up to block_max + 1, the class borders, and one of 2^17 + 1 keys
static std::vector<std::uint64_t> make_lengths(std::uint64_t wm, std::uint64_t bm, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<std::uint64_t> lengths{0, 1, 2, 65, wm, wm + 1, 1025, 0, bm, bm + 1, 3};
    for (int i = 0; i < 240; ++i) lengths.push_back(rng() % (i % 10 == 0 ? bm + 2 : 2 * wm));
    lengths.insert(lengths.begin() + 100, (1ull << 17) + 1);
    return lengths;
}

template <typename T, typename Off, typename Idx>  // Idx = void: keys only
static void run(const std::vector<std::uint64_t>& lengths, const std::vector<rdst_rank_spec>& specs, bool largest, bool wait_mode, uint64_t seed) {
    constexpr bool INDEXED = !std::is_void<Idx>::value;
    using I = typename std::conditional<INDEXED, Idx, std::uint32_t>::type;
    const std::vector<Off> off = make_table<Off>(lengths, 5);
    const size_t nseg = off.size() - 1, n = off.back() + 3, far = wait_mode ? n : 0, nr = specs.size();
    const std::vector<T> keys = make_keys<T>(n, seed);
    const T fill_key = static_cast<T>(77);
    const I fill_idx = static_cast<I>(0xABCDEF);
    DeviceArray<T> d_keys(keys), d_out(std::vector<T>(nseg * nr, fill_key));
    DeviceArray<I> d_idx(std::vector<I>(nseg * nr, fill_idx));
    DeviceArray<Off> d_off(off);
    size_t bytes;
    if constexpr (INDEXED) bytes = rdst::select_segments_device_offsets_scratch_bytes<T, I>(nseg, far, nr);
    else bytes = rdst::select_segments_device_offsets_scratch_bytes<T>(nseg, far, nr);
    CHECK(bytes >= rdst_hip_sort_segments_device_offsets_scratch_bytes(nseg) && (wait_mode || bytes == rdst_hip_sort_segments_device_offsets_scratch_bytes(nseg)));
    DeviceArray<unsigned char> d_scratch(bytes);
    if constexpr (INDEXED)
        rdst::select_segments_device_offsets(d_keys.p, n, d_off.p, nseg, specs.data(), nr, d_out.p, d_idx.p, static_cast<void*>(d_scratch.p), bytes, far, largest);
    else rdst::select_segments_device_offsets(d_keys.p, n, d_off.p, nseg, specs.data(), nr, d_out.p, static_cast<void*>(d_scratch.p), bytes, far, largest);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    const std::vector<T> got = d_out.host();
    const std::vector<I> idx = d_idx.host();
    for (size_t s = 0; s < nseg; ++s) {
        const auto want = ordered(keys, off[s], off[s + 1], largest);
        for (size_t i = 0; i < nr; ++i) {
            std::uint64_t r = 0;
            if (rdst::rank_for_length(specs[i], want.size(), &r)) {
                CHECK(r < want.size());
                CHECK(got[s * nr + i] == want[r].first);
                CHECK(!INDEXED || idx[s * nr + i] == static_cast<I>(want[r].second));
            } else {  // not written
                CHECK(got[s * nr + i] == fill_key && idx[s * nr + i] == fill_idx);
            }
        }
    }
    CHECK(d_keys.host() == keys);
}

int main() {
    std::uint32_t lim[4];
    CHECK(rdst_hip_select_segments_limits(4, 4, lim) == RDST_OK);
    const std::uint64_t wm = lim[0], bm = lim[1];
    const std::vector<std::uint64_t> lengths = make_lengths(wm, bm, 21);
    CHECK(lengths.size() > 250);
    const std::vector<rdst_rank_spec> few{rdst::rank_at(0), rdst::rank_quantile(1, 2), rdst::rank_quantile(9, 10, RDST_RANK_NEAREST),
                                          rdst::rank_at(static_cast<std::uint32_t>(wm)), rdst::rank_quantile(1, 1, RDST_RANK_HIGHER)};
    std::vector<rdst_rank_spec> many;  // more than one round, the modes mixed
    for (std::uint32_t i = 0; i < 40; ++i) many.push_back(i % 7 == 3 ? rdst::rank_at(i * 50) : rdst::rank_quantile(i, 39, i % 3));
    run<std::int32_t, std::uint32_t, void>(lengths, few, false, false, 1);
    run<std::uint64_t, std::uint64_t, void>(lengths, many, true, false, 2);
    run<std::int16_t, std::uint64_t, void>(lengths, few, true, true, 3);
    run<double, std::uint32_t, void>(lengths, few, false, true, 4);
    run<float, std::uint32_t, std::uint32_t>(lengths, many, true, false, 5);
    run<std::int64_t, std::uint64_t, std::uint64_t>(lengths, few, false, false, 6);
    run<double, std::uint64_t, std::uint32_t>(lengths, few, true, true, 7);
    run<std::uint32_t, std::uint32_t, std::uint64_t>(lengths, many, false, true, 8);
    // all four classes: the border of the stream class below the longest rows, which go far in the wait mode
    CHECK(rdst_hip_set_topk_segments_stream_max(static_cast<std::uint32_t>(bm + 1)) == RDST_OK);
    run<float, std::uint64_t, std::uint32_t>(lengths, few, true, true, 9);
    run<std::uint32_t, std::uint32_t, void>(lengths, few, false, false, 10);  // (the asynchronous mode does not look at the border)
    CHECK(rdst_hip_set_topk_segments_stream_max(0) == RDST_OK);
    run<std::uint8_t, std::uint32_t, void>({3, 1, 0, 2}, few, false, false, 12);

    // no rank and no segment do nothing and need nothing; argument errors throw rdst::Error with the C entry's status
    {
        const std::vector<std::uint32_t> keys = make_keys<std::uint32_t>(1000, 13);
        const std::vector<std::uint64_t> table{0, 10, 500, 1000}, decreasing{0, 10, 9, 1000};
        DeviceArray<std::uint32_t> d_keys(keys), d_out(std::vector<std::uint32_t>(15, 77u));
        DeviceArray<std::uint64_t> d_table(table), d_decreasing(decreasing);
        const size_t bytes = rdst::select_segments_device_offsets_scratch_bytes<std::uint32_t>(3, 1000, 5);
        DeviceArray<unsigned char> d_scratch(bytes);
        const std::uint64_t* no_table = nullptr;
        const rdst_rank_spec bad{3, 2, 0, 0};
        rdst::select_segments_device_offsets(d_keys.p, 1000, d_table.p, 3, few.data(), 0, static_cast<std::uint32_t*>(nullptr), static_cast<void*>(nullptr), 0);
        rdst::select_segments_device_offsets(d_keys.p, 1000, no_table, 0, few.data(), 5, static_cast<std::uint32_t*>(nullptr), static_cast<void*>(nullptr), 0);
        int threw = 0;
        try {  // the wait mode sees the plan's flags
            rdst::select_segments_device_offsets(d_keys.p, 1000, d_decreasing.p, 3, few.data(), 5, d_out.p, static_cast<void*>(d_scratch.p), bytes, 1000);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        try {
            rdst::select_segments_device_offsets(d_keys.p, 999, d_table.p, 3, few.data(), 5, d_out.p, static_cast<void*>(d_scratch.p), bytes, 999);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
        try {
            rdst::select_segments_device_offsets(d_keys.p, 1000, no_table, 3, few.data(), 5, d_out.p, static_cast<void*>(d_scratch.p), bytes);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        try {
            rdst::select_segments_device_offsets(d_keys.p, 1000, d_table.p, 3, &bad, 1, d_out.p, static_cast<void*>(d_scratch.p), bytes);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        try {
            rdst::select_segments_device_offsets(d_keys.p, 1000, d_table.p, 3, few.data(), 5, d_out.p, static_cast<void*>(d_scratch.p + 16), bytes);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ALIGN;
        }
        try {
            rdst::select_segments_device_offsets(d_keys.p, 1000, d_table.p, 3, few.data(), 5, d_out.p, static_cast<void*>(d_scratch.p), bytes - 1, 1000);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        try {
            DeviceArray<std::uint16_t> d_small(1000), d_small_out(15);
            DeviceArray<std::uint32_t> d_idx(15);
            rdst::select_segments_device_offsets(d_small.p, 1000, d_table.p, 3, few.data(), 5, d_small_out.p, d_idx.p, static_cast<void*>(d_scratch.p), bytes);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_UNSUPPORTED;
        }
        CHECK(threw == 7);
        // the asynchronous mode cannot answer by the return code: nothing written, the error word says so once
        rdst::select_segments_device_offsets(d_keys.p, 1000, d_decreasing.p, 3, few.data(), 5, d_out.p, static_cast<void*>(d_scratch.p), bytes);
        CHECK(rdst_hip_device_status(nullptr) == RDST_ERR_DEVICE);
        CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
        CHECK(d_out.host() == std::vector<std::uint32_t>(15, 77u));
        CHECK(d_keys.host() == keys);
    }
    printf("ok\n");
    return 0;
}
