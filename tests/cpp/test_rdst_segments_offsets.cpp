// C++ caller of include/rdst.hpp for the segmented sort with its table of borders in device memory
// (rdst::sort_segments_device_offsets): the EDGES lengths — every border of the wave, block and long classes — in both
// modes and with both offset widths, against std::sort per segment.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "rdst.hpp"

// the four HIP runtime calls this program needs (no HIP headers: it is built with the host compiler alone)
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

template <typename T, typename Off>
static void run(bool with_long, uint64_t seed) {
    uint32_t lim[2];
    CHECK(rdst_hip_sort_segments_limits(sizeof(T), 0, lim) == RDST_OK);
    const uint64_t wm = lim[0], bm = lim[1];
    std::vector<uint64_t> lengths = {0, 0, 1, 2, 3, 63, 64, 65, wm - 1, wm, wm + 1, 1023, 1024, 1025, bm - 1, bm};
    if (with_long) lengths.insert(lengths.end(), {bm + 1, 2 * bm + 17});
    std::mt19937_64 rng(seed);
    std::shuffle(lengths.begin(), lengths.end(), rng);
    lengths.push_back(0);
    std::vector<Off> off{5};
    for (uint64_t n : lengths) off.push_back(static_cast<Off>(off.back() + n));
    const size_t len = off.back() + 7;
    std::vector<T> keys(len);
    for (T& k : keys) k = static_cast<T>(rng());
    std::vector<T> want = keys;
    for (size_t s = 0; s + 1 < off.size(); ++s) std::sort(want.begin() + off[s], want.begin() + off[s + 1]);

    DeviceArray<T> d_keys(keys);
    DeviceArray<Off> d_off(off);
    const size_t n_segments = off.size() - 1;
    const size_t scratch_bytes = rdst::segments_device_offsets_scratch_bytes(n_segments);
    CHECK(scratch_bytes > 0 && scratch_bytes % 256 == 0);
    DeviceArray<unsigned char> d_scratch(scratch_bytes);
    const size_t tmp_elems = with_long ? 2 * bm + 17 : 0;
    DeviceArray<T> d_tmp(tmp_elems);
    rdst::sort_segments_device_offsets(d_keys.p, len, d_off.p, n_segments, d_scratch.p, scratch_bytes, with_long ? d_tmp.p : nullptr, tmp_elems);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    CHECK(d_keys.host() == want);
    CHECK(d_off.host() == off);
}

int main() {
    run<std::uint32_t, std::uint32_t>(false, 1);
    run<std::uint32_t, std::uint64_t>(true, 2);
    run<std::int64_t, std::uint32_t>(true, 3);
    run<std::uint16_t, std::uint64_t>(false, 4);
    // a table the asynchronous mode has to refuse: reported by the status call, the keys as they were
    {
        std::vector<std::uint32_t> keys(100);
        for (size_t i = 0; i < keys.size(); ++i) keys[i] = static_cast<std::uint32_t>(1000 - i);
        const std::vector<std::uint64_t> off = {0, 60, 40, 100};
        DeviceArray<std::uint32_t> d_keys(keys);
        DeviceArray<std::uint64_t> d_off(off);
        const size_t scratch_bytes = rdst::segments_device_offsets_scratch_bytes(3);
        DeviceArray<unsigned char> d_scratch(scratch_bytes);
        rdst::sort_segments_device_offsets(d_keys.p, keys.size(), d_off.p, 3, d_scratch.p, scratch_bytes);
        CHECK(rdst_hip_device_status(nullptr) == RDST_ERR_DEVICE);
        CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
        CHECK(d_keys.host() == keys);
        bool threw = false;
        try {
            rdst::sort_segments_device_offsets(d_keys.p, keys.size(), d_off.p, 3, d_scratch.p, scratch_bytes - 1);
        } catch (const rdst::Error&) {
            threw = true;
        }
        CHECK(threw);
    }
    printf("ok\n");
    return 0;
}
