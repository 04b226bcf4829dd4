// C++ caller of include/rdst.hpp for the segmented sort that never visits the host (rdst::sort_segments_device_offsets_nowait):
// the lengths at which the classes and the tiled route's shapes change, with both offset widths, keys against std::sort and
// pairs against std::stable_sort per segment; tmp outside the long segments stays as it was.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
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

template <typename Off>
static std::vector<Off> table(uint32_t val_bytes, size_t key_bytes, uint64_t seed, uint64_t* block_max) {
    uint32_t lim[2];
    CHECK(rdst_hip_sort_segments_limits(static_cast<uint32_t>(key_bytes), val_bytes, lim) == RDST_OK);
    const uint64_t wm = lim[0], T = lim[1];
    *block_max = T;
    std::vector<uint64_t> lengths = {0, 1, 2, wm, wm + 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 17};
    std::mt19937_64 rng(seed);
    std::shuffle(lengths.begin(), lengths.end(), rng);
    std::vector<Off> off{5};
    for (uint64_t n : lengths) off.push_back(static_cast<Off>(off.back() + n));
    return off;
}

template <typename T, typename Off>
static void run_keys(uint64_t seed) {
    uint64_t bm = 0;
    const std::vector<Off> off = table<Off>(0, sizeof(T), seed, &bm);
    const size_t len = off.back() + 7, n_segments = off.size() - 1;
    std::mt19937_64 rng(seed + 100);
    std::vector<T> keys(len), tmp(len);
    for (T& k : keys) k = static_cast<T>(rng());
    for (T& k : tmp) k = static_cast<T>(rng());
    std::vector<T> want = keys;
    for (size_t s = 0; s < n_segments; ++s) std::sort(want.begin() + off[s], want.begin() + off[s + 1]);
    DeviceArray<T> d_keys(keys), d_tmp(tmp);
    DeviceArray<Off> d_off(off);
    const size_t scratch_bytes = rdst::segments_nowait_scratch_bytes<T>(n_segments, len);
    CHECK(scratch_bytes > rdst::segments_device_offsets_scratch_bytes(n_segments) && scratch_bytes % 256 == 0);
    DeviceArray<unsigned char> d_scratch(scratch_bytes);
    rdst::sort_segments_device_offsets_nowait(d_keys.p, d_tmp.p, len, d_off.p, n_segments, d_scratch.p, scratch_bytes);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    CHECK(d_keys.host() == want);
    CHECK(d_off.host() == off);
    const std::vector<T> tmp_after = d_tmp.host();
    for (size_t s = 0; s < n_segments; ++s)
        if (off[s + 1] - off[s] <= bm) CHECK(std::equal(tmp.begin() + off[s], tmp.begin() + off[s + 1], tmp_after.begin() + off[s]));
    CHECK(std::equal(tmp.begin(), tmp.begin() + off[0], tmp_after.begin()) && std::equal(tmp.begin() + off.back(), tmp.end(), tmp_after.begin() + off.back()));
}

template <typename T, typename V, typename Off>
static void run_pairs(uint64_t seed) {
    uint64_t bm = 0;
    const std::vector<Off> off = table<Off>(sizeof(V), sizeof(T), seed, &bm);
    const size_t len = off.back() + 7, n_segments = off.size() - 1;
    std::mt19937_64 rng(seed + 200);
    std::vector<T> keys(len);
    for (T& k : keys) k = static_cast<T>(rng() % 5);  // ties everywhere
    std::vector<V> vals(len);
    std::iota(vals.begin(), vals.end(), V(0));
    std::vector<size_t> order(len);
    std::iota(order.begin(), order.end(), size_t(0));
    for (size_t s = 0; s < n_segments; ++s)
        std::stable_sort(order.begin() + off[s], order.begin() + off[s + 1], [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    std::vector<T> want_k(len);
    std::vector<V> want_v(len);
    for (size_t i = 0; i < len; ++i) {
        want_k[i] = keys[order[i]];
        want_v[i] = vals[order[i]];
    }
    DeviceArray<T> d_keys(keys), d_tmp_k(len);
    DeviceArray<V> d_vals(vals), d_tmp_v(len);
    DeviceArray<Off> d_off(off);
    const size_t scratch_bytes = rdst::segments_nowait_scratch_bytes<T, V>(n_segments, len);
    DeviceArray<unsigned char> d_scratch(scratch_bytes);
    rdst::sort_segments_device_offsets_nowait(d_keys.p, d_vals.p, d_tmp_k.p, d_tmp_v.p, len, d_off.p, n_segments, d_scratch.p, scratch_bytes);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    CHECK(d_keys.host() == want_k);
    CHECK(d_vals.host() == want_v);
}

int main() {
    run_keys<std::uint32_t, std::uint32_t>(1);
    run_keys<std::int64_t, std::uint64_t>(2);
    run_keys<std::uint8_t, std::uint32_t>(3);
    run_keys<float, std::uint64_t>(4);
    run_pairs<std::uint32_t, std::uint32_t, std::uint32_t>(5);
    run_pairs<std::int64_t, std::uint64_t, std::uint64_t>(6);
    // an invalid table: reported once by the status call; keys and tmp as they were.  A scratch one byte short and a NULL tmp throw.
    {
        uint32_t lim[2];
        CHECK(rdst_hip_sort_segments_limits(4, 0, lim) == RDST_OK);
        const size_t len = 2 * lim[1] + 100;
        std::vector<std::uint32_t> keys(len), tmp(len, 7u);
        for (size_t i = 0; i < len; ++i) keys[i] = static_cast<std::uint32_t>(len - i);
        const std::vector<std::uint64_t> off = {0, lim[1] + 60, 40, len};
        DeviceArray<std::uint32_t> d_keys(keys), d_tmp(tmp);
        DeviceArray<std::uint64_t> d_off(off);
        const size_t scratch_bytes = rdst::segments_nowait_scratch_bytes<std::uint32_t>(3, len);
        DeviceArray<unsigned char> d_scratch(scratch_bytes);
        rdst::sort_segments_device_offsets_nowait(d_keys.p, d_tmp.p, len, d_off.p, 3, d_scratch.p, scratch_bytes);
        CHECK(rdst_hip_device_status(nullptr) == RDST_ERR_DEVICE);
        CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
        CHECK(d_keys.host() == keys);
        CHECK(d_tmp.host() == tmp);
        int threw = 0;
        try {
            rdst::sort_segments_device_offsets_nowait(d_keys.p, d_tmp.p, len, d_off.p, 3, d_scratch.p, scratch_bytes - 1);
        } catch (const rdst::Error&) {
            ++threw;
        }
        try {
            rdst::sort_segments_device_offsets_nowait(d_keys.p, static_cast<std::uint32_t*>(nullptr), len, d_off.p, 3, d_scratch.p, scratch_bytes);
        } catch (const rdst::Error&) {
            ++threw;
        }
        CHECK(threw == 2);
    }
    printf("ok\n");
    return 0;
}
