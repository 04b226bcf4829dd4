// C++ caller of include/rdst.hpp for the sorts of a prefix whose length lives in device memory (rdst::sort_device_devlen,
// rdst::sort_pairs_device_devlen): the prefix against std::stable_sort, the tail and the length untouched, both length
// types, a key-value case (a payload telling the input order of equal keys) and a keys-only case, and a length past the
// capacity, which changes nothing and makes rdst_hip_device_status fail once.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
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

// keys only: the first m of `capacity` keys sorted, the rest as it was
template <typename T, typename Len>
static void run_keys(size_t capacity, size_t m, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<T> keys(capacity);
    for (T& k : keys) k = static_cast<T>(static_cast<std::int64_t>(rng() % 2001) - 1000);
    std::vector<T> want = keys;
    std::stable_sort(want.begin(), want.begin() + static_cast<std::ptrdiff_t>(m));
    DeviceArray<T> d_keys(keys), d_tmp(capacity);
    DeviceArray<Len> d_len(std::vector<Len>{static_cast<Len>(m)});
    rdst::sort_device_devlen(d_keys.p, d_tmp.p, capacity, d_len.p);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    CHECK(d_keys.host() == want);
    CHECK(d_len.host()[0] == static_cast<Len>(m));
}

// key-value: values are the input positions, so equal keys must come out in increasing value order
template <typename T, typename V, typename Len>
static void run_pairs(size_t capacity, size_t m, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<T> keys(capacity);
    std::vector<V> vals(capacity);
    for (size_t i = 0; i < capacity; ++i) {
        keys[i] = static_cast<T>(static_cast<double>(static_cast<int>(rng() % 401) - 200) * 0.25);
        vals[i] = static_cast<V>(i);
    }
    std::vector<std::pair<T, V>> want(capacity);
    for (size_t i = 0; i < capacity; ++i) want[i] = {keys[i], vals[i]};
    std::stable_sort(want.begin(), want.begin() + static_cast<std::ptrdiff_t>(m),
                     [](const std::pair<T, V>& a, const std::pair<T, V>& b) { return a.first < b.first; });
    DeviceArray<T> d_keys(keys), d_tmp_keys(capacity);
    DeviceArray<V> d_vals(vals), d_tmp_vals(capacity);
    DeviceArray<Len> d_len(std::vector<Len>{static_cast<Len>(m)});
    rdst::sort_pairs_device_devlen(d_keys.p, d_vals.p, d_tmp_keys.p, d_tmp_vals.p, capacity, d_len.p);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    const std::vector<T> got_keys = d_keys.host();
    const std::vector<V> got_vals = d_vals.host();
    for (size_t i = 0; i < capacity; ++i) CHECK(got_keys[i] == want[i].first && got_vals[i] == want[i].second);
}

int main() {
    const size_t capacity = 50021;
    for (size_t m : {size_t(0), size_t(1), size_t(2), size_t(777), size_t(8449), size_t(33333), capacity - 1, capacity}) {
        run_keys<std::int32_t, std::uint32_t>(capacity, m, 1);
        run_keys<std::uint64_t, std::uint64_t>(capacity, m, 2);
        run_keys<std::int16_t, std::uint64_t>(capacity, m, 3);
        run_pairs<float, std::uint32_t, std::uint32_t>(capacity, m, 4);
        run_pairs<std::int64_t, std::uint64_t, std::uint64_t>(capacity, m, 5);
        run_pairs<double, std::uint32_t, std::uint32_t>(capacity, m, 6);
    }
    run_keys<std::uint32_t, std::uint32_t>(3, 2, 7);
    run_pairs<std::int32_t, std::uint32_t, std::uint64_t>(2, 2, 8);

    // a length past the capacity: the call itself succeeds (nothing is read on the host), nothing changes, the status
    // fails once with RDST_ERR_DEVICE; argument errors throw rdst::Error with the C entry's status
    {
        std::vector<std::uint32_t> keys(capacity);
        for (size_t i = 0; i < capacity; ++i) keys[i] = static_cast<std::uint32_t>((capacity - i) * 2654435761u);
        DeviceArray<std::uint32_t> d_keys(keys), d_tmp(capacity);
        DeviceArray<std::uint64_t> d_len(std::vector<std::uint64_t>{capacity + 1});
        rdst::sort_device_devlen(d_keys.p, d_tmp.p, capacity, d_len.p);
        CHECK(rdst_hip_device_status(nullptr) == RDST_ERR_DEVICE);
        CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
        CHECK(d_keys.host() == keys);
        int threw = 0;
        try {
            rdst::sort_device_devlen(d_keys.p, d_tmp.p, capacity, static_cast<const std::uint64_t*>(nullptr));
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        try {
            rdst::sort_device_devlen(d_keys.p, d_tmp.p, capacity, reinterpret_cast<const std::uint64_t*>(reinterpret_cast<const char*>(d_len.p) + 4));
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ALIGN;
        }
        try {
            DeviceArray<std::uint32_t> d_vals(capacity);
            rdst::sort_pairs_device_devlen(d_keys.p, d_vals.p, d_tmp.p, static_cast<std::uint32_t*>(nullptr), capacity, d_len.p);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        CHECK(threw == 3);
        CHECK(d_keys.host() == keys);
        // and a valid call right after sorts
        DeviceArray<std::uint64_t> d_ok(std::vector<std::uint64_t>{capacity});
        rdst::sort_device_devlen(d_keys.p, d_tmp.p, capacity, d_ok.p);
        CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
        std::sort(keys.begin(), keys.end());
        CHECK(d_keys.host() == keys);
    }
    printf("ok\n");
    return 0;
}
