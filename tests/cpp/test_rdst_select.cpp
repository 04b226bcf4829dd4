// C++ caller of include/rdst.hpp for the order statistics (rdst::select_device): keys only and with an index of both
// widths, smallest and largest, against std::stable_sort of (key, position) pairs indexed at the ranks; the input unchanged;
// one length at a border of the streaming reader and one that takes several groups, several levels and more than one round;
// argument errors as rdst::Error with the C entry's status.
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

// a stable sort by the key (largest: by the key descending, equal keys still in ascending position)
template <typename T>
static std::vector<std::pair<T, size_t>> sorted_pairs(const std::vector<T>& keys, bool largest) {
    std::vector<std::pair<T, size_t>> want(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) want[i] = {keys[i], i};
    std::stable_sort(want.begin(), want.end(), [largest](const std::pair<T, size_t>& a, const std::pair<T, size_t>& b) {
        return largest ? a.first > b.first : a.first < b.first;
    });
    return want;
}

// ranks out of order and with a repeat; `count` of them
static std::vector<std::uint64_t> make_ranks(size_t n, size_t count) {
    std::vector<std::uint64_t> r;
    for (size_t i = 0; i < count; ++i) r.push_back((i * 7919 + n / 2) % n);
    if (count > 2) r[count - 1] = r[0];
    if (count > 1) r[1] = n - 1;
    r[0] = 0;
    return r;
}

// what the device reports about its last round (rdst_hip_debug_select_state): with the default capacity (>= n here) everything
// is a candidate and no level runs; with a small capacity the select runs levels
static void check_state(const void* d_scratch, size_t n, size_t cand_capacity) {
    std::uint64_t st[4] = {9, 9, 9, 9};
    CHECK(rdst_hip_debug_select_state(d_scratch, nullptr, st) == RDST_OK);
    if (cand_capacity == 0 || cand_capacity >= n) CHECK(st[0] == 0 && st[1] == 1 && st[2] == n && st[3] == 0);
    else CHECK(st[0] >= 1 && st[1] >= 1 && st[1] <= 64 && (st[3] == 1 ? st[2] == 0 : st[2] <= cand_capacity));
}

template <typename T>
static void run_keys(size_t n, size_t n_ranks, bool largest, size_t cand_capacity, uint64_t seed) {
    const std::vector<T> keys = make_keys<T>(n, seed);
    const auto want = sorted_pairs(keys, largest);
    const std::vector<std::uint64_t> ranks = make_ranks(n, n_ranks);
    DeviceArray<T> d_keys(keys), d_out(n_ranks);
    const size_t bytes = rdst::select_scratch_bytes<T>(n, n_ranks, cand_capacity);
    DeviceArray<unsigned char> d_scratch(bytes);
    rdst::select_device(d_keys.p, n, ranks.data(), n_ranks, d_out.p, static_cast<void*>(d_scratch.p), bytes, largest, cand_capacity);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    const std::vector<T> got = d_out.host();
    for (size_t i = 0; i < n_ranks; ++i) CHECK(got[i] == want[ranks[i]].first);
    CHECK(d_keys.host() == keys);
    check_state(d_scratch.p, n, cand_capacity);
}

template <typename T, typename Idx>
static void run_indexed(size_t n, size_t n_ranks, bool largest, size_t cand_capacity, uint64_t seed) {
    const std::vector<T> keys = make_keys<T>(n, seed);
    const auto want = sorted_pairs(keys, largest);
    const std::vector<std::uint64_t> ranks = make_ranks(n, n_ranks);
    DeviceArray<T> d_keys(keys), d_out(n_ranks);
    DeviceArray<Idx> d_idx(n_ranks);
    const size_t bytes = rdst::select_scratch_bytes<T, Idx>(n, n_ranks, cand_capacity);
    DeviceArray<unsigned char> d_scratch(bytes);
    rdst::select_device(d_keys.p, n, ranks.data(), n_ranks, d_out.p, d_idx.p, static_cast<void*>(d_scratch.p), bytes, largest, cand_capacity);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    const std::vector<T> got = d_out.host();
    const std::vector<Idx> idx = d_idx.host();
    for (size_t i = 0; i < n_ranks; ++i) CHECK(got[i] == want[ranks[i]].first && idx[i] == static_cast<Idx>(want[ranks[i]].second));
    CHECK(d_keys.host() == keys);
    check_state(d_scratch.p, n, cand_capacity);
}

int main() {
    // 4097: one block batch of 4-byte keys and one key; 50021 keys at 70 ranks: several groups, levels and two rounds
    for (size_t n : {size_t(4097), size_t(50021)}) {
        for (size_t n_ranks : {size_t(1), size_t(9), size_t(70)}) {
            for (bool largest : {false, true}) {
                for (size_t cap : {size_t(0), size_t(5)}) {  // (4001 values: about 12 keys tie with any key at the larger length)
                    run_keys<std::int32_t>(n, n_ranks, largest, cap, 1);
                    run_keys<std::uint64_t>(n, n_ranks, largest, cap, 2);
                    run_keys<std::int16_t>(n, n_ranks, largest, cap, 3);
                    run_keys<double>(n, n_ranks, largest, cap, 4);
                    run_indexed<float, std::uint32_t>(n, n_ranks, largest, cap, 5);
                    run_indexed<std::int64_t, std::uint64_t>(n, n_ranks, largest, cap, 6);
                    run_indexed<double, std::uint32_t>(n, n_ranks, largest, cap, 7);
                    run_indexed<std::uint32_t, std::uint64_t>(n, n_ranks, largest, cap, 8);
                }
            }
        }
    }
    run_keys<std::uint8_t>(3, 2, false, 0, 9);
    run_indexed<std::int32_t, std::uint32_t>(1, 1, true, 0, 10);

    // no ranks: nothing is done and nothing needed; argument errors throw rdst::Error with the C entry's status
    {
        const std::vector<std::uint32_t> keys = make_keys<std::uint32_t>(1000, 11);
        DeviceArray<std::uint32_t> d_keys(keys), d_out(10);
        const std::vector<std::uint64_t> ranks = make_ranks(1000, 10);
        const size_t bytes = rdst::select_scratch_bytes<std::uint32_t>(1000, 10);
        DeviceArray<unsigned char> d_scratch(bytes);
        rdst::select_device(d_keys.p, 1000, static_cast<const std::uint64_t*>(nullptr), 0, static_cast<std::uint32_t*>(nullptr), static_cast<void*>(nullptr), 0);
        int threw = 0;
        try {
            std::vector<std::uint64_t> bad = ranks;
            bad[3] = 1000;
            rdst::select_device(d_keys.p, 1000, bad.data(), 10, d_out.p, static_cast<void*>(d_scratch.p), bytes);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        try {
            rdst::select_device(d_keys.p, 1000, ranks.data(), 10, d_out.p, static_cast<void*>(d_scratch.p + 16), bytes);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ALIGN;
        }
        try {
            rdst::select_device(d_keys.p, 1000, ranks.data(), 10, d_out.p, static_cast<void*>(d_scratch.p), bytes - 1);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        try {
            DeviceArray<std::uint16_t> d_small(1000), d_small_out(10);
            DeviceArray<std::uint32_t> d_idx(10);
            rdst::select_device(d_small.p, 1000, ranks.data(), 10, d_small_out.p, d_idx.p, static_cast<void*>(d_scratch.p), bytes);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_UNSUPPORTED;
        }
        CHECK(threw == 4);
        CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
        CHECK(d_keys.host() == keys);
    }
    printf("ok\n");
    return 0;
}
