// C++ caller of include/rdst.hpp for the runs of equal keys (rdst::runs_device): per instantiation — key types of every
// width the mirror has, both border widths — the lengths around the tile (0, 1, 2, T - 1, T, T + 1, 2 T, 3 T + 5) with
// random runs, heads at T - 1, T and T + 1, all equal, all distinct; then the capacity: R - 1 (truncated: the first R - 1 runs
// complete, the true count, the device status RDST_ERR_DEVICE once and clean afterwards), R, 0 (count only, null outputs),
// keys only and starts only.  Every comparison is exact, against a loop over the bits on the host.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <type_traits>
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

template <typename T>
static bool same_bits(const T& a, const T& b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// keys whose heads are exactly `heads`: run r holds r * an odd constant cut to the key's width (floats: as bits)
template <typename T>
static std::vector<T> keys_from_heads(const std::vector<bool>& heads) {
    std::vector<T> keys(heads.size());
    std::uint64_t run = 0;
    for (size_t i = 0; i < heads.size(); ++i) {
        if (heads[i] && i) ++run;
        const std::uint64_t v = run * 0x9E3779B97F4A7C15ull;
        std::memcpy(&keys[i], &v, sizeof(T));  // (little endian: the low bytes)
    }
    return keys;
}

static std::vector<bool> random_heads(size_t n, std::mt19937_64& rng) {
    std::vector<bool> h(n, false);
    for (size_t i = 0; i < n; i += 1 + rng() % 9) h[i] = true;
    return h;
}

static std::vector<bool> heads_at(size_t n, std::initializer_list<size_t> at) {
    std::vector<bool> h(n, false);
    if (n) h[0] = true;
    for (size_t p : at)
        if (p < n) h[p] = true;
    return h;
}

constexpr std::uint64_t POISON = 0xA5A5A5A5A5A5A5A5ull;

// one call at `capacity` (keys_out / starts_out: which outputs are asked for) against the loop
template <typename T, typename Off>
static void check_call(const std::vector<T>& keys, size_t capacity, bool keys_out, bool starts_out) {
    const size_t n = keys.size();
    std::vector<size_t> starts;
    for (size_t i = 0; i < n; ++i)
        if (i == 0 || !same_bits(keys[i], keys[i - 1])) starts.push_back(i);
    const size_t R = starts.size(), kept = std::min(R, capacity);
    T poison_key;
    std::memcpy(&poison_key, &POISON, sizeof(T));
    DeviceArray<T> d_keys(keys);
    DeviceArray<T> d_out(std::vector<T>(capacity + 1, poison_key));
    DeviceArray<Off> d_starts(std::vector<Off>(capacity + 2, static_cast<Off>(POISON)));
    DeviceArray<Off> d_count(std::vector<Off>(2, static_cast<Off>(POISON)));
    const size_t sbytes = rdst::runs_scratch_bytes<T>(n);
    CHECK(sbytes >= 512 && sbytes % 256 == 0);
    DeviceArray<unsigned char> d_scratch(sbytes);
    rdst::runs_device<T, Off>(d_keys.p, n, keys_out && capacity ? d_out.p : nullptr, starts_out && capacity ? d_starts.p : nullptr, d_count.p, capacity, d_scratch.p,
                              sbytes);
    const int status = rdst_hip_device_status(nullptr);
    if (capacity > 0 && R > capacity) {
        CHECK(status == RDST_ERR_DEVICE);
        CHECK(rdst_hip_device_status(nullptr) == RDST_OK);  // reported once
    } else {
        CHECK(status == RDST_OK);
    }
    const std::vector<Off> count = d_count.host(), got_starts = d_starts.host();
    const std::vector<T> got_keys = d_out.host();
    CHECK(count[0] == static_cast<Off>(R) && count[1] == static_cast<Off>(POISON));
    for (size_t r = 0; r <= capacity; ++r) {
        const bool key_written = keys_out && capacity && r < kept;
        CHECK(same_bits(got_keys[r], key_written ? keys[starts[r]] : poison_key));
    }
    for (size_t r = 0; r <= capacity + 1; ++r) {
        Off want = static_cast<Off>(POISON);
        if (starts_out && capacity) {
            if (r < kept) want = static_cast<Off>(starts[r]);
            else if (r == kept) want = static_cast<Off>(R > capacity ? starts[capacity] : n);  // the end of the last kept run
        }
        CHECK(got_starts[r] == want);
    }
    CHECK(std::memcmp(d_keys.host().data(), keys.data(), n * sizeof(T)) == 0);  // the input is never written
}

template <typename T, typename Off>
static void run(std::uint64_t seed) {
    std::uint32_t lim[2];
    CHECK(rdst_hip_runs_limits(sizeof(T), lim) == RDST_OK && lim[0] == (sizeof(T) >= 8 ? 65536u : sizeof(T) == 1 ? 16384u : 32768u) / sizeof(T) && lim[1] >= 1);
    const size_t t = lim[0];
    std::mt19937_64 rng(seed);
    // case 1: every border
    for (size_t n : {size_t(0), size_t(1), size_t(2), t - 1, t, t + 1, 2 * t, 3 * t + 5}) {
        const std::vector<T> keys = keys_from_heads<T>(random_heads(n, rng));
        check_call<T, Off>(keys, n, true, true);
    }
    const size_t n = 3 * t + 5;
    for (const std::vector<bool>& heads : {heads_at(n, {t - 1}), heads_at(n, {t}), heads_at(n, {t + 1}), heads_at(n, {t - 1, t, t + 1}), heads_at(n, {}),
                                           std::vector<bool>(n, true)})
        check_call<T, Off>(keys_from_heads<T>(heads), n, true, true);
    // case 4: the capacity
    const std::vector<bool> heads = random_heads(2 * t + 77, rng);
    const std::vector<T> keys = keys_from_heads<T>(heads);
    const size_t R = static_cast<size_t>(std::count(heads.begin(), heads.end(), true));
    check_call<T, Off>(keys, R - 1, true, true);
    check_call<T, Off>(keys, R, true, true);
    check_call<T, Off>(keys, 0, false, false);
    check_call<T, Off>(keys, R, true, false);
    check_call<T, Off>(keys, R, false, true);
    check_call<T, Off>(keys, R - 1, false, true);
}

int main() {
    run<std::uint8_t, std::uint32_t>(1);
    run<std::int16_t, std::uint64_t>(2);
    run<std::uint32_t, std::uint32_t>(3);
    run<float, std::uint64_t>(4);
    run<std::int64_t, std::uint32_t>(5);
    run<double, std::uint64_t>(6);
    // argument errors arrive as rdst::Error with the C entry's status
    DeviceArray<std::uint32_t> a(64);
    DeviceArray<std::uint64_t> c(1);
    DeviceArray<unsigned char> s(4096);
    try {
        rdst::runs_device<std::uint32_t, std::uint64_t>(a.p, 64, a.p, nullptr, c.p, 64, s.p, 4096);  // the key output is the input
        CHECK(false);
    } catch (const rdst::Error& e) {
        CHECK(e.status == RDST_ERR_ARG);
    }
    try {
        rdst::runs_device<std::uint32_t, std::uint64_t>(a.p, 64, nullptr, nullptr, c.p, 64, s.p, 4096, true);  // pad without starts
        CHECK(false);
    } catch (const rdst::Error& e) {
        CHECK(e.status == RDST_ERR_ARG);
    }
    printf("ok\n");
    return 0;
}
