// C++ caller of include/rdst.hpp for the binary search (rdst::search_device): per instantiation — key types of every width
// the mirror has, both position widths — haystacks of the lengths around the splitter table and the staged window
// (0, 1, 2, S - 1, S, S + 1, W - 1, W, W + 1, 3 W + 5) with repeated keys, needles that are present, between two neighbours,
// below the first, above the last and the type's extremes, at the counts around the tile; lower only, upper only and both;
// then a length in device memory and the argument errors.  Every comparison is exact, against std::lower_bound and
// std::upper_bound over the mapped bits on the host.
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

// the order-preserving image of a key's bits (src/radix_key_impl.rs), and its inverse
template <typename T>
static std::uint64_t mapped(T key) {
    std::uint64_t u = 0;
    std::memcpy(&u, &key, sizeof(T));
    const std::uint64_t msb = 1ull << (8 * sizeof(T) - 1), all = msb | (msb - 1);
    if (std::is_floating_point<T>::value) return (u & msb) ? (~u & all) : (u ^ msb);
    return std::is_signed<T>::value ? (u ^ msb) : u;
}
template <typename T>
static T from_mapped(std::uint64_t m) {
    const std::uint64_t msb = 1ull << (8 * sizeof(T) - 1), all = msb | (msb - 1);
    m &= all;
    std::uint64_t u = m;
    if (std::is_floating_point<T>::value) u = (m & msb) ? (m ^ msb) : (~m & all);
    else if (std::is_signed<T>::value) u = m ^ msb;
    T key;
    std::memcpy(&key, &u, sizeof(T));
    return key;
}

constexpr std::uint64_t POISON = 0xA5A5A5A5A5A5A5A5ull;

template <typename T, typename Off, typename Len = std::uint64_t>
static void check_call(const std::vector<T>& hay, size_t m, const std::vector<T>& needles, bool want_lower, bool want_upper, bool device_length = false) {
    std::vector<std::uint64_t> hm(m), lower(needles.size()), upper(needles.size());
    for (size_t i = 0; i < m; ++i) hm[i] = mapped(hay[i]);
    CHECK(std::is_sorted(hm.begin(), hm.end()));
    for (size_t i = 0; i < needles.size(); ++i) {
        lower[i] = static_cast<std::uint64_t>(std::lower_bound(hm.begin(), hm.end(), mapped(needles[i])) - hm.begin());
        upper[i] = static_cast<std::uint64_t>(std::upper_bound(hm.begin(), hm.end(), mapped(needles[i])) - hm.begin());
    }
    DeviceArray<T> d_hay(hay), d_needles(needles);
    DeviceArray<Off> d_lower(std::vector<Off>(needles.size() + 1, static_cast<Off>(POISON))), d_upper(std::vector<Off>(needles.size() + 1, static_cast<Off>(POISON)));
    DeviceArray<Len> d_len(std::vector<Len>(1, static_cast<Len>(m)));
    const size_t sbytes = rdst::search_scratch_bytes<T>(hay.size(), needles.size());
    CHECK(sbytes == 256 + 1024 * sizeof(T));
    DeviceArray<unsigned char> d_scratch(sbytes);
    rdst::search_device<T, Off, Len>(d_hay.p, device_length ? hay.size() : m, d_needles.p, needles.size(), want_lower ? d_lower.p : nullptr,
                                     want_upper ? d_upper.p : nullptr, d_scratch.p, sbytes, device_length ? d_len.p : nullptr);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    const std::vector<Off> got_lower = d_lower.host(), got_upper = d_upper.host();
    for (size_t i = 0; i < needles.size(); ++i) {
        CHECK(got_lower[i] == (want_lower ? static_cast<Off>(lower[i]) : static_cast<Off>(POISON)));
        CHECK(got_upper[i] == (want_upper ? static_cast<Off>(upper[i]) : static_cast<Off>(POISON)));
    }
    CHECK(got_lower[needles.size()] == static_cast<Off>(POISON) && got_upper[needles.size()] == static_cast<Off>(POISON));
    CHECK(std::memcmp(d_hay.host().data(), hay.data(), hay.size() * sizeof(T)) == 0);  // the inputs are never written
    CHECK(std::memcmp(d_needles.host().data(), needles.data(), needles.size() * sizeof(T)) == 0);
}

// m sorted keys with images in the middle half of the range, low bit clear, about three of each
template <typename T>
static std::vector<T> haystack(size_t m, std::mt19937_64& rng) {
    const int bits = 8 * sizeof(T);
    const std::uint64_t quarter = 1ull << (bits - 2);
    std::vector<std::uint64_t> pool(std::max<size_t>(m / 3, 1));
    for (auto& x : pool) x = (quarter + rng() % (2 * quarter)) & ~1ull;
    std::vector<std::uint64_t> img(m);
    for (auto& x : img) x = pool[rng() % pool.size()];
    std::sort(img.begin(), img.end());
    std::vector<T> keys(m);
    for (size_t i = 0; i < m; ++i) keys[i] = from_mapped<T>(img[i]);
    return keys;
}

template <typename T>
static std::vector<T> needles_for(const std::vector<T>& hay, size_t n, std::mt19937_64& rng) {
    const int bits = 8 * sizeof(T);
    const std::uint64_t quarter = 1ull << (bits - 2);
    std::vector<std::uint64_t> img(n);
    for (size_t i = 0; i < n; ++i) {
        const std::uint64_t present = hay.empty() ? rng() : mapped(hay[rng() % hay.size()]);
        switch (rng() % 8) {
            case 0: img[i] = present | 1; break;                    // between two neighbours
            case 1: img[i] = rng() % quarter; break;                // below the first
            case 2: img[i] = 3 * quarter + rng() % quarter; break;  // above the last
            case 3: img[i] = (rng() & 1) ? 0 : ~0ull; break;        // the extremes
            default: img[i] = present;
        }
    }
    std::vector<T> keys(n);
    for (size_t i = 0; i < n; ++i) keys[i] = from_mapped<T>(img[i]);
    return keys;
}

template <typename T, typename Off>
static void run(std::uint64_t seed) {
    std::uint32_t lim[3];
    CHECK(rdst_hip_search_limits(sizeof(T), lim) == RDST_OK && lim[1] == 1024 && lim[2] >= lim[1]);
    const size_t t = lim[0], s = lim[1], w = lim[2];
    std::mt19937_64 rng(seed);
    for (size_t m : {size_t(0), size_t(1), size_t(2), s - 1, s, s + 1, w - 1, w, w + 1, 3 * w + 5}) {
        const std::vector<T> hay = haystack<T>(m, rng);
        for (size_t n : {size_t(1), t - 1, t + 1, 3 * t + 5}) {
            const std::vector<T> needles = needles_for<T>(hay, n, rng);
            check_call<T, Off>(hay, m, needles, true, true);
            if (n == t + 1) {
                check_call<T, Off>(hay, m, needles, true, false);
                check_call<T, Off>(hay, m, needles, false, true);
            }
        }
    }
    // sorted needles (the staged path), and the array searched for its own keys
    const std::vector<T> hay = haystack<T>(3 * w + 5, rng);
    std::vector<T> needles = needles_for<T>(hay, 3 * t + 5, rng);
    std::sort(needles.begin(), needles.end(), [](T a, T b) { return mapped(a) < mapped(b); });
    check_call<T, Off>(hay, hay.size(), needles, true, true);
    check_call<T, Off>(hay, hay.size(), hay, true, true);
    // the length in device memory, 4 and 8 bytes wide: the keys behind it are not part of the haystack
    check_call<T, Off, std::uint32_t>(hay, w + 1, needles, true, true, true);
    check_call<T, Off, std::uint64_t>(hay, s - 1, needles, true, true, true);
    check_call<T, Off, std::uint64_t>(hay, 0, needles, true, true, true);
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
    DeviceArray<std::uint64_t> p(64);
    DeviceArray<unsigned char> s(8192);
    try {
        rdst::search_device<std::uint32_t, std::uint64_t>(a.p, 64, a.p, 64, nullptr, nullptr, s.p, 8192);  // no output at all
        CHECK(false);
    } catch (const rdst::Error& e) {
        CHECK(e.status == RDST_ERR_ARG);
    }
    try {
        rdst::search_device<std::uint32_t, std::uint64_t>(a.p, 64, a.p, 64, p.p, p.p, s.p, 8192);  // the outputs are one array
        CHECK(false);
    } catch (const rdst::Error& e) {
        CHECK(e.status == RDST_ERR_ARG);
    }
    rdst::search_device<std::uint32_t, std::uint64_t>(a.p, 64, a.p, 0, p.p, nullptr, s.p, 8192);  // no needles: nothing to do
    printf("ok\n");
    return 0;
}
