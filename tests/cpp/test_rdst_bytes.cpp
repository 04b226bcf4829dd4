// C++ caller of include/rdst.hpp for [u8; N] keys wider than 16 bytes: std::array<std::uint8_t, N> slices against
// std::sort, and structs keyed by such a field against std::stable_sort.  Built and run by tests/test_gpu_bytes_cpp.py.
// Exit code 0 = all checks passed.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "rdst.hpp"

#define PROGRESS(what, n) do { std::fprintf(stderr, "[check] %s n=%zu\n", what, (std::size_t)(n)); std::fflush(stderr); } while (0)

template <std::size_t N>
static std::array<std::uint8_t, N> random_key(std::mt19937_64& rng, unsigned prefix) {
    std::array<std::uint8_t, N> k{};
    for (std::size_t i = 0; i < N; ++i) {
        const std::uint8_t b = static_cast<std::uint8_t>(rng());
        k[i] = i < prefix ? 0x5a : (rng() % 10 < 3 ? 0 : b);  // a shared prefix, then 30 % zeros
    }
    return k;
}

template <std::size_t N>
static int check_array(std::size_t n, unsigned prefix, unsigned seed) {
    PROGRESS(__PRETTY_FUNCTION__, n);
    static_assert(rdst::RadixKey<std::array<std::uint8_t, N>>::LEVELS == N, "LEVELS = N");
    std::mt19937_64 rng(seed);
    std::vector<std::array<std::uint8_t, N>> v(n);
    for (auto& x : v) x = random_key<N>(rng, prefix);
    for (std::size_t i = 0; i + 7 < n; i += 7) v[i + 3] = v[i];  // duplicates
    auto expect = v;
    std::sort(expect.begin(), expect.end());  // std::array compares lexicographically, as [u8; N] does
    rdst::radix_sort_unstable(v);
    return v == expect ? 0 : 1;
}

template <std::size_t N>
struct Row {
    std::uint8_t tag;
    std::array<std::uint8_t, N> id;
    std::uint32_t seq;
    std::uint8_t pad[3];
};

template <std::size_t N>
static int check_field(std::size_t n, unsigned seed) {
    PROGRESS(__PRETTY_FUNCTION__, n);
    std::mt19937_64 rng(seed);
    std::vector<Row<N>> v(n);
    for (std::size_t i = 0; i < n; ++i) {
        v[i].tag = static_cast<std::uint8_t>(i);
        v[i].id = random_key<N>(rng, 0);
        v[i].id[0] &= 3;  // few distinct leading bytes ...
        if (i % 3 == 1) v[i].id = v[i - 1].id;  // ... and equal keys that must keep their order
        v[i].seq = static_cast<std::uint32_t>(i);
    }
    auto expect = v;
    std::stable_sort(expect.begin(), expect.end(), [](const Row<N>& a, const Row<N>& b) { return a.id < b.id; });
    rdst::radix_sort_unstable_by_field(v, &Row<N>::id);
    for (std::size_t i = 0; i < n; ++i)
        if (v[i].seq != expect[i].seq || v[i].id != expect[i].id || v[i].tag != expect[i].tag) return 1;
    return 0;
}

int main() {
    int bad = 0;
    for (std::size_t n : {2ul, 3ul, 1000ul, 100003ul}) {
        bad += check_array<20>(n, 0, 1);
        bad += check_array<32>(n, 0, 2);
        bad += check_array<64>(n, 0, 3);
        bad += check_array<32>(n, 20, 4);  // rounds past the prefix
        bad += check_array<64>(n, 59, 5);
        bad += check_field<20>(n, 6);
        bad += check_field<32>(n, 7);
    }
    bad += check_field<3>(5000, 8);
    std::printf("%s\n", bad ? "FAIL" : "ok");
    return bad ? 1 : 0;
}
