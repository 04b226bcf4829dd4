// C++ caller of include/rdst.hpp for keys described by a field table: a #[repr(C)]-style struct ordered by (u16, i64)
// through rdst::sort_records_by against std::stable_sort, the packed form of the same struct (fields at odd offsets), a
// descending field, and the three keys of the reference's examples/impl_radix_key.rs.  Built and run by
// tests/test_gpu_fields_cpp.py.  Exit code 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <tuple>
#include <vector>

#include "rdst.hpp"

#define PROGRESS(what, n) do { std::fprintf(stderr, "[check] %s n=%zu\n", what, (std::size_t)(n)); std::fflush(stderr); } while (0)

struct Event {  // #[repr(C)] struct Event { tenant: u16, flags: u8, ts: i64, seq: u32 }
    std::uint16_t tenant;
    std::uint8_t flags;
    std::int64_t ts;
    std::uint32_t seq;
};

#pragma pack(push, 1)
struct PackedEvent {  // #[repr(C, packed)]: ts at offset 3
    std::uint8_t flags;
    std::uint16_t tenant;
    std::int64_t ts;
    std::uint32_t seq;
};
#pragma pack(pop)

template <typename E>
static std::vector<E> events(std::size_t n, unsigned seed) {
    std::mt19937_64 rng(seed);
    const std::int64_t specials[] = {INT64_MIN, -1, 0, 1, INT64_MAX};
    std::vector<E> v(n);
    for (std::size_t i = 0; i < n; ++i) {
        std::memset(&v[i], 0, sizeof(E));  // the padding too: rows are compared as bytes
        v[i].tenant = static_cast<std::uint16_t>(rng() % 7 * 9000);
        v[i].flags = static_cast<std::uint8_t>(i);
        v[i].ts = rng() % 4 == 0 ? specials[rng() % 5] : static_cast<std::int64_t>(rng()) >> (rng() % 60);
        if (i % 3 == 1) { v[i].tenant = v[i - 1].tenant; v[i].ts = v[i - 1].ts; }  // equal keys that must keep their order
        v[i].seq = static_cast<std::uint32_t>(i);
    }
    return v;
}

template <typename E>
static int check_events(std::size_t n, unsigned seed, bool ts_descending) {
    PROGRESS(__PRETTY_FUNCTION__, n);
    auto v = events<E>(n, seed);
    auto expect = v;
    std::stable_sort(expect.begin(), expect.end(), [&](const E& a, const E& b) {
        const std::uint16_t ta = a.tenant, tb = b.tenant;
        const std::int64_t sa = a.ts, sb = b.ts;
        return ts_descending ? std::make_tuple(ta, sb) < std::make_tuple(tb, sa) : std::make_tuple(ta, sa) < std::make_tuple(tb, sb);
    });
    if (ts_descending) rdst::sort_records_by(v, {RDST_FIELD(E, tenant, RDST_KEY_UNSIGNED), RDST_FIELD_DESC(E, ts, RDST_KEY_SIGNED)});
    else rdst::sort_records_by(v.data(), v.size(), {RDST_FIELD(E, tenant, RDST_KEY_UNSIGNED), RDST_FIELD(E, ts, RDST_KEY_SIGNED)});
    return std::memcmp(v.data(), expect.data(), n * sizeof(E)) == 0 ? 0 : 1;
}

struct PackedU8 { std::uint8_t b[4]; };  // examples/impl_radix_key.rs

static int check_example() {
    PROGRESS("impl_radix_key example", 3);
    auto same = [](const std::vector<PackedU8>& v, const std::uint8_t (&e)[3][4]) { return std::memcmp(v.data(), e, 12) == 0; };
    int bad = 0;
    std::vector<PackedU8> v = {{{3, 2, 2, 3}}, {{2, 2, 2, 2}}, {{3, 1, 3, 1}}};
    rdst::sort_records_by(v, {RDST_FIELD(PackedU8, b, RDST_KEY_BYTES_BE)});  // all bytes
    const std::uint8_t all[3][4] = {{2, 2, 2, 2}, {3, 1, 3, 1}, {3, 2, 2, 3}};
    bad += !same(v, all);
    auto even = v, odd = v;
    rdst::sort_records_by(even, {{1, 1, RDST_KEY_UNSIGNED, 0}, {3, 1, RDST_KEY_UNSIGNED, 0}});  // LEVELS = 2, get_level(l) = b[3 - 2 l]
    const std::uint8_t by_even[3][4] = {{3, 1, 3, 1}, {2, 2, 2, 2}, {3, 2, 2, 3}};
    bad += !same(even, by_even);
    rdst::sort_records_by(odd, {{0, 1, RDST_KEY_UNSIGNED, 0}, {2, 1, RDST_KEY_UNSIGNED, 0}});   // get_level(l) = b[3 - (2 l + 1)]
    const std::uint8_t by_odd[3][4] = {{2, 2, 2, 2}, {3, 2, 2, 3}, {3, 1, 3, 1}};
    bad += !same(odd, by_odd);
    return bad;
}

static int check_errors() {
    PROGRESS("errors", 4);
    std::vector<Event> v = events<Event>(4, 9);
    const auto before = v;
    int bad = 0;
    try {
        rdst::sort_records_by(v, {});
        ++bad;
    } catch (const rdst::Error& e) { bad += e.status != RDST_ERR_ARG; }
    try {
        rdst::sort_records_by(v, {{20, 8, RDST_KEY_SIGNED, 0}});  // past the 24-byte record
        ++bad;
    } catch (const rdst::Error& e) { bad += e.status != RDST_ERR_ARG; }
    bad += std::memcmp(v.data(), before.data(), v.size() * sizeof(Event)) != 0;
    return bad;
}

int main() {
    static_assert(sizeof(Event) == 24 && offsetof(Event, ts) == 8, "the repr(C) layout");
    static_assert(sizeof(PackedEvent) == 15 && offsetof(PackedEvent, ts) == 3, "the packed layout");
    int bad = check_errors();
    bad += check_example();
    for (std::size_t n : {2ul, 3ul, 1000ul, 100003ul}) {
        bad += check_events<Event>(n, 1, false);
        bad += check_events<Event>(n, 2, true);
        bad += check_events<PackedEvent>(n, 3, false);
        bad += check_events<PackedEvent>(n, 4, true);
    }
    std::printf("%s\n", bad ? "FAIL" : "ok");
    return bad ? 1 : 0;
}
