// C++ caller of include/rdst.hpp for the wide-key sorts that never visit the host (rdst::sort_bytes_device_nowait,
// rdst::sort_records_by_device_nowait): [u8; N] rows against std::stable_sort at the chunk borders of the round loop, with
// random rows (no tied prefixes) and with rows that share their first bytes; structs ordered by a described key of 8, 10 and
// 26 bytes against std::stable_sort on the fields, a payload telling the input order of equal keys.
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// shared: the number of leading bytes every row has in common (0: random rows)
template <std::size_t N>
static void run_bytes(size_t n, size_t shared, uint64_t seed) {
    using Row = std::array<std::uint8_t, N>;
    std::mt19937_64 rng(seed);
    std::vector<Row> rows(n);
    for (Row& r : rows)
        for (size_t b = 0; b < N; ++b) r[b] = b < shared ? static_cast<std::uint8_t>(17 * b + 3) : static_cast<std::uint8_t>(rng() % (shared ? 3 : 256));
    std::vector<Row> want = rows;
    std::stable_sort(want.begin(), want.end());
    DeviceArray<Row> d_rows(rows);
    const size_t scratch_bytes = rdst_hip_sort_bytes_scratch_bytes(n, N);
    CHECK(scratch_bytes >= n * N);
    DeviceArray<unsigned char> d_scratch(scratch_bytes);
    rdst::sort_bytes_device_nowait<N>(d_rows.p, n, d_scratch.p, scratch_bytes);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    CHECK(d_rows.host() == want);
}

#pragma pack(push, 1)
struct Event {
    std::uint8_t tag;
    std::uint16_t tenant;
    std::int64_t ts;
    float score;
    std::array<std::uint8_t, 12> id;
    std::uint32_t seq;  // payload: the input position
};
#pragma pack(pop)
static_assert(sizeof(Event) == 31, "packed");

static bool same(const Event& a, const Event& b) {
    return a.tag == b.tag && a.tenant == b.tenant && a.ts == b.ts && a.score == b.score && a.id == b.id && a.seq == b.seq;
}

template <typename Less>
static void run_records(size_t n, std::initializer_list<rdst_key_field> fields, Less less, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<Event> v(n);
    for (size_t i = 0; i < n; ++i) {
        v[i].tag = static_cast<std::uint8_t>(rng() % 3);
        v[i].tenant = static_cast<std::uint16_t>(rng() % 5);
        v[i].ts = static_cast<std::int64_t>(rng() % 7) - 3;
        v[i].score = static_cast<float>(static_cast<int>(rng() % 9) - 4) * 0.5f;
        for (std::uint8_t& b : v[i].id) b = static_cast<std::uint8_t>(rng() % 2);
        v[i].seq = static_cast<std::uint32_t>(i);
    }
    std::vector<Event> want = v;
    std::stable_sort(want.begin(), want.end(), less);
    DeviceArray<Event> d(v);
    const size_t scratch_bytes = rdst_hip_sort_records_by_fields_scratch_bytes(n, sizeof(Event), fields.begin(), static_cast<std::uint32_t>(fields.size()));
    CHECK(scratch_bytes >= n * sizeof(Event));
    DeviceArray<unsigned char> d_scratch(scratch_bytes);
    rdst::sort_records_by_device_nowait(d.p, n, fields, d_scratch.p, scratch_bytes);
    CHECK(rdst_hip_device_status(nullptr) == RDST_OK);
    const std::vector<Event> got = d.host();
    for (size_t i = 0; i < n; ++i) CHECK(same(got[i], want[i]));
}

int main() {
    for (size_t n : {size_t(2), size_t(3), size_t(300), size_t(20001)}) {
        run_bytes<3>(n, 0, 1);      // forwarded: the widened integer route
        run_bytes<16>(n, 9, 2);
        run_bytes<17>(n, 0, 3);     // no tied prefix: every round's keys are 0
        run_bytes<17>(n, 16, 4);    // decided in the one-byte last chunk
        run_bytes<24>(n, 10, 5);
        run_bytes<25>(n, 8, 6);
        run_bytes<32>(n, 31, 7);
        run_bytes<64>(n, 20, 8);
        run_bytes<128>(n, 120, 9);
        run_bytes<128>(n, 0, 10);
    }
    for (size_t n : {size_t(2), size_t(300), size_t(20001)}) {
        // L = 8: one pair sort (forwarded)
        run_records(n, {RDST_FIELD(Event, ts, RDST_KEY_SIGNED)}, [](const Event& a, const Event& b) { return a.ts < b.ts; }, 20);
        // L = 10: (u16, i64), the i64 descending
        run_records(n, {RDST_FIELD(Event, tenant, RDST_KEY_UNSIGNED), RDST_FIELD_DESC(Event, ts, RDST_KEY_SIGNED)},
                    [](const Event& a, const Event& b) { return a.tenant != b.tenant ? a.tenant < b.tenant : a.ts > b.ts; }, 21);
        // L = 26: a byte string, a float, a signed integer, two one-byte fields
        run_records(n,
                    {RDST_FIELD(Event, id, RDST_KEY_BYTES_BE), RDST_FIELD(Event, score, RDST_KEY_FLOAT), RDST_FIELD(Event, ts, RDST_KEY_SIGNED),
                     RDST_FIELD_DESC(Event, tag, RDST_KEY_UNSIGNED), RDST_FIELD(Event, tag, RDST_KEY_UNSIGNED)},
                    [](const Event& a, const Event& b) {
                        if (a.id != b.id) return a.id < b.id;
                        if (a.score != b.score) return a.score < b.score;
                        if (a.ts != b.ts) return a.ts < b.ts;
                        return a.tag > b.tag;
                    },
                    22);
    }
    // a key past the cap, a scratch one byte short: both throw, with the C entry's status
    {
        DeviceArray<Event> d(4);
        DeviceArray<unsigned char> d_scratch(1 << 16);
        int threw = 0;
        try {
            const std::initializer_list<rdst_key_field> two = {RDST_FIELD(Event, tenant, RDST_KEY_UNSIGNED), RDST_FIELD(Event, ts, RDST_KEY_SIGNED)};
            rdst::sort_records_by_device_nowait(d.p, 4, two, d_scratch.p, rdst_hip_sort_records_by_fields_scratch_bytes(4, sizeof(Event), two.begin(), 2) - 1);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_ARG;
        }
        try {
            std::initializer_list<rdst_key_field> wide = {RDST_FIELD(Event, id, RDST_KEY_BYTES_BE), RDST_FIELD(Event, id, RDST_KEY_BYTES_BE),
                                                          RDST_FIELD(Event, id, RDST_KEY_BYTES_BE), RDST_FIELD(Event, id, RDST_KEY_BYTES_BE),
                                                          RDST_FIELD(Event, id, RDST_KEY_BYTES_BE), RDST_FIELD(Event, id, RDST_KEY_BYTES_BE),
                                                          RDST_FIELD(Event, id, RDST_KEY_BYTES_BE), RDST_FIELD(Event, id, RDST_KEY_BYTES_BE),
                                                          RDST_FIELD(Event, id, RDST_KEY_BYTES_BE), RDST_FIELD(Event, id, RDST_KEY_BYTES_BE),
                                                          RDST_FIELD(Event, tenant, RDST_KEY_UNSIGNED), RDST_FIELD(Event, ts, RDST_KEY_SIGNED)};  // 130 bytes
            rdst::sort_records_by_device_nowait(d.p, 4, wide, d_scratch.p, 1 << 16);
        } catch (const rdst::Error& e) {
            threw += e.status == RDST_ERR_UNSUPPORTED;
        }
        CHECK(threw == 2);
    }
    printf("ok\n");
    return 0;
}
