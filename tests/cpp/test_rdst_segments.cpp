// Stand-alone check of rdst_segments.cpp (host only; built by tests/test_segments_plan.py with -fsanitize=address,undefined):
// the work list of hand-made and seeded random offset tables against the documented order, with exactly sized buffers
// so that a write past the list shows.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "rdst_hip.h"

static std::string g_error;
namespace rdst_internal {
int note_error(int code, const char* what) {  // the library's own lives in rdst_kernels.hip
    g_error = what;
    return code;
}
}  // namespace rdst_internal

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

struct Seg { uint64_t start, len; uint32_t seg; };

static void check_table(const std::vector<uint64_t>& off, uint64_t len, uint32_t kb, uint32_t vb) {
    uint32_t lim[2];
    CHECK(rdst_hip_sort_segments_limits(kb, vb, lim) == RDST_OK);
    const uint64_t nseg = off.size() - 1;
    std::vector<Seg> wave, block, lng;
    uint64_t longest = 0;
    for (uint64_t s = 0; s < nseg; ++s) {
        const uint64_t n = off[s + 1] - off[s];
        if (n < 2) continue;
        const Seg x{off[s], n, (uint32_t)s};
        if (n <= lim[0]) wave.push_back(x);
        else if (n <= lim[1]) block.push_back(x);
        else { lng.push_back(x); longest = std::max(longest, n); }
    }
    std::stable_sort(block.begin(), block.end(), [](const Seg& a, const Seg& b) { return a.len > b.len; });
    std::vector<Seg> want = wave;
    want.insert(want.end(), block.begin(), block.end());
    want.insert(want.end(), lng.begin(), lng.end());
    uint64_t counts[3] = {9, 9, 9}, tmp = 9;
    std::vector<rdst_segment_item> items(want.size());  // exactly the list: one item more is a heap overflow
    CHECK(rdst_segments_plan(off.data(), nseg, len, kb, vb, items.data(), items.size(), counts, &tmp) == RDST_OK);
    CHECK(counts[0] == wave.size() && counts[1] == block.size() && counts[2] == lng.size() && tmp == longest);
    for (size_t i = 0; i < want.size(); ++i) CHECK(items[i].start == want[i].start && items[i].len == want[i].len && items[i].seg == want[i].seg);
    if (!want.empty()) {
        std::vector<rdst_segment_item> fewer(want.size() - 1);
        uint64_t c2[3] = {9, 9, 9}, t2 = 9;
        g_error.clear();
        CHECK(rdst_segments_plan(off.data(), nseg, len, kb, vb, fewer.data(), fewer.size(), c2, &t2) == RDST_ERR_ARG);
        CHECK(!g_error.empty() && c2[0] == counts[0] && c2[1] == counts[1] && c2[2] == counts[2] && t2 == tmp);
    }
}

int main() {
    const uint32_t widths[][2] = {{1, 0}, {2, 0}, {4, 0}, {8, 0}, {16, 0}, {4, 4}, {4, 8}, {8, 4}, {8, 8}};
    std::mt19937_64 rng(0x5E65);
    for (const auto& w : widths) {
        uint32_t lim[2];
        CHECK(rdst_hip_sort_segments_limits(w[0], w[1], lim) == RDST_OK);
        CHECK(lim[0] >= 64 && lim[0] < lim[1] && lim[1] >= 4096);
        const uint64_t wm = lim[0], bm = lim[1];
        const uint64_t lengths[] = {0, 0, 1, 2, 3, 63, 64, 65, wm - 1, wm, wm + 1, 1023, 1024, 1025, bm - 1, bm, bm + 1, 2 * bm + 17, bm, wm + 1, 0};
        std::vector<uint64_t> off{5};
        for (uint64_t n : lengths) off.push_back(off.back() + n);
        check_table(off, off.back() + 7, w[0], w[1]);
        for (int t = 0; t < 50; ++t) {
            const uint64_t nseg = 1 + rng() % 300;
            std::vector<uint64_t> r{rng() % 9};
            for (uint64_t s = 0; s < nseg; ++s) {
                uint64_t n;
                switch (rng() % 4) {
                    case 0: n = rng() % 4; break;
                    case 1: n = rng() % (wm + 2); break;
                    case 2: n = wm + rng() % (bm + 2 - wm); break;
                    default: n = bm + rng() % (2 * bm); break;
                }
                r.push_back(r.back() + n);
            }
            check_table(r, r.back() + rng() % 3, w[0], w[1]);
        }
    }
    uint64_t counts[3], tmp;
    // zero segments (NULL offsets are fine), all-empty segments, bad tables
    CHECK(rdst_segments_plan(nullptr, 0, 10, 4, 0, nullptr, 0, counts, &tmp) == RDST_OK && counts[0] + counts[1] + counts[2] == 0 && tmp == 0);
    const uint64_t empty[] = {0, 0, 1, 1, 2, 2};
    CHECK(rdst_segments_plan(empty, 5, 2, 4, 0, nullptr, 0, counts, &tmp) == RDST_OK && counts[0] + counts[1] + counts[2] == 0);
    const uint64_t decreasing[] = {0, 10, 9, 20};
    CHECK(rdst_segments_plan(decreasing, 3, 20, 4, 0, nullptr, 0, counts, &tmp) == RDST_ERR_ARG);
    const uint64_t past[] = {0, 10, 21};
    CHECK(rdst_segments_plan(past, 2, 20, 4, 0, nullptr, 0, counts, &tmp) == RDST_ERR_ARG);
    CHECK(rdst_segments_plan(nullptr, 2, 20, 4, 0, nullptr, 0, counts, &tmp) == RDST_ERR_ARG);
    CHECK(rdst_segments_plan(past, 2, 21, 3, 0, nullptr, 0, counts, &tmp) == RDST_ERR_UNSUPPORTED);
    CHECK(rdst_segments_plan(past, 2, 21, 2, 4, nullptr, 0, counts, &tmp) == RDST_ERR_UNSUPPORTED);
    uint32_t lim[2];
    CHECK(rdst_hip_sort_segments_limits(4, 2, lim) == RDST_ERR_UNSUPPORTED);
    printf("ok\n");
    return 0;
}
