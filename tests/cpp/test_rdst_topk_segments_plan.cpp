// Stand-alone check of the segmented partial sort's plan in rdst_segments.cpp (host only; built by
// tests/test_topk_segments_inputs.py with -fsanitize=address,undefined): the work list of hand-made and seeded random offset
// tables against the documented order, at k on both sides of k_stream_max and stream borders on both sides of block_max, with
// exactly sized buffers so that a write past the list shows.
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

static void check_table(const std::vector<uint64_t>& off, uint64_t len, uint64_t k, uint32_t kb, uint32_t ib) {
    uint32_t lim[4];
    CHECK(rdst_hip_topk_segments_limits(kb, ib, lim) == RDST_OK);
    const uint64_t nseg = off.size() - 1;
    std::vector<Seg> cls[4];
    uint64_t longest = 0;
    for (uint64_t s = 0; s < nseg && k != 0; ++s) {
        const uint64_t n = off[s + 1] - off[s];
        if (n == 0) continue;  // a segment of ONE key is work
        const Seg x{off[s], n, (uint32_t)s};
        if (n <= lim[0]) cls[0].push_back(x);
        else if (n <= lim[1]) cls[1].push_back(x);
        else if (n <= lim[2] && k <= lim[3]) cls[2].push_back(x);
        else { cls[3].push_back(x); longest = std::max(longest, n); }
    }
    const auto longer = [](const Seg& a, const Seg& b) { return a.len > b.len; };
    std::stable_sort(cls[1].begin(), cls[1].end(), longer);
    std::stable_sort(cls[2].begin(), cls[2].end(), longer);
    std::vector<Seg> want;
    for (const auto& c : cls) want.insert(want.end(), c.begin(), c.end());
    uint64_t counts[4] = {9, 9, 9, 9}, far = 9;
    std::vector<rdst_segment_item> items(want.size());  // exactly the list: one item more is a heap overflow
    CHECK(rdst_topk_segments_plan(off.data(), nseg, len, k, kb, ib, items.data(), items.size(), counts, &far) == RDST_OK);
    for (int c = 0; c < 4; ++c) CHECK(counts[c] == cls[c].size());
    CHECK(far == longest);
    for (size_t i = 0; i < want.size(); ++i) CHECK(items[i].start == want[i].start && items[i].len == want[i].len && items[i].seg == want[i].seg);
    if (!want.empty()) {
        std::vector<rdst_segment_item> fewer(want.size() - 1);
        uint64_t c2[4] = {9, 9, 9, 9}, f2 = 9;
        g_error.clear();
        CHECK(rdst_topk_segments_plan(off.data(), nseg, len, k, kb, ib, fewer.data(), fewer.size(), c2, &f2) == RDST_ERR_ARG);
        CHECK(!g_error.empty() && c2[0] == counts[0] && c2[1] == counts[1] && c2[2] == counts[2] && c2[3] == counts[3] && f2 == far);
    }
}

int main() {
    const uint32_t widths[][2] = {{1, 0}, {2, 0}, {4, 0}, {8, 0}, {16, 0}, {4, 4}, {4, 8}, {8, 4}, {8, 8}};
    std::mt19937_64 rng(0x70B5);
    for (const auto& w : widths) {
        uint32_t lim[4];
        CHECK(rdst_hip_set_topk_segments_stream_max(0) == RDST_OK);
        CHECK(rdst_hip_topk_segments_limits(w[0], w[1], lim) == RDST_OK);
        CHECK(lim[0] >= 64 && lim[0] < lim[1] && lim[1] >= 4096 && lim[2] == (1u << 17) && lim[3] == lim[1]);
        const uint64_t wm = lim[0], bm = lim[1];
        for (uint32_t border : {0u, (uint32_t)bm, (uint32_t)(3 * bm), 1u}) {
            CHECK(rdst_hip_set_topk_segments_stream_max(border) == RDST_OK);
            CHECK(rdst_hip_topk_segments_limits(w[0], w[1], lim) == RDST_OK && lim[2] == std::max<uint64_t>(bm, border ? border : 1u << 17));
            const uint64_t lengths[] = {0, 0, 1, 2, 3, 63, 64, 65, wm - 1, wm, wm + 1, 1023, 1024, 1025, bm - 1, bm, bm + 1, 2 * bm + 17, 3 * bm, 3 * bm + 1, bm, wm + 1, 1, 0};
            std::vector<uint64_t> off{5};
            for (uint64_t n : lengths) off.push_back(off.back() + n);
            for (uint64_t k : {uint64_t(0), uint64_t(1), bm, bm + 1, uint64_t(1) << 40}) check_table(off, off.back() + 7, k, w[0], w[1]);
            for (int t = 0; t < 12; ++t) {
                const uint64_t nseg = 1 + rng() % 300;
                std::vector<uint64_t> r{rng() % 9};
                for (uint64_t s = 0; s < nseg; ++s) {
                    uint64_t n;
                    switch (rng() % 4) {
                        case 0: n = rng() % 4; break;
                        case 1: n = rng() % (wm + 2); break;
                        case 2: n = wm + rng() % (bm + 2 - wm); break;
                        default: n = bm + rng() % (4 * bm); break;
                    }
                    r.push_back(r.back() + n);
                }
                check_table(r, r.back() + rng() % 3, t % 2 ? bm + 1 - rng() % 2 : 1 + rng() % bm, w[0], w[1]);
            }
        }
    }
    CHECK(rdst_hip_set_topk_segments_stream_max(0) == RDST_OK);
    uint64_t counts[4], far;
    // zero segments (NULL offsets are fine), all-empty segments, bad tables
    CHECK(rdst_topk_segments_plan(nullptr, 0, 10, 3, 4, 0, nullptr, 0, counts, &far) == RDST_OK && counts[0] + counts[1] + counts[2] + counts[3] == 0 && far == 0);
    const uint64_t empty[] = {0, 0, 1, 1, 2, 2};
    CHECK(rdst_topk_segments_plan(empty, 5, 2, 3, 4, 0, nullptr, 0, counts, &far) == RDST_ERR_ARG && counts[0] == 2);  // two segments of one key
    const uint64_t decreasing[] = {0, 10, 9, 20};
    CHECK(rdst_topk_segments_plan(decreasing, 3, 20, 3, 4, 0, nullptr, 0, counts, &far) == RDST_ERR_ARG);
    const uint64_t past[] = {0, 10, 21};
    CHECK(rdst_topk_segments_plan(past, 2, 20, 3, 4, 0, nullptr, 0, counts, &far) == RDST_ERR_ARG);
    CHECK(rdst_topk_segments_plan(nullptr, 2, 20, 3, 4, 0, nullptr, 0, counts, &far) == RDST_ERR_ARG);
    CHECK(rdst_topk_segments_plan(past, 2, 21, 3, 3, 0, nullptr, 0, counts, &far) == RDST_ERR_UNSUPPORTED);
    CHECK(rdst_topk_segments_plan(past, 2, 21, 3, 2, 4, nullptr, 0, counts, &far) == RDST_ERR_UNSUPPORTED);
    CHECK(rdst_topk_segments_plan(past, 2, 21, 3, 4, 3, nullptr, 0, counts, &far) == RDST_ERR_ARG);
    uint32_t lim[4];
    CHECK(rdst_hip_topk_segments_limits(2, 8, lim) == RDST_ERR_UNSUPPORTED);
    printf("ok\n");
    return 0;
}
