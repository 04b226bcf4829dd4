// Stand-alone check of the host-only half of rdst_hip_select_segments_device_offsets (built by
// tests/test_select_segments_offsets_abi.py with -fsanitize=address,undefined from rdst_rank_args.cpp and
// rdst_segments.cpp): the scratch-size function over edge values — zeros, the sum it documents, monotone in every argument —,
// and the plan it runs on: sorting the class keys of a table for k = 1 (rdst_segments_layout.h) gives the order of
// rdst_topk_segments_plan with k = 1, with the stream class bounded (wait mode) and unbounded (asynchronous mode).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "rdst_hip.h"
#include "../../rdst_amd/csrc/rdst_segments_layout.h"

namespace L = rdst_segments_layout;

static std::string g_error;
namespace rdst_internal {
int note_error(int code, const char* what) {  // the library's own lives in rdst_kernels.hip
    g_error = what;
    return code;
}
// the library's own lives in rdst_kernels.hip too; nothing here reaches the entries' checks, which call it
int check_key_args(const void*, uint64_t, uint32_t, rdst_key_kind, uint32_t) { return note_error(RDST_ERR_ARG, "not reached"); }
}  // namespace rdst_internal

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static const uint32_t WIDTHS[9][2] = {{1, 0}, {2, 0}, {4, 0}, {8, 0}, {16, 0}, {4, 4}, {4, 8}, {8, 4}, {8, 8}};

static void check_scratch_bytes() {
    const auto f = rdst_hip_select_segments_device_offsets_scratch_bytes;
    for (uint32_t kb : {0u, 3u, 5u, 32u}) CHECK(f(10, 100, 5, kb, 0) == 0);
    for (uint32_t kb : {1u, 2u, 16u}) CHECK(f(10, 100, 5, kb, 4) == 0 && f(10, 100, 5, kb, 0) > 0);
    CHECK(f(10, 100, 5, 4, 3) == 0);
    CHECK(f(0, 100, 5, 4, 0) == 0 && f((1ull << 30) + 1, 100, 5, 4, 0) == 0 && f(1ull << 30, 0, 5, 4, 0) > 0);
    CHECK(f(10, 1ull << 32, 5, 4, 0) == 0 && f(10, ~0ull, 5, 4, 0) == 0 && f(10, (1ull << 32) - 1, 5, 4, 0) > 0);
    const std::vector<uint64_t> segs{1, 2, 63, 64, 65, 1000, 1000000, 1ull << 30};
    const std::vector<uint64_t> fars{0, 1, 2, 4096, 4097, 1ull << 17, (1ull << 17) + 1, 1ull << 24, (1ull << 32) - 1};
    const std::vector<uint64_t> nrs{0, 1, 32, 33, 70, 1ull << 21, 1ull << 40, ~0ull};
    for (const auto& w : WIDTHS) {
        for (size_t i = 0; i < segs.size(); ++i) {
            const uint64_t plan = rdst_hip_sort_segments_device_offsets_scratch_bytes(segs[i]);
            CHECK(plan == L::plan_layout(segs[i]).total && plan % 256 == 0 && plan >= 256 + 32 * segs[i]);
            for (size_t j = 0; j < fars.size(); ++j)
                for (size_t m = 0; m < nrs.size(); ++m) {
                    const uint64_t got = f(segs[i], fars[j], nrs[m], w[0], w[1]);
                    CHECK(got == f(segs[i], fars[j], nrs[m], w[0], w[1]));  // pure
                    CHECK(got == plan + (fars[j] ? rdst_hip_select_scratch_bytes(fars[j], nrs[m], w[0], w[1], 0) : 0));
                    if (i) CHECK(f(segs[i - 1], fars[j], nrs[m], w[0], w[1]) <= got);  // monotone in all three
                    if (j) CHECK(f(segs[i], fars[j - 1], nrs[m], w[0], w[1]) <= got);
                    if (m) CHECK(f(segs[i], fars[j], nrs[m - 1], w[0], w[1]) <= got);
                }
        }
    }
}

// (key, segment) pairs sorted by the key, stable — what the device plan's pair sort does — against rdst_topk_segments_plan, k = 1
static void check_class_keys(const std::vector<uint64_t>& off, uint32_t kb, uint32_t ib) {
    uint32_t lim[4], topk[4];
    CHECK(rdst_hip_select_segments_limits(kb, ib, lim) == RDST_OK && rdst_hip_topk_segments_limits(kb, ib, topk) == RDST_OK);
    CHECK(lim[0] == topk[0] && lim[1] == topk[1] && lim[2] == topk[2] && lim[3] == L::SELECT_SEGMENTS_MAX_RANKS && topk[3] >= 1);
    const uint64_t nseg = off.size() - 1;
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    for (uint64_t s = 0; s < nseg; ++s) pairs.push_back({L::topk_class_key(off[s + 1] - off[s], lim[0], lim[1], lim[2]), (uint32_t)s});
    std::stable_sort(pairs.begin(), pairs.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<rdst_segment_item> items(nseg);
    uint64_t counts[4], longest = 0;
    CHECK(rdst_topk_segments_plan(off.data(), nseg, off.back(), 1, kb, ib, items.data(), nseg, counts, &longest) == RDST_OK);
    const uint64_t total = counts[0] + counts[1] + counts[2] + counts[3];
    for (uint64_t i = 0; i < nseg; ++i) {
        if (i < total) CHECK(pairs[i].first != L::TOPK_KEY_NONE && pairs[i].second == items[i].seg);
        else CHECK(pairs[i].first == L::TOPK_KEY_NONE);
    }
    // the asynchronous mode's keys: no far class, every far segment among the stream class, longest first
    uint64_t n_stream = 0;
    for (uint64_t s = 0; s < nseg; ++s) {
        const uint64_t n = off[s + 1] - off[s];
        const uint32_t key = L::topk_class_key(n, lim[0], lim[1], 0xFFFFFFFFu);
        CHECK(key != L::TOPK_KEY_FAR);
        if (n > lim[1]) {
            ++n_stream;
            CHECK(L::topk_class(n, lim[0], lim[1], 0xFFFFFFFFu) == 2);
        }
    }
    CHECK(n_stream == counts[2] + counts[3]);
}

int main() {
    check_scratch_bytes();
    std::mt19937_64 rng(11);
    for (const auto& w : WIDTHS) {
        uint32_t lim[4];
        CHECK(rdst_hip_select_segments_limits(w[0], w[1], lim) == RDST_OK);
        const uint64_t wm = lim[0], bm = lim[1];
        for (uint32_t border : {0u, (uint32_t)bm - 1, (uint32_t)(bm + 1000), 0xFFFFFFFFu}) {
            CHECK(rdst_hip_set_topk_segments_stream_max(border) == RDST_OK);
            CHECK(rdst_hip_select_segments_limits(w[0], w[1], lim) == RDST_OK);
            std::vector<uint64_t> lengths{0, 1, 2, wm, wm + 1, bm, bm + 1, bm + 1, 3 * bm, (uint64_t)lim[2], std::min<uint64_t>((uint64_t)lim[2] + 1, 0xFFFFFFFFull),
                                          wm, bm, 0, bm - 1};  // (an item's len saturates at 2^32 - 1)
            for (int i = 0; i < 40; ++i) lengths.push_back(rng() % (i % 4 == 0 ? 4 * bm : 2 * wm));
            std::shuffle(lengths.begin(), lengths.end(), rng);
            std::vector<uint64_t> off{5};
            for (uint64_t n : lengths) off.push_back(off.back() + n);
            check_class_keys(off, w[0], w[1]);
        }
        CHECK(rdst_hip_set_topk_segments_stream_max(0) == RDST_OK);
    }
    printf("ok\n");
    return 0;
}
