// Stand-alone check of the host-only half of the six rank entries (built by tests/test_rank_args_host.py with
// -fsanitize=address,undefined from rdst_rank_args.cpp and rdst_segments.cpp): the address ranges of rdst_args.h at the end of
// the address space, the scratch layouts of rdst_topk_layout.h and rdst_select_layout.h over edge values, the two shared check
// steps in their documented order over made-up pointers — none is ever dereferenced here — and the size and limits functions.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "rdst_hip.h"
#include "../../rdst_amd/csrc/rdst_args.h"
#include "../../rdst_amd/csrc/rdst_segments_layout.h"
#include "../../rdst_amd/csrc/rdst_select_layout.h"
#include "../../rdst_amd/csrc/rdst_topk_layout.h"

namespace A = rdst_args;
namespace S = rdst_segments_layout;
namespace Q = rdst_select_layout;
namespace T = rdst_topk_layout;
typedef unsigned __int128 u128;

static std::string g_error;
namespace rdst_internal {
int note_error(int code, const char* what) {  // the library's own lives in rdst_kernels.hip; it keeps a copy too
    g_error = what;
    return code;
}
// the library's own lives in rdst_kernels.hip too; here: the width, the levels, the pointer and its alignment
int check_key_args(const void* p, uint64_t len, uint32_t elem_bytes, rdst_key_kind, uint32_t levels) {
    if (!A::key_width_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "width");
    if (levels != elem_bytes) return note_error(RDST_ERR_ARG, "levels");
    if (len > 0 && p == nullptr) return note_error(RDST_ERR_ARG, "null key pointer");
    if (reinterpret_cast<uintptr_t>(p) % elem_bytes) return note_error(RDST_ERR_ALIGN, "key pointer");
    return RDST_OK;
}
}  // namespace rdst_internal

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_error.c_str()); \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }
static bool said(const std::string& text) { return g_error == text; }
static const uint32_t WIDTHS[] = {1, 2, 4, 8, 16}, INDEX[] = {0, 4, 8};
static const uint64_t M32 = (1ull << 32) - 1;
static const std::vector<uint64_t> SIZES{0, 1, 2, 255, 256, 257, 1ull << 20, (1ull << 20) + 1, M32};  // len and k
static const std::vector<uint64_t> CAPS{1, 1ull << 20, M32, 0};                                       // ascending, then 0: the default

// ---- rdst_args.h: ranges ---------------------------------------------------------------------------------------------------------

static void check_ranges() {
    std::vector<uintptr_t> bases{0, 1, 0x10000};
    for (uintptr_t d = 0; d <= 16; ++d) bases.push_back(UINTPTR_MAX - d);
    for (uintptr_t base : bases)
        for (uint64_t elems : {(uint64_t)0, (uint64_t)1, M32, ~(uint64_t)0})
            for (uint64_t each : {(uint64_t)1, (uint64_t)16, (uint64_t)1 << 15}) {
                const A::Range r = A::range_of(at(base), elems, each);
                const u128 want = (u128)elems * each, room = UINTPTR_MAX - base;
                CHECK(r.lo == base && r.hi >= r.lo);                                        // never wrapped
                CHECK(r.hi - r.lo == (uintptr_t)(want <= room ? want : room));              // exact, or saturated at the last address
                if (elems == 0) {                                                           // an empty range overlaps nothing
                    const A::Range all{0, UINTPTR_MAX};
                    CHECK(r.lo == r.hi && !A::overlap(r, r) && !A::overlap(r, all) && !A::overlap(all, r));
                }
            }
    for (uintptr_t x : {(uintptr_t)0x1000, UINTPTR_MAX - 40}) {
        const A::Range a = A::range_of(at(x), 10, 1), one = A::range_of(at(x + 9), 11, 1), next = A::range_of(at(x + 10), 10, 1);
        CHECK(A::overlap(a, one) && A::overlap(one, a));      // they share exactly the byte x + 9
        CHECK(!A::overlap(a, next) && !A::overlap(next, a));  // adjacent
        CHECK(A::overlap(a, a) && A::overlap(one, next));
        const A::Range wide = A::range_of(at(x), 5, 2), inner = A::range_of(at(x + 4), 1, 1);
        CHECK(A::overlap(wide, inner) && A::overlap(inner, wide));
    }
    CHECK(A::misaligned(at(0x1001), 2) && !A::misaligned(at(0x1000), 256) && A::misaligned(at(0x1080), 256) && !A::misaligned(nullptr, 16));
    CHECK(A::align256(0) == 0 && A::align256(1) == 256 && A::align256(256) == 256 && A::align256(257) == 512);
    CHECK(A::levels_over(32, 12) == 3 && A::levels_over(8, 8) == 1 && A::levels_over(128, 12) == 11 && A::levels_over(24, 8) == 3);
    for (uint32_t kb = 0; kb <= 40; ++kb) {
        CHECK(A::key_width_ok(kb) == (kb == 1 || kb == 2 || kb == 4 || kb == 8 || kb == 16));
        CHECK(S::key_width_ok(kb) == A::key_width_ok(kb));
        for (uint32_t ib = 0; ib <= 9; ++ib)
            CHECK(A::index_widths_ok(kb, ib) == (ib == 0 || ((ib == 4 || ib == 8) && (kb == 4 || kb == 8))));
    }
}

// ---- the layouts -------------------------------------------------------------------------------------------------------------------

// the offsets of a layout, in order, and the bytes of the array that starts at each: every offset is a multiple of 256, the next
// one lies exactly the array's bytes rounded up to 256 further (so the offsets never decrease, and strictly increase past
// every array of at least one byte: only the two arrays of min(k, len) == 0 selected elements are empty), and the exact sum in
// 128 bits is the 64-bit total: nothing overflowed
static void check_offsets(const std::vector<uint64_t>& offsets, const std::vector<u128>& bytes, uint64_t total) {
    u128 sum = 0;
    for (size_t i = 0; i < offsets.size(); ++i) {
        CHECK(offsets[i] % 256 == 0 && (u128)offsets[i] == sum);
        const u128 room = (bytes[i] + 255) / 256 * 256;
        const uint64_t next = i + 1 < offsets.size() ? offsets[i + 1] : total;
        CHECK(next >= offsets[i] && (bytes[i] == 0 || next > offsets[i]));
        sum += room;
    }
    CHECK(sum == (u128)total && total % 256 == 0 && total < (1ull << 40));
}

static void check_layouts() {
    for (uint32_t kb : WIDTHS)
        for (uint32_t ib : INDEX) {
            const bool built = ib == 0 || kb == 4 || kb == 8;
            const u128 c_bytes = ib ? 2 * kb : kb;
            for (uint64_t len : SIZES)
                for (uint64_t cc : CAPS) {
                    const Q::SelectLayout q = Q::select_layout(len, kb, ib, cc);
                    CHECK(q.cap >= 1 && q.cap <= std::max<uint64_t>(len, 1) && q.cap == std::min<uint64_t>(cc ? cc : Q::DEFAULT_CAND_CAPACITY, std::max<uint64_t>(len, 1)));
                    check_offsets({0, q.table, q.counters, q.cand, q.cand_tmp},
                                  {Q::HEADER_BYTES, Q::TABLE_BYTES, (u128)Q::COUNTER_WORDS * 4, q.cap * c_bytes, q.cap * c_bytes}, q.total);
                    CHECK(rdst_hip_select_scratch_bytes(len, 7, kb, ib, cc) == (built ? q.total : 0));
                    CHECK(rdst_hip_select_scratch_bytes(len, ~0ull, kb, ib, cc) == (built ? q.total : 0));  // n_ranks costs nothing
                    for (uint64_t k : SIZES) {
                        const T::TopkLayout t = T::topk_layout(len, k, kb, ib, cc);
                        const u128 kk = std::min(k, len);
                        CHECK(t.cap >= 1 && t.cap <= std::max<uint64_t>(len, 1) && t.cap == std::min<uint64_t>(cc ? cc : T::DEFAULT_CAND_CAPACITY, std::max<uint64_t>(len, 1)));
                        check_offsets({0, t.counters, t.sel, t.sel_tmp, t.cand, t.cand_tmp},
                                      {T::HEADER_BYTES, (u128)T::COUNTERS * 4, kk * c_bytes, kk * c_bytes, t.cap * c_bytes, t.cap * c_bytes}, t.total);
                        CHECK(rdst_hip_topk_scratch_bytes(len, k, kb, ib, cc) == (built ? t.total : 0));
                    }
                }
            // monotone in each argument (cand_capacity from 1 on; 0 stands for the default), and the index width costs nothing
            for (size_t i = 0; i < SIZES.size(); ++i)
                for (size_t c = 0; c < CAPS.size(); ++c) {
                    const uint64_t len = SIZES[i], cc = CAPS[c];
                    const uint64_t q = Q::select_layout(len, kb, ib, cc).total;
                    if (i) CHECK(Q::select_layout(SIZES[i - 1], kb, ib, cc).total <= q);
                    if (c && cc) CHECK(Q::select_layout(len, kb, ib, CAPS[c - 1]).total <= q);
                    if (cc == 0) CHECK(q == Q::select_layout(len, kb, ib, Q::DEFAULT_CAND_CAPACITY).total);
                    if (ib) CHECK(Q::select_layout(len, kb, 0, cc).total <= q && q == Q::select_layout(len, kb, 12 - ib, cc).total);
                    for (size_t j = 0; j < SIZES.size(); ++j) {
                        const uint64_t k = SIZES[j], t = T::topk_layout(len, k, kb, ib, cc).total;
                        if (i) CHECK(T::topk_layout(SIZES[i - 1], k, kb, ib, cc).total <= t);
                        if (j) CHECK(T::topk_layout(len, SIZES[j - 1], kb, ib, cc).total <= t);
                        if (c && cc) CHECK(T::topk_layout(len, k, kb, ib, CAPS[c - 1]).total <= t);
                        if (cc == 0) CHECK(t == T::topk_layout(len, k, kb, ib, T::DEFAULT_CAND_CAPACITY).total);
                        if (ib) CHECK(T::topk_layout(len, k, kb, 0, cc).total <= t && t == T::topk_layout(len, k, kb, 12 - ib, cc).total);
                    }
                }
        }
    // what the headers promise in figures
    CHECK(rdst_hip_topk_scratch_bytes(1000000, 1000, 4, 0, 4096) == 256 + 4 * 4096 + 2 * 4096 + 2 * 16384);
    CHECK(rdst_hip_topk_scratch_bytes(100, 100, 8, 0, 0) == 256 + 4 * 4096 + 4 * 1024);  // the capacity never exceeds len
    CHECK(rdst_hip_select_scratch_bytes(1000000, 3, 4, 0, 4096) == 256 + 2304 + 65536 + 2 * 16384 && Q::TABLE_BYTES == 2304);
    for (uint32_t kb : {0u, 3u, 5u, 12u, 32u}) CHECK(rdst_hip_topk_scratch_bytes(1000, 10, kb, 0, 0) == 0 && rdst_hip_select_scratch_bytes(1000, 10, kb, 0, 0) == 0);
    for (uint32_t ib : {1u, 2u, 3u, 16u}) CHECK(rdst_hip_topk_scratch_bytes(1000, 10, 4, ib, 0) == 0 && rdst_hip_select_scratch_bytes(1000, 10, 4, ib, 0) == 0);
}

// ---- the two shared steps ------------------------------------------------------------------------------------------------------------

struct Head {
    const char* what;
    void* keys = at(0x10000);
    uint64_t len = 1000;
    uint32_t elem_bytes = 4, levels = 4;
    rdst_key_kind kind = RDST_KEY_UNSIGNED;
    int run() const {
        g_error.clear();
        return rdst_internal::rank_check_head(what, keys, len, elem_bytes, kind, levels);
    }
};

struct Outputs {
    const char* what;
    void* out_keys = at(0x20000);
    void* out_index = at(0x30000);
    uint32_t index_bytes = 4;
    void* scratch = at(0x50000);
    uint32_t elem_bytes = 4;
    uint32_t seen = 0;  // index_bytes as the step left it
    int run() {
        g_error.clear();
        seen = index_bytes;
        return rdst_internal::rank_check_outputs(what, out_keys, out_index, &seen, scratch, elem_bytes);
    }
};

static void check_steps(const char* what) {
    const std::string p = std::string(what) + ": ";
    // the head: every later step is broken as well, the first in the documented order answers
    Head good{what};
    CHECK(good.run() == RDST_OK);
    Head all_bad{what};
    all_bad.kind = RDST_KEY_BYTES_BE;
    all_bad.len = 1ull << 32;
    Head h = all_bad;
    h.elem_bytes = 3; CHECK(h.run() == RDST_ERR_UNSUPPORTED && said("width"));                      // the key arguments: the sort's own texts
    h = all_bad; h.levels = 3; CHECK(h.run() == RDST_ERR_ARG && said("levels"));
    h = all_bad; h.keys = nullptr; CHECK(h.run() == RDST_ERR_ARG && said("null key pointer"));
    h = all_bad; h.keys = at(0x10002); CHECK(h.run() == RDST_ERR_ALIGN && said("key pointer"));
    h = all_bad; CHECK(h.run() == RDST_ERR_UNSUPPORTED && said(p + "[u8; N] keys are not built"));
    h.kind = RDST_KEY_FLOAT; CHECK(h.run() == RDST_ERR_UNSUPPORTED && said(p + "len must be below 2^32"));
    h.len = ~0ull; CHECK(h.run() == RDST_ERR_UNSUPPORTED && said(p + "len must be below 2^32"));
    h.len = M32; CHECK(h.run() == RDST_OK);
    h.len = 0; h.keys = nullptr; CHECK(h.run() == RDST_OK);
    // the outputs and the scratch
    Outputs ok{what};
    CHECK(ok.run() == RDST_OK && ok.seen == 4);
    Outputs c{what};
    c.out_keys = nullptr; c.out_index = at(0x30001); c.index_bytes = 3; c.elem_bytes = 2; c.scratch = nullptr;
    CHECK(c.run() == RDST_ERR_ARG && said(p + "null key output"));                                     // 1
    c.out_keys = at(0x20001); CHECK(c.run() == RDST_ERR_ALIGN && said(p + "key output not aligned to the element size"));   // 2
    c.out_keys = at(0x20002);
    for (uint32_t ib : {0u, 1u, 2u, 3u, 5u, 16u}) {
        c.index_bytes = ib; CHECK(c.run() == RDST_ERR_ARG && said(p + "index_bytes must be 4 or 8"));  // 3
    }
    for (uint32_t ib : {4u, 8u})
        for (uint32_t kb : {1u, 2u, 16u}) {
            c.index_bytes = ib; c.elem_bytes = kb; c.out_keys = at(0x20000);
            CHECK(c.run() == RDST_ERR_UNSUPPORTED && said(p + "an index output takes 4- or 8-byte keys"));   // 4
        }
    c.elem_bytes = 8;
    for (uintptr_t off : {1, 2, 4}) {
        c.index_bytes = off == 4 ? 8 : 4; c.out_index = at(0x30000 + off);
        CHECK(c.run() == RDST_ERR_ALIGN && said(p + "index output not aligned to index_bytes"));       // 5
    }
    c.index_bytes = 4; CHECK(c.run() == RDST_ERR_ARG && said(p + "null scratch"));                     // 6 (0x30004 is aligned to 4)
    for (uintptr_t off : {1, 16, 128, 255}) {
        c.scratch = at(0x50000 + off); CHECK(c.run() == RDST_ERR_ALIGN && said(p + "scratch not aligned to 256 bytes"));   // 7
    }
    c.scratch = at(0x50100); CHECK(c.run() == RDST_OK && c.seen == 4);
    // without an index output index_bytes is not looked at, and comes back 0: every key width
    for (uint32_t kb : WIDTHS)
        for (uint32_t ib : {0u, 3u, 4u, 99u}) {
            Outputs k{what};
            k.out_index = nullptr; k.index_bytes = ib; k.elem_bytes = kb;
            CHECK(k.run() == RDST_OK && k.seen == 0);
            k.scratch = nullptr; CHECK(k.run() == RDST_ERR_ARG && said(p + "null scratch"));
        }
    // the scratch step alone (the blocking test hooks call it)
    g_error.clear();
    CHECK(rdst_internal::rank_check_scratch(what, nullptr) == RDST_ERR_ARG && said(p + "null scratch"));
    CHECK(rdst_internal::rank_check_scratch(what, at(0x50040)) == RDST_ERR_ALIGN && said(p + "scratch not aligned to 256 bytes"));
    CHECK(rdst_internal::rank_check_scratch(what, at(0x50000)) == RDST_OK);
}

// ---- the limits and the segmented sizes ------------------------------------------------------------------------------------------------

static void check_limits_and_sizes() {
    uint32_t t[3], q[5];
    // null output, then the key width, then the index width, then the keys an index takes
    CHECK(rdst_hip_topk_limits(3, 3, nullptr) == RDST_ERR_ARG && said("null output"));
    CHECK(rdst_hip_select_limits(3, 3, nullptr) == RDST_ERR_ARG && said("null output"));
    CHECK(rdst_hip_topk_limits(3, 3, t) == RDST_ERR_UNSUPPORTED && said("device path is built for 1-, 2-, 4-, 8- and 16-byte keys"));
    CHECK(rdst_hip_select_limits(32, 3, q) == RDST_ERR_UNSUPPORTED && said("device path is built for 1-, 2-, 4-, 8- and 16-byte keys"));
    CHECK(rdst_hip_topk_limits(2, 3, t) == RDST_ERR_ARG && said("topk: index_bytes must be 4 or 8"));
    CHECK(rdst_hip_select_limits(2, 3, q) == RDST_ERR_ARG && said("select: index_bytes must be 4 or 8"));
    CHECK(rdst_hip_topk_limits(2, 4, t) == RDST_ERR_UNSUPPORTED && said("topk: an index output takes 4- or 8-byte keys"));
    CHECK(rdst_hip_select_limits(16, 8, q) == RDST_ERR_UNSUPPORTED && said("select: an index output takes 4- or 8-byte keys"));
    const uint32_t topk_levels[] = {1, 2, 3, 6, 11}, select_levels[] = {1, 2, 4, 8, 16};
    for (int w = 0; w < 5; ++w)
        for (uint32_t ib : INDEX) {
            const uint32_t kb = WIDTHS[w];
            if (ib && kb != 4 && kb != 8) continue;
            CHECK(rdst_hip_topk_limits(kb, ib, t) == RDST_OK && t[0] == (kb == 1 ? 8u : 12u) && t[1] == 1u << 20 && t[2] == topk_levels[w] + (ib ? 3 : 0));
            CHECK(rdst_hip_select_limits(kb, ib, q) == RDST_OK && q[0] == 64 && q[1] == (kb == 1 ? 8u : 12u) && q[2] == 8 && q[3] == 1u << 24 &&
                  q[4] == select_levels[w] + (ib ? 4 : 0));
        }
    // borders on the host: the item table, and the whole-array scratch behind it exactly when a far segment is possible
    CHECK(S::table_bytes(0) == 0 && S::table_bytes(1) == 256 && S::table_bytes(16) == 256 && S::table_bytes(17) == 512);
    for (uint32_t kb : WIDTHS)
        for (uint32_t ib : INDEX) {
            if (ib && kb != 4 && kb != 8) {
                CHECK(rdst_hip_topk_segments_scratch_bytes(10, 100, 5, kb, ib) == 0 && rdst_hip_select_segments_scratch_bytes(10, 100, 5, kb, ib) == 0);
                continue;
            }
            uint32_t lim[4];
            CHECK(rdst_hip_topk_segments_limits(kb, ib, lim) == RDST_OK);
            CHECK(rdst_hip_topk_segments_scratch_bytes(0, 100, 5, kb, ib) == 0 && rdst_hip_topk_segments_scratch_bytes(1ull << 32, 100, 5, kb, ib) == 0);
            CHECK(rdst_hip_topk_segments_scratch_bytes(10, 1ull << 32, 5, kb, ib) == 0 && rdst_hip_select_segments_scratch_bytes(10, 1ull << 32, 5, kb, ib) == 0);
            CHECK(rdst_hip_select_segments_scratch_bytes(0, 100, 5, kb, ib) == 0 && rdst_hip_select_segments_scratch_bytes(1ull << 32, 100, 5, kb, ib) == 0);
            for (uint64_t nseg : {(uint64_t)1, (uint64_t)17, (uint64_t)1000000, M32})
                for (uint64_t longest : {(uint64_t)0, (uint64_t)1, (uint64_t)lim[1], (uint64_t)lim[1] + 1, (uint64_t)lim[2], (uint64_t)lim[2] + 1, M32})
                    for (uint64_t k : {(uint64_t)0, (uint64_t)1, (uint64_t)lim[3], (uint64_t)lim[3] + 1, ~(uint64_t)0}) {
                        const bool far = longest > lim[2] || (longest > lim[1] && k > lim[3]);
                        CHECK(rdst_hip_topk_segments_scratch_bytes(nseg, longest, k, kb, ib) ==
                              S::table_bytes(nseg) + (far ? rdst_hip_topk_scratch_bytes(longest, std::min(k, longest), kb, ib, 0) : 0));
                        CHECK(rdst_hip_select_segments_scratch_bytes(nseg, longest, k, kb, ib) ==
                              S::table_bytes(nseg) + (longest > lim[2] ? rdst_hip_select_scratch_bytes(longest, k, kb, ib, 0) : 0));
                    }
        }
}

int main() {
    check_ranges();
    check_layouts();
    check_steps("topk");
    check_steps("select");
    check_limits_and_sizes();
    printf("ok\n");
    return 0;
}
