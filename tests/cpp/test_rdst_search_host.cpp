// Stand-alone check of the host-only half of rdst_hip_search_device (built by tests/test_search_abi.py with
// -fsanitize=address,undefined from rdst_search.cpp): the scratch-size function and the limits over edge values, the splitter
// positions of the layout, and the argument checks in their documented order over made-up pointers — none is ever
// dereferenced here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "rdst_hip.h"
#include "../../rdst_amd/csrc/rdst_search_layout.h"

namespace L = rdst_search_layout;

static std::string g_error;
namespace rdst_internal {
int note_error(int code, const char* what) {  // the library's own lives in rdst_kernels.hip
    g_error = what;
    return code;
}
// the library's own lives in rdst_kernels.hip too; here: the width, the pointer and its alignment
int check_key_args(const void* p, uint64_t len, uint32_t elem_bytes, rdst_key_kind, uint32_t levels) {
    if (!L::key_width_ok(elem_bytes)) return note_error(RDST_ERR_UNSUPPORTED, "width");
    if (levels != elem_bytes) return note_error(RDST_ERR_ARG, "levels");
    if (len > 0 && p == nullptr) return note_error(RDST_ERR_ARG, "null key pointer");
    if (reinterpret_cast<uintptr_t>(p) % elem_bytes) return note_error(RDST_ERR_ALIGN, "key pointer");
    return RDST_OK;
}
}  // namespace rdst_internal

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, g_error.c_str()); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

struct Call {
    void* hay = at(0x10000);
    uint64_t len = 1000;
    void* dev_len = nullptr;
    uint32_t len_bytes = 0;
    void* needles = at(0x20000);
    uint64_t n_needles = 500;
    void* lower = at(0x30000);
    void* upper = at(0x40000);
    uint32_t offset_bytes = 8;
    void* scratch = at(0x50000);
    uint64_t scratch_bytes = 1ull << 40;
    uint32_t elem_bytes = 4;
    rdst_key_kind kind = RDST_KEY_UNSIGNED;
    uint32_t flags = 0;
    int run() const {
        g_error.clear();
        return rdst_internal::search_check_args(hay, len, dev_len, len_bytes, needles, n_needles, lower, upper, offset_bytes, scratch, scratch_bytes, elem_bytes,
                                                kind, elem_bytes, flags);
    }
};

static bool said(const char* word) { return g_error.find(word) != std::string::npos; }

static void check_sizes() {
    for (uint32_t kb : {0u, 3u, 5u, 32u}) CHECK(rdst_hip_search_scratch_bytes(10, 10, kb) == 0);
    uint32_t lim[3];
    CHECK(rdst_hip_search_limits(4, nullptr) == RDST_ERR_ARG && rdst_hip_search_limits(3, lim) == RDST_ERR_UNSUPPORTED);
    const std::vector<uint64_t> sizes{0, 1, 2, 1023, 1024, 1025, 8192, 8193, 1000000, 1ull << 31, (1ull << 32) - 1};
    for (uint32_t kb : {1u, 2u, 4u, 8u, 16u}) {
        CHECK(rdst_hip_search_limits(kb, lim) == RDST_OK && lim[0] == 256u * (kb == 1 ? 16u : kb == 16 ? 4u : 8u) && lim[1] == L::SPLITTERS);
        CHECK(lim[2] == (kb == 16 ? 2048u : kb == 8 ? 4096u : 8192u) && lim[2] >= lim[1] && lim[2] * kb <= 32768u);   // the window holds the table; 32 KiB of LDS
        CHECK(rdst_hip_search_scratch_bytes(1ull << 32, 1, kb) == 0 && rdst_hip_search_scratch_bytes(1, 1ull << 32, kb) == 0);
        CHECK(rdst_hip_search_scratch_bytes(~0ull, 1, kb) == 0 && rdst_hip_search_scratch_bytes(1, ~0ull, kb) == 0);
        uint64_t before = 0;
        for (uint64_t n : sizes)
            for (uint64_t nn : sizes) {
                const uint64_t got = rdst_hip_search_scratch_bytes(n, nn, kb);
                CHECK(got == rdst_hip_search_scratch_bytes(n, nn, kb));          // pure
                CHECK(got == 256 + 1024ull * kb && got >= before && got % 256 == 0);  // the documented sum; monotone
                before = got;
            }
    }
}

// what the kernels rely on: splitter positions below m, never decreasing, and no gap longer than longest_gap(m)
static void check_splitters() {
    for (uint32_t m : {1u, 2u, 3u, 1023u, 1024u, 1025u, 2047u, 2048u, 2049u, 1000003u, 0x7FFFFFFFu, 0x80000000u, 0xC0000000u, 0xFFFFFFFFu}) {
        uint32_t prev = 0;
        CHECK(L::splitter_pos(0, m) == 0);
        for (uint32_t j = 0; j < L::SPLITTERS; ++j) {
            const uint32_t p = L::splitter_pos(j, m);
            CHECK(p < m && p >= prev);
            CHECK(j == 0 || p - prev <= L::longest_gap(m));   // the stretch [prev + 1, p] a search is left with
            prev = p;
        }
        CHECK(m - prev - 1 <= L::longest_gap(m));             // ... and [last + 1, m]
    }
}

static void check_order() {
    Call good;
    CHECK(good.run() == RDST_OK);
    Call c;
    // every later argument is wrong as well: the first check in the documented order answers
    Call all_bad;
    all_bad.dev_len = at(0x60001);
    all_bad.len_bytes = 3;
    all_bad.needles = nullptr;
    all_bad.offset_bytes = 3;
    all_bad.lower = nullptr;
    all_bad.upper = nullptr;
    all_bad.scratch = nullptr;
    c = all_bad; c.elem_bytes = 3; CHECK(c.run() == RDST_ERR_UNSUPPORTED && said("width"));                 // 1
    c = all_bad; c.kind = RDST_KEY_BYTES_BE; CHECK(c.run() == RDST_ERR_UNSUPPORTED && said("[u8; N]"));     // 2
    c = all_bad; c.len = 1ull << 32; c.flags = 2; CHECK(c.run() == RDST_ERR_UNSUPPORTED && said("2^32"));   // 3
    c = all_bad; c.n_needles = 1ull << 32; c.flags = 2; CHECK(c.run() == RDST_ERR_UNSUPPORTED && said("2^32"));
    c = all_bad; c.flags = 1; CHECK(c.run() == RDST_ERR_ARG && said("flag"));                               // 4
    c = all_bad; CHECK(c.run() == RDST_ERR_ARG && said("device-resident length"));                          // 5
    c = all_bad; c.len_bytes = 4; CHECK(c.run() == RDST_ERR_ALIGN && said("length pointer"));
    c = all_bad; c.dev_len = nullptr; CHECK(c.run() == RDST_ERR_ARG && said("null needle"));                // 6 (len_bytes is not looked at)
    c.needles = at(0x20002); CHECK(c.run() == RDST_ERR_ALIGN && said("needle pointer"));
    c.needles = at(0x20000); CHECK(c.run() == RDST_ERR_ARG && said("offset_bytes"));                        // 7
    c.offset_bytes = 4; CHECK(c.run() == RDST_ERR_ARG && said("both outputs"));                             // 8
    c.lower = at(0x30002); CHECK(c.run() == RDST_ERR_ALIGN && said("lower output"));
    c.lower = nullptr; c.upper = at(0x40002); CHECK(c.run() == RDST_ERR_ALIGN && said("upper output"));
    c.upper = at(0x10000 + 4 * 999); CHECK(c.run() == RDST_ERR_ARG && said("an output overlaps"));          // the last key
    c.upper = at(0x10000 + 4 * 1000); CHECK(c.run() == RDST_ERR_ARG && said("null scratch"));               // begins where the keys end
    c.upper = at(0x20000 - 4 * 500 + 4); CHECK(c.run() == RDST_ERR_ARG && said("an output overlaps"));      // its last slot is needles[0]
    c.upper = at(0x20000 - 4 * 500); CHECK(c.run() == RDST_ERR_ARG && said("null scratch"));
    c.lower = at(0x40000); c.upper = at(0x40000 + 4 * 499); CHECK(c.run() == RDST_ERR_ARG && said("overlap each other"));
    c.upper = at(0x40000 + 4 * 500); CHECK(c.run() == RDST_ERR_ARG && said("null scratch"));
    c.dev_len = at(0x40000 + 4 * 999); c.len_bytes = 4; CHECK(c.run() == RDST_ERR_ARG && said("an output overlaps"));   // the length in the last slot
    c.dev_len = at(0x40000 + 4 * 1000); CHECK(c.run() == RDST_ERR_ARG && said("null scratch"));
    // the inputs may overlap each other in any way: the same array, a part of it, the length inside it
    c = good; c.needles = c.hay; c.n_needles = 1000; c.upper = at(0x48000); CHECK(c.run() == RDST_OK);
    c = good; c.needles = at(0x10000 + 4 * 900); CHECK(c.run() == RDST_OK);
    c = good; c.dev_len = at(0x10000 + 8); c.len_bytes = 8; CHECK(c.run() == RDST_OK);
    // 9
    c = good; c.scratch = at(0x50080); CHECK(c.run() == RDST_ERR_ALIGN && said("scratch not aligned"));
    const uint64_t sb = rdst_hip_search_scratch_bytes(1000, 500, 4);
    c = good; c.scratch_bytes = sb - 1; CHECK(c.run() == RDST_ERR_ARG && said("rdst_hip_search_scratch_bytes"));
    c.scratch_bytes += 1; CHECK(c.run() == RDST_OK);
    // the scratch (its documented size, not scratch_bytes) overlaps nothing that is read or written
    c = good; c.scratch = at(0x10000 - sb + 256); CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));              // the haystack
    c = good; c.scratch = at(0x10000 - sb); CHECK(c.run() == RDST_OK);
    c = good; c.scratch = at(0x20000 + 4 * 500 / 256 * 256); CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));   // the last needle
    c = good; c.scratch = at(0x20000 + (4 * 500 + 255) / 256 * 256); CHECK(c.run() == RDST_OK);
    c = good; c.scratch = at(0x30000 + 8 * 499 / 256 * 256); CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));   // the lower output
    c = good; c.scratch = at(0x40000 - sb + 256); CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));              // the upper output
    c = good; c.dev_len = at(0x50008); c.len_bytes = 8; CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));
    c.dev_len = at(0x50000 + sb); CHECK(c.run() == RDST_OK);
    // len == 0 with a NULL haystack and n_needles == 0 with NULL needles are calls like any other; the largest counts do not wrap
    c = good; c.len = 0; c.hay = nullptr; CHECK(c.run() == RDST_OK);
    c = good; c.n_needles = 0; c.needles = nullptr; CHECK(c.run() == RDST_OK);
    c = good; c.hay = at(0x100000000ull); c.len = (1ull << 32) - 1; c.elem_bytes = 16; c.needles = at(0x1000); c.n_needles = 16; CHECK(c.run() == RDST_OK);
    c.lower = at(0x100000000ull + 16 * ((1ull << 32) - 2)); CHECK(c.run() == RDST_ERR_ARG && said("an output overlaps"));
    c = good; c.n_needles = (1ull << 32) - 1; CHECK(c.run() == RDST_ERR_ARG && said("overlap"));
    c = good; c.hay = at(~uintptr_t(0) - 15); c.elem_bytes = 16; c.len = 1000; CHECK(c.run() == RDST_OK);                   // saturates at the end of the address space
}

int main() {
    check_sizes();
    check_splitters();
    check_order();
    printf("ok\n");
    return 0;
}
