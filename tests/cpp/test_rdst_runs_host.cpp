// Stand-alone check of the host-only half of rdst_hip_runs_device (built by tests/test_runs_abi.py with
// -fsanitize=address,undefined from rdst_runs.cpp): the scratch-size function and the limits over edge values, and the
// argument checks in their documented order over made-up pointers — none is ever dereferenced here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "rdst_hip.h"
#include "../../rdst_amd/csrc/rdst_runs_layout.h"

namespace L = rdst_runs_layout;

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
    void* keys = at(0x10000);
    uint64_t len = 1000;
    void* dev_len = nullptr;
    uint32_t len_bytes = 0;
    void* out_keys = at(0x20000);
    void* out_starts = at(0x30000);
    void* n_runs = at(0x40000);
    uint32_t offset_bytes = 8;
    uint64_t capacity = 1000;
    void* scratch = at(0x50000);
    uint64_t scratch_bytes = 1ull << 40;
    uint32_t elem_bytes = 4;
    rdst_key_kind kind = RDST_KEY_UNSIGNED;
    uint32_t flags = 0;
    int run() const {
        g_error.clear();
        return rdst_internal::runs_check_args(keys, len, dev_len, len_bytes, out_keys, out_starts, n_runs, offset_bytes, capacity, scratch, scratch_bytes,
                                              elem_bytes, kind, elem_bytes, flags);
    }
};

static bool said(const char* word) { return g_error.find(word) != std::string::npos; }

static void check_sizes() {
    for (uint32_t kb : {0u, 3u, 5u, 32u}) CHECK(rdst_hip_runs_scratch_bytes(10, kb) == 0);
    uint32_t lim[2];
    CHECK(rdst_hip_runs_limits(4, nullptr) == RDST_ERR_ARG && rdst_hip_runs_limits(3, lim) == RDST_ERR_UNSUPPORTED);
    const std::vector<uint64_t> lens{0, 1, 2, 4095, 4096, 4097, 16384, 16385, 1000000, 1ull << 31, (1ull << 32) - 1};
    for (uint32_t kb : {1u, 2u, 4u, 8u, 16u}) {
        CHECK(rdst_hip_runs_limits(kb, lim) == RDST_OK && lim[0] == (kb >= 8 ? 65536u : kb == 1 ? 16384u : 32768u) / kb && lim[1] == L::LOOKBACK_WINDOW);
        CHECK(rdst_hip_runs_scratch_bytes(1ull << 32, kb) == 0 && rdst_hip_runs_scratch_bytes(~0ull, kb) == 0);
        uint64_t before = 0;
        for (uint64_t n : lens) {
            const uint64_t got = rdst_hip_runs_scratch_bytes(n, kb);
            const uint64_t tiles = n == 0 ? 1 : (n + lim[0] - 1) / lim[0];
            CHECK(got == rdst_hip_runs_scratch_bytes(n, kb));                     // pure
            CHECK(got == 256 + (8 * tiles + 255) / 256 * 256 && got >= before);  // the documented sum; monotone
            before = got;
        }
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
    all_bad.offset_bytes = 3;
    all_bad.n_runs = nullptr;
    all_bad.out_keys = at(0x10000);
    all_bad.scratch = nullptr;
    c = all_bad; c.elem_bytes = 3; CHECK(c.run() == RDST_ERR_UNSUPPORTED && said("width"));          // 1
    c = all_bad; c.len = 1ull << 32; c.flags = 2; CHECK(c.run() == RDST_ERR_UNSUPPORTED && said("2^32"));  // 3
    c = all_bad; c.flags = 2; CHECK(c.run() == RDST_ERR_ARG && said("flag"));                           // 4
    c = all_bad; CHECK(c.run() == RDST_ERR_ARG && said("device-resident length"));                      // 5
    c = all_bad; c.len_bytes = 4; CHECK(c.run() == RDST_ERR_ALIGN && said("length pointer"));
    c = all_bad; c.dev_len = nullptr; CHECK(c.run() == RDST_ERR_ARG && said("offset_bytes"));             // 6 (len_bytes is not looked at)
    c.offset_bytes = 4; CHECK(c.run() == RDST_ERR_ARG && said("null run count"));                        // 7
    c.n_runs = at(0x40002); CHECK(c.run() == RDST_ERR_ALIGN && said("run count pointer"));
    c.n_runs = at(0x10000 + 4 * 999); CHECK(c.run() == RDST_ERR_ARG && said("run count overlaps the input"));
    c.n_runs = at(0x10000 + 4 * 1000); CHECK(c.run() == RDST_ERR_ARG && said("overlaps the input"));     // 8: the key output is the input
    c.out_keys = at(0x20002); CHECK(c.run() == RDST_ERR_ALIGN && said("key output"));
    c.out_keys = at(0x20000); c.out_starts = at(0x30002); CHECK(c.run() == RDST_ERR_ALIGN && said("starts output"));
    c.out_starts = at(0x10000 - 4 * 1001 + 4); CHECK(c.run() == RDST_ERR_ARG && said("overlaps the input"));   // its last slot is keys[0]
    c.out_starts = at(0x10000 - 4 * 1001); CHECK(c.run() == RDST_ERR_ARG && said("null scratch"));             // ends where the keys begin
    c.out_starts = at(0x20000 + 4 * 999); CHECK(c.run() == RDST_ERR_ARG && said("overlap each other"));
    c.out_starts = at(0x30000); c.n_runs = at(0x30000 + 4 * 1000); CHECK(c.run() == RDST_ERR_ARG && said("overlap each other"));
    c.n_runs = at(0x30000 + 4 * 1001); CHECK(c.run() == RDST_ERR_ARG && said("null scratch"));
    c.flags = RDST_RUNS_PAD_STARTS; c.out_starts = nullptr; CHECK(c.run() == RDST_ERR_ARG && said("RDST_RUNS_PAD_STARTS"));
    c.out_keys = nullptr; c.flags = 0; CHECK(c.run() == RDST_ERR_ARG && said("null scratch"));           // both outputs may be NULL
    // capacity 0: the outputs are not looked at
    c = good; c.capacity = 0; c.out_keys = at(0x10001); c.out_starts = at(0x10003); c.flags = RDST_RUNS_PAD_STARTS; CHECK(c.run() == RDST_OK);
    // 9
    c = good; c.scratch = at(0x50080); CHECK(c.run() == RDST_ERR_ALIGN && said("scratch not aligned"));
    c = good; c.scratch_bytes = rdst_hip_runs_scratch_bytes(1000, 4) - 1; CHECK(c.run() == RDST_ERR_ARG && said("rdst_hip_runs_scratch_bytes"));
    c.scratch_bytes += 1; CHECK(c.run() == RDST_OK);
    // the scratch (its documented size, not scratch_bytes) and the length overlap nothing that is read or written
    const uint64_t sb = rdst_hip_runs_scratch_bytes(1000, 4);
    c = good; c.scratch = at(0x30000 + 8 * 1001 / 256 * 256); CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));   // the last start
    c = good; c.scratch = at(0x30000 + (8 * 1001 + 255) / 256 * 256); CHECK(c.run() == RDST_OK);
    c = good; c.scratch = at(0x40000 - sb + 256); CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));              // the count
    c = good; c.scratch = at(0x40000 - sb); CHECK(c.run() == RDST_OK);
    c = good; c.scratch = at(0x10000 - sb + 256); CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));              // the input
    c = good; c.scratch = at(0x20000 + 4 * 1000 / 256 * 256); CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));  // the key output
    c = good; c.dev_len = at(0x50008); c.len_bytes = 8; CHECK(c.run() == RDST_ERR_ARG && said("scratch overlaps"));
    c.dev_len = at(0x50000 + sb); CHECK(c.run() == RDST_OK);
    c.dev_len = at(0x40000); CHECK(c.run() == RDST_ERR_ARG && said("run count overlaps"));
    c.dev_len = at(0x30000 + 8 * 1000); CHECK(c.run() == RDST_ERR_ARG && said("overlaps the input"));                     // the last start
    c.dev_len = at(0x20000 + 4 * 999); c.len_bytes = 4; CHECK(c.run() == RDST_ERR_ARG && said("overlaps the input"));
    c.dev_len = at(0x20000 + 4 * 1000); CHECK(c.run() == RDST_OK);
    // len == 0 with a NULL key pointer is a call like any other; a capacity beyond the address space does not wrap
    c = good; c.len = 0; c.keys = nullptr; CHECK(c.run() == RDST_OK);
    c = good; c.capacity = ~0ull; CHECK(c.run() == RDST_ERR_ARG && said("overlap"));
    c = good; c.capacity = ~0ull; c.out_keys = nullptr; c.out_starts = at(0x60000); CHECK(c.run() == RDST_OK);
}

int main() {
    check_sizes();
    check_order();
    printf("ok\n");
    return 0;
}
