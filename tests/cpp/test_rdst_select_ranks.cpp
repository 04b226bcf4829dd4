// Stand-alone check of the segmented select's rank rule in rdst_segments.cpp (rdst_rank_for_length; host only; built by
// tests/test_select_segments_inputs.py with -fsanitize=address,undefined): the edges of the rule — the overflow corners of the
// one 64-bit product, the bad specs, n == 0 and 1 — against 128-bit arithmetic, and the limits beside rdst_hip_topk_segments_limits.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>

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

typedef unsigned __int128 u128;

// the rule in 128-bit integers: nothing here can overflow
static bool wide_rule(uint32_t num, uint32_t den, uint32_t mode, uint64_t n, uint64_t* rank) {
    if (n == 0) return false;
    if (den == 0) {
        *rank = num;
        return num < n;
    }
    const u128 v = (u128)(n - 1) * num, q = v / den, r = v % den;
    u128 up = 0;
    if (mode == RDST_RANK_HIGHER) up = r != 0;
    if (mode == RDST_RANK_NEAREST) up = 2 * r > den || (2 * r == den && (q & 1));
    *rank = (uint64_t)(q + up);
    return true;
}

int main() {
    const uint32_t top = 0xFFFFFFFFu;
    const uint32_t nums[] = {0, 1, 2, 3, 5, 9, 10, 1000, 0x7FFFFFFFu, 0x80000000u, top - 1, top};
    const uint64_t ns[] = {0, 1, 2, 3, 4, 5, 6, 7, 1000, 1001, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFEull, 0xFFFFFFFFull, 0x100000000ull};
    uint64_t checked = 0;
    for (uint32_t num : nums)
        for (uint32_t den : nums)
            for (uint32_t mode = 0; mode < 3; ++mode)
                for (uint64_t n : ns) {
                    const rdst_rank_spec spec{num, den, mode, 0};
                    const bool ok = den == 0 ? mode == 0 : num <= den;
                    uint64_t got = ~0ull, want = 0;
                    const int rc = rdst_rank_for_length(&spec, n, &got);
                    if (!ok) {
                        CHECK(rc == RDST_ERR_ARG && got == ~0ull && !g_error.empty());
                        continue;
                    }
                    const bool has = wide_rule(num, den, mode, n, &want);
                    CHECK(rc == (has ? 1 : 0));
                    if (has) CHECK(got == want && got < n);
                    else CHECK(got == ~0ull);  // not written
                    ++checked;
                }
    CHECK(checked > 1000);
    // the far corner: (2^32 - 1) * (2^32 - 1) is the largest product, and it fits
    {
        const rdst_rank_spec one{top, top, RDST_RANK_NEAREST, 0}, almost{top - 1, top, RDST_RANK_HIGHER, 0};
        uint64_t r = 0;
        CHECK(rdst_rank_for_length(&one, 0x100000000ull, &r) == 1 && r == 0xFFFFFFFFull);
        CHECK(rdst_rank_for_length(&almost, 0x100000000ull, &r) == 1 && r == 0xFFFFFFFEull);
        CHECK(rdst_rank_for_length(&one, 0x100000001ull, &r) == RDST_ERR_ARG);  // n - 1 no longer below 2^32
        const rdst_rank_spec abs{top, 0, 0, 0};
        CHECK(rdst_rank_for_length(&abs, 0x100000001ull, &r) == 1 && r == top);  // an absolute rank takes any n
        CHECK(rdst_rank_for_length(&abs, top, &r) == 0);
    }
    // half-way cases go to even
    {
        const rdst_rank_spec half{1, 2, RDST_RANK_NEAREST, 0};
        const uint64_t want[] = {0, 0, 1, 2, 2, 2, 3, 4, 4};  // n = 1 .. 9: virtual 0, .5, 1, 1.5, 2, 2.5, 3, 3.5, 4
        for (uint64_t n = 1; n <= 9; ++n) {
            uint64_t r = 99;
            CHECK(rdst_rank_for_length(&half, n, &r) == 1 && r == want[n - 1]);
        }
    }
    // bad specs and null arguments
    {
        uint64_t r = 0;
        const rdst_rank_spec good{1, 2, 0, 0};
        CHECK(rdst_rank_for_length(nullptr, 5, &r) == RDST_ERR_ARG && rdst_rank_for_length(&good, 5, nullptr) == RDST_ERR_ARG);
        const rdst_rank_spec bad[] = {{3, 2, 0, 0}, {1, 2, 3, 0}, {1, 2, top, 0}, {1, 2, 0, 1}, {5, 0, 1, 0}, {5, 0, 2, 0}, {0, 0, 0, top}};
        for (const rdst_rank_spec& b : bad) CHECK(rdst_rank_for_length(&b, 5, &r) == RDST_ERR_ARG);
    }
    // the limits: the plan's classes, and the round
    for (uint32_t kb : {1u, 2u, 4u, 8u, 16u})
        for (uint32_t ib : {0u, 4u, 8u}) {
            uint32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
            const int rc = rdst_hip_select_segments_limits(kb, ib, a);
            CHECK(rc == rdst_hip_topk_segments_limits(kb, ib, b));
            if (rc == RDST_OK) CHECK(a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == 32);
        }
    CHECK(rdst_hip_select_segments_limits(4, 0, nullptr) == RDST_ERR_ARG);
    printf("ok %llu\n", (unsigned long long)checked);
    return 0;
}
