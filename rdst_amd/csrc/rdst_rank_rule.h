// rdst_rank_rule.h — the rank a rank spec (include/rdst_hip.h: rdst_rank_spec) stands for in a segment of n keys, stated once
// for the host (rdst_segments.cpp: rdst_rank_for_length; the far class of rdst_select_segments.hip) and for the kernels of
// rdst_select_segments.hip.  Integer arithmetic only: both factors of the one product are below 2^32.
#ifndef RDST_RANK_RULE_H
#define RDST_RANK_RULE_H

#include <stdint.h>

#include "rdst_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RDST_RANK_RULE_FN __host__ __device__ inline
#else
#define RDST_RANK_RULE_FN inline
#endif

namespace rdst_rank_rule {

// what rdst_rank_for_length refuses (RDST_ERR_ARG)
RDST_RANK_RULE_FN bool spec_ok(const rdst_rank_spec& s) {
    if (s.reserved != 0 || s.mode > RDST_RANK_NEAREST) return false;
    return s.den == 0 ? s.mode == RDST_RANK_LOWER : s.num <= s.den;
}

// A checked spec against a segment of n <= 2^32 keys (so that n - 1 is below 2^32; rdst_rank_for_length refuses a quantile
// of more).  True: *rank < n.  False: the segment has no such element.
RDST_RANK_RULE_FN bool resolve(const rdst_rank_spec& s, uint64_t n, uint64_t* rank) {
    if (n == 0) return false;
    if (s.den == 0) {  // an absolute rank
        *rank = s.num;
        return s.num < n;
    }
    // the virtual index (n - 1) * num / den as quotient and remainder; num <= den, so q <= n - 1, and q == n - 1 leaves r == 0
    const uint64_t v = (n - 1) * (uint64_t)s.num, q = v / s.den, r = v % s.den;
    uint64_t up = 0;
    if (s.mode == RDST_RANK_HIGHER) up = r != 0 ? 1 : 0;
    else if (s.mode == RDST_RANK_NEAREST) up = 2 * r > s.den ? 1 : (2 * r == s.den ? (q & 1) : 0);  // half to even
    *rank = q + up;
    return true;
}

}  // namespace rdst_rank_rule

#endif  // RDST_RANK_RULE_H
