// fl_for_decide.hpp -- the predicate arithmetic of unfor_compare (fl_for_compare.hpp), shared by the kernel, the C ABI's host side
// and a CPU test that compiles this header with a plain C++ compiler (tests/test_for_compare_cpu.py).  No HIP dependency.
//
// All arithmetic is mod 2^T, M = 2^T - 1.  Each unsigned predicate `v <op> k` (fl_cmp) is ONE cyclic interval of satisfying values,
//     (v - a) mod 2^T <= s,
// or none at all (x < 0, x > M).  A FoR block with reference r and width W holds v = (f + r) mod 2^T for its packed fields
// f in [0, 2^W - 1] (ffor.rs:46-48, wrapping_add), so with c = (r - a) mod 2^T every element costs one add and one unsigned compare,
//     ((f + c) mod 2^T) <= s,
// and the fields cover the cyclic range [c, c + 2^W - 1]: when that range lies inside [0, s] the whole block satisfies the predicate,
// when it lies inside [s + 1, M] none of it does -- decided from the block's metadata alone, its packed bytes never read.
#pragma once
#include <stdint.h>

#ifndef FL_HD            // (also defined, identically, by fl_tile_map.hpp)
#if defined(__HIPCC__) || defined(__HIP__)
#define FL_HD __host__ __device__
#else
#define FL_HD
#endif
#endif

namespace fl {

// per-block verdicts of for_compare_decide
enum ForCompareVerdict { FOR_CMP_EACH = 0, FOR_CMP_ALL = 1, FOR_CMP_NONE = 2 };

// the predicate as the cyclic interval [a, a + s] (none: no value satisfies it); reduced once per call, on the host
struct ForPredicate {
    uint64_t a;
    uint64_t s;
    bool none;
};

FL_HD inline uint64_t type_max(unsigned type_bits) { return type_bits >= 64 ? ~0ull : ((1ull << type_bits) - 1ull); }

// op: FL_CMP_EQ 0, NE 1, LT 2, LE 3, GT 4, GE 5 (include/fastlanes_amd.h); the callers refuse any other op
FL_HD inline ForPredicate for_compare_predicate(unsigned type_bits, int op, uint64_t k)
{
    const uint64_t M = type_max(type_bits);
    k &= M;
    switch (op) {
    case 0: return {k, 0, false};                                        // v == k
    case 1: return {(k + 1) & M, M - 1, false};                          // v != k: every value but k
    case 2: return {0, k ? k - 1 : 0, k == 0};                           // v < k: [0, k - 1]; none for k = 0
    case 3: return {0, k, false};                                        // v <= k: [0, k]
    case 4: return {(k + 1) & M, k == M ? 0 : M - k - 1, k == M};        // v > k: [k + 1, M]; none for k = M
    default: return {k, M - k, false};                                   // v >= k: [k, M]
    }
}

// the cyclic interval [lo, hi] itself (unfor_compare_range): lo <= hi is BETWEEN, lo > hi wraps (v >= lo OR v <= hi), hi == lo - 1
// is every value (s = M); never none.  A signed comparison is such an interval of the two's-complement bit patterns.
FL_HD inline ForPredicate for_range_predicate(unsigned type_bits, uint64_t lo, uint64_t hi)
{
    const uint64_t M = type_max(type_bits);
    return {lo & M, (hi - lo) & M, false};
}

// c = (r - a) mod 2^T of a block with reference r, and the block's verdict for fields of `width` bits (width <= type_bits)
FL_HD inline int for_compare_decide(unsigned type_bits, const ForPredicate& p, uint64_t reference, unsigned width, uint64_t& c)
{
    const uint64_t M = type_max(type_bits);
    c = (reference - p.a) & M;
    if (p.none) return FOR_CMP_NONE;
    if (p.s == M) return FOR_CMP_ALL;                                    // every value: also a field range that wraps (W = T, c != 0)
    const uint64_t span = width >= 64 ? ~0ull : ((1ull << width) - 1ull); // the fields cover [c, c + span], in exact arithmetic
    if (c <= p.s && span <= p.s - c) return FOR_CMP_ALL;
    if (c > p.s && span <= M - c) return FOR_CMP_NONE;
    return FOR_CMP_EACH;
}

}  // namespace fl
