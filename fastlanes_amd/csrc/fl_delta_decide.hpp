// fl_delta_decide.hpp -- the block decision of undelta_compare_range (fl_delta_compare_range.hpp), shared by the kernel and a CPU test
// that compiles this header with a plain C++ compiler (tests/test_delta_compare_range_cpu.py).  No HIP dependency.
//
// All arithmetic is mod 2^T, M = 2^T - 1; the predicate is fl_for_decide.hpp's cyclic interval (v - a) mod 2^T <= s.  A Delta block of
// width W holds, for each of its LANES chains, base_l plus a running sum of fields f in [0, span], span = 2^W - 1 (delta.rs:56-61,
// wrapping_add): row r of lane l is base_l plus r + 1 of them, r = 0 .. T - 1.  With c_l = (base_l - a) mod 2^T every value of the lane
// lies, before any wrap, in [c_l, c_l + reach], reach = T * span in exact arithmetic.  Over the block's bases cmin <= c_l <= cmax, so
//   * cmax <= s and cmax + reach <= s: every value of the block lies inside [0, s]: ALL, the packed bytes are never read;
//   * cmin  > s and cmax + reach <= M: every value lies inside [s + 1, M]: NONE, likewise;
//   * W == 0: every delta is 0, each chain repeats its base: lane l's T rows all answer (c_l <= s) -- BASES, no packed byte exists;
//   * otherwise every element is judged: EACH.
// reach exceeds 64 bits for u64 at W >= 59: it saturates at 2^64 - 1, which no comparison below accepts unless it is exact (s < M and
// cmax >= 0 in the ALL rule; cmax >= cmin > s >= 0 in the NONE rule).
#pragma once
#include "fl_for_decide.hpp"

namespace fl {

// per-block verdicts of delta_compare_decide; EACH / ALL / NONE have fl_for_decide.hpp's values
enum DeltaCompareVerdict { DELTA_CMP_EACH = FOR_CMP_EACH, DELTA_CMP_ALL = FOR_CMP_ALL, DELTA_CMP_NONE = FOR_CMP_NONE, DELTA_CMP_BASES = 3 };

// T * (2^W - 1), saturated at 2^64 - 1 (width <= type_bits <= 64)
FL_HD inline uint64_t delta_reach(unsigned type_bits, unsigned width)
{
    const uint64_t span = width >= 64 ? ~0ull : ((1ull << width) - 1ull);
    return span > ~0ull / type_bits ? ~0ull : span * type_bits;
}

// the block's verdict from cmin / cmax = the least and the greatest c_l = (base_l - p.a) mod 2^T of its LANES bases
FL_HD inline int delta_compare_decide(unsigned type_bits, const ForPredicate& p, uint64_t cmin, uint64_t cmax, unsigned width)
{
    const uint64_t M = type_max(type_bits);
    if (p.none) return DELTA_CMP_NONE;
    if (p.s == M) return DELTA_CMP_ALL;                                  // every value: also chains that wrap
    const uint64_t reach = delta_reach(type_bits, width);
    if (cmax <= p.s && reach <= p.s - cmax) return DELTA_CMP_ALL;
    if (cmin > p.s && reach <= M - cmax) return DELTA_CMP_NONE;
    if (width == 0) return DELTA_CMP_BASES;
    return DELTA_CMP_EACH;
}

}  // namespace fl
