// fl_columns_decide.hpp -- the decision rule of unfor_compare_columns (fl_for_compare_columns.hpp): what a pair of FoR blocks'
// references and widths alone say about `a <op> b`.  Shared by the kernel, the C ABI's host side and a CPU test that compiles this
// header with a plain C++ compiler (tests/test_for_compare_columns_cpu.py).  No HIP dependency.
//
// All arithmetic is mod 2^T, M = 2^T - 1.  A signed comparison is the unsigned one after bias = 2^(T-1) is added to both sides (the
// order domain); the bias is folded into the two references.  There block `a` holds values in the cyclic range that starts at
// r_a = (reference + bias) mod 2^T and spans 2^WA - 1.  A range that wraps past M contains both 0 and M: its hull is [0, M]; otherwise
// the hull is [r_a, r_a + span].  The six ops reduce, once per call, to ONE base relation -- a < b, or a == b -- plus "swap the
// columns" and "invert the answer" (columns_relation):
//     a <  b : ALL when hi_a < lo_b, NONE when lo_a >= hi_b                       (hulls)
//     a == b : NONE when the two cyclic ranges are disjoint, ALL when both widths are 0 and the references are equal
// The rule is exact both ways: ALL iff every value pair of the two ranges satisfies the predicate, NONE iff none does (checked
// exhaustively at a 4-bit model type by the CPU test).
#pragma once
#include "fl_for_decide.hpp"

namespace fl {

// a <op> b  ==  invert ^ (swap ? base(b, a) : base(a, b)), base = is_eq ? (x == y) : (x < y)
struct ColumnsRelation {
    bool is_eq, swap, invert;
};

// op: FL_CMP_EQ 0, NE 1, LT 2, LE 3, GT 4, GE 5 (include/fastlanes_amd.h); the callers refuse any other op
FL_HD inline ColumnsRelation columns_relation(int op)
{
    switch (op) {
    case 0: return {true, false, false};                                 // a == b
    case 1: return {true, false, true};                                  // a != b: not (a == b)
    case 2: return {false, false, false};                                // a <  b
    case 3: return {false, true, true};                                  // a <= b: not (b < a)
    case 4: return {false, true, false};                                 // a >  b: b < a
    default: return {false, false, true};                                // a >= b: not (a < b)
    }
}

FL_HD inline uint64_t columns_bias(unsigned type_bits, bool is_signed) { return is_signed ? 1ull << (type_bits - 1u) : 0ull; }

// the hull [lo, hi] of the cyclic range [r, r + 2^width - 1] (r already in the order domain, r <= M, width <= type_bits)
FL_HD inline void columns_hull(unsigned type_bits, uint64_t r, unsigned width, uint64_t& lo, uint64_t& hi)
{
    const uint64_t M = type_max(type_bits);
    const uint64_t span = width >= 64 ? ~0ull : ((1ull << width) - 1ull);
    if (span > M - r) { lo = 0; hi = M; }                                // wraps: holds both 0 and M
    else { lo = r; hi = r + span; }
}

// the verdict of the base relation for blocks (ra, wa) and (rb, wb), references in the order domain
FL_HD inline int columns_decide_base(unsigned type_bits, bool is_eq, uint64_t ra, unsigned wa, uint64_t rb, unsigned wb)
{
    const uint64_t M = type_max(type_bits);
    if (is_eq) {
        const uint64_t span_a = wa >= 64 ? ~0ull : ((1ull << wa) - 1ull), span_b = wb >= 64 ? ~0ull : ((1ull << wb) - 1ull);
        if (((rb - ra) & M) > span_a && ((ra - rb) & M) > span_b) return FOR_CMP_NONE;   // neither range holds the other's start
        if (wa == 0 && wb == 0 && ra == rb) return FOR_CMP_ALL;
        return FOR_CMP_EACH;
    }
    uint64_t lo_a, hi_a, lo_b, hi_b;
    columns_hull(type_bits, ra, wa, lo_a, hi_a);
    columns_hull(type_bits, rb, wb, lo_b, hi_b);
    if (hi_a < lo_b) return FOR_CMP_ALL;
    if (lo_a >= hi_b) return FOR_CMP_NONE;
    return FOR_CMP_EACH;
}

FL_HD inline int columns_invert_verdict(int verdict)
{
    return verdict == FOR_CMP_ALL ? (int)FOR_CMP_NONE : verdict == FOR_CMP_NONE ? (int)FOR_CMP_ALL : (int)FOR_CMP_EACH;
}

// the whole rule: the verdict of `a <op> b` for raw references (the bias is added here), signed or unsigned
FL_HD inline int columns_decide(unsigned type_bits, int op, bool is_signed, uint64_t ref_a, unsigned wa, uint64_t ref_b, unsigned wb)
{
    const uint64_t M = type_max(type_bits), bias = columns_bias(type_bits, is_signed);
    const ColumnsRelation rel = columns_relation(op);
    const uint64_t ra = (ref_a + bias) & M, rb = (ref_b + bias) & M;
    const int v = rel.swap ? columns_decide_base(type_bits, rel.is_eq, rb, wb, ra, wa) : columns_decide_base(type_bits, rel.is_eq, ra, wa, rb, wb);
    return rel.invert ? columns_invert_verdict(v) : v;
}

}  // namespace fl
