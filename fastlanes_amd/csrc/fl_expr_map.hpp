// fl_expr_map.hpp -- the plain integer part of unfor_aggregate_columns (fl_aggregate_columns.hpp), shared by the kernels, the C ABI and a
// CPU test that compiles this header with a plain C++ compiler (tests/test_aggregate_columns_cpu.py).  No HIP dependency.
//
// Two decoded values of one element type are zero-extended to 64 bits BEFORE they meet:  x = (zext64(va) o zext64(vb)) mod 2^64, o one
// of MUL, ADD, SUB (a - b).  So a u8 / u16 / u32 product or sum is exact, a u64 one wraps, and a difference below zero is its
// two's-complement bit pattern: a SUM of such differences is still right mod 2^64, MIN and MAX compare the patterns as UNSIGNED numbers
// (every negative difference lies above every non-negative one).
//
// What a block pair needs follows from the rows its mask keeps and the two widths alone (fl_aggregate_map.hpp's rule, for two columns):
//   * an EMPTY mask: the identity, neither column is read;
//   * both widths 0: every row holds ra o rb (the two references), neither column is read;
//   * exactly one width 0: that side is its reference in every row, only the OTHER column is read;
//   * otherwise both columns are read.
#pragma once
#include "fl_aggregate_map.hpp"

namespace fl {

// the values of fl_expr (include/fastlanes_amd.h)
enum ExprOp { EXPR_MUL = 0, EXPR_ADD = 1, EXPR_SUB = 2 };

FL_HD inline bool expr_valid(int expr) { return expr >= EXPR_MUL && expr <= EXPR_SUB; }

// x o y mod 2^64 of two zero-extended values (`expr` valid)
FL_HD inline uint64_t expr_apply(int expr, uint64_t x, uint64_t y)
{
    return expr == EXPR_MUL ? x * y : expr == EXPR_ADD ? x + y : x - y;
}

// what a block pair of `count` kept rows and widths `wa`, `wb` needs
enum ExprRoute { EXPR_IDENTITY = 0, EXPR_CONSTANT = 1, EXPR_DECODE_A = 2, EXPR_DECODE_B = 3, EXPR_DECODE_BOTH = 4 };
FL_HD inline ExprRoute expr_route(unsigned count, unsigned wa, unsigned wb)
{
    if (count == 0u) return EXPR_IDENTITY;
    if (wa == 0u && wb == 0u) return EXPR_CONSTANT;
    return wb == 0u ? EXPR_DECODE_A : wa == 0u ? EXPR_DECODE_B : EXPR_DECODE_BOTH;
}

// `count` kept rows (>= 0) of a block pair whose widths are both 0: every row holds ra o rb.  The answer of EXPR_IDENTITY and
// EXPR_CONSTANT.
FL_HD inline BlockAggregate expr_constant_block(int expr, unsigned count, uint64_t ra, uint64_t rb)
{
    return aggregate_constant_block(count, expr_apply(expr, ra, rb));
}

}  // namespace fl
