// fl_aggregate_by_columns_map.hpp -- the route of unfor_aggregate_by_columns (fl_aggregate_by_columns.hpp), shared by the kernel and a
// CPU test that compiles this header with a plain C++ compiler (tests/test_aggregate_by_columns_cpu.py).  No HIP dependency.
//
// Three FoR-packed columns of the same block count are joined row by row: two VALUE columns a and b of one type T, met under an fl_expr
// (fl_expr_map.hpp), and a KEY column of type u8 (fl_aggregate_by_map.hpp).  A block is judged from its three blocks' metadata and its
// mask before any packed byte is requested.  The route is the COMPOSITION of the two parents' rules, neither restated here:
//   * aggregate_by_route decides from the mask, the three device checks and the key width: SKIP, ONE_KEY or DECODE;
//   * under ONE_KEY the block is unfor_aggregate_columns' block and expr_route names its sub-route (never EXPR_IDENTITY: an empty mask
//     is SKIP); its one BlockAggregate is folded into the slot of the key reference and no key byte is read;
//   * under DECODE the key block and every value column of width >= 1 are read (expr is what expr_route says of the two widths; the
//     kernel has one path for all of them: a width-0 side requests nothing and decodes to its reference).
#pragma once
#include "fl_aggregate_by_map.hpp"
#include "fl_expr_map.hpp"

namespace fl {

struct AggregateByColumnsRoute {
    AggregateByRoute by;       // aggregate_by_route of the mask, the three columns' checks and the key width
    ExprRoute expr;            // expr_route of the two value widths; EXPR_IDENTITY under AGGBY_SKIP
};
FL_HD inline AggregateByColumnsRoute aggregate_by_columns_route(bool mask_empty, bool precondition_ok, unsigned key_width, unsigned wa, unsigned wb)
{
    const AggregateByRoute by = aggregate_by_route(mask_empty, precondition_ok, key_width);
    return AggregateByColumnsRoute{by, expr_route(by == AGGBY_SKIP ? 0u : 1u, wa, wb)};
}

// whether the route requests packed bytes of the key column / of column a / of column b
FL_HD inline bool aggregate_by_columns_reads_keys(AggregateByColumnsRoute r) { return aggregate_by_reads_keys(r.by); }
FL_HD inline bool aggregate_by_columns_reads_a(AggregateByColumnsRoute r)
{
    return r.by != AGGBY_SKIP && (r.expr == EXPR_DECODE_A || r.expr == EXPR_DECODE_BOTH);
}
FL_HD inline bool aggregate_by_columns_reads_b(AggregateByColumnsRoute r)
{
    return r.by != AGGBY_SKIP && (r.expr == EXPR_DECODE_B || r.expr == EXPR_DECODE_BOTH);
}

}  // namespace fl
