// fl_aggregate_by_window_map.hpp -- the block decisions of unfor_aggregate_by_window (fl_aggregate_by_window.hpp), shared by the kernel,
// the C ABI's host side and a CPU test that compiles this header with a plain C++ compiler (tests/test_aggregate_by_window_cpu.py).
// No HIP dependency.
//
// unfor_aggregate_by_window groups a VALUE column by a KEY column of the same element type inside a dense WINDOW of the key domain:
// a kept row with key k updates slot j = (k - key_lo) mod 2^T of the caller's arrays when j < n_groups, and is counted as `outside`
// otherwise.  The window is unfor_set_build's (fl_set_decide.hpp: set_window, set_block_decide), so a block is judged from its KEY
// metadata and its mask before any packed byte of either column is requested:
//   SKIP       the mask keeps nothing (or one of the two columns fails a device check): nothing is read, nothing is counted;
//   OUTSIDE    set_block_decide says SET_NONE -- no key of the block lies in the window: neither column is read, every kept row counts
//              as outside;
//   ONE_GROUP  key width 0 inside the window (SET_PROBE): every kept row has the key reference, the value side is unfor_aggregate's
//              block and its ONE BlockAggregate is folded into slot c, every kept row counts as inside -- no key byte is read;
//   EACH       everything else: the key block is decoded, and the value block with it when an array needs values.
#pragma once
#include "fl_aggregate_map.hpp"
#include "fl_set_decide.hpp"

namespace fl {

enum AggregateByWindowRoute { AGGW_SKIP = 0, AGGW_OUTSIDE = 1, AGGW_ONE_GROUP = 2, AGGW_EACH = 3 };

// Up to this many groups a wavefront keeps a PRIVATE table of BlockAggregate in LDS (8 KiB: the table unfor_aggregate_by ships with) and
// flushes it once; a larger window is updated in device memory, one atomic per element and array.
constexpr uint64_t AGGREGATE_BY_WINDOW_LDS_GROUPS = 256;
constexpr unsigned AGGREGATE_BY_WINDOW_TABLE_BYTES = (unsigned)AGGREGATE_BY_WINDOW_LDS_GROUPS * (unsigned)sizeof(BlockAggregate);

// the largest window of an element type: min(2^T, 2^32) groups
FL_HD inline uint64_t aggregate_by_window_max_groups(unsigned type_bits) { return set_max_bits(type_bits); }

// the route of a block and c = (key reference - key_lo) mod 2^T (ONE_GROUP: the slot, c <= window.s; EACH: the summand of every key field)
FL_HD inline AggregateByWindowRoute aggregate_by_window_route(unsigned type_bits, const ForPredicate& window, bool mask_empty, bool precondition_ok,
                                                              uint64_t key_reference, unsigned key_width, uint64_t& c)
{
    c = (key_reference - window.a) & type_max(type_bits);
    if (mask_empty || !precondition_ok) return AGGW_SKIP;
    const int v = set_block_decide(type_bits, window, key_reference, key_width, c);
    return v == SET_NONE ? AGGW_OUTSIDE : v == SET_PROBE ? AGGW_ONE_GROUP : AGGW_EACH;
}
// whether the route requests packed bytes of the key column (a width-0 key block never does: it is OUTSIDE or ONE_GROUP) ...
FL_HD inline bool aggregate_by_window_reads_keys(AggregateByWindowRoute route) { return route == AGGW_EACH; }
// ... and of the value column: only when sums, mins or maxs is maintained (need_values), and never of a width-0 value block
FL_HD inline bool aggregate_by_window_reads_values(AggregateByWindowRoute route, unsigned value_width, bool need_values)
{
    return (route == AGGW_ONE_GROUP || route == AGGW_EACH) && need_values && value_width != 0u;
}

// what a decided block adds to {inside, outside}, given the rows its mask keeps
FL_HD inline uint64_t aggregate_by_window_inside(AggregateByWindowRoute route, uint64_t kept) { return route == AGGW_ONE_GROUP ? kept : 0; }
FL_HD inline uint64_t aggregate_by_window_outside(AggregateByWindowRoute route, uint64_t kept) { return route == AGGW_OUTSIDE ? kept : 0; }

FL_HD inline bool aggregate_by_window_lds_tier(uint64_t n_groups) { return n_groups <= AGGREGATE_BY_WINDOW_LDS_GROUPS; }

// per-wavefront LDS: the block's image (it serves the key block, then the value block), then (LDS tier) the private table
FL_HD constexpr unsigned aggregate_by_window_wave_lds(unsigned block_bytes, bool lds_tier)
{
    return block_bytes + (lds_tier ? AGGREGATE_BY_WINDOW_TABLE_BYTES : 0u);
}

}  // namespace fl
