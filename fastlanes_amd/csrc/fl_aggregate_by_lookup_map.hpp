// fl_aggregate_by_lookup_map.hpp -- the block routes of unfor_aggregate_by_lookup (fl_aggregate_by_lookup.hpp), shared by the kernel,
// the C ABI's host side and a CPU test that compiles this header with a plain C++ compiler (tests/test_aggregate_by_lookup_cpu.py).
// No HIP dependency.
//
// unfor_aggregate_by_lookup groups a VALUE column by a u8 attribute fetched through a KEY column of the same element type: a kept row
// with key k and j = (k - key_lo) mod 2^T updates group table[j] when j < n_slots (and bit j of `present` is set, when a bitmap is
// given) and is counted as a miss otherwise.  The window is unfor_lookup's (fl_set_decide.hpp: set_window, set_block_decide), so a
// block is judged from its KEY metadata and its mask before any packed byte of either column is requested:
//   SKIP       one of the two columns fails a device check: nothing is read, nothing is counted or accumulated;
//   NOTHING    the mask keeps no row: nothing is read, nothing is counted;
//   MISSING    set_block_decide says SET_NONE (an empty window among them) -- no key of the block lies in the window: neither column
//              and no table byte is read, every kept row counts as a miss;
//   ONE_GROUP  key width 0 inside the window (SET_PROBE): every kept row has the key reference, so ONE wave-uniform table read (slot c)
//              and at most one `present` bit decide the block: an absent slot makes every kept row a miss and reads no value byte, a
//              present one makes the value side unfor_aggregate's block, folded into group table[c] -- no key byte is read;
//   EACH       everything else: both columns are decoded and every kept in-window row is gathered.
#pragma once
#include "fl_aggregate_map.hpp"
#include "fl_lookup_map.hpp"
#include "fl_set_decide.hpp"

namespace fl {

enum AggregateByLookupRoute { AGGL_SKIP = 0, AGGL_NOTHING = 1, AGGL_MISSING = 2, AGGL_ONE_GROUP = 3, AGGL_EACH = 4 };

// the groups of a call: the values of a u8 code, the 256 slots of unfor_aggregate_by's result
constexpr unsigned AGGREGATE_BY_LOOKUP_GROUPS = 256;
constexpr unsigned AGGREGATE_BY_LOOKUP_TABLE_BYTES = AGGREGATE_BY_LOOKUP_GROUPS * (unsigned)sizeof(BlockAggregate);

// the route of a block and c = (key reference - key_lo) mod 2^T (ONE_GROUP: the slot, c <= window.s; EACH: the summand of every key field)
FL_HD inline AggregateByLookupRoute aggregate_by_lookup_route(unsigned type_bits, const ForPredicate& window, bool mask_empty, bool precondition_ok,
                                                              uint64_t key_reference, unsigned key_width, uint64_t& c)
{
    c = (key_reference - window.a) & type_max(type_bits);
    if (!precondition_ok) return AGGL_SKIP;
    if (mask_empty) return AGGL_NOTHING;
    const int v = set_block_decide(type_bits, window, key_reference, key_width, c);
    return v == SET_NONE ? AGGL_MISSING : v == SET_PROBE ? AGGL_ONE_GROUP : AGGL_EACH;
}
// whether the route requests packed bytes of the key column (a width-0 key block never does: it is MISSING or ONE_GROUP) ...
FL_HD inline bool aggregate_by_lookup_reads_keys(AggregateByLookupRoute route) { return route == AGGL_EACH; }
// ... of the value column (ONE_GROUP: only when the slot is present; never of a width-0 value block) ...
FL_HD inline bool aggregate_by_lookup_reads_values(AggregateByLookupRoute route, unsigned value_width, bool slot_present)
{
    return (route == AGGL_EACH || (route == AGGL_ONE_GROUP && slot_present)) && value_width != 0u;
}
// ... and any byte of the table or the bitmap
FL_HD inline bool aggregate_by_lookup_reads_table(AggregateByLookupRoute route) { return route == AGGL_ONE_GROUP || route == AGGL_EACH; }

// what a block decided WITHOUT a gather adds to {hits, misses}, given the rows its mask keeps (ONE_GROUP: by the slot's `present` bit)
FL_HD inline uint64_t aggregate_by_lookup_decided_hits(AggregateByLookupRoute route, uint64_t kept, bool slot_present)
{
    return route == AGGL_ONE_GROUP && slot_present ? kept : 0;
}
FL_HD inline uint64_t aggregate_by_lookup_decided_misses(AggregateByLookupRoute route, uint64_t kept, bool slot_present)
{
    return route == AGGL_MISSING || (route == AGGL_ONE_GROUP && !slot_present) ? kept : 0;
}

// per-wavefront LDS: the block's image (it serves the key block, then the value block), then the private group table
FL_HD constexpr unsigned aggregate_by_lookup_wave_lds(unsigned block_bytes) { return block_bytes + AGGREGATE_BY_LOOKUP_TABLE_BYTES; }

}  // namespace fl
