// fl_delta_aggregate_map.hpp -- the block routes of undelta_aggregate (fl_delta_aggregate.hpp) and the arithmetic of the route that needs no
// decode, shared by the kernel and a CPU test that compiles this header with a plain C++ compiler (tests/test_delta_aggregate_cpu.py).
// No HIP dependency.
//
// A block is judged before any packed byte is requested, in this order:
//   SKIP      a mixed-width device check fails: its FL_DEVERR_* bit is raised and its slot receives the IDENTITY (the slot feeds a
//             reduction, as unfor_aggregate's does);
//   IDENTITY  the block's mask is empty: nothing of the block is used, neither bases nor packed bytes;
//   BASES     W == 0: every row of the chain of FastLanes lane l equals base_l (macros.rs:118-125 + delta.rs:58-60).  With p_l the
//             popcount of lane l's mask group (the T bits at delta_group_bit(l), fl_delta_compare_range_map.hpp):
//             count = sum p_l, sum = sum p_l * base_l (mod 2^64), min / max over the lanes with p_l > 0; 128 B of bases (+ 128 B of mask)
//             read, no packed load;
//   EACH      everything else: the packed rows are decoded along their chains and every kept element is accumulated.
#pragma once
#include "fl_aggregate_map.hpp"
#include "fl_delta_compare_range_map.hpp"

namespace fl {

enum DeltaAggregateRoute { DAGG_SKIP = 0, DAGG_IDENTITY = 1, DAGG_BASES = 2, DAGG_EACH = 3 };

FL_HD inline DeltaAggregateRoute delta_aggregate_route(bool precondition_ok, bool mask_empty, unsigned width)
{
    return !precondition_ok ? DAGG_SKIP : mask_empty ? DAGG_IDENTITY : width == 0u ? DAGG_BASES : DAGG_EACH;
}
// whether the route uses the block's bases / requests packed bytes
FL_HD inline bool delta_aggregate_reads_bases(DeltaAggregateRoute r) { return r >= DAGG_BASES; }
FL_HD inline bool delta_aggregate_reads_packed(DeltaAggregateRoute r) { return r == DAGG_EACH; }

// one chain of a width-0 block: p kept rows (0 .. T) that all hold `base` (zero-extended)
FL_HD inline void delta_aggregate_add_chain(BlockAggregate& g, unsigned p, uint64_t base)
{
    const bool on = p != 0u;
    g.count += p;
    g.sum += (uint64_t)p * base;
    g.min = on && base < g.min ? base : g.min;
    g.max = on && base > g.max ? base : g.max;
}

// the BASES route of a whole block: bases[l] and p[l] of FastLanes lanes l = 0 .. 1024 / type_bits - 1
FL_HD inline BlockAggregate delta_aggregate_bases_block(unsigned type_bits, const uint64_t* bases, const unsigned* p)
{
    const uint64_t ones = type_bits >= 64u ? ~0ull : (1ull << type_bits) - 1ull;
    BlockAggregate g = aggregate_identity();
    for (unsigned l = 0; l < 1024u / type_bits; ++l) delta_aggregate_add_chain(g, p[l], bases[l] & ones);
    return g;
}

}  // namespace fl
