// fl_delta_compare_range_map.hpp -- the block routes of undelta_compare_range (fl_delta_compare_range.hpp) and the placement of its
// verdict groups, shared by the kernel and a CPU test that compiles this header with a plain C++ compiler
// (tests/test_delta_compare_range_cpu.py).  No HIP dependency.
//
// A block is judged before any packed byte is requested, in this order:
//   SKIP   a mixed-width device check fails: its FL_DEVERR_* bit is raised, its 32 mask words are left as they were;
//   KEEP   the incoming mask already decides it (AND of all zero, OR of all ones): neither bases nor packed bytes are needed, the
//          incoming 128 bytes are the answer;
//   ALL / NONE / BASES   fl_delta_decide.hpp decides it from its 128 bytes of bases: 128 B read, 128 B of mask written, no packed load;
//   EACH   everything else: the packed rows are decoded along their chains and every element is compared.
//
// Placement.  Delta's chain of FastLanes lane l runs over rows r = 0 .. T - 1, whose ORIGINAL positions are lane_base(l) + r
// (transpose.rs:29-36; fl_device.hpp: lane_base): T consecutive rows starting at a multiple of T.  One lane's chain therefore yields one
// T-bit aligned group of the block's 1024-bit original-order mask -- a byte (u8), a half word (u16), a word (u32), two words (u64) --
// and no value is untransposed: group l lands at bit delta_group_bit(l).
#pragma once
#include "fl_delta_decide.hpp"

namespace fl {

enum DeltaRangeRoute { DRANGE_SKIP = 0, DRANGE_KEEP = 1, DRANGE_ALL = 2, DRANGE_NONE = 3, DRANGE_BASES = 4, DRANGE_EACH = 5 };

// mask_live: the incoming mask leaves the block's answer open (NEW: always; AND: some bit set; OR: some bit clear)
FL_HD inline DeltaRangeRoute delta_range_route(unsigned type_bits, const ForPredicate& p, bool precondition_ok, bool mask_live, uint64_t cmin,
                                               uint64_t cmax, unsigned width)
{
    if (!precondition_ok) return DRANGE_SKIP;
    if (!mask_live) return DRANGE_KEEP;
    const int v = delta_compare_decide(type_bits, p, cmin, cmax, width);
    return v == DELTA_CMP_ALL ? DRANGE_ALL : v == DELTA_CMP_NONE ? DRANGE_NONE : v == DELTA_CMP_BASES ? DRANGE_BASES : DRANGE_EACH;
}
// whether the route needs the block's bases / requests packed bytes
FL_HD inline bool delta_range_reads_bases(DeltaRangeRoute r) { return r >= DRANGE_ALL; }
FL_HD inline bool delta_range_reads_packed(DeltaRangeRoute r) { return r == DRANGE_EACH; }

// first original row of FastLanes lane l's chain = the bit of its T-bit group in the block's mask (FL_ORDER = 0 4 2 6 1 5 3 7, lib.rs:22)
FL_HD constexpr unsigned delta_group_bit(unsigned l) { return (l % 16u) * 64u + ((0x73516240u >> (4u * (l / 16u))) & 7u) * 8u; }

}  // namespace fl
