// fl_delta_select_map.hpp -- the block routes of undelta_select (fl_delta_select.hpp) and its landing map, shared by the kernel and a CPU
// test that compiles this header with a plain C++ compiler (tests/test_delta_select_cpu.py).  No HIP dependency.
//
// A block is judged before any packed byte is requested, in this order:
//   SKIP    a device check fails: its FL_DEVERR_* bit is raised, its output slots are left as they were;
//   EMPTY   the block's mask is all zero: no packed load, no store;
//   BOUNDS  the block's run [out_offsets[b], + count) does not lie inside [0, out_len): FL_DEVERR_BOUNDS is raised, nothing is written;
//   BASES   W == 0: every row of the chain of FastLanes lane l equals base_l (macros.rs:118-125 + delta.rs:58-60); no packed byte is read;
//   EACH    everything else: the packed rows are decoded along their chains.
//
// Landing.  Delta's chain of FastLanes lane l runs over rows r = 0 .. T - 1, whose ORIGINAL positions are p = delta_group_bit(l) + r
// (fl_delta_compare_range_map.hpp): the mask bits that govern it are one aligned T-bit group, and the run is in original row order, so
// a kept row lands at
//     rank(p) = the mask bits of the block below p
//             = (the bits below the group: GROUP PREFIX) + popcount(group_l & ((1 << r) - 1)).
// The group prefix is (the bits of the 32-bit words below the group's word: one exclusive scan of the 32 words' popcounts, whose total
// is the block's count) + (the bits of the group's own word below the group: u8 / u16 only, a wider group starts its word).  It is known
// before a packed byte arrives, and no value is untransposed.
//
// What the kernel itself calls: delta_group_bit, delta_select_group_prefix and delta_select_landing (the landing arithmetic runs on the
// device as it is written here).  delta_select_route and its three predicates STATE the order the kernel's straight-line code keeps (its
// count is known only after the mask is staged, so it spells the order out; family 27 does the same), and delta_select_group,
// delta_select_scan_words and delta_select_block_landing compose a whole block on the host the way the wavefront does across its lanes
// (the kernel takes the groups out of registers, lane_group, and scans by DPP).  The CPU test therefore pins the arithmetic the kernel
// runs and a restatement of its order; the order itself is pinned on the GPU (tests/test_gpu_delta_select.py: a failing block with an
// empty mask still raises its bit, an empty block whose offset lies past out_len raises nothing).
#pragma once
#include "fl_delta_compare_range_map.hpp"

namespace fl {

enum DeltaSelectRoute { DSEL_SKIP = 0, DSEL_EMPTY = 1, DSEL_BOUNDS = 2, DSEL_BASES = 3, DSEL_EACH = 4 };

FL_HD inline DeltaSelectRoute delta_select_route(bool precondition_ok, bool mask_empty, bool run_inside, unsigned width)
{
    return !precondition_ok ? DSEL_SKIP : mask_empty ? DSEL_EMPTY : !run_inside ? DSEL_BOUNDS : width == 0u ? DSEL_BASES : DSEL_EACH;
}
// whether the route uses the block's bases / requests packed bytes / stores a run
FL_HD inline bool delta_select_reads_bases(DeltaSelectRoute r) { return r >= DSEL_BASES; }
FL_HD inline bool delta_select_reads_packed(DeltaSelectRoute r) { return r == DSEL_EACH; }
FL_HD inline bool delta_select_writes(DeltaSelectRoute r) { return r >= DSEL_BASES; }

// the bits of `bits` below bit n (n < 64)
FL_HD inline unsigned delta_select_bits_below(uint64_t bits, unsigned n) { return (unsigned)__builtin_popcountll(bits & ((1ull << n) - 1ull)); }

// the mask bits of the block below the group at bit `group_bit`: `words_below` = the bits of the words below word group_bit / 32 (the
// exclusive scan's value there), `word` = that word
FL_HD inline unsigned delta_select_group_prefix(unsigned words_below, uint32_t word, unsigned group_bit)
{
    return words_below + delta_select_bits_below(word, group_bit & 31u);
}
// where row r of the chain lands in the block's run, if its bit is set: `group` = the chain's T mask bits, bit r = row r
FL_HD inline unsigned delta_select_landing(unsigned group_prefix, uint64_t group, unsigned r) { return group_prefix + delta_select_bits_below(group, r); }

// the T-bit group at `group_bit` of a block's 32 mask words
FL_HD inline uint64_t delta_select_group(unsigned type_bits, const uint32_t* mask, unsigned group_bit)
{
    const unsigned wi = group_bit >> 5;
    if (type_bits == 64u) return ((uint64_t)mask[wi + 1u] << 32) | mask[wi];
    return ((uint64_t)mask[wi] >> (group_bit & 31u)) & ((1ull << type_bits) - 1ull);
}
// A whole block, as the kernel composes it: the exclusive scan of the words' popcounts, then the two steps above.  scan[k] = the bits of
// words 0 .. k - 1; returns the block's count.
FL_HD inline unsigned delta_select_scan_words(const uint32_t* mask, unsigned* scan)
{
    unsigned s = 0;
    for (unsigned k = 0; k < 32u; ++k) {
        scan[k] = s;
        s += (unsigned)__builtin_popcount(mask[k]);
    }
    return s;
}
FL_HD inline unsigned delta_select_block_landing(unsigned type_bits, const uint32_t* mask, const unsigned* scan, unsigned l, unsigned r)
{
    const unsigned gb = delta_group_bit(l);
    return delta_select_landing(delta_select_group_prefix(scan[gb >> 5], mask[gb >> 5], gb), delta_select_group(type_bits, mask, gb), r);
}

}  // namespace fl
