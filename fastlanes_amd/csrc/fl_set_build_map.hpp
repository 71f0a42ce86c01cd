// fl_set_build_map.hpp -- the block decisions of unfor_set_build (fl_set_build.hpp), shared by the kernel, the C ABI's host side and a
// CPU test that compiles this header with a plain C++ compiler (tests/test_set_build_cpu.py).  No HIP dependency.
//
// unfor_set_build is the BUILD side of the semi-join unfor_compare_in probes: every kept value v of a FoR-packed column sets bit
// j = (v - set_lo) mod 2^T of a member set's bitmap when j < set_bits, and is counted as `outside` otherwise.  The window and the
// bitmap's layout are unfor_compare_in's (fl_set_decide.hpp: set_window, set_block_decide), so a block is judged from its metadata and
// its mask before any packed byte is requested, by the very rules the probe side uses:
//   SKIP     the mask keeps nothing (or the block fails a device check): nothing is read, nothing is counted;
//   OUTSIDE  set_block_decide says SET_NONE -- no value of the block lies in the window: no packed byte is read, every kept row counts
//            as outside;
//   ONE_BIT  width 0 inside the window (SET_PROBE): every kept row is the reference, ONE lane sets bit c, every kept row counts as
//            inserted;
//   EACH     everything else is decoded.
#pragma once
#include "fl_set_decide.hpp"

namespace fl {

enum SetBuildRoute { SETB_SKIP = 0, SETB_OUTSIDE = 1, SETB_ONE_BIT = 2, SETB_EACH = 3 };

// Up to this many bits a wavefront builds a PRIVATE bitmap in LDS (8 KiB: the whole domain of u8 and u16) and flushes it once; a larger
// window is updated in device memory, one atomic per element.
constexpr uint64_t SET_BUILD_LDS_BITS = 65536;

// the route of a block and c = (reference - set_lo) mod 2^T (ONE_BIT: the bit to set, c <= window.s; EACH: the summand of every field)
FL_HD inline SetBuildRoute set_build_route(unsigned type_bits, const ForPredicate& window, bool mask_empty, bool precondition_ok,
                                           uint64_t reference, unsigned width, uint64_t& c)
{
    c = (reference - window.a) & type_max(type_bits);
    if (mask_empty || !precondition_ok) return SETB_SKIP;
    const int v = set_block_decide(type_bits, window, reference, width, c);
    return v == SET_NONE ? SETB_OUTSIDE : v == SET_PROBE ? SETB_ONE_BIT : SETB_EACH;
}
// whether the route requests packed bytes (a width-0 block never does: it is OUTSIDE or ONE_BIT)
FL_HD inline bool set_build_reads_packed(SetBuildRoute route) { return route == SETB_EACH; }

// what a decided block adds to {inserted, outside}, given the rows its mask keeps
FL_HD inline uint64_t set_build_inserted(SetBuildRoute route, uint64_t kept) { return route == SETB_ONE_BIT ? kept : 0; }
FL_HD inline uint64_t set_build_outside(SetBuildRoute route, uint64_t kept) { return route == SETB_OUTSIDE ? kept : 0; }

FL_HD inline bool set_build_lds_tier(uint64_t set_bits) { return set_bits <= SET_BUILD_LDS_BITS; }

// the bits of the window's LAST word that belong to the window: the others are never changed
FL_HD inline uint32_t set_build_last_word_mask(uint64_t set_bits)
{
    const unsigned tail = (unsigned)(set_bits & 31u);
    return tail ? (1u << tail) - 1u : ~0u;
}

// the private bitmap of the LDS tier: the largest window of the tier the element type can have
FL_HD constexpr unsigned set_build_lds_bitmap_bytes(unsigned type_bits)
{
    return type_bits >= 16 ? (unsigned)(SET_BUILD_LDS_BITS / 8) : (1u << type_bits) / 8u;
}
// per-wavefront LDS: the block's image, then (LDS tier) the private bitmap
FL_HD constexpr unsigned set_build_wave_lds(unsigned block_bytes, unsigned type_bits, bool lds_tier)
{
    return block_bytes + (lds_tier ? set_build_lds_bitmap_bytes(type_bits) : 0u);
}

}  // namespace fl
