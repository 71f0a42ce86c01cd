// fl_set_decide.hpp -- the block decisions of unfor_compare_in (fl_for_compare_in.hpp), shared by the kernel, the C ABI's host side and
// a CPU test that compiles this header with a plain C++ compiler (tests/test_for_compare_in_cpu.py).  No HIP dependency.
//
// A member set is a WINDOW of the value domain plus a bitmap: bit j of set_words says whether (set_lo + j) mod 2^T is a member,
// 0 <= j < set_bits <= min(2^T, 2^32); bits at positions >= set_bits of the last word are ignored.  The window is the cyclic interval
// [set_lo, set_lo + set_bits - 1], i.e. the ForPredicate {a = set_lo, s = set_bits - 1, none = set_bits == 0} of fl_for_decide.hpp: with
// c = (r - set_lo) mod 2^T the per-element f + c of the compare kernels IS the bitmap index j, and their `<= s` is the in-window test.
//   * for_compare_decide on the window returning FOR_CMP_NONE: no value of the block lies in the window, so none is a member -- decided
//     from the metadata alone.  FOR_CMP_ALL only says that every value lies INSIDE the window, which is no hit (set_bits == 2^T: always).
//   * a width-0 block holds 1024 copies of its reference: inside the window, ONE bitmap bit (bit c) decides it (SET_PROBE).
// `negate` turns a decided block's ALL into NONE and back.
#pragma once
#include "fl_for_decide.hpp"

namespace fl {

// SET_EACH .. SET_NONE are ForCompareVerdict's values; SET_PROBE: bit c of the bitmap decides the block
enum SetVerdict { SET_EACH = 0, SET_ALL = 1, SET_NONE = 2, SET_PROBE = 3 };

constexpr uint64_t SET_REGISTER_BITS = 2048;     // a bitmap of at most 64 words lives in one VGPR of the wavefront: word l in lane l

// the largest window of an element type: min(2^T, 2^32) bits
FL_HD inline uint64_t set_max_bits(unsigned type_bits) { return type_bits >= 32 ? (1ull << 32) : (1ull << type_bits); }
FL_HD inline uint64_t set_word_count(uint64_t set_bits) { return (set_bits + 31u) >> 5; }

// the window as a predicate (set_bits <= set_max_bits(type_bits): the callers refuse anything else)
FL_HD inline ForPredicate set_window(unsigned type_bits, uint64_t set_lo, uint64_t set_bits)
{
    return {set_lo & type_max(type_bits), set_bits ? set_bits - 1 : 0, set_bits == 0};
}

// c = (r - set_lo) mod 2^T, and what the block's metadata says about its MEMBERSHIP: SET_NONE, SET_PROBE (then c <= window.s) or SET_EACH
FL_HD inline int set_block_decide(unsigned type_bits, const ForPredicate& window, uint64_t reference, unsigned width, uint64_t& c)
{
    if (for_compare_decide(type_bits, window, reference, width, c) == FOR_CMP_NONE) return SET_NONE;
    return width == 0 ? SET_PROBE : SET_EACH;      // (width 0: the one value is inside the window, for_compare_decide said ALL)
}

// a SET_PROBE block, given the bitmap word that holds bit c (word c >> 5)
FL_HD inline int set_probe_verdict(uint32_t word, uint64_t c) { return (word >> (c & 31u)) & 1u ? SET_ALL : SET_NONE; }

// membership -> hit: the mask bits a decided block receives
FL_HD inline int set_hit_verdict(int membership, bool negate)
{
    if (membership == SET_EACH || !negate) return membership;
    return membership == SET_ALL ? SET_NONE : SET_ALL;
}

// member(v) of the definition, for the host side and the tests
FL_HD inline bool set_member(unsigned type_bits, const ForPredicate& window, const uint32_t* set_words, uint64_t v)
{
    const uint64_t j = (v - window.a) & type_max(type_bits);
    return !window.none && j <= window.s && ((set_words[j >> 5] >> (j & 31u)) & 1u);
}

}  // namespace fl
