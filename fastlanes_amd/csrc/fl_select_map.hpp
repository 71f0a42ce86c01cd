// fl_select_map.hpp -- the index arithmetic of unfor_select (fl_select.hpp), shared by the kernel and a CPU test that compiles this
// header with a plain C++ compiler (tests/test_select_cpu.py).  No HIP dependency.
//
// A wavefront decodes one 1024-value block: lane l (0..63) holds, for every 1-KiB group k of the unpacked block, the 16-byte cell of the
// N = 16 / sizeof(T) consecutive indices starting at k * 1024 / sizeof(T) + l * N (fl_widths.hpp).  The block's 1024-bit mask (32 words,
// bit i = bit i % 32 of word i / 32) therefore gives the lane an N-bit SLICE per group -- N divides 32, so a slice never straddles a
// word -- and sizeof(T) groups x N bits = 16 mask bits per lane for every element type.
//
// The kept values leave as one contiguous run in index order.  Index order is (group, lane, element), so the k-th kept element of a lane
// in group g lands at
//     (kept elements of groups < g) + (kept elements of group g in lanes < l) + k.
// Both sums come out of ONE wave scan: the lane's per-group counts are packed into one word, FIELD_BITS per group (a group holds
// 1024 / sizeof(T) elements, and FIELD_BITS is wide enough for that total: no carry crosses a field), the inclusive scan of that word
// over the lanes gives every group's prefix at once, and its value in lane 63 the groups' totals.
#pragma once
#include <stdint.h>

#ifndef FL_HD            // (also defined, identically, by fl_tile_map.hpp and fl_for_decide.hpp)
#if defined(__HIPCC__) || defined(__HIP__)
#define FL_HD __host__ __device__
#else
#define FL_HD
#endif
#endif

namespace fl {

constexpr unsigned SELECT_MASK_WORDS = 32;      // uint32 words of one block's mask

// SZ = sizeof(T)
template <unsigned SZ> struct SelectMap {
    static_assert(SZ == 1 || SZ == 2 || SZ == 4 || SZ == 8, "u8 / u16 / u32 / u64");
    static constexpr unsigned N = 16 / SZ;                    // indices (mask bits) of a lane per group
    static constexpr unsigned GROUPS = SZ;                    // 1-KiB groups of an unpacked block
    static constexpr unsigned GROUP_ELEMS = 1024 / SZ;
    static constexpr unsigned SCAN_BITS = SZ <= 2 ? 32 : 64;  // width of the packed per-group counts
    static constexpr unsigned FIELD_BITS = SCAN_BITS / GROUPS;   // u8 32, u16 16, u32 16, u64 8 (a u64 group holds 128 elements)
    static_assert((1ull << FIELD_BITS) > GROUP_ELEMS, "a group's total must fit its field");

    // first index (= mask bit) lane `lane` owns in group k; it owns [first_bit, first_bit + N)
    FL_HD static unsigned first_bit(unsigned k, unsigned lane) { return k * GROUP_ELEMS + lane * N; }
    // the mask word that holds the lane's slice of group k, and the slice taken out of it (bit e = index first_bit + e)
    FL_HD static unsigned mask_word(unsigned k, unsigned lane) { return first_bit(k, lane) >> 5; }
    FL_HD static uint32_t slice(uint32_t word, unsigned k, unsigned lane) { return (word >> (first_bit(k, lane) & 31u)) & ((1u << N) - 1u); }

    // a lane's count of group k in its field of the packed word; a field of a packed word
    FL_HD static uint64_t pack_count(unsigned count, unsigned k) { return (uint64_t)count << (k * FIELD_BITS); }
    FL_HD static unsigned field(uint64_t packed, unsigned k) { return (unsigned)((packed >> (k * FIELD_BITS)) & ((1ull << FIELD_BITS) - 1ull)); }
    // kept elements of the groups before k (`totals`: the inclusive scan's value in lane 63); k = GROUPS: of the whole block
    FL_HD static unsigned group_base(uint64_t totals, unsigned k)
    {
        unsigned s = 0;
        for (unsigned j = 0; j < k; ++j) s += field(totals, j);
        return s;
    }
    // where element e of the lane's group-k cell lands in the run, if its bit is set (`excl`: the lane's EXCLUSIVE scan value)
    FL_HD static unsigned landing(uint64_t totals, uint64_t excl, unsigned k, uint32_t slice_bits, unsigned e)
    {
        return group_base(totals, k) + field(excl, k) + (unsigned)__builtin_popcount(slice_bits & ((1u << e) - 1u));
    }
};

}  // namespace fl
