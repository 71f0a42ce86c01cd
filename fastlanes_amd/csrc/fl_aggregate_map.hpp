// fl_aggregate_map.hpp -- the arithmetic of unfor_aggregate (fl_aggregate.hpp) that needs no decode, shared by the kernels and a CPU test
// that compiles this header with a plain C++ compiler (tests/test_aggregate_cpu.py).  No HIP dependency.
//
// A block's aggregate over the rows its mask keeps is {count, sum, min, max}: unsigned values zero-extended to 64 bits, the sum wrapping
// mod 2^64 (as unpack_block_sums).  Nothing kept gives the IDENTITY of `combine`: {0, 0, UINT64_MAX, 0}.  Integer add, min and max are
// associative and commutative, so any order of combining the blocks gives the same bits.
//
// Two kinds of block are answered from their metadata alone -- no packed byte is read:
//   * an EMPTY mask: the identity;
//   * width 0: every value is the block's reference r (macros.rs:118-125 + ffor.rs:46-48), so count = popcount(mask),
//     sum = count * r (wrapping), min = max = r.
#pragma once
#include <stdint.h>

#ifndef FL_HD            // (also defined, identically, by fl_tile_map.hpp, fl_for_decide.hpp and fl_select_map.hpp)
#if defined(__HIPCC__) || defined(__HIP__)
#define FL_HD __host__ __device__
#else
#define FL_HD
#endif
#endif

namespace fl {

// the layout of fl_block_aggregate (include/fastlanes_amd.h): 32 bytes
struct BlockAggregate {
    uint64_t count, sum, min, max;
};
static_assert(sizeof(BlockAggregate) == 32, "fl_block_aggregate");

FL_HD inline BlockAggregate aggregate_identity() { return BlockAggregate{0ull, 0ull, ~0ull, 0ull}; }

FL_HD inline BlockAggregate aggregate_combine(const BlockAggregate& a, const BlockAggregate& b)
{
    return BlockAggregate{a.count + b.count, a.sum + b.sum, a.min < b.min ? a.min : b.min, a.max > b.max ? a.max : b.max};
}

// what a block of `count` kept rows and width `w` needs
enum AggregateRoute { AGG_IDENTITY = 0, AGG_CONSTANT = 1, AGG_DECODE = 2 };
FL_HD inline AggregateRoute aggregate_route(unsigned count, unsigned w)
{
    return count == 0u ? AGG_IDENTITY : w == 0u ? AGG_CONSTANT : AGG_DECODE;
}

// `count` kept rows (>= 0) that all hold `value` (the reference, zero-extended): the answer of AGG_IDENTITY and AGG_CONSTANT
FL_HD inline BlockAggregate aggregate_constant_block(unsigned count, uint64_t value)
{
    if (count == 0u) return aggregate_identity();
    return BlockAggregate{count, (uint64_t)count * value, value, value};
}

}  // namespace fl
