// fl_aggregate_by_map.hpp -- the arithmetic of unfor_aggregate_by (fl_aggregate_by.hpp) that needs no decode, shared by the kernel and a
// CPU test that compiles this header with a plain C++ compiler (tests/test_aggregate_by_cpu.py).  No HIP dependency.
//
// Two FoR-packed columns of the same block count are joined row by row: a VALUE column of type T and a KEY column of type u8.  The
// answer is one BlockAggregate (fl_aggregate_map.hpp) per possible key, 256 of them, each the combination of the kept rows that carry
// that key.  A block is judged from its metadata and its mask before any packed byte is requested (aggregate_by_route), and the two
// columns meet through 1 KiB of LDS that holds the block's 1024 decoded keys IN INDEX ORDER (aggregate_by_key_store /
// aggregate_by_key_byte): the lane maps of a u8 block and of a block of T differ, the index order is what they share.
#pragma once
#include "fl_aggregate_map.hpp"
#include "fl_select_map.hpp"

namespace fl {

constexpr unsigned AGGREGATE_BY_GROUPS = 256;      // one slot per possible u8 key: a key can never be out of range
constexpr unsigned AGGREGATE_BY_KEY_BYTES = 1024;  // a block's decoded keys (and, before that, its packed key rows: at most 128 * 8 bytes)
constexpr unsigned AGGREGATE_BY_TABLE_BYTES = AGGREGATE_BY_GROUPS * (unsigned)sizeof(BlockAggregate);

// What a block needs.
//   SKIP     the mask keeps nothing, or one of the two columns fails a device check: nothing is read, nothing is contributed;
//   ONE_KEY  key width 0: every kept row has the key column's reference, so the value side is unfor_aggregate's block (its own width-0
//            constant route included) and its ONE BlockAggregate is folded into one slot -- no key byte is read;
//   DECODE   both columns are decoded (a value width of 0 requests no value byte).
enum AggregateByRoute { AGGBY_SKIP = 0, AGGBY_ONE_KEY = 1, AGGBY_DECODE = 2 };
FL_HD inline AggregateByRoute aggregate_by_route(bool mask_empty, bool precondition_ok, unsigned key_width)
{
    return mask_empty || !precondition_ok ? AGGBY_SKIP : key_width == 0u ? AGGBY_ONE_KEY : AGGBY_DECODE;
}
// whether the route requests packed bytes of the key / of the value column
FL_HD inline bool aggregate_by_reads_keys(AggregateByRoute route) { return route == AGGBY_DECODE; }
FL_HD inline bool aggregate_by_reads_values(AggregateByRoute route, unsigned value_width) { return route != AGGBY_SKIP && value_width != 0u; }

// The key area.  A u8 block is ONE 1-KiB group: lane l decodes the 16 keys of indices 16 l .. 16 l + 15 and stores its cell there.
FL_HD inline unsigned aggregate_by_key_store(unsigned lane) { return SelectMap<1>::first_bit(0, lane); }
// The lane of the VALUE decode holds, of group k, the N = 16 / SZ indices from SelectMap<SZ>::first_bit(k, lane) on: the key of its
// element e is the byte at that index -- N consecutive bytes, N-aligned: one LDS read per cell.
template <unsigned SZ> FL_HD inline unsigned aggregate_by_key_byte(unsigned k, unsigned lane, unsigned e)
{
    return SelectMap<SZ>::first_bit(k, lane) + e;
}

// per-wavefront LDS: the value block's image, the key area, the table
FL_HD constexpr unsigned aggregate_by_wave_lds(unsigned value_block_bytes)
{
    return value_block_bytes + AGGREGATE_BY_KEY_BYTES + AGGREGATE_BY_TABLE_BYTES;
}

}  // namespace fl
