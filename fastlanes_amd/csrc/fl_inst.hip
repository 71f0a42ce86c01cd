// fl_inst.hip -- explicit instantiation unit.  Compiled once per
// (element type, family) with -DFL_T=<type> -DFL_FAMILY=<n> so the 124 (T,W)
// pairs x 5 width-parameterised kernels build in parallel:
//   0 unpack (store)   1 unfor_pack   2 undelta_pack   3 pack   4 for_pack
//   5 delta / undelta / transpose / untranspose / unpack_single
//   6 wave-per-block kernels: unpack / pack over per-block (or uniform) widths (fl_widths.hpp), Delta chains (fl_chain.hpp)
//   10 fused consumers: unpack_block_sums, block_min_max   11 / 12 unpack_compare (selection masks: x <= k / x == k)
//   8 undelta_pack+untranspose (fused decode to original order)   9 transpose+delta+pack (fused encode)
//   13 unfor_compare (selection masks from FoR-packed columns, uniform or mixed width; fl_for_compare.hpp)
//   14 unfor_select (only the rows a selection mask keeps, from the same columns; fl_select.hpp)
//   15 unfor_aggregate (count / sum / min / max per block of the rows a mask keeps, from the same columns; fl_aggregate.hpp)
//   16 unfor_compare_range (interval predicates over the same columns, chained through the mask so far; fl_for_compare_range.hpp)
//   17 unfor_aggregate_by (count / sum / min / max per u8 key of the rows a mask keeps, value and key column both FoR-packed; fl_aggregate_by.hpp)
//   18 unfor_compare_columns (a <op> b between two FoR-packed columns of one type, chained through the mask so far; fl_for_compare_columns.hpp)
//   19 unfor_aggregate_columns (count / sum / min / max per block of a * b, a + b or a - b between two such columns under a mask; fl_aggregate_columns.hpp)
//   20 unfor_compare_in (set membership over the same columns: a window of the value domain plus a bitmap, chained through the mask so far; fl_for_compare_in.hpp)
//   21 unfor_aggregate_by_columns (count / sum / min / max per u8 key of a * b, a + b or a - b between two such columns under a mask, all three columns FoR-packed; fl_aggregate_by_columns.hpp)
//   22 unfor_set_build (the member set of the values a mask keeps of such a column, ORed into a window's bitmap: the build side of unfor_compare_in; fl_set_build.hpp)
//   23 unfor_aggregate_by_window (count / sum / min / max per key of a dense window of the key domain, value and key column FoR-packed and of one type, accumulated into the caller's arrays; fl_aggregate_by_window.hpp)
//   24 unfor_lookup (a dimension attribute of the key's own type or u8 fetched through such a column inside a dense window of the key domain under a mask, written in full-width packed order: the probe side of a payload join; fl_lookup.hpp)
//   25 unfor_aggregate_by_lookup (count / sum / min / max per u8 attribute fetched through a key column inside a dense window of the key domain, value and key column FoR-packed and of one type: unfor_lookup_u8 and unfor_aggregate_by in one pass with no per-row output; fl_aggregate_by_lookup.hpp)
//   26 undelta_compare_range (an interval predicate over a Delta-packed column, joined with the mask so far: the chains are decoded in place of the rows, no value is untransposed, a block its bases decide reads no packed byte; fl_delta_compare_range.hpp)
//   27 undelta_aggregate (count / sum / min / max per block of the rows a mask keeps of a Delta-packed column: the chains are aggregated where they are decoded, each under its T-bit group of the mask, no value is untransposed, an empty-mask or width-0 block reads no packed byte; fl_delta_aggregate.hpp)
//   28 undelta_select (the rows a mask keeps of a Delta-packed column, compacted in original row order: the chains are compacted where they are decoded, a kept row lands at the popcount of the mask below it, no value is untransposed, an empty-mask or width-0 block reads no packed byte; fl_delta_select.hpp)
#include "fl_kernels.hpp"
#include "fl_misc.hpp"
#include "fl_widths.hpp"
#include "fl_chain.hpp"
#include "fl_batch.hpp"
#include "fl_consume.hpp"
#include "fl_for_compare.hpp"
#include "fl_for_compare_range.hpp"
#include "fl_select.hpp"
#include "fl_aggregate.hpp"
#include "fl_aggregate_by.hpp"
#include "fl_for_compare_columns.hpp"
#include "fl_aggregate_columns.hpp"
#include "fl_for_compare_in.hpp"
#include "fl_aggregate_by_columns.hpp"
#include "fl_set_build.hpp"
#include "fl_aggregate_by_window.hpp"
#include "fl_lookup.hpp"
#include "fl_aggregate_by_lookup.hpp"
#include "fl_delta_compare_range.hpp"
#include "fl_delta_aggregate.hpp"
#include "fl_delta_select.hpp"

namespace fl {
using T = FL_T;
using Ws = std::make_integer_sequence<int, Elem<T>::BITS + 1>;

#if FL_FAMILY == 0
static constexpr WidthTable<T> t_store = make_unpack_table<T, BODY_STORE>(Ws{});
template <> const WidthTable<T>& unpack_table_impl<T, BODY_STORE>() { return t_store; }
#elif FL_FAMILY == 1
static constexpr WidthTable<T> t_addref = make_unpack_table<T, BODY_ADD_REF>(Ws{});
template <> const WidthTable<T>& unpack_table_impl<T, BODY_ADD_REF>() { return t_addref; }
#elif FL_FAMILY == 2
static constexpr WidthTable<T> t_undelta = make_unpack_table<T, BODY_UNDELTA>(Ws{});
template <> const WidthTable<T>& unpack_table_impl<T, BODY_UNDELTA>() { return t_undelta; }
#elif FL_FAMILY == 3
static constexpr WidthTable<T> t_pack = make_pack_table<T, PACK_PLAIN>(Ws{});
template <> const WidthTable<T>& pack_table_impl<T, PACK_PLAIN>() { return t_pack; }
#elif FL_FAMILY == 4
static constexpr WidthTable<T> t_forpack = make_pack_table<T, PACK_FOR>(Ws{});
template <> const WidthTable<T>& pack_table_impl<T, PACK_FOR>() { return t_forpack; }
#elif FL_FAMILY == 5
template <> stream_launch_t delta_launcher<T>(bool inverse)
{
    return inverse ? &launch_delta<T, true> : &launch_delta<T, false>;
}
template <> stream_launch_t transpose_launcher<T>(bool inverse)
{
    return inverse ? &launch_transpose<T, true> : &launch_transpose<T, false>;
}
template <> hipError_t unpack_single_launch<T>(const SingleArgs& a, hipStream_t s)
{
    return launch_unpack_single<T>(a, s);
}
#elif FL_FAMILY == 6
template <> widths_launch_t widths_launcher<T>(bool pack)
{
    return pack ? &launch_widths<T, true> : &launch_widths<T, false>;
}
template <> batch_launch_t batch_launcher<T>(bool pack)
{
    return pack ? &launch_batch<T, true> : &launch_batch<T, false>;
}
template <> batch_launch_t batch_chain_launcher<T>(int op)
{
    switch (op) {
    case OP_UNDELTA_PACK: return &launch_batch_chain<T, SRC_PACKED, CHAIN_UNDELTA, SNK_ROWS>;
    case OP_UNDELTA_PACK_UNTRANSPOSE: return &launch_batch_chain<T, SRC_PACKED, CHAIN_UNDELTA, SNK_ORIGINAL>;
    case OP_TRANSPOSE_DELTA_PACK: return &launch_batch_chain<T, SRC_ORIGINAL, CHAIN_DELTA, SNK_PACKED>;
    default: return nullptr;
    }
}
template <> chain_launch_t chain_launcher<T>(int op)
{
    switch (op) {
    case OP_UNDELTA_PACK: return &launch_chain<T, SRC_PACKED, CHAIN_UNDELTA, SNK_ROWS, RD_AUTO>;
    case OP_UNDELTA: return &launch_chain<T, SRC_ROWS, CHAIN_UNDELTA, SNK_ROWS>;
    case OP_DELTA: return &launch_chain<T, SRC_ROWS, CHAIN_DELTA, SNK_ROWS>;
    case OP_UNTRANSPOSE: return &launch_chain<T, SRC_ROWS, CHAIN_NONE, SNK_ORIGINAL>;
    case OP_TRANSPOSE: return &launch_chain<T, SRC_ORIGINAL, CHAIN_NONE, SNK_ROWS>;
    case OP_UNDELTA_PACK_UNTRANSPOSE: return &launch_chain<T, SRC_PACKED, CHAIN_UNDELTA, SNK_ORIGINAL, RD_AUTO>;
    case OP_TRANSPOSE_DELTA_PACK: return &launch_chain<T, SRC_ORIGINAL, CHAIN_DELTA, SNK_PACKED>;
    default: return nullptr;
    }
}
template <> chain_launch_t chain_launcher_two_blocks<T>(int op)
{
    if constexpr (sizeof(T) >= 4) {
        if (op == OP_UNDELTA_PACK) return &launch_chain<T, SRC_PACKED, CHAIN_UNDELTA, SNK_ROWS, RD_VGPR, 2>;
    }
    return nullptr;
}
template <> chain_launch_t chain_widths_launcher<T>(int op)
{
    constexpr unsigned B = chain_blocks_per_wave<T>();
    if constexpr (sizeof(T) == 1) {                         // u8's decode: column lanes, pipelined (fl_chain.hpp)
        if (op == OP_UNDELTA_PACK) return &launch_chain_columns_pipelined<T, SNK_ROWS>;
        if (op == OP_UNDELTA_PACK_UNTRANSPOSE) return &launch_chain_columns_pipelined<T, SNK_ORIGINAL>;
        if (op == OP_TRANSPOSE_DELTA_PACK) return &launch_chain_columns_encode_pipelined<T>;
    }
    switch (op) {
    // (one block per wavefront -- u32 / u64 -- goes through chain_stage_source: RD_AUTO = a mixed-width column's packed rows stream
    // non-temporally by LDS-DMA, as in unpack_widths; the lockstep form of the narrow types always did)
    case OP_UNDELTA_PACK: return &launch_chain<T, SRC_PACKED, CHAIN_UNDELTA, SNK_ROWS, RD_AUTO, B>;
    case OP_UNDELTA_PACK_UNTRANSPOSE: return &launch_chain<T, SRC_PACKED, CHAIN_UNDELTA, SNK_ORIGINAL, RD_AUTO, B>;
    case OP_TRANSPOSE_DELTA_PACK: return &launch_chain<T, SRC_ORIGINAL, CHAIN_DELTA, SNK_PACKED, RD_VGPR, B>;
    default: return nullptr;
    }
}
#elif FL_FAMILY == 8
static constexpr WidthTable<T> t_undelta_untr = make_unpack_table<T, BODY_UNDELTA_UNTRANSPOSE>(Ws{});
template <> const WidthTable<T>& unpack_table_impl<T, BODY_UNDELTA_UNTRANSPOSE>() { return t_undelta_untr; }
#elif FL_FAMILY == 9
static constexpr WidthTable<T> t_tr_delta_pack = make_pack_table<T, PACK_TRANSPOSE_DELTA>(Ws{});
template <> const WidthTable<T>& pack_table_impl<T, PACK_TRANSPOSE_DELTA>() { return t_tr_delta_pack; }
#elif FL_FAMILY == 10
static constexpr ReduceTable<T> t_sums = make_sum_table<T>(Ws{});
template <> const ReduceTable<T>& sum_table_impl<T>() { return t_sums; }
template <> reduce_launch_t min_max_launcher<T>() { return &launch_block_min_max<T>; }
#elif FL_FAMILY == 11
static constexpr CompareTable<T> t_compare_le = make_compare_table<T, false>(Ws{});
template <> const CompareTable<T>& compare_table_impl<T, false>() { return t_compare_le; }
#elif FL_FAMILY == 12
static constexpr CompareTable<T> t_compare_eq = make_compare_table<T, true>(Ws{});
template <> const CompareTable<T>& compare_table_impl<T, true>() { return t_compare_eq; }
#elif FL_FAMILY == 13
template <> for_compare_launch_t for_compare_launcher<T>() { return &launch_block_consumer<T, ForCompareArgs, k_unfor_compare<T>, false>; }
#elif FL_FAMILY == 14
template <> select_launch_t select_launcher<T>() { return &launch_block_consumer<T, SelectArgs, k_unfor_select<T>, true>; }
#elif FL_FAMILY == 15
template <> aggregate_launch_t aggregate_launcher<T>() { return &launch_block_consumer<T, AggregateArgs, k_unfor_aggregate<T>, true>; }
#elif FL_FAMILY == 16
template <> for_range_launch_t for_range_launcher<T>() { return &launch_block_consumer<T, ForRangeArgs, k_unfor_compare_range<T>, false>; }
#elif FL_FAMILY == 17
template <> aggregate_by_launch_t aggregate_by_launcher<T>() { return &launch_aggregate_by<T>; }
#elif FL_FAMILY == 18
template <> for_columns_launch_t for_columns_launcher<T>() { return &launch_block_consumer<T, ForColumnsArgs, k_unfor_compare_columns<T>, false>; }
#elif FL_FAMILY == 19
template <> aggregate_columns_launch_t aggregate_columns_launcher<T>() { return &launch_block_consumer<T, AggregateColumnsArgs, k_unfor_aggregate_columns<T>, false>; }
#elif FL_FAMILY == 20
template <> for_in_launch_t for_in_launcher<T>(bool register_tier)
{
    return register_tier ? &launch_block_consumer<T, ForInArgs, k_unfor_compare_in<T, true>, false>
                         : &launch_block_consumer<T, ForInArgs, k_unfor_compare_in<T, false>, false>;
}
#elif FL_FAMILY == 21
template <> aggregate_by_columns_launch_t aggregate_by_columns_launcher<T>() { return &launch_aggregate_by_columns<T>; }
#elif FL_FAMILY == 22
template <> set_build_launch_t set_build_launcher<T>(int tier)
{
    if constexpr (sizeof(T) >= 4) {                         // a window above SET_BUILD_LDS_BITS: only the wide types have one
        if (tier == SETB_MEM) return &launch_set_build<T, SETB_MEM>;
        if (tier == SETB_MEM_TEST) return &launch_set_build<T, SETB_MEM_TEST>;
    }
    return tier == SETB_LDS ? &launch_set_build<T, SETB_LDS> : nullptr;
}
#elif FL_FAMILY == 23
template <> aggregate_by_window_launch_t aggregate_by_window_launcher<T>(int tier)
{
    if constexpr (sizeof(T) >= 2) {                         // a window above AGGREGATE_BY_WINDOW_LDS_GROUPS: u8 has none
        if (tier == AGGW_MEM) return &launch_aggregate_by_window<T, AGGW_MEM>;
    }
    return tier == AGGW_LDS ? &launch_aggregate_by_window<T, AGGW_LDS> : nullptr;
}
#elif FL_FAMILY == 24
template <> lookup_launch_t lookup_launcher<T>(unsigned payload_bytes, int tier)
{
    if (payload_bytes == sizeof(T)) {
        if constexpr (sizeof(T) >= 2) {                     // a table above LOOKUP_LDS_BYTES: 256 slots of u8 never are
            if (tier == LOOKUP_MEM) return &launch_lookup<T, T, LOOKUP_MEM>;
        }
        return tier == LOOKUP_LDS ? &launch_lookup<T, T, LOOKUP_LDS> : nullptr;
    }
    if constexpr (sizeof(T) >= 2) {                         // the u8 payload of a wider key (u8's own is the pair above)
        if (payload_bytes == 1u) return tier == LOOKUP_LDS ? &launch_lookup<T, uint8_t, LOOKUP_LDS> : tier == LOOKUP_MEM ? &launch_lookup<T, uint8_t, LOOKUP_MEM> : nullptr;
    }
    return nullptr;
}
#elif FL_FAMILY == 25
template <> aggregate_by_lookup_launch_t aggregate_by_lookup_launcher<T>() { return &launch_aggregate_by_lookup<T>; }
#elif FL_FAMILY == 26
template <> delta_range_launch_t delta_range_launcher<T>() { return &launch_block_consumer<T, DeltaRangeArgs, k_undelta_compare_range<T>, false>; }
#elif FL_FAMILY == 27
template <> delta_aggregate_launch_t delta_aggregate_launcher<T>() { return &launch_block_consumer<T, DeltaAggregateArgs, k_undelta_aggregate<T>, false>; }
#elif FL_FAMILY == 28
template <> delta_select_launch_t delta_select_launcher<T>() { return &launch_block_consumer<T, DeltaSelectArgs, k_undelta_select<T>, false>; }
#else
#error "FL_FAMILY must be 0..6 or 8..28"
#endif
}  // namespace fl
