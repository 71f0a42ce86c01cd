// fl_consumer_tier.hpp -- the host side of the consumers of a packed column (fl_for_block.hpp), and their extern "C" entry points:
// unfor_compare, _compare_range, _compare_in, _compare_columns, _select, _aggregate, _aggregate_columns, _aggregate_by,
// _aggregate_by_columns, _aggregate_by_window, _aggregate_by_lookup, _set_build, _lookup (and _lookup_u8) over a FoR-packed column,
// undelta_compare_range, undelta_select and undelta_aggregate over a Delta-packed one.  Included by exactly one translation unit of the library (fl_capi.hip), as
// fl_host_tier.hpp and fl_scan.hpp are, below that file's Column, WaveShape, with_policy, widths_args, no_bytes and FL_FOR_EACH_TYPE.
// In this order: the column value; the refusal steps, once each; the repeated parts of the argument blocks, once each; the sixteen
// run_*, each composing the steps top to bottom in ITS order -- the status of a call with two faults depends on it, and
// tests/test_cabi_refusals_cpu.py records it; extern "C".
#pragma once
#include "fl_consume.hpp"
#include "fl_for_compare.hpp"
#include "fl_for_compare_range.hpp"
#include "fl_for_compare_in.hpp"
#include "fl_for_compare_columns.hpp"
#include "fl_delta_compare_range.hpp"
#include "fl_delta_aggregate.hpp"
#include "fl_delta_select.hpp"
#include "fl_select.hpp"
#include "fl_aggregate.hpp"
#include "fl_aggregate_columns.hpp"
#include "fl_aggregate_by.hpp"
#include "fl_aggregate_by_columns.hpp"
#include "fl_aggregate_by_window.hpp"
#include "fl_aggregate_by_lookup.hpp"
#include "fl_set_build.hpp"
#include "fl_lookup.hpp"

namespace {

using namespace fl;

// One packed column of a consumer: uniform-width (form.width, blocks back to back) or mixed-width (widths[] / offsets[], checked per
// block by the kernel).  refs: FoR's references, block b's at refs[b * ref_stride] (stride 1: one per block, 0: one for the column)
// -- or, for undelta_compare_range, undelta_select and undelta_aggregate, Delta's bases, with stride 0.  All columns of one call have one form.
template <typename T> struct PackedColumn {
    Column form;
    const T* packed;
    const T* refs;
    size_t ref_stride;
};
template <typename T> PackedColumn<T> uniform_column(unsigned width, const T* packed, const T* refs, size_t ref_stride)
{
    return {{false, width}, packed, refs, ref_stride};
}
template <typename T>
PackedColumn<T> mixed_column(const uint8_t* widths, const uint64_t* offsets, const T* packed, size_t packed_bytes, const T* refs, size_t ref_stride)
{
    return {{true, 0, widths, offsets, packed_bytes}, packed, refs, ref_stride};
}

// ---- the refusal steps ------------------------------------------------------------------------------------------------------------
// FL_ERR_WIDTH: a uniform column wider than its type (a mixed column's widths are the kernel's to check)
template <typename... C> bool any_over_width(const PackedColumn<C>&... c) { return ((!c.form.mixed && over_width<C>(c.form.width)) || ...); }
// Inputs that are read only under a condition -- mask_in unless FL_MASK_NEW, a set's words or a table and its `present` unless there
// are zero bits or slots, a window's four arrays unless there are zero groups: when unused they are dropped, so never read and never
// checked.  Returns `unused`; where it is false the caller requires what it must have.
template <typename... P> bool dropped(bool unused, P*&... p)
{
    if (unused) ((p = nullptr), ...);
    return unused;
}
// FL_ERR_NULL: one of a column's pointers is missing.  A mixed-width column whose blocks all have width 0 has no packed bytes: its
// packed pointer may be NULL (run_widths) and is replaced here; so may a uniform column's of width 0, which is never read.
template <typename T> bool block_consumer_column(PackedColumn<T>& c)
{
    if (c.form.mixed && !c.packed && c.form.packed_bytes == 0) c.packed = no_bytes<T>();
    return c.refs && (!c.form.mixed || (c.form.widths && c.form.offsets)) && (c.packed || (!c.form.mixed && c.form.width == 0));
}
template <typename... C> bool columns_present(PackedColumn<C>&... c) { return (block_consumer_column(c) && ...); }
// FL_ERR_ALIGN (NULL is aligned: what may be NULL is judged before)
template <typename... P> bool any_misaligned(const P*... p) { return (misaligned(p) || ...); }

// ---- the repeated parts of the argument blocks ------------------------------------------------------------------------------------
// The two launch shapes: that of unfor_pack_widths -- the same blocks, the same reads -- and the persistent grid, which takes the
// policy's waves as its residency and the policy's blocks per wavefront as the least length of a wavefront's run (0: the column
// divided evenly).
template <typename T> WaveShape block_consumer_shape()
{
    return with_policy({mixed_waves(Elem<T>::BITS, false), mixed_blocks_per_wave(Elem<T>::BITS, false), mixed_prefetch(Elem<T>::BITS)});
}
inline WaveShape persistent_grid_shape() { return with_policy({0, 0u, 0u}); }
// The WidthsArgs of one column; the kernels load the references with the block's metadata, so they travel beside it.  Only a
// mixed-width column's blocks can fail a kernel's checks, so only it gets the error flag (unfor_select and undelta_select are the exceptions).
template <typename T> void column_args(WidthsArgs& a, const PackedColumn<T>& c, size_t n_blocks, uint32_t* err_flag, const WaveShape& sh)
{
    widths_args<T>(a, c.form, c.packed, nullptr, nullptr, c.ref_stride, c.form.mixed ? err_flag : nullptr, n_blocks, sh);
}
template <typename T> WaveShape block_consumer_args(WidthsArgs& a, const PackedColumn<T>& c, size_t n_blocks, uint32_t* err_flag)
{
    const WaveShape sh = block_consumer_shape<T>();
    column_args<T>(a, c, n_blocks, err_flag, sh);
    return sh;
}
// the predicate (a cyclic interval, or a set's or table's window) and the mask chain, in whichever block has them
template <typename A> void predicate_args(A& a, const ForPredicate& p)
{
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = p.none ? 1u : 0u;
}
template <typename A> void chain_args(A& a, const uint32_t* mask_in, int combine)
{
    a.mask_in = reinterpret_cast<const char*>(mask_in);
    a.combine = (unsigned)combine;
}

// ---- the consumers ----------------------------------------------------------------------------------------------------------------
// unfor_compare (fl_for_compare.hpp).  The predicate becomes its cyclic interval here, once per call.
// Order: width; op; the empty column; the column and `mask`; alignment.
template <typename T>
int run_unfor_compare(PackedColumn<T> col, int op, T constant, size_t n_blocks, uint32_t* mask, uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (op < FL_CMP_EQ || op > FL_CMP_GE) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!columns_present(col) || !mask) return FL_ERR_NULL;
    if (any_misaligned(col.packed, mask)) return FL_ERR_ALIGN;
    ForCompareArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, n_blocks, err_flag);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = col.refs;
    predicate_args(a, for_compare_predicate(Elem<T>::BITS, op, constant));
    return hip_status(for_compare_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_compare_range (fl_for_compare_range.hpp): the cyclic interval [lo, hi] as the predicate and the mask so far beside it; `mask`
// may be `mask_in`.  Order: width; combine; the empty column; mask_in; the column and `mask`; alignment.
template <typename T>
int run_unfor_compare_range(PackedColumn<T> col, T lo, T hi, int combine, const uint32_t* mask_in, size_t n_blocks, uint32_t* mask,
                            uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (combine < FL_MASK_NEW || combine > FL_MASK_OR) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!dropped(combine == FL_MASK_NEW, mask_in) && !mask_in) return FL_ERR_NULL;
    if (!columns_present(col) || !mask) return FL_ERR_NULL;
    if (any_misaligned(col.packed, mask, mask_in)) return FL_ERR_ALIGN;
    ForRangeArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, n_blocks, err_flag);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = col.refs;
    predicate_args(a, for_range_predicate(Elem<T>::BITS, lo, hi));
    chain_args(a, mask_in, combine);
    return hip_status(for_range_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// undelta_compare_range (fl_delta_compare_range.hpp): unfor_compare_range over a Delta-packed column -- col.refs are the bases (LANES per
// block, 128 bytes, read as 16-byte cells), required and aligned.  One block per wavefront for every type, at unfor_pack_widths'
// occupancy; `mask` may be `mask_in`.  Order: width; combine; the empty column; mask_in; the column, its bases and `mask`; alignment.
template <typename T>
int run_undelta_compare_range(PackedColumn<T> col, T lo, T hi, int combine, const uint32_t* mask_in, size_t n_blocks, uint32_t* mask,
                              uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (combine < FL_MASK_NEW || combine > FL_MASK_OR) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!dropped(combine == FL_MASK_NEW, mask_in) && !mask_in) return FL_ERR_NULL;
    if (!columns_present(col) || !mask) return FL_ERR_NULL;
    if (any_misaligned(col.packed, col.refs, mask, mask_in)) return FL_ERR_ALIGN;
    const WaveShape sh = with_policy({mixed_waves(Elem<T>::BITS, false), 1u, 0u});
    DeltaRangeArgs a;
    column_args<T>(a, col, n_blocks, err_flag, sh);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = nullptr;
    predicate_args(a, for_range_predicate(Elem<T>::BITS, lo, hi));
    chain_args(a, mask_in, combine);
    a.bases = reinterpret_cast<const char*>(col.refs);
    return hip_status(delta_range_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_compare_in (fl_for_compare_in.hpp, fl_set_decide.hpp): the member set's window as the predicate and its bitmap beside it.
// set_bits decides the tier here, once per call: up to SET_REGISTER_BITS the bitmap rides in a VGPR.  Order: width; combine, negate
// and set_bits; the empty column; mask_in; set_words; the column and `mask`; alignment.
template <typename T>
int run_unfor_compare_in(PackedColumn<T> col, T set_lo, uint64_t set_bits, const uint32_t* set_words, int negate, int combine,
                         const uint32_t* mask_in, size_t n_blocks, uint32_t* mask, uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (combine < FL_MASK_NEW || combine > FL_MASK_OR || negate < 0 || negate > 1 || set_bits > set_max_bits(Elem<T>::BITS)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!dropped(combine == FL_MASK_NEW, mask_in) && !mask_in) return FL_ERR_NULL;
    if (!dropped(set_bits == 0, set_words) && !set_words) return FL_ERR_NULL;
    if (!columns_present(col) || !mask) return FL_ERR_NULL;
    if (any_misaligned(col.packed, mask, mask_in, set_words)) return FL_ERR_ALIGN;
    ForInArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, n_blocks, err_flag);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = col.refs;
    predicate_args(a, set_window(Elem<T>::BITS, set_lo, set_bits));
    chain_args(a, mask_in, combine);
    a.set_words = set_words;
    a.set_bytes = (unsigned)(4u * set_word_count(set_bits));
    a.negate = (unsigned)negate;
    return hip_status(for_in_launcher<T>(set_bits <= SET_REGISTER_BITS)(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_compare_columns (fl_for_compare_columns.hpp): two columns of T.  The six ops become one base relation, "swap the columns" and
// "invert" here, once per call (fl_columns_decide.hpp: columns_relation); the swap is done here, so the kernel's column a is always
// the base relation's left side.  `mask` may be `mask_in`.  Order: widths; op and combine; the empty column; mask_in; the columns and
// `mask`; alignment.
template <typename T>
int run_unfor_compare_columns(PackedColumn<T> cola, PackedColumn<T> colb, int op, int is_signed, int combine, const uint32_t* mask_in,
                              size_t n_blocks, uint32_t* mask, uint32_t* err_flag, void* stream)
{
    if (any_over_width(cola, colb)) return FL_ERR_WIDTH;
    if (op < FL_CMP_EQ || op > FL_CMP_GE || combine < FL_MASK_NEW || combine > FL_MASK_OR) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!dropped(combine == FL_MASK_NEW, mask_in) && !mask_in) return FL_ERR_NULL;
    if (!columns_present(cola, colb) || !mask) return FL_ERR_NULL;
    if (any_misaligned(cola.packed, colb.packed, mask, mask_in)) return FL_ERR_ALIGN;
    const ColumnsRelation rel = columns_relation(op);
    const PackedColumn<T>&left = rel.swap ? colb : cola, &right = rel.swap ? cola : colb;
    ForColumnsArgs a;
    const WaveShape sh = block_consumer_args<T>(a, left, n_blocks, err_flag);
    block_consumer_args<T>(a.b, right, n_blocks, err_flag);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = left.refs;
    a.b_refs = right.refs;
    predicate_args(a, ForPredicate{0, 0, false});
    chain_args(a, mask_in, combine);
    a.bias = columns_bias(Elem<T>::BITS, is_signed != 0);
    a.is_eq = rel.is_eq ? 1u : 0u;
    a.invert = rel.invert ? 1u : 0u;
    return hip_status(for_columns_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_select (fl_select.hpp).  Order: width; the empty column; the column, `mask`, `out_offsets` and `out`; alignment.
template <typename T>
int run_unfor_select(PackedColumn<T> col, const uint32_t* mask, const uint64_t* out_offsets, T* out, size_t out_len, size_t n_blocks,
                     uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (n_blocks == 0) return FL_OK;
    // a selection that keeps nothing has no output: `out` may be NULL with out_len == 0 (a non-empty block then fails the kernel's
    // bounds check; nothing is ever written through this pointer)
    if (!out && out_len == 0) out = const_cast<T*>(no_bytes<T>());
    if (!columns_present(col) || !mask || !out_offsets || !out) return FL_ERR_NULL;
    if (any_misaligned(col.packed, mask, out)) return FL_ERR_ALIGN;
    SelectArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, n_blocks, err_flag);
    // err_flag for a uniform-width column too, the only consumer that takes one: this form raises FL_DEVERR_BOUNDS (a run outside `out`)
    a.err_flag = err_flag;
    a.mask = mask;
    a.out_offsets = out_offsets;
    a.out = reinterpret_cast<char*>(out);
    a.out_len = out_len;
    a.sel_refs = col.refs;
    return hip_status(select_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// undelta_select (fl_delta_select.hpp): unfor_select over a Delta-packed column -- col.refs are the bases (LANES per block, 128 bytes,
// read as 16-byte cells), required and aligned.  One block per wavefront for every type, at unfor_pack_widths' occupancy.  Order
// (unfor_select's): width; the empty column; the column, its bases, `mask`, `out_offsets` and `out`; alignment.
template <typename T>
int run_undelta_select(PackedColumn<T> col, const uint32_t* mask, const uint64_t* out_offsets, T* out, size_t out_len, size_t n_blocks,
                       uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (n_blocks == 0) return FL_OK;
    // a selection that keeps nothing has no output: `out` may be NULL with out_len == 0, as for unfor_select
    if (!out && out_len == 0) out = const_cast<T*>(no_bytes<T>());
    if (!columns_present(col) || !mask || !out_offsets || !out) return FL_ERR_NULL;
    if (any_misaligned(col.packed, col.refs, mask, out)) return FL_ERR_ALIGN;
    const WaveShape sh = with_policy({mixed_waves(Elem<T>::BITS, false), 1u, 0u});
    DeltaSelectArgs a;
    column_args<T>(a, col, n_blocks, err_flag, sh);
    a.err_flag = err_flag;                 // for a uniform-width column too: this form raises FL_DEVERR_BOUNDS (a run outside `out`)
    a.mask = mask;
    a.out_offsets = out_offsets;
    a.out = reinterpret_cast<char*>(out);
    a.out_len = out_len;
    a.sel_refs = nullptr;
    a.bases = reinterpret_cast<const char*>(col.refs);
    return hip_status(delta_select_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate (fl_aggregate.hpp: a block that fails the kernel's checks leaves the identity in its slot).  `mask` may be NULL:
// every row is kept and no mask is read.  Order: width; the empty column; the column and `block_aggs`; alignment.
template <typename T>
int run_unfor_aggregate(PackedColumn<T> col, const uint32_t* mask, size_t n_blocks, void* block_aggs, uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (n_blocks == 0) return FL_OK;
    if (!columns_present(col) || !block_aggs) return FL_ERR_NULL;
    if (any_misaligned(col.packed, mask, block_aggs)) return FL_ERR_ALIGN;
    AggregateArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, n_blocks, err_flag);
    a.mask = mask;
    a.aggs = static_cast<char*>(block_aggs);
    a.agg_refs = col.refs;
    return hip_status(aggregate_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// undelta_aggregate (fl_delta_aggregate.hpp): unfor_aggregate over a Delta-packed column -- col.refs are the bases (LANES per block, 128
// bytes, read as 16-byte cells), required and aligned; a block that fails the kernel's checks leaves the identity in its slot; `mask` may
// be NULL.  One block per wavefront for every type, at unfor_pack_widths' occupancy.  Order (unfor_aggregate's): width; the empty
// column; the column, its bases and `block_aggs`; alignment.
template <typename T>
int run_undelta_aggregate(PackedColumn<T> col, const uint32_t* mask, size_t n_blocks, void* block_aggs, uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (n_blocks == 0) return FL_OK;
    if (!columns_present(col) || !block_aggs) return FL_ERR_NULL;
    if (any_misaligned(col.packed, col.refs, mask, block_aggs)) return FL_ERR_ALIGN;
    const WaveShape sh = with_policy({mixed_waves(Elem<T>::BITS, false), 1u, 0u});
    DeltaAggregateArgs a;
    column_args<T>(a, col, n_blocks, err_flag, sh);
    a.mask = mask;
    a.aggs = static_cast<char*>(block_aggs);
    a.agg_refs = nullptr;
    a.bases = reinterpret_cast<const char*>(col.refs);
    return hip_status(delta_aggregate_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate_columns (fl_aggregate_columns.hpp): two columns of T met element by element under `expr` and aggregated per block as
// unfor_aggregate does (a block that fails either column's checks leaves the identity in its slot).  Order: widths; expr; the empty
// column; the columns and `block_aggs`; alignment.
template <typename T>
int run_unfor_aggregate_columns(int expr, PackedColumn<T> cola, PackedColumn<T> colb, const uint32_t* mask, size_t n_blocks, void* block_aggs,
                                uint32_t* err_flag, void* stream)
{
    if (any_over_width(cola, colb)) return FL_ERR_WIDTH;
    if (!expr_valid(expr)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!columns_present(cola, colb) || !block_aggs) return FL_ERR_NULL;
    if (any_misaligned(cola.packed, colb.packed, mask, block_aggs)) return FL_ERR_ALIGN;
    AggregateColumnsArgs a;
    const WaveShape sh = block_consumer_args<T>(a, cola, n_blocks, err_flag);
    block_consumer_args<T>(a.b, colb, n_blocks, err_flag);
    a.mask = mask;
    a.aggs = static_cast<char*>(block_aggs);
    a.agg_refs = cola.refs;
    a.b_refs = colb.refs;
    a.expr = (unsigned)expr;
    return hip_status(aggregate_columns_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate_by (fl_aggregate_by.hpp): a value column of T and a u8 key column; a block that fails either column's checks
// contributes nothing.  `result` (256 slots) is written by EVERY call -- the init launch also answers an empty column -- so it is
// required and checked whatever n_blocks is.  Order: widths; `result`; the columns unless empty; alignment, the columns' and the
// mask's unless empty, then `result`'s.
template <typename T>
int run_unfor_aggregate_by(PackedColumn<T> col, PackedColumn<uint8_t> kcol, const uint32_t* mask, size_t n_blocks, void* result,
                           uint32_t* err_flag, void* stream)
{
    if (any_over_width(col, kcol)) return FL_ERR_WIDTH;
    if (!result) return FL_ERR_NULL;
    if (n_blocks && !columns_present(col, kcol)) return FL_ERR_NULL;
    if ((n_blocks && any_misaligned(col.packed, kcol.packed, mask)) || misaligned(result)) return FL_ERR_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipError_t e = launch_aggregate_by_init(static_cast<BlockAggregate*>(result), s); e != hipSuccess || n_blocks == 0) return hip_status(e);
    const WaveShape sh = persistent_grid_shape();
    AggregateByArgs a;
    column_args<T>(a.val, col, n_blocks, err_flag, sh);
    column_args<uint8_t>(a.key, kcol, n_blocks, err_flag, sh);
    a.val_refs = col.refs;
    a.key_refs = kcol.refs;
    a.mask = mask;
    a.result = static_cast<BlockAggregate*>(result);
    a.run = 0;
    return hip_status(aggregate_by_launcher<T>()(a, sh.waves, s));
}

// unfor_aggregate_by_columns (fl_aggregate_by_columns.hpp): two value columns of T met under `expr` and a u8 key column; a block that
// fails any column's checks contributes nothing.  `result` as unfor_aggregate_by has it.  Order: widths; expr; `result`; the columns
// unless empty; alignment, the columns' and the mask's unless empty, then `result`'s.
template <typename T>
int run_unfor_aggregate_by_columns(int expr, PackedColumn<T> cola, PackedColumn<T> colb, PackedColumn<uint8_t> kcol, const uint32_t* mask,
                                   size_t n_blocks, void* result, uint32_t* err_flag, void* stream)
{
    if (any_over_width(cola, colb, kcol)) return FL_ERR_WIDTH;
    if (!expr_valid(expr)) return FL_ERR_INDEX;
    if (!result) return FL_ERR_NULL;
    if (n_blocks && !columns_present(cola, colb, kcol)) return FL_ERR_NULL;
    if ((n_blocks && any_misaligned(cola.packed, colb.packed, kcol.packed, mask)) || misaligned(result)) return FL_ERR_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipError_t e = launch_aggregate_by_init(static_cast<BlockAggregate*>(result), s); e != hipSuccess || n_blocks == 0) return hip_status(e);
    const WaveShape sh = persistent_grid_shape();
    AggregateByColumnsArgs a;
    column_args<T>(a.a, cola, n_blocks, err_flag, sh);
    column_args<T>(a.b, colb, n_blocks, err_flag, sh);
    column_args<uint8_t>(a.key, kcol, n_blocks, err_flag, sh);
    a.a_refs = cola.refs;
    a.b_refs = colb.refs;
    a.key_refs = kcol.refs;
    a.mask = mask;
    a.result = static_cast<BlockAggregate*>(result);
    a.run = 0;
    a.expr = (unsigned)expr;
    return hip_status(aggregate_by_columns_launcher<T>()(a, sh.waves, s));
}

// unfor_set_build (fl_set_build.hpp): the member set unfor_compare_in probes, built from a column under a mask; `mask` and `stats` may
// be NULL.  set_bits decides the tier here, once per call (fl_set_build_map.hpp: set_build_lds_tier).  The memory tier ships
// SET_BUILD_MEMORY_TIER; the timing tool measures the other variant beside it through the environment variable
// FL_INTERNAL_SET_BUILD_VARIANT (1: one atomic per element, 2: test before set; read on every memory-tier call, bits identical either
// way).  Order: width; set_bits; the empty column; set_words; the column; alignment, set_words' and stats' included.
constexpr int SET_BUILD_MEMORY_TIER = SETB_MEM_TEST;
inline int set_build_tier(uint64_t set_bits)
{
    if (set_build_lds_tier(set_bits)) return SETB_LDS;
    if (const char* v = std::getenv("FL_INTERNAL_SET_BUILD_VARIANT")) {
        if (v[0] == '1' && !v[1]) return SETB_MEM;
        if (v[0] == '2' && !v[1]) return SETB_MEM_TEST;
    }
    return SET_BUILD_MEMORY_TIER;
}
template <typename T>
int run_unfor_set_build(PackedColumn<T> col, const uint32_t* mask, size_t n_blocks, T set_lo, uint64_t set_bits, uint32_t* set_words,
                        uint64_t* stats, uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (set_bits > set_max_bits(Elem<T>::BITS)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!dropped(set_bits == 0, set_words) && !set_words) return FL_ERR_NULL;
    if (!columns_present(col)) return FL_ERR_NULL;
    if (any_misaligned(col.packed, mask, set_words, stats)) return FL_ERR_ALIGN;
    const WaveShape sh = persistent_grid_shape();
    SetBuildArgs a;
    column_args<T>(a.col, col, n_blocks, err_flag, sh);
    a.refs = col.refs;
    a.mask = mask;
    a.set_words = set_words;
    a.stats = stats;
    predicate_args(a, set_window(Elem<T>::BITS, set_lo, set_bits));
    a.n_words = (unsigned)set_word_count(set_bits);
    a.last_mask = set_build_last_word_mask(set_bits);
    a.run = 0;
    const set_build_launch_t fn = set_build_launcher<T>(set_build_tier(set_bits));
    if (!fn) return hip_fail(hipErrorInvalidDeviceFunction);
    return hip_status(fn(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate_by_window (fl_aggregate_by_window.hpp): a value column and a key column of T, grouped inside the window [key_lo,
// key_lo + n_groups - 1] into the caller's four arrays; they, `mask` and `stats` may be NULL.  An empty window touches no array.
// Order: widths; n_groups; the empty column; the columns; alignment, the arrays' and stats' included.
struct WindowArrays {
    uint64_t *counts, *sums, *mins, *maxs, *stats;
};
template <typename T>
int run_unfor_aggregate_by_window(PackedColumn<T> col, PackedColumn<T> kcol, const uint32_t* mask, size_t n_blocks, T key_lo, uint64_t n_groups,
                                  WindowArrays t, uint32_t* err_flag, void* stream)
{
    if (any_over_width(col, kcol)) return FL_ERR_WIDTH;
    if (n_groups > aggregate_by_window_max_groups(Elem<T>::BITS)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    dropped(n_groups == 0, t.counts, t.sums, t.mins, t.maxs);
    if (!columns_present(col, kcol)) return FL_ERR_NULL;
    if (any_misaligned(col.packed, kcol.packed, mask, t.counts, t.sums, t.mins, t.maxs, t.stats)) return FL_ERR_ALIGN;
    const WaveShape sh = persistent_grid_shape();
    AggregateByWindowArgs a;
    column_args<T>(a.val, col, n_blocks, err_flag, sh);
    column_args<T>(a.key, kcol, n_blocks, err_flag, sh);
    a.val_refs = col.refs;
    a.key_refs = kcol.refs;
    a.mask = mask;
    a.counts = t.counts;
    a.sums = t.sums;
    a.mins = t.mins;
    a.maxs = t.maxs;
    a.stats = t.stats;
    predicate_args(a, set_window(Elem<T>::BITS, key_lo, n_groups));
    a.need_values = t.sums || t.mins || t.maxs ? 1u : 0u;
    a.n_slots = aggregate_by_window_lds_tier(n_groups) ? (unsigned)n_groups : 0u;
    a.run = 0;
    const aggregate_by_window_launch_t fn = aggregate_by_window_launcher<T>(aggregate_by_window_lds_tier(n_groups) ? AGGW_LDS : AGGW_MEM);
    if (!fn) return hip_fail(hipErrorInvalidDeviceFunction);
    return hip_status(fn(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_lookup (fl_lookup.hpp): table[(key - key_lo) mod 2^T] of every kept row of a key column, the payload of T or of uint8_t,
// written in full-width packed order with the hits as a mask beside it; `mask`, `present`, `hit_mask` and `stats` may be NULL.  An
// empty window reads neither the table nor the bitmap.  n_slots decides the tier here, once per call (fl_lookup_map.hpp:
// lookup_tier).  Order: width; n_slots (above min(2^T, 2^32) slots, or a table of 2^31 bytes or more); the empty column; `table`; the
// column and `out`; alignment.
struct LookupTable {
    const void* table;
    const uint32_t* present;
    uint64_t missing;
    void* out;
    uint32_t* hit_mask;
    uint64_t* stats;
};
template <typename T>
int run_unfor_lookup(PackedColumn<T> col, const uint32_t* mask, size_t n_blocks, T key_lo, uint64_t n_slots, unsigned payload_bytes,
                     LookupTable t, uint32_t* err_flag, void* stream)
{
    if (any_over_width(col)) return FL_ERR_WIDTH;
    if (lookup_slots_refused(Elem<T>::BITS, n_slots, payload_bytes)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!dropped(n_slots == 0, t.table, t.present) && !t.table) return FL_ERR_NULL;
    if (!columns_present(col) || !t.out) return FL_ERR_NULL;
    if (any_misaligned(col.packed, mask, t.hit_mask, t.present, t.table, t.out, t.stats)) return FL_ERR_ALIGN;
    const WaveShape sh = persistent_grid_shape();
    LookupArgs a;
    column_args<T>(a.col, col, n_blocks, err_flag, sh);
    a.refs = col.refs;
    a.mask = mask;
    a.table = t.table;
    a.present = t.present;
    a.out = static_cast<char*>(t.out);
    a.hit_mask = t.hit_mask;
    a.stats = t.stats;
    predicate_args(a, set_window(Elem<T>::BITS, key_lo, n_slots));
    a.missing = t.missing;
    a.table_bytes = (unsigned)(n_slots * payload_bytes);
    a.present_bytes = t.present ? (unsigned)(4u * set_word_count(n_slots)) : 0u;
    a.run = 0;
    const lookup_launch_t fn = lookup_launcher<T>(payload_bytes, lookup_tier(n_slots, payload_bytes));
    if (!fn) return hip_fail(hipErrorInvalidDeviceFunction);
    return hip_status(fn(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate_by_lookup (fl_aggregate_by_lookup.hpp): unfor_lookup_u8 and unfor_aggregate_by in one pass -- a value column and a key
// column of T, a u8 table over the window [key_lo, key_lo + n_slots - 1], 256 groups; `mask`, `present` and `stats` may be NULL.
// `result` as unfor_aggregate_by has it.  Order: widths; n_slots (lookup_slots_refused with a one-byte payload); `result`; unless
// empty: `table`, the columns, and the alignment of all but `result`; then `result`'s alignment.
struct LookupGroups {
    const uint8_t* table;
    const uint32_t* present;
    void* result;
    uint64_t* stats;
};
template <typename T>
int run_unfor_aggregate_by_lookup(PackedColumn<T> col, PackedColumn<T> kcol, const uint32_t* mask, size_t n_blocks, T key_lo, uint64_t n_slots,
                                  LookupGroups t, uint32_t* err_flag, void* stream)
{
    if (any_over_width(col, kcol)) return FL_ERR_WIDTH;
    if (lookup_slots_refused(Elem<T>::BITS, n_slots, 1u)) return FL_ERR_INDEX;
    if (!t.result) return FL_ERR_NULL;
    if (n_blocks) {
        if (!dropped(n_slots == 0, t.table, t.present) && !t.table) return FL_ERR_NULL;
        if (!columns_present(col, kcol)) return FL_ERR_NULL;
        if (any_misaligned(col.packed, kcol.packed, mask, t.present, t.table, t.stats)) return FL_ERR_ALIGN;
    }
    if (misaligned(t.result)) return FL_ERR_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipError_t e = launch_aggregate_by_init(static_cast<BlockAggregate*>(t.result), s); e != hipSuccess || n_blocks == 0) return hip_status(e);
    const WaveShape sh = persistent_grid_shape();
    AggregateByLookupArgs a;
    column_args<T>(a.val, col, n_blocks, err_flag, sh);
    column_args<T>(a.key, kcol, n_blocks, err_flag, sh);
    a.val_refs = col.refs;
    a.key_refs = kcol.refs;
    a.mask = mask;
    a.table = t.table;
    a.present = t.present;
    a.result = static_cast<BlockAggregate*>(t.result);
    a.stats = t.stats;
    predicate_args(a, set_window(Elem<T>::BITS, key_lo, n_slots));
    a.table_bytes = (unsigned)n_slots;
    a.present_bytes = t.present ? (unsigned)(4u * set_word_count(n_slots)) : 0u;
    a.run = 0;
    return hip_status(aggregate_by_lookup_launcher<T>()(a, sh.waves, s));
}

}  // namespace

// ---- extern "C": both forms of every consumer; the column values are made here, once -----------------------------------------------
extern "C" {

// the parameters of one column in either form, and the value they make (P: the prefix of the parameters' names, T: the column's type)
#define FL_UNIFORM_PARAMS(T, P) unsigned P##w, const T* P##pk, const T* P##r, size_t P##rs
#define FL_MIXED_PARAMS(T, P) const uint8_t* P##w, const uint64_t* P##o, const T* P##pk, size_t P##pb, const T* P##r, size_t P##rs
#define FL_UNIFORM(T, P) uniform_column<T>(P##w, P##pk, P##r, P##rs)
#define FL_MIXED(T, P) mixed_column<T>(P##w, P##o, P##pk, P##pb, P##r, P##rs)

#define FL_DEFINE_FOR_COMPARE(T, S)                                                                                                  \
    int fl_##S##_unfor_compare(FL_UNIFORM_PARAMS(T, ), int op, T k, size_t n, uint32_t* mask, void* s)                               \
    { FL_DEVICE_TIER(s, pk, r, mask); return run_unfor_compare<T>(FL_UNIFORM(T, ), op, k, n, mask, nullptr, s); }                    \
    int fl_##S##_unfor_compare_widths(FL_MIXED_PARAMS(T, ), int op, T k, size_t n, uint32_t* mask, uint32_t* ef, void* s)            \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, ef); return run_unfor_compare<T>(FL_MIXED(T, ), op, k, n, mask, ef, s); }
FL_FOR_EACH_TYPE(FL_DEFINE_FOR_COMPARE)

#define FL_DEFINE_FOR_COMPARE_RANGE(T, S)                                                                                            \
    int fl_##S##_unfor_compare_range(FL_UNIFORM_PARAMS(T, ), T lo, T hi, int cb, const uint32_t* mi, size_t n, uint32_t* mask, void* s) \
    { FL_DEVICE_TIER(s, pk, r, mi, mask); return run_unfor_compare_range<T>(FL_UNIFORM(T, ), lo, hi, cb, mi, n, mask, nullptr, s); } \
    int fl_##S##_unfor_compare_range_widths(FL_MIXED_PARAMS(T, ), T lo, T hi, int cb, const uint32_t* mi, size_t n, uint32_t* mask,  \
                                            uint32_t* ef, void* s)                                                                   \
    { FL_DEVICE_TIER(s, w, o, pk, r, mi, mask, ef); return run_unfor_compare_range<T>(FL_MIXED(T, ), lo, hi, cb, mi, n, mask, ef, s); }
FL_FOR_EACH_TYPE(FL_DEFINE_FOR_COMPARE_RANGE)

// Delta's bases stand where the references stood, with stride 0
#define FL_DEFINE_DELTA_COMPARE_RANGE(T, S)                                                                                          \
    int fl_##S##_undelta_compare_range(unsigned w, const T* pk, const T* b, T lo, T hi, int cb, const uint32_t* mi, size_t n,        \
                                       uint32_t* mask, void* s)                                                                      \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, pk, b, mi, mask);                                                                                          \
        return run_undelta_compare_range<T>(uniform_column<T>(w, pk, b, 0), lo, hi, cb, mi, n, mask, nullptr, s);                    \
    }                                                                                                                                \
    int fl_##S##_undelta_compare_range_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* b, T lo, T hi, int cb, \
                                              const uint32_t* mi, size_t n, uint32_t* mask, uint32_t* ef, void* s)                   \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, w, o, pk, b, mi, mask, ef);                                                                                \
        return run_undelta_compare_range<T>(mixed_column<T>(w, o, pk, pb, b, 0), lo, hi, cb, mi, n, mask, ef, s);                    \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_DELTA_COMPARE_RANGE)

#define FL_DEFINE_FOR_COMPARE_IN(T, S)                                                                                               \
    int fl_##S##_unfor_compare_in(FL_UNIFORM_PARAMS(T, ), T lo, uint64_t sb, const uint32_t* sw, int ng, int cb, const uint32_t* mi, \
                                  size_t n, uint32_t* mask, void* s)                                                                 \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, pk, r, sw, mi, mask);                                                                                      \
        return run_unfor_compare_in<T>(FL_UNIFORM(T, ), lo, sb, sw, ng, cb, mi, n, mask, nullptr, s);                                \
    }                                                                                                                                \
    int fl_##S##_unfor_compare_in_widths(FL_MIXED_PARAMS(T, ), T lo, uint64_t sb, const uint32_t* sw, int ng, int cb, const uint32_t* mi, \
                                         size_t n, uint32_t* mask, uint32_t* ef, void* s)                                            \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, w, o, pk, r, sw, mi, mask, ef);                                                                            \
        return run_unfor_compare_in<T>(FL_MIXED(T, ), lo, sb, sw, ng, cb, mi, n, mask, ef, s);                                       \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_FOR_COMPARE_IN)

#define FL_DEFINE_FOR_COMPARE_COLUMNS(T, S)                                                                                          \
    int fl_##S##_unfor_compare_columns(FL_UNIFORM_PARAMS(T, a), FL_UNIFORM_PARAMS(T, b), int op, int sg, int cb, const uint32_t* mi, \
                                       size_t n, uint32_t* mask, void* s)                                                            \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, apk, ar, bpk, br, mi, mask);                                                                               \
        return run_unfor_compare_columns<T>(FL_UNIFORM(T, a), FL_UNIFORM(T, b), op, sg, cb, mi, n, mask, nullptr, s);                \
    }                                                                                                                                \
    int fl_##S##_unfor_compare_columns_widths(FL_MIXED_PARAMS(T, a), FL_MIXED_PARAMS(T, b), int op, int sg, int cb, const uint32_t* mi, \
                                              size_t n, uint32_t* mask, uint32_t* ef, void* s)                                       \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, aw, ao, apk, ar, bw, bo, bpk, br, mi, mask, ef);                                                           \
        return run_unfor_compare_columns<T>(FL_MIXED(T, a), FL_MIXED(T, b), op, sg, cb, mi, n, mask, ef, s);                         \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_FOR_COMPARE_COLUMNS)

#define FL_DEFINE_SELECT(T, S)                                                                                                       \
    int fl_##S##_unfor_select(FL_UNIFORM_PARAMS(T, ), const uint32_t* mask, const uint64_t* oo, T* out, size_t ol, size_t n,         \
                              uint32_t* ef, void* s)                                                                                 \
    { FL_DEVICE_TIER(s, pk, r, mask, oo, out, ef); return run_unfor_select<T>(FL_UNIFORM(T, ), mask, oo, out, ol, n, ef, s); }       \
    int fl_##S##_unfor_select_widths(FL_MIXED_PARAMS(T, ), const uint32_t* mask, const uint64_t* oo, T* out, size_t ol, size_t n,    \
                                     uint32_t* ef, void* s)                                                                          \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, oo, out, ef); return run_unfor_select<T>(FL_MIXED(T, ), mask, oo, out, ol, n, ef, s); }
FL_FOR_EACH_TYPE(FL_DEFINE_SELECT)

#define FL_DEFINE_AGGREGATE(T, S)                                                                                                    \
    int fl_##S##_unfor_aggregate(FL_UNIFORM_PARAMS(T, ), const uint32_t* mask, size_t n, void* aggs, uint32_t* ef, void* s)          \
    { FL_DEVICE_TIER(s, pk, r, mask, aggs, ef); return run_unfor_aggregate<T>(FL_UNIFORM(T, ), mask, n, aggs, ef, s); }              \
    int fl_##S##_unfor_aggregate_widths(FL_MIXED_PARAMS(T, ), const uint32_t* mask, size_t n, void* aggs, uint32_t* ef, void* s)     \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, aggs, ef); return run_unfor_aggregate<T>(FL_MIXED(T, ), mask, n, aggs, ef, s); }
FL_FOR_EACH_TYPE(FL_DEFINE_AGGREGATE)

// Delta's bases stand where the references stood, with stride 0
#define FL_DEFINE_DELTA_AGGREGATE(T, S)                                                                                              \
    int fl_##S##_undelta_aggregate(unsigned w, const T* pk, const T* b, const uint32_t* mask, size_t n, void* aggs, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, pk, b, mask, aggs, ef); return run_undelta_aggregate<T>(uniform_column<T>(w, pk, b, 0), mask, n, aggs, ef, s); } \
    int fl_##S##_undelta_aggregate_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* b, const uint32_t* mask, \
                                          size_t n, void* aggs, uint32_t* ef, void* s)                                               \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, w, o, pk, b, mask, aggs, ef);                                                                              \
        return run_undelta_aggregate<T>(mixed_column<T>(w, o, pk, pb, b, 0), mask, n, aggs, ef, s);                                  \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_DELTA_AGGREGATE)

// Delta's bases stand where the reference stood, with stride 0
#define FL_DEFINE_DELTA_SELECT(T, S)                                                                                                 \
    int fl_##S##_undelta_select(unsigned w, const T* pk, const T* b, const uint32_t* mask, const uint64_t* oo, T* out, size_t ol,    \
                                size_t n, uint32_t* ef, void* s)                                                                     \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, pk, b, mask, oo, out, ef);                                                                                 \
        return run_undelta_select<T>(uniform_column<T>(w, pk, b, 0), mask, oo, out, ol, n, ef, s);                                   \
    }                                                                                                                                \
    int fl_##S##_undelta_select_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* b, const uint32_t* mask, \
                                       const uint64_t* oo, T* out, size_t ol, size_t n, uint32_t* ef, void* s)                       \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, w, o, pk, b, mask, oo, out, ef);                                                                           \
        return run_undelta_select<T>(mixed_column<T>(w, o, pk, pb, b, 0), mask, oo, out, ol, n, ef, s);                              \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_DELTA_SELECT)

#define FL_DEFINE_AGGREGATE_COLUMNS(T, S)                                                                                            \
    int fl_##S##_unfor_aggregate_columns(int ex, FL_UNIFORM_PARAMS(T, a), FL_UNIFORM_PARAMS(T, b), const uint32_t* mask, size_t n,   \
                                         void* aggs, uint32_t* ef, void* s)                                                          \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, apk, ar, bpk, br, mask, aggs, ef);                                                                         \
        return run_unfor_aggregate_columns<T>(ex, FL_UNIFORM(T, a), FL_UNIFORM(T, b), mask, n, aggs, ef, s);                         \
    }                                                                                                                                \
    int fl_##S##_unfor_aggregate_columns_widths(int ex, FL_MIXED_PARAMS(T, a), FL_MIXED_PARAMS(T, b), const uint32_t* mask, size_t n, \
                                                void* aggs, uint32_t* ef, void* s)                                                   \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, aw, ao, apk, ar, bw, bo, bpk, br, mask, aggs, ef);                                                         \
        return run_unfor_aggregate_columns<T>(ex, FL_MIXED(T, a), FL_MIXED(T, b), mask, n, aggs, ef, s);                             \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_AGGREGATE_COLUMNS)

#define FL_DEFINE_AGGREGATE_BY(T, S)                                                                                                 \
    int fl_##S##_unfor_aggregate_by(FL_UNIFORM_PARAMS(T, ), FL_UNIFORM_PARAMS(uint8_t, k), const uint32_t* mask, size_t n, void* res, \
                                    uint32_t* ef, void* s)                                                                           \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, pk, r, kpk, kr, mask, res, ef);                                                                            \
        return run_unfor_aggregate_by<T>(FL_UNIFORM(T, ), FL_UNIFORM(uint8_t, k), mask, n, res, ef, s);                              \
    }                                                                                                                                \
    int fl_##S##_unfor_aggregate_by_widths(FL_MIXED_PARAMS(T, ), FL_MIXED_PARAMS(uint8_t, k), const uint32_t* mask, size_t n, void* res, \
                                           uint32_t* ef, void* s)                                                                    \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, w, o, pk, r, kw, ko, kpk, kr, mask, res, ef);                                                              \
        return run_unfor_aggregate_by<T>(FL_MIXED(T, ), FL_MIXED(uint8_t, k), mask, n, res, ef, s);                                  \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_AGGREGATE_BY)

#define FL_DEFINE_AGGREGATE_BY_COLUMNS(T, S)                                                                                         \
    int fl_##S##_unfor_aggregate_by_columns(int ex, FL_UNIFORM_PARAMS(T, a), FL_UNIFORM_PARAMS(T, b), FL_UNIFORM_PARAMS(uint8_t, k), \
                                            const uint32_t* mask, size_t n, void* res, uint32_t* ef, void* s)                        \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, apk, ar, bpk, br, kpk, kr, mask, res, ef);                                                                 \
        return run_unfor_aggregate_by_columns<T>(ex, FL_UNIFORM(T, a), FL_UNIFORM(T, b), FL_UNIFORM(uint8_t, k), mask, n, res, ef, s); \
    }                                                                                                                                \
    int fl_##S##_unfor_aggregate_by_columns_widths(int ex, FL_MIXED_PARAMS(T, a), FL_MIXED_PARAMS(T, b), FL_MIXED_PARAMS(uint8_t, k), \
                                                   const uint32_t* mask, size_t n, void* res, uint32_t* ef, void* s)                 \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, aw, ao, apk, ar, bw, bo, bpk, br, kw, ko, kpk, kr, mask, res, ef);                                         \
        return run_unfor_aggregate_by_columns<T>(ex, FL_MIXED(T, a), FL_MIXED(T, b), FL_MIXED(uint8_t, k), mask, n, res, ef, s);     \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_AGGREGATE_BY_COLUMNS)

#define FL_DEFINE_SET_BUILD(T, S)                                                                                                    \
    int fl_##S##_unfor_set_build(FL_UNIFORM_PARAMS(T, ), const uint32_t* mask, size_t n, T lo, uint64_t sb, uint32_t* sw, uint64_t* st, \
                                 void* s)                                                                                            \
    { FL_DEVICE_TIER(s, pk, r, mask, sw, st); return run_unfor_set_build<T>(FL_UNIFORM(T, ), mask, n, lo, sb, sw, st, nullptr, s); } \
    int fl_##S##_unfor_set_build_widths(FL_MIXED_PARAMS(T, ), const uint32_t* mask, size_t n, T lo, uint64_t sb, uint32_t* sw,       \
                                        uint64_t* st, uint32_t* ef, void* s)                                                         \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, sw, st, ef); return run_unfor_set_build<T>(FL_MIXED(T, ), mask, n, lo, sb, sw, st, ef, s); }
FL_FOR_EACH_TYPE(FL_DEFINE_SET_BUILD)

#define FL_DEFINE_AGGREGATE_BY_WINDOW(T, S)                                                                                          \
    int fl_##S##_unfor_aggregate_by_window(FL_UNIFORM_PARAMS(T, ), FL_UNIFORM_PARAMS(T, k), const uint32_t* mask, size_t n, T lo,    \
                                           uint64_t ng, uint64_t* cn, uint64_t* sm, uint64_t* mn, uint64_t* mx, uint64_t* st, void* s) \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, pk, r, kpk, kr, mask, cn, sm, mn, mx, st);                                                                 \
        return run_unfor_aggregate_by_window<T>(FL_UNIFORM(T, ), FL_UNIFORM(T, k), mask, n, lo, ng, {cn, sm, mn, mx, st}, nullptr, s); \
    }                                                                                                                                \
    int fl_##S##_unfor_aggregate_by_window_widths(FL_MIXED_PARAMS(T, ), FL_MIXED_PARAMS(T, k), const uint32_t* mask, size_t n, T lo, \
                                                  uint64_t ng, uint64_t* cn, uint64_t* sm, uint64_t* mn, uint64_t* mx, uint64_t* st, \
                                                  uint32_t* ef, void* s)                                                             \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, w, o, pk, r, kw, ko, kpk, kr, mask, cn, sm, mn, mx, st, ef);                                               \
        return run_unfor_aggregate_by_window<T>(FL_MIXED(T, ), FL_MIXED(T, k), mask, n, lo, ng, {cn, sm, mn, mx, st}, ef, s);        \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_AGGREGATE_BY_WINDOW)

// U: the payload's type, T (unfor_lookup) or uint8_t (unfor_lookup_u8)
#define FL_DEFINE_LOOKUP_FORMS(T, S, U, NAME)                                                                                        \
    int fl_##S##_##NAME(FL_UNIFORM_PARAMS(T, ), const uint32_t* mask, size_t n, T lo, uint64_t ns, const U* tb, const uint32_t* pr, U ms, \
                        U* out, uint32_t* hm, uint64_t* st, void* s)                                                                 \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, pk, r, mask, tb, pr, out, hm, st);                                                                         \
        return run_unfor_lookup<T>(FL_UNIFORM(T, ), mask, n, lo, ns, (unsigned)sizeof(U), {tb, pr, ms, out, hm, st}, nullptr, s);    \
    }                                                                                                                                \
    int fl_##S##_##NAME##_widths(FL_MIXED_PARAMS(T, ), const uint32_t* mask, size_t n, T lo, uint64_t ns, const U* tb, const uint32_t* pr, \
                                 U ms, U* out, uint32_t* hm, uint64_t* st, uint32_t* ef, void* s)                                    \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, w, o, pk, r, mask, tb, pr, out, hm, st, ef);                                                               \
        return run_unfor_lookup<T>(FL_MIXED(T, ), mask, n, lo, ns, (unsigned)sizeof(U), {tb, pr, ms, out, hm, st}, ef, s);           \
    }
#define FL_DEFINE_LOOKUP(T, S) FL_DEFINE_LOOKUP_FORMS(T, S, T, unfor_lookup)
#define FL_DEFINE_LOOKUP_U8(T, S) FL_DEFINE_LOOKUP_FORMS(T, S, uint8_t, unfor_lookup_u8)
FL_FOR_EACH_TYPE(FL_DEFINE_LOOKUP)
FL_FOR_EACH_TYPE(FL_DEFINE_LOOKUP_U8)

#define FL_DEFINE_AGGREGATE_BY_LOOKUP(T, S)                                                                                          \
    int fl_##S##_unfor_aggregate_by_lookup(FL_UNIFORM_PARAMS(T, ), FL_UNIFORM_PARAMS(T, k), const uint32_t* mask, size_t n, T lo,    \
                                           uint64_t ns, const uint8_t* tb, const uint32_t* pr, void* res, uint64_t* st, uint32_t* ef, \
                                           void* s)                                                                                  \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, pk, r, kpk, kr, mask, tb, pr, res, st, ef);                                                                \
        return run_unfor_aggregate_by_lookup<T>(FL_UNIFORM(T, ), FL_UNIFORM(T, k), mask, n, lo, ns, {tb, pr, res, st}, ef, s);       \
    }                                                                                                                                \
    int fl_##S##_unfor_aggregate_by_lookup_widths(FL_MIXED_PARAMS(T, ), FL_MIXED_PARAMS(T, k), const uint32_t* mask, size_t n, T lo, \
                                                  uint64_t ns, const uint8_t* tb, const uint32_t* pr, void* res, uint64_t* st,       \
                                                  uint32_t* ef, void* s)                                                             \
    {                                                                                                                                \
        FL_DEVICE_TIER(s, w, o, pk, r, kw, ko, kpk, kr, mask, tb, pr, res, st, ef);                                                  \
        return run_unfor_aggregate_by_lookup<T>(FL_MIXED(T, ), FL_MIXED(T, k), mask, n, lo, ns, {tb, pr, res, st}, ef, s);           \
    }
FL_FOR_EACH_TYPE(FL_DEFINE_AGGREGATE_BY_LOOKUP)

}  // extern "C"
