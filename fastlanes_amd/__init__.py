"""fastlanes_amd -- MI355X-native FastLanes codec hot path (pack / unpack /
FoR / Delta / transpose of 1024-value blocks) behind the reference's trait
names.  The compute lives in libfastlanes_amd.so (hand-written gfx950 HIP
kernels, C ABI in include/fastlanes_amd.h); this package is the thin host-side
mirror of the reference interface.  No CPU fallback exists."""
from ._lib import (LIB_PATH, aggregate_by_columns_symbols, aggregate_by_window_symbols, aggregate_by_symbols, aggregate_columns_symbols, aggregate_symbols, exported_symbols, for_compare_columns_symbols, for_compare_in_symbols, for_compare_range_symbols, for_compare_symbols, load,  # noqa: F401
                   aggregate_by_lookup_symbols, delta_aggregate_symbols, delta_compare_range_symbols, delta_select_symbols, lookup_symbols, select_symbols, set_build_symbols)
from .codec import (Batch, BitPacking, Delta, FastLanesError, FoR, MemberSet, MixedWidthPlan,  # noqa: F401
                    Transpose, aggregate_reduce, for_pack_widths, for_widths, mask_offsets, member_set, pack_widths, packed_len, predicate_interval,
                    transpose_delta_pack_widths, undelta_pack_widths, unfor_aggregate_by_columns_widths, unfor_aggregate_by_widths, unfor_aggregate_columns_widths, unfor_aggregate_widths, unfor_compare_columns_widths, unfor_compare_in_widths, unfor_compare_range_widths, unfor_compare_widths, unfor_pack_widths,
                    unfor_select_widths, column_window, unfor_set_build_widths, GroupTable, unfor_aggregate_by_window_widths,
                    unfor_lookup_widths, full_width_column, unfor_aggregate_by_lookup_widths, undelta_compare_range_widths,
                    undelta_aggregate_widths, undelta_select_widths, unpack_single_widths, unpack_widths, widths_to_offsets)

FL_ORDER = (0, 4, 2, 6, 1, 5, 3, 7)  # lib.rs:22

__all__ = ["BitPacking", "FoR", "Delta", "Transpose", "FastLanesError", "packed_len", "MixedWidthPlan", "Batch",
           "unpack_widths", "pack_widths", "unpack_single_widths", "widths_to_offsets",
           "unfor_pack_widths", "for_pack_widths", "for_widths", "undelta_pack_widths", "transpose_delta_pack_widths",
           "unfor_compare_widths", "unfor_compare_range_widths", "predicate_interval", "mask_offsets", "unfor_select_widths", "unfor_aggregate_widths", "aggregate_reduce",
           "unfor_aggregate_by_widths", "aggregate_by_symbols", "aggregate_symbols", "FL_ORDER", "load", "exported_symbols", "for_compare_symbols", "for_compare_range_symbols",
           "unfor_compare_columns_widths", "for_compare_columns_symbols",
           "unfor_aggregate_columns_widths", "aggregate_columns_symbols",
           "member_set", "MemberSet", "unfor_compare_in_widths", "for_compare_in_symbols",
           "unfor_aggregate_by_columns_widths", "aggregate_by_columns_symbols",
           "unfor_set_build_widths", "column_window", "set_build_symbols",
           "unfor_aggregate_by_window_widths", "GroupTable", "aggregate_by_window_symbols",
           "unfor_lookup_widths", "full_width_column", "lookup_symbols",
           "unfor_aggregate_by_lookup_widths", "aggregate_by_lookup_symbols",
           "undelta_compare_range_widths", "delta_compare_range_symbols",
           "undelta_aggregate_widths", "delta_aggregate_symbols",
           "undelta_select_widths", "delta_select_symbols",
           "select_symbols", "LIB_PATH"]
