"""ctypes loader for libfastlanes_amd.so (the C ABI of include/fastlanes_amd.h).

There is no fallback: if the HIP library is missing or fails to load, importing
the codec raises.  Nothing here (or anywhere in this package) touches oracle/.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FL_LIB=<path> selects another build of the same library -- the A/B tools use it to load libfastlanes_amd_full.so
# (make -C fastlanes_amd/csrc FULL=1: every cell-column instance, whatever the dispatch table says).  Never a fallback.
LIB_PATH = os.environ.get("FL_LIB") or os.path.join(_HERE, "libfastlanes_amd.so")

TYPES = ("u8", "u16", "u32", "u64")
CTYPE = {"u8": ctypes.c_uint8, "u16": ctypes.c_uint16, "u32": ctypes.c_uint32, "u64": ctypes.c_uint64}
BITS = {"u8": 8, "u16": 16, "u32": 32, "u64": 64}

_P = ctypes.c_void_p
_U = ctypes.c_uint
_Z = ctypes.c_size_t
_Q = ctypes.c_uint64
_I = ctypes.c_int
_U32 = ctypes.c_uint32
_S = ctypes.c_char_p
_T = "T"                                # the element type of a per-type row: CTYPE[ty]
_U8 = ctypes.c_uint8


def _ptr(*types):
    return [ctypes.POINTER(t) for t in types]


# THE table of the C ABI: (header macro group, symbol, restype, argtypes), in header order.  A symbol with "{ty}" (or "{vty}", "{dty}") is declared once per
# element type by its group's FL_DECLARE_* macro (_T in its argtypes is that type's scalar); the groups "API" (include/fastlanes_amd.h)
# and "INTERNAL" (include/fastlanes_amd_internal.h: test / measurement hooks, not part of the stable ABI) are plain prototypes.
# argtypes None: left unset.  Every symbol list below, and load(), is derived from it.
_SIGNATURES = (
    ("API", "fl_version", _S, None),
    ("API", "fl_status_string", _S, [_I]),
    ("API", "fl_last_hip_error", _I, None),
    ("API", "fl_packed_len", _Z, [_U, _U]),
    ("API", "fl_mixed_plan_create", _I, [_U, _P, _Z, ctypes.POINTER(_P)]),
    ("API", "fl_mixed_plan_destroy", None, [_P]),
    ("API", "fl_mixed_plan_n_blocks", _Z, [_P]),
    ("API", "fl_mixed_plan_packed_bytes", _Q, [_P]),
    ("API", "fl_mixed_plan_offsets", _P, [_P]),
    ("API", "fl_mixed_plan_widths", _P, [_P]),
    ("API", "fl_widths_to_offsets", _I, [_U, _P, _Z, _P, _P, _P, _P]),
    ("API", "fl_fill_random", _I, [_P, _Z, _Q, _P]),
    ("API", "fl_host_release", None, []),
    ("API", "fl_column_pair_alloc", _I, [_Z, _Z, _Z, _I, _P] + _ptr(_P, _P, _P, _P, _I, _U32)),
    ("API", "fl_column_pair_free", _I, [_P]),
    ("INTERNAL", "fl_internal_set_kernel_policy", None, [_I]),
    ("INTERNAL", "fl_internal_get_kernel_policy", _I, []),
    ("INTERNAL", "fl_internal_probe_memory_classes", _I, [_P, _Z, ctypes.POINTER(_I), _P]),
    ("INTERNAL", "fl_internal_bare_stream", _I, [_P, _Z, _P, _Z, _P, _Z, _Z, _I, _I, _I, _P]),
    ("INTERNAL", "fl_internal_bare_stream_shape", _I, [_I, _U, _U] + _ptr(_Z, _Z, _Z, _I, _I, _I, _U)),
    ("INTERNAL", "fl_internal_zero_copy_fallbacks", _Q, []),
    ("INTERNAL", "fl_internal_column_pair_classes", _S, [_P]),
    ("INTERNAL", "fl_internal_selftune_check", _I, [_I, _U, _U, _P, _P, _P, _Z, _P] + _ptr(ctypes.c_float, ctypes.c_float, _I)),
    ("INTERNAL", "fl_internal_choose_chunks", _Z, [ctypes.POINTER(_I), _Z, _Z, _Z, _I, ctypes.POINTER(_I)]),
    ("INTERNAL", "fl_internal_choose_layout", _I, [ctypes.POINTER(ctypes.c_double)]),
    ("INTERNAL", "fl_internal_pair_chunk_cache", _Z, [_Z]),
    # FL_DECLARE_TYPE: the device tier ...
    ("TYPE", "fl_{ty}_pack", _I, [_U, _P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_unpack", _I, [_U, _P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_unpack_single", _I, [_U, _P, _Z, _P, _Z, _P, _P, _P]),
    ("TYPE", "fl_{ty}_for_pack", _I, [_U, _P, _P, _Z, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_unfor_pack", _I, [_U, _P, _P, _Z, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_delta", _I, [_P, _P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_undelta", _I, [_P, _P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_undelta_pack", _I, [_U, _P, _P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_transpose", _I, [_P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_untranspose", _I, [_P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_undelta_pack_untranspose", _I, [_U, _P, _P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_transpose_delta_pack", _I, [_U, _P, _P, _P, _Z, _P]),
    ("TYPE", "fl_{ty}_unpack_block_sums", _I, [_U, _P, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_block_min_max", _I, [_P, _Z, _P, _P, _P]),
    ("TYPE", "fl_{ty}_unpack_compare", _I, [_U, _P, _I, _T, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_unpack_mixed", _I, [_P, _P, _P, _P]),
    ("TYPE", "fl_{ty}_pack_mixed", _I, [_P, _P, _P, _P]),
    ("TYPE", "fl_{ty}_unpack_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_pack_widths", _I, [_P, _P, _P, _P, _Z, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_unpack_single_widths", _I, [_P, _P, _P, _Z, _Z, _P, _Z, _P, _P, _P]),
    ("TYPE", "fl_{ty}_unfor_pack_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_for_pack_widths", _I, [_P, _P, _P, _P, _Z, _P, _Z, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_undelta_pack_widths", _I, [_P, _P, _P, _Z, _P, _P, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_undelta_pack_untranspose_widths", _I, [_P, _P, _P, _Z, _P, _P, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_transpose_delta_pack_widths", _I, [_P, _P, _P, _P, _P, _Z, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_for_widths", _I, [_P, _P, _Z, _P, _P]),
    ("TYPE", "fl_{ty}_unpack_batch", _I, [_P, _P, _P, _P, _Z, _U32, _P, _P]),
    ("TYPE", "fl_{ty}_pack_batch", _I, [_P, _P, _P, _P, _Z, _U32, _P, _P]),
    ("TYPE", "fl_{ty}_unfor_pack_batch", _I, [_P, _P, _P, _P, _P, _Z, _U32, _P, _P]),
    ("TYPE", "fl_{ty}_for_pack_batch", _I, [_P, _P, _P, _P, _P, _Z, _U32, _P, _P]),
    ("TYPE", "fl_{ty}_undelta_pack_batch", _I, [_P, _P, _P, _P, _P, _Z, _U32, _I, _P, _P]),
    ("TYPE", "fl_{ty}_transpose_delta_pack_batch", _I, [_P, _P, _P, _P, _P, _Z, _U32, _P, _P]),
    # ... and the host tier
    ("TYPE", "fl_{ty}_pack_host", _I, [_U, _P, _P, _Z]),
    ("TYPE", "fl_{ty}_unpack_host", _I, [_U, _P, _P, _Z]),
    ("TYPE", "fl_{ty}_unpack_single_host", _I, [_U, _P, _Z, _Q, _P]),
    ("TYPE", "fl_{ty}_for_pack_host", _I, [_U, _P, _T, _P, _Z]),
    ("TYPE", "fl_{ty}_unfor_pack_host", _I, [_U, _P, _T, _P, _Z]),
    ("TYPE", "fl_{ty}_delta_host", _I, [_P, _P, _P, _Z]),
    ("TYPE", "fl_{ty}_undelta_host", _I, [_P, _P, _P, _Z]),
    ("TYPE", "fl_{ty}_undelta_pack_host", _I, [_U, _P, _P, _P, _Z]),
    ("TYPE", "fl_{ty}_transpose_host", _I, [_P, _P, _Z]),
    ("TYPE", "fl_{ty}_untranspose_host", _I, [_P, _P, _Z]),
    # FL_DECLARE_FOR_COMPARE (device tier): selection masks from FoR-packed columns
    ("FOR_COMPARE", "fl_{ty}_unfor_compare", _I, [_U, _P, _P, _Z, _I, _T, _Z, _P, _P]),
    ("FOR_COMPARE", "fl_{ty}_unfor_compare_widths", _I, [_P, _P, _P, _Z, _P, _Z, _I, _T, _Z, _P, _P, _P]),
    # FL_DECLARE_FOR_COMPARE_RANGE (device tier): interval predicates chained through a mask
    ("FOR_COMPARE_RANGE", "fl_{ty}_unfor_compare_range", _I, [_U, _P, _P, _Z, _T, _T, _I, _P, _Z, _P, _P]),
    ("FOR_COMPARE_RANGE", "fl_{ty}_unfor_compare_range_widths", _I, [_P, _P, _P, _Z, _P, _Z, _T, _T, _I, _P, _Z, _P, _P, _P]),
    # FL_DECLARE_MASK_OFFSETS / FL_DECLARE_SELECT (device tier): only the rows a selection mask keeps, from FoR-packed columns
    ("MASK_OFFSETS", "fl_mask_offsets", _I, [_P, _Z, _P, _P, _P]),
    ("SELECT", "fl_{ty}_unfor_select", _I, [_U, _P, _P, _Z, _P, _P, _P, _Z, _Z, _P, _P]),
    ("SELECT", "fl_{ty}_unfor_select_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _P, _P, _Z, _Z, _P, _P]),
    # FL_DECLARE_AGGREGATE / FL_DECLARE_AGGREGATE_REDUCE (device tier): count / sum / min / max per block of the rows a mask keeps
    ("AGGREGATE", "fl_{ty}_unfor_aggregate", _I, [_U, _P, _P, _Z, _P, _Z, _P, _P, _P]),
    ("AGGREGATE", "fl_{ty}_unfor_aggregate_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _Z, _P, _P, _P]),
    ("AGGREGATE_REDUCE", "fl_aggregate_reduce", _I, [_P, _Z, _P, _P]),
    # FL_DECLARE_AGGREGATE_BY (device tier): count / sum / min / max per u8 key of the rows a mask keeps, 256 slots
    # ({vty}: the element type of the VALUE column -- the key column is always u8.  The recorded refusal matrix of
    # tests/test_cabi_refusals_cpu.py covers the "{ty}" rows in its PER_TYPE and every "{vty}" row below in its PER_VALUE_TYPE.)
    ("AGGREGATE_BY", "fl_{vty}_unfor_aggregate_by", _I, [_U, _P, _P, _Z, _U, _P, _P, _Z, _P, _Z, _P, _P, _P]),
    ("AGGREGATE_BY", "fl_{vty}_unfor_aggregate_by_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _P, _P, _Z, _P, _Z, _P, _Z, _P, _P, _P]),
    # FL_DECLARE_FOR_COMPARE_COLUMNS (device tier): a <op> b between two FoR-packed columns of one element type, chained through a mask
    # ({vty} as above)
    ("FOR_COMPARE_COLUMNS", "fl_{vty}_unfor_compare_columns", _I, [_U, _P, _P, _Z, _U, _P, _P, _Z, _I, _I, _I, _P, _Z, _P, _P]),
    ("FOR_COMPARE_COLUMNS", "fl_{vty}_unfor_compare_columns_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _P, _P, _Z, _P, _Z, _I, _I, _I, _P, _Z, _P, _P, _P]),
    # FL_DECLARE_AGGREGATE_COLUMNS (device tier): count / sum / min / max per block of a * b, a + b or a - b between two FoR-packed columns
    # of one element type under a mask ({vty} as above)
    ("AGGREGATE_COLUMNS", "fl_{vty}_unfor_aggregate_columns", _I, [_I, _U, _P, _P, _Z, _U, _P, _P, _Z, _P, _Z, _P, _P, _P]),
    ("AGGREGATE_COLUMNS", "fl_{vty}_unfor_aggregate_columns_widths", _I, [_I, _P, _P, _P, _Z, _P, _Z, _P, _P, _P, _Z, _P, _Z, _P, _Z, _P, _P, _P]),
    # FL_DECLARE_FOR_COMPARE_IN (device tier): set membership (a window of the value domain plus a bitmap) chained through a mask
    # ({vty} as above)
    ("FOR_COMPARE_IN", "fl_{vty}_unfor_compare_in", _I, [_U, _P, _P, _Z, _T, _Q, _P, _I, _I, _P, _Z, _P, _P]),
    ("FOR_COMPARE_IN", "fl_{vty}_unfor_compare_in_widths", _I, [_P, _P, _P, _Z, _P, _Z, _T, _Q, _P, _I, _I, _P, _Z, _P, _P, _P]),
    # FL_DECLARE_AGGREGATE_BY_COLUMNS (device tier): count / sum / min / max per u8 key of a * b, a + b or a - b between two FoR-packed
    # columns of one element type under a mask ({vty} as above)
    ("AGGREGATE_BY_COLUMNS", "fl_{vty}_unfor_aggregate_by_columns", _I, [_I, _U, _P, _P, _Z, _U, _P, _P, _Z, _U, _P, _P, _Z, _P, _Z, _P, _P, _P]),
    ("AGGREGATE_BY_COLUMNS", "fl_{vty}_unfor_aggregate_by_columns_widths", _I,
     [_I, _P, _P, _P, _Z, _P, _Z, _P, _P, _P, _Z, _P, _Z, _P, _P, _P, _Z, _P, _Z, _P, _Z, _P, _P, _P]),
    # FL_DECLARE_SET_BUILD (device tier): the member set of the values a mask keeps, ORed into a window's bitmap -- the build side of
    # unfor_compare_in ({vty} as above)
    ("SET_BUILD", "fl_{vty}_unfor_set_build", _I, [_U, _P, _P, _Z, _P, _Z, _T, _Q, _P, _P, _P]),
    ("SET_BUILD", "fl_{vty}_unfor_set_build_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _Z, _T, _Q, _P, _P, _P, _P]),
    # FL_DECLARE_AGGREGATE_BY_WINDOW (device tier): COUNT / SUM / MIN / MAX per key of a dense window, value and key column of one type,
    # accumulated into the caller's four arrays ({vty} as above)
    ("AGGREGATE_BY_WINDOW", "fl_{vty}_unfor_aggregate_by_window", _I, [_U, _P, _P, _Z, _U, _P, _P, _Z, _P, _Z, _T, _Q, _P, _P, _P, _P, _P, _P]),
    ("AGGREGATE_BY_WINDOW", "fl_{vty}_unfor_aggregate_by_window_widths", _I,
     [_P, _P, _P, _Z, _P, _Z, _P, _P, _P, _Z, _P, _Z, _P, _Z, _T, _Q, _P, _P, _P, _P, _P, _P, _P]),
    # FL_DECLARE_LOOKUP (device tier): table[(key - key_lo) mod 2^T] of the rows a mask keeps, the payload of the key's own type, written
    # in full-width packed order -- the probe side of a payload join ({vty} as above)
    ("LOOKUP", "fl_{vty}_unfor_lookup", _I, [_U, _P, _P, _Z, _P, _Z, _T, _Q, _P, _P, _T, _P, _P, _P, _P]),
    ("LOOKUP", "fl_{vty}_unfor_lookup_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _Z, _T, _Q, _P, _P, _T, _P, _P, _P, _P, _P]),
    # FL_DECLARE_LOOKUP_U8 (device tier): the same with a uint8_t payload (for u8 keys the pair above under a second name: every
    # element type has one surface)
    ("LOOKUP_U8", "fl_{vty}_unfor_lookup_u8", _I, [_U, _P, _P, _Z, _P, _Z, _T, _Q, _P, _P, _U8, _P, _P, _P, _P]),
    ("LOOKUP_U8", "fl_{vty}_unfor_lookup_u8_widths", _I, [_P, _P, _P, _Z, _P, _Z, _P, _Z, _T, _Q, _P, _P, _U8, _P, _P, _P, _P, _P]),
    # FL_DECLARE_AGGREGATE_BY_LOOKUP (device tier): unfor_lookup_u8 and unfor_aggregate_by in one pass -- COUNT / SUM / MIN / MAX per u8
    # attribute fetched through a key column of the value column's own type, no per-row output ({vty} as above)
    ("AGGREGATE_BY_LOOKUP", "fl_{vty}_unfor_aggregate_by_lookup", _I, [_U, _P, _P, _Z, _U, _P, _P, _Z, _P, _Z, _T, _Q, _P, _P, _P, _P, _P, _P]),
    ("AGGREGATE_BY_LOOKUP", "fl_{vty}_unfor_aggregate_by_lookup_widths", _I,
     [_P, _P, _P, _Z, _P, _Z, _P, _P, _P, _Z, _P, _Z, _P, _Z, _T, _Q, _P, _P, _P, _P, _P, _P]),
    # FL_DECLARE_DELTA_COMPARE_RANGE (device tier): interval predicates over DELTA-packed columns, chained through a mask ({vty} as
    # above)
    ("DELTA_COMPARE_RANGE", "fl_{vty}_undelta_compare_range", _I, [_U, _P, _P, _T, _T, _I, _P, _Z, _P, _P]),
    ("DELTA_COMPARE_RANGE", "fl_{vty}_undelta_compare_range_widths", _I, [_P, _P, _P, _Z, _P, _T, _T, _I, _P, _Z, _P, _P, _P]),
    # FL_DECLARE_DELTA_AGGREGATE (device tier): count / sum / min / max per block of the rows a mask keeps of a DELTA-packed column
    # ({dty}: the element type of the Delta column; these rows' refusals are recorded by tests/test_delta_aggregate_cpu.py)
    ("DELTA_AGGREGATE", "fl_{dty}_undelta_aggregate", _I, [_U, _P, _P, _P, _Z, _P, _P, _P]),
    ("DELTA_AGGREGATE", "fl_{dty}_undelta_aggregate_widths", _I, [_P, _P, _P, _Z, _P, _P, _Z, _P, _P, _P]),
    # FL_DECLARE_DELTA_SELECT (device tier): the rows a mask keeps of a DELTA-packed column, compacted in original row order
    # (these rows' refusals are recorded by tests/test_delta_select_cpu.py)
    ("DELTA_SELECT", "fl_{dty}_undelta_select", _I, [_U, _P, _P, _P, _P, _P, _Z, _Z, _P, _P]),
    ("DELTA_SELECT", "fl_{dty}_undelta_select_widths", _I, [_P, _P, _P, _Z, _P, _P, _P, _P, _Z, _Z, _P, _P]),
)

# include/fastlanes_amd.h: fl_mask_combine
MASK_COMBINE = {"new": 0, "and": 1, "or": 2}


def _rows(*groups):
    """(symbol, restype, argtypes) of the given groups (none: of all), group by group: a plain prototype once, a per-type declaration
    for every element type -- all of u8's symbols, then u16's, ... as the header's macros expand."""
    for group in groups or dict.fromkeys(g for g, *_ in _SIGNATURES):
        rows = [r for r in _SIGNATURES if r[0] == group]
        for ty in TYPES if any(t in rows[0][1] for t in ("{ty}", "{vty}", "{dty}")) else (None,):
            for _, name, restype, argtypes in rows:
                yield name.format(ty=ty, vty=ty, dty=ty), restype, argtypes and [CTYPE[ty] if a is _T else a for a in argtypes]


def _symbols(*groups):
    return [name for name, _, _ in _rows(*groups)]


INTERNAL_SYMBOLS = _symbols("INTERNAL")


def exported_symbols():
    """Every symbol include/fastlanes_amd.h and include/fastlanes_amd_internal.h declare outside the extension macros of their own:
    the plain prototypes, the internal hooks and FL_DECLARE_TYPE's per-type list (a pinned surface)."""
    return _symbols("API", "INTERNAL", "TYPE")


def for_compare_symbols():
    """The symbols FL_DECLARE_FOR_COMPARE declares, all four element types."""
    return _symbols("FOR_COMPARE")


def for_compare_range_symbols():
    """The symbols FL_DECLARE_FOR_COMPARE_RANGE declares, all four element types."""
    return _symbols("FOR_COMPARE_RANGE")


def select_symbols():
    """The symbols FL_DECLARE_MASK_OFFSETS and FL_DECLARE_SELECT declare: the mask prefix sum and, for all four element types, the
    two select entry points."""
    return _symbols("MASK_OFFSETS", "SELECT")


def aggregate_symbols():
    """The symbols FL_DECLARE_AGGREGATE and FL_DECLARE_AGGREGATE_REDUCE declare: for all four element types the two aggregate entry
    points, and the reduction of their per-block slots."""
    return _symbols("AGGREGATE", "AGGREGATE_REDUCE")


def aggregate_by_symbols():
    """The symbols FL_DECLARE_AGGREGATE_BY declares: for all four value types the two grouped-aggregate entry points."""
    return _symbols("AGGREGATE_BY")


def for_compare_columns_symbols():
    """The symbols FL_DECLARE_FOR_COMPARE_COLUMNS declares: for all four element types the two column-against-column entry points."""
    return _symbols("FOR_COMPARE_COLUMNS")


def aggregate_columns_symbols():
    """The symbols FL_DECLARE_AGGREGATE_COLUMNS declares: for all four element types the two aggregate-of-two-columns entry points."""
    return _symbols("AGGREGATE_COLUMNS")


def for_compare_in_symbols():
    """The symbols FL_DECLARE_FOR_COMPARE_IN declares: for all four element types the two set-membership entry points."""
    return _symbols("FOR_COMPARE_IN")


def aggregate_by_columns_symbols():
    """The symbols FL_DECLARE_AGGREGATE_BY_COLUMNS declares: for all four value types the two grouped aggregate-of-two-columns entry
    points."""
    return _symbols("AGGREGATE_BY_COLUMNS")


def set_build_symbols():
    """The symbols FL_DECLARE_SET_BUILD declares: for all four element types the two member-set build entry points."""
    return _symbols("SET_BUILD")


def aggregate_by_window_symbols():
    """The symbols FL_DECLARE_AGGREGATE_BY_WINDOW declares: for all four element types the two windowed group-by entry points."""
    return _symbols("AGGREGATE_BY_WINDOW")


def lookup_symbols():
    """The symbols FL_DECLARE_LOOKUP and FL_DECLARE_LOOKUP_U8 declare: for all four key types the two lookups with a payload of the
    key's own type and the two with a uint8_t payload (for u8 keys the same two functions under a second name)."""
    return _symbols("LOOKUP", "LOOKUP_U8")


def aggregate_by_lookup_symbols():
    """The symbols FL_DECLARE_AGGREGATE_BY_LOOKUP declares: for all four element types the fused lookup + grouped aggregate over a
    uniform-width and over a mixed-width column pair."""
    return _symbols("AGGREGATE_BY_LOOKUP")


def delta_compare_range_symbols():
    """The symbols FL_DECLARE_DELTA_COMPARE_RANGE declares: for all four element types the interval predicate over a uniform-width and
    over a mixed-width Delta-packed column."""
    return _symbols("DELTA_COMPARE_RANGE")


def delta_aggregate_symbols():
    """The symbols FL_DECLARE_DELTA_AGGREGATE declares: for all four element types the aggregate over a uniform-width and over a
    mixed-width Delta-packed column."""
    return _symbols("DELTA_AGGREGATE")


def delta_select_symbols():
    """The symbols FL_DECLARE_DELTA_SELECT declares: for all four element types the select over a uniform-width and over a mixed-width
    Delta-packed column."""
    return _symbols("DELTA_SELECT")


_LIB = None


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C fastlanes_amd/csrc). "
            "fastlanes_amd has no CPU fallback.")
    # ONE HIP runtime per process: PyTorch ships its own libamdhip64.so, libfastlanes_amd.so is linked against /opt/rocm's.  Whichever
    # is loaded first serves both (same SONAME) -- but if this library came first, torch would still load its bundled copy next to
    # it, and a kernel launched through one runtime on memory allocated through the other fails with hipErrorNoDevice (seen in
    # round 4).  The Python mirror exists to be used with torch tensors, so torch goes first whenever it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in _rows():
        fn = getattr(lib, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _LIB = lib
    return lib
