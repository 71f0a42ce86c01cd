"""CPU: the refusal matrix of the C ABI.  Every entry point that validates its arguments -- the 42 per-type ones of FL_DECLARE_TYPE, the
eight first consumers of a FoR-packed column, the 22 later ones (the "{vty}" rows of _lib._SIGNATURES: unfor_aggregate_by ...
undelta_compare_range, both forms), fl_widths_to_offsets, fl_mask_offsets, fl_aggregate_reduce, fl_fill_random and
fl_mixed_plan_create -- is called for all four element types and under kernel policy 0, 1 and 2 (the uniform-width entry points take
another path, with another order of checks, under each) with calls that are refused before anything is launched, and must answer
what it answered when its rows were recorded: at 1fd1295 for PER_TYPE's and PLAIN's, at 7eb97a5 for PER_VALUE_TYPE's.

The literal table below was recorded from those commits' libraries on a machine without a GPU, where a call that gets past validation
answers FL_ERR_HIP; such calls were pruned, so every call kept here ends in FL_ERR_WIDTH, FL_ERR_INDEX, FL_ERR_NULL or FL_ERR_ALIGN
(or in FL_OK, for an empty call) before it reaches the device, and none launches a kernel on the made-up pointers.  A case is a
well-formed call -- every pointer a distinct 16-byte-aligned address inside one zeroed buffer, width 3, one block, packed_bytes to
match, a valid op / combine / negate / expr, 64 set bits, 4 groups or slots -- with one to three faults, joined by "+":
    null:X     pointer X is NULL                      off8:X    pointer X moved by 8 bytes
    width      width = T + 1                          w0        width = 0: only beside a fault, where it moves the checks
    widthb / widthk, w0b / w0k    the same for the second column `b` and the key column `keys` (a u8 key column is over its width at 9)
    op=V / cb=V / neg=V / ex=V    the compare op / the mask combine / negate / expr set to V (cb=0, FL_MASK_NEW, drops mask_in: only
               beside a fault)
    sb=V / ng=V / ns=V    set_bits / n_groups / n_slots set to V: "over" the least count that is refused (over_count), 0 the empty set
               or window, which drops the pointers read under it -- a NULL or unaligned one is then accepted, so only beside a fault
    mb         max_blocks = 2^30 + 1                  empty     the count that makes the call empty is 0 and every pointer NULL
    zero:X     X is NULL and its byte count (packed_bytes, out_len) is 0: allowed, so kept only beside a fault that is refused
    index      unpack_single_host: index = 1024       plan=other    a plan of another element type
    n=0        no blocks, the pointers as they are: the three aggregate_by* judge `result` even then (their init kernel always runs)
    type=12 / n=0 / n=60 / badwidths    fl_widths_to_offsets / fl_mixed_plan_create / fl_fill_random: their own arguments
Adding an entry point means adding its row here, from a library that is known to be right."""
import ctypes

import numpy as np
import pytest

from cpu_support import TYPE_BITS, lib  # noqa: F401 (lib: fixture)

# the arguments of every entry point, in order: "*name" a pointer, w the width, n the count that makes the call empty, one a size_t 1
# (a stride, or a block count that does not), pb packed_bytes, ol out_len, op / cb, k a scalar of the element type, mb max_blocks,
# i0 an int 0, q the lookup index, s the stream, plan a 0-block fl_mixed_plan of the element type, tb type_bits, n64 / seed fl_fill_random's
PER_TYPE = {
    "pack": "w *in *out n s",
    "unpack": "w *in *out n s",
    "unpack_single": "w *pk one *idx n *out *ef s",
    "for_pack": "w *in *refs one *out n s",
    "unfor_pack": "w *in *refs one *out n s",
    "delta": "*in *bases *out n s",
    "undelta": "*in *bases *out n s",
    "undelta_pack": "w *in *bases *out n s",
    "transpose": "*in *out n s",
    "untranspose": "*in *out n s",
    "undelta_pack_untranspose": "w *in *bases *out n s",
    "transpose_delta_pack": "w *in *bases *out n s",
    "unpack_block_sums": "w *in n *sums s",
    "block_min_max": "*in n *mins *maxs s",
    "unpack_compare": "w *in op k n *mask s",
    "unpack_mixed": "plan *pk *out s",
    "pack_mixed": "plan *in *pk s",
    "unpack_widths": "*widths *offsets *pk pb *out n *ef s",
    "pack_widths": "*widths *offsets *in *pk pb n *ef s",
    "unpack_single_widths": "*widths *offsets *pk pb one *idx n *out *ef s",
    "unfor_pack_widths": "*widths *offsets *pk pb *refs one *out n *ef s",
    "for_pack_widths": "*widths *offsets *in *refs one *pk pb n *ef s",
    "undelta_pack_widths": "*widths *offsets *pk pb *bases *out n *ef s",
    "undelta_pack_untranspose_widths": "*widths *offsets *pk pb *bases *out n *ef s",
    "transpose_delta_pack_widths": "*widths *offsets *in *bases *pk pb n *ef s",
    "for_widths": "*mins *maxs n *widths s",
    "unpack_batch": "*pk *out *widths *nb n mb *ef s",
    "pack_batch": "*in *pk *widths *nb n mb *ef s",
    "unfor_pack_batch": "*pk *out *widths *refs *nb n mb *ef s",
    "for_pack_batch": "*in *pk *widths *refs *nb n mb *ef s",
    "undelta_pack_batch": "*pk *bases *out *widths *nb n mb i0 *ef s",
    "transpose_delta_pack_batch": "*in *bases *pk *widths *nb n mb *ef s",
    "pack_host": "w *in *out n",
    "unpack_host": "w *in *out n",
    "unpack_single_host": "w *pk one q *value",
    "for_pack_host": "w *in k *out n",
    "unfor_pack_host": "w *in k *out n",
    "delta_host": "*in *bases *out n",
    "undelta_host": "*in *bases *out n",
    "undelta_pack_host": "w *in *bases *out n",
    "transpose_host": "*in *out n",
    "untranspose_host": "*in *out n",
    "unfor_compare": "w *in *refs one op k n *mask s",
    "unfor_compare_widths": "*widths *offsets *pk pb *refs one op k n *mask *ef s",
    "unfor_compare_range": "w *in *refs one k k cb *mask_in n *mask s",
    "unfor_compare_range_widths": "*widths *offsets *pk pb *refs one k k cb *mask_in n *mask *ef s",
    "unfor_select": "w *in *refs one *mask *out_offsets *out ol n *ef s",
    "unfor_select_widths": "*widths *offsets *pk pb *refs one *mask *out_offsets *out ol n *ef s",
    "unfor_aggregate": "w *in *refs one *mask n *aggs *ef s",
    "unfor_aggregate_widths": "*widths *offsets *pk pb *refs one *mask n *aggs *ef s",
}
# the later consumers (the "{vty}" rows of _lib._SIGNATURES), which take up to three columns: wb / pbb the width / packed_bytes of the
# second column `b`, kw / pbk those of the key column `keys` (kw8: a u8 key column), ex / neg / sg expr, negate, signed, sb / ng / ns
# the uint64 counts set_bits, n_groups, n_slots (ns1: of a one-byte payload), pl the payload scalar
PER_VALUE_TYPE = {
    "unfor_aggregate_by": "w *in *refs one kw8 *keys *k_refs one *mask n *result *ef s",
    "unfor_aggregate_by_widths": "*widths *offsets *pk pb *refs one *k_widths *k_offsets *keys pbk *k_refs one *mask n *result *ef s",
    "unfor_compare_columns": "w *in *refs one wb *b *b_refs one op sg cb *mask_in n *mask s",
    "unfor_compare_columns_widths": "*widths *offsets *pk pb *refs one *b_widths *b_offsets *b pbb *b_refs one op sg cb *mask_in n *mask *ef s",
    "unfor_aggregate_columns": "ex w *in *refs one wb *b *b_refs one *mask n *aggs *ef s",
    "unfor_aggregate_columns_widths": "ex *widths *offsets *pk pb *refs one *b_widths *b_offsets *b pbb *b_refs one *mask n *aggs *ef s",
    "unfor_compare_in": "w *in *refs one k sb *set_words neg cb *mask_in n *mask s",
    "unfor_compare_in_widths": "*widths *offsets *pk pb *refs one k sb *set_words neg cb *mask_in n *mask *ef s",
    "unfor_aggregate_by_columns": "ex w *in *refs one wb *b *b_refs one kw8 *keys *k_refs one *mask n *result *ef s",
    "unfor_aggregate_by_columns_widths": "ex *widths *offsets *pk pb *refs one *b_widths *b_offsets *b pbb *b_refs one *k_widths *k_offsets *keys pbk "
                                         "*k_refs one *mask n *result *ef s",
    "unfor_set_build": "w *in *refs one *mask n k sb *set_words *stats s",
    "unfor_set_build_widths": "*widths *offsets *pk pb *refs one *mask n k sb *set_words *stats *ef s",
    "unfor_aggregate_by_window": "w *in *refs one kw *keys *k_refs one *mask n k ng *counts *sums *mins *maxs *stats s",
    "unfor_aggregate_by_window_widths": "*widths *offsets *pk pb *refs one *k_widths *k_offsets *keys pbk *k_refs one *mask n k ng *counts *sums *mins "
                                        "*maxs *stats *ef s",
    "unfor_lookup": "w *in *refs one *mask n k ns *table *present pl *out *hit_mask *stats s",
    "unfor_lookup_widths": "*widths *offsets *pk pb *refs one *mask n k ns *table *present pl *out *hit_mask *stats *ef s",
    "unfor_lookup_u8": "w *in *refs one *mask n k ns1 *table *present pl *out *hit_mask *stats s",
    "unfor_lookup_u8_widths": "*widths *offsets *pk pb *refs one *mask n k ns1 *table *present pl *out *hit_mask *stats *ef s",
    "unfor_aggregate_by_lookup": "w *in *refs one kw *keys *k_refs one *mask n k ns1 *table *present *result *stats *ef s",
    "unfor_aggregate_by_lookup_widths": "*widths *offsets *pk pb *refs one *k_widths *k_offsets *keys pbk *k_refs one *mask n k ns1 *table *present "
                                        "*result *stats *ef s",
    "undelta_compare_range": "w *in *bases k k cb *mask_in n *mask s",
    "undelta_compare_range_widths": "*widths *offsets *pk pb *bases k k cb *mask_in n *mask *ef s",
}
SPECS = {**PER_TYPE, **PER_VALUE_TYPE}
PLAIN = {
    "fl_widths_to_offsets": "tb *widths n *offsets *total *ef s",
    "fl_mask_offsets": "*mask n *out_offsets *total s",
    "fl_aggregate_reduce": "*aggs n *result s",
    "fl_fill_random": "*dst n64 seed s",
    "fl_mixed_plan_create": "tb *widths n *plan",
}
POLICIES = (0, 1, 2)
TYS = tuple(TYPE_BITS)
SLOT = 4096                                                 # bytes between two of a call's pointers


WIDTH_FAULTS = {"w": ("width", "w0"), "wb": ("widthb", "w0b"), "kw": ("widthk", "w0k"), "kw8": ("widthk", "w0k")}
BYTES_OF = {"pb": ("pk", "in"), "pbb": ("b",), "pbk": ("keys",)}      # packed_bytes -> the pointer it goes to 0 with under "zero:"
COUNTS = {"sb": 64, "ng": 4, "ns": 4, "ns1": 4}                        # set_bits, n_groups, n_slots: the well-formed value


def over_count(tok, ty):
    """the least count the entry point refuses: one past 2^min(T, 32) members, groups or slots -- or, for a lookup table (ns: a payload
    of the element type, ns1: of one byte), the least number of slots whose table reaches 2^31 bytes, where that is fewer"""
    members = (1 << min(TYPE_BITS[ty], 32)) + 1
    payload = {"ns": TYPE_BITS[ty] // 8, "ns1": 1}.get(tok)
    return min(members, (1 << 31) // payload) if payload else members


def arguments(spec, case, ty, base, plans):
    """the argument list of one call: the well-formed one of `spec` with the faults of `case`"""
    faults = {}                                             # kind -> what its faults name, or the values they set
    for f in case.split("+"):
        kind, _, what = f.replace("=", ":").partition(":")
        faults.setdefault(kind, []).append(what)
    names = lambda kind: faults.get(kind, ())               # noqa: E731
    empty = "empty" in faults
    args, slot = [], 0
    for tok in spec.split():
        if tok[0] == "*":
            slot += 1
            name, p = tok[1:], base + slot * SLOT
            if empty or name in names("null") or name in names("zero"):
                p = None
            elif name in names("off8"):
                p += 8
            elif name == "widths" and "badwidths" in faults:
                p = base                                    # slot 0 holds 0xff: a width no type has
            args.append(p)
        elif tok in WIDTH_FAULTS:                           # kw8: the u8 key column, over its width at 9 whatever T is
            over, zero = WIDTH_FAULTS[tok]
            args.append((9 if tok == "kw8" else TYPE_BITS[ty] + 1) if over in faults else 0 if zero in faults else 3)
        elif tok in ("n", "n64"):
            args.append(0 if empty else int(faults["n"][0]) if "n" in faults else 64 if tok == "n64" else 1)
        elif tok in BYTES_OF:
            args.append(0 if set(names("zero")) & set(BYTES_OF[tok]) else 384)
        elif tok == "ol":
            args.append(0 if "out" in names("zero") else 1024)
        elif tok in ("op", "cb", "neg", "ex"):
            args.append(int(faults[tok][0]) if tok in faults else 1)
        elif tok in COUNTS:
            v = faults.get(tok[:2], [None])[0]
            args.append(COUNTS[tok] if v is None else over_count(tok, ty) if v == "over" else int(v))
        elif tok == "mb":
            args.append((1 << 30) + 1 if "mb" in faults else 1)
        elif tok == "q":
            args.append(1024 if "index" in faults else 0)
        elif tok == "tb":
            args.append(int(faults["type"][0]) if "type" in faults else TYPE_BITS[ty])
        elif tok == "plan":
            args.append(None if "plan" in names("null") else plans[TYS[(TYS.index(ty) + 1) % 4] if "plan" in faults else ty])
        else:
            args.append({"one": 1, "k": 0, "pl": 0, "i0": 0, "sg": 0, "seed": 1, "s": None}[tok])
    return args


class Calls:
    """one zeroed buffer for every call's pointers, and a 0-block plan per element type (fl_mixed_plan_create allocates nothing for it)"""

    def __init__(self, lib):
        self.lib = lib
        self.buf = np.zeros(16 * SLOT + 64, dtype=np.uint8)
        self.base = (self.buf.ctypes.data + 63) & ~63
        ctypes.memset(self.base, 0xff, 16)
        self.plans = {}
        for ty in TYS:
            h = ctypes.c_void_p()
            assert lib.fl_mixed_plan_create(TYPE_BITS[ty], None, 0, ctypes.byref(h)) == 0
            self.plans[ty] = h.value

    def __call__(self, entry, case, ty):
        plain = entry in PLAIN
        args = arguments(PLAIN[entry] if plain else SPECS[entry], case, ty, self.base, self.plans)
        if entry == "fl_mixed_plan_create":                 # a 0-block plan is host memory only; it is freed again here
            slot = args[3]
            args[3] = slot and ctypes.cast(slot, ctypes.POINTER(ctypes.c_void_p))
        rc = getattr(self.lib, entry if plain else f"fl_{ty}_{entry}")(*args)
        if entry == "fl_mixed_plan_create" and slot and args[3][0]:
            self.lib.fl_mixed_plan_destroy(args[3][0])
            args[3][0] = None
        return rc

    def close(self):
        for h in self.plans.values():
            self.lib.fl_mixed_plan_destroy(h)


def rows(table):
    """(entry, case, status) of every case of the table; the status holds for all four element types and the three policies"""
    return [(entry, case, status) for entry, by_status in table.items() for status, cases in by_status.items() for case in cases.split()]


TABLE = {
    "pack": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:out w0+null:in null:in+off8:out null:out+off8:in",
        4: "off8:in off8:out",
    },
    "unpack": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:out w0+null:out null:in+off8:out null:out+off8:in",
        4: "off8:in off8:out w0+off8:in",
    },
    "unpack_single": {
        0: "empty w0+empty",
        1: "width width+null:pk width+null:idx width+null:out width+null:ef width+off8:pk width+empty width+w0",
        3: "null:pk null:idx null:out w0+null:idx w0+null:out null:pk+off8:ef null:pk+off8:idx null:idx+off8:out null:idx+off8:pk "
           "null:out+off8:ef null:out+off8:idx",
    },
    "for_pack": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:refs width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:refs null:out w0+null:in w0+null:refs null:in+off8:refs null:in+off8:out null:refs+off8:in null:refs+off8:out "
           "null:out+off8:in null:out+off8:refs",
        4: "off8:in off8:out",
    },
    "unfor_pack": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:refs width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:refs null:out w0+null:refs w0+null:out null:in+off8:refs null:in+off8:out null:refs+off8:in null:refs+off8:out "
           "null:out+off8:in null:out+off8:refs",
        4: "off8:in off8:out w0+off8:in",
    },
    "delta": {
        0: "empty",
        3: "null:in null:bases null:out null:in+off8:out null:bases+off8:in null:bases+off8:out null:out+off8:in",
        4: "off8:in off8:bases off8:out null:in+off8:bases null:out+off8:bases off8:bases+null:in off8:bases+null:out",
    },
    "undelta": {
        0: "empty",
        3: "null:in null:bases null:out null:in+off8:out null:bases+off8:in null:bases+off8:out null:out+off8:in",
        4: "off8:in off8:bases off8:out null:in+off8:bases null:out+off8:bases off8:bases+null:in off8:bases+null:out",
    },
    "undelta_pack": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:bases width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:bases null:out w0+null:bases w0+null:out null:in+off8:out null:bases+off8:in null:bases+off8:out "
           "null:out+off8:in",
        4: "off8:in off8:bases off8:out w0+off8:in null:in+off8:bases null:out+off8:bases off8:bases+null:in off8:bases+null:out",
    },
    "transpose": {
        0: "empty",
        3: "null:in null:out null:in+off8:out null:out+off8:in",
        4: "off8:in off8:out",
    },
    "untranspose": {
        0: "empty",
        3: "null:in null:out null:in+off8:out null:out+off8:in",
        4: "off8:in off8:out",
    },
    "undelta_pack_untranspose": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:bases width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:bases null:out w0+null:bases w0+null:out null:in+off8:out null:bases+off8:in null:bases+off8:out "
           "null:out+off8:in",
        4: "off8:in off8:bases off8:out w0+off8:in null:in+off8:bases null:out+off8:bases off8:bases+null:in off8:bases+null:out",
    },
    "transpose_delta_pack": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:bases width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:bases null:out w0+null:in w0+null:bases null:in+off8:out null:bases+off8:in null:bases+off8:out null:out+off8:in",
        4: "off8:in off8:bases off8:out w0+off8:in null:in+off8:bases null:out+off8:bases off8:bases+null:in off8:bases+null:out",
    },
    "unpack_block_sums": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:sums width+off8:in width+empty width+w0",
        3: "null:in null:sums w0+null:sums null:in+off8:sums null:sums+off8:in",
        4: "off8:in w0+off8:in",
    },
    "block_min_max": {
        0: "empty",
        3: "null:in null:mins null:maxs null:in+off8:maxs null:in+off8:mins null:mins+off8:in null:mins+off8:maxs null:maxs+off8:in "
           "null:maxs+off8:mins",
        4: "off8:in",
    },
    "unpack_compare": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:mask width+off8:in width+empty width+w0 width+op=-1 width+op=6",
        2: "op=-1 op=6 op=-1+null:in op=-1+null:mask op=-1+off8:in op=-1+empty op=6+null:in op=6+null:mask op=6+off8:in op=6+empty "
           "w0+op=-1 w0+op=6",
        3: "null:in null:mask w0+null:mask null:in+off8:mask null:mask+off8:in",
        4: "off8:in off8:mask w0+off8:in",
    },
    "unpack_mixed": {
        0: "empty",
        1: "plan=other plan=other+null:pk plan=other+null:out plan=other+off8:pk plan=other+empty",
        3: "null:plan null:plan+off8:pk null:plan+empty",
    },
    "pack_mixed": {
        0: "empty",
        1: "plan=other plan=other+null:in plan=other+null:pk plan=other+off8:in plan=other+empty",
        3: "null:plan null:plan+off8:in null:plan+empty",
    },
    "unpack_widths": {
        0: "empty",
        3: "null:widths null:offsets null:pk null:out null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:widths "
           "null:offsets+off8:pk null:pk+off8:offsets null:pk+off8:out null:out+off8:ef null:out+off8:pk zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:out",
        4: "off8:pk off8:out null:ef+off8:out zero:pk+off8:out",
    },
    "pack_widths": {
        0: "empty",
        3: "null:widths null:offsets null:in null:pk null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:in "
           "null:offsets+off8:widths null:in+off8:offsets null:in+off8:pk null:pk+off8:in null:pk+off8:ef zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:in",
        4: "off8:in off8:pk null:ef+off8:pk zero:pk+off8:in",
    },
    "unpack_single_widths": {
        0: "empty",
        3: "null:widths null:offsets null:pk null:idx null:out null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:widths "
           "null:offsets+off8:pk null:pk+off8:offsets null:pk+off8:idx null:idx+off8:out null:idx+off8:pk null:out+off8:ef "
           "null:out+off8:idx zero:pk+null:widths zero:pk+null:offsets zero:pk+null:idx zero:pk+null:out",
    },
    "unfor_pack_widths": {
        0: "empty",
        3: "null:widths null:offsets null:pk null:refs null:out null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:widths "
           "null:offsets+off8:pk null:pk+off8:refs null:pk+off8:offsets null:refs+off8:out null:refs+off8:pk null:out+off8:refs "
           "null:out+off8:ef zero:pk+null:widths zero:pk+null:offsets zero:pk+null:refs zero:pk+null:out",
        4: "off8:pk off8:out null:ef+off8:out zero:pk+off8:out",
    },
    "for_pack_widths": {
        0: "empty",
        3: "null:widths null:offsets null:in null:refs null:pk null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:in "
           "null:offsets+off8:widths null:in+off8:refs null:in+off8:offsets null:refs+off8:in null:refs+off8:pk null:pk+off8:refs "
           "null:pk+off8:ef zero:pk+null:widths zero:pk+null:offsets zero:pk+null:in zero:pk+null:refs",
        4: "off8:in off8:pk null:ef+off8:pk zero:pk+off8:in",
    },
    "undelta_pack_widths": {
        0: "empty",
        3: "null:widths null:offsets null:pk null:bases null:out null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:widths "
           "null:offsets+off8:pk null:pk+off8:bases null:pk+off8:offsets null:bases+off8:out null:bases+off8:pk null:out+off8:bases "
           "null:out+off8:ef off8:bases+null:widths off8:bases+null:offsets off8:bases+null:pk off8:bases+null:out zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:bases zero:pk+null:out",
        4: "off8:pk off8:bases off8:out null:ef+off8:out off8:bases+null:ef zero:pk+off8:bases zero:pk+off8:out",
    },
    "undelta_pack_untranspose_widths": {
        0: "empty",
        3: "null:widths null:offsets null:pk null:bases null:out null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:widths "
           "null:offsets+off8:pk null:pk+off8:bases null:pk+off8:offsets null:bases+off8:out null:bases+off8:pk null:out+off8:bases "
           "null:out+off8:ef off8:bases+null:widths off8:bases+null:offsets off8:bases+null:pk off8:bases+null:out zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:bases zero:pk+null:out",
        4: "off8:pk off8:bases off8:out null:ef+off8:out off8:bases+null:ef zero:pk+off8:bases zero:pk+off8:out",
    },
    "transpose_delta_pack_widths": {
        0: "empty",
        3: "null:widths null:offsets null:in null:bases null:pk null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:in "
           "null:offsets+off8:widths null:in+off8:bases null:in+off8:offsets null:bases+off8:in null:bases+off8:pk null:pk+off8:bases "
           "null:pk+off8:ef off8:bases+null:widths off8:bases+null:offsets off8:bases+null:in off8:bases+null:pk zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:in zero:pk+null:bases",
        4: "off8:in off8:bases off8:pk null:ef+off8:pk off8:bases+null:ef zero:pk+off8:in zero:pk+off8:bases",
    },
    "for_widths": {
        0: "empty",
        3: "null:mins null:maxs null:widths null:mins+off8:maxs null:mins+off8:widths null:maxs+off8:mins null:maxs+off8:widths "
           "null:widths+off8:maxs null:widths+off8:mins",
    },
    "unpack_batch": {
        0: "empty mb+empty",
        2: "mb mb+null:ef mb+off8:pk",
        3: "null:pk null:out null:widths null:nb mb+null:pk mb+null:out mb+null:widths mb+null:nb null:pk+off8:ef null:pk+off8:out "
           "null:out+off8:widths null:out+off8:pk null:widths+off8:nb null:widths+off8:out null:nb+off8:ef null:nb+off8:widths",
    },
    "pack_batch": {
        0: "empty mb+empty",
        2: "mb mb+null:ef mb+off8:in",
        3: "null:in null:pk null:widths null:nb mb+null:in mb+null:pk mb+null:widths mb+null:nb null:in+off8:ef null:in+off8:pk "
           "null:pk+off8:in null:pk+off8:widths null:widths+off8:nb null:widths+off8:pk null:nb+off8:ef null:nb+off8:widths",
    },
    "unfor_pack_batch": {
        0: "empty mb+empty",
        2: "mb mb+null:ef mb+off8:pk",
        3: "null:pk null:out null:widths null:refs null:nb mb+null:pk mb+null:out mb+null:widths mb+null:refs mb+null:nb null:pk+off8:ef "
           "null:pk+off8:out null:out+off8:widths null:out+off8:pk null:widths+off8:refs null:widths+off8:out null:refs+off8:nb "
           "null:refs+off8:widths null:nb+off8:refs null:nb+off8:ef",
    },
    "for_pack_batch": {
        0: "empty mb+empty",
        2: "mb mb+null:ef mb+off8:in",
        3: "null:in null:pk null:widths null:refs null:nb mb+null:in mb+null:pk mb+null:widths mb+null:refs mb+null:nb null:in+off8:ef "
           "null:in+off8:pk null:pk+off8:in null:pk+off8:widths null:widths+off8:refs null:widths+off8:pk null:refs+off8:nb "
           "null:refs+off8:widths null:nb+off8:refs null:nb+off8:ef",
    },
    "undelta_pack_batch": {
        0: "empty mb+empty",
        2: "mb mb+null:ef mb+off8:pk",
        3: "null:pk null:bases null:out null:widths null:nb mb+null:pk mb+null:bases mb+null:out mb+null:widths mb+null:nb "
           "null:pk+off8:bases null:pk+off8:ef null:bases+off8:out null:bases+off8:pk null:out+off8:bases null:out+off8:widths "
           "null:widths+off8:nb null:widths+off8:out null:nb+off8:ef null:nb+off8:widths off8:bases+null:pk off8:bases+null:out "
           "off8:bases+null:widths off8:bases+null:nb",
    },
    "transpose_delta_pack_batch": {
        0: "empty mb+empty",
        2: "mb mb+null:ef mb+off8:in",
        3: "null:in null:bases null:pk null:widths null:nb mb+null:in mb+null:bases mb+null:pk mb+null:widths mb+null:nb "
           "null:in+off8:bases null:in+off8:ef null:bases+off8:in null:bases+off8:pk null:pk+off8:bases null:pk+off8:widths "
           "null:widths+off8:nb null:widths+off8:pk null:nb+off8:ef null:nb+off8:widths off8:bases+null:in off8:bases+null:pk "
           "off8:bases+null:widths off8:bases+null:nb",
    },
    "pack_host": {
        1: "width width+null:in width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:out w0+null:in null:in+off8:out null:out+off8:in",
    },
    "unpack_host": {
        1: "width width+null:in width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:out w0+null:out null:in+off8:out null:out+off8:in",
    },
    "unpack_single_host": {
        1: "width width+null:pk width+null:value width+off8:pk width+w0 width+index",
        2: "index index+null:pk index+off8:pk",
        3: "null:pk null:value w0+null:value index+null:value null:pk+off8:value null:value+off8:pk",
    },
    "for_pack_host": {
        1: "width width+null:in width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:out w0+null:in null:in+off8:out null:out+off8:in",
    },
    "unfor_pack_host": {
        1: "width width+null:in width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:out w0+null:out null:in+off8:out null:out+off8:in",
    },
    "delta_host": {
        3: "null:in null:bases null:out null:in+off8:bases null:in+off8:out null:bases+off8:in null:bases+off8:out null:out+off8:in "
           "null:out+off8:bases off8:bases+null:in off8:bases+null:out",
    },
    "undelta_host": {
        3: "null:in null:bases null:out null:in+off8:bases null:in+off8:out null:bases+off8:in null:bases+off8:out null:out+off8:in "
           "null:out+off8:bases off8:bases+null:in off8:bases+null:out",
    },
    "undelta_pack_host": {
        1: "width width+null:in width+null:bases width+null:out width+off8:in width+empty width+w0",
        3: "null:in null:bases null:out w0+null:bases w0+null:out null:in+off8:bases null:in+off8:out null:bases+off8:in "
           "null:bases+off8:out null:out+off8:in null:out+off8:bases off8:bases+null:in off8:bases+null:out",
    },
    "transpose_host": {
        3: "null:in null:out null:in+off8:out null:out+off8:in",
    },
    "untranspose_host": {
        3: "null:in null:out null:in+off8:out null:out+off8:in",
    },
    "unfor_compare": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:refs width+null:mask width+off8:in width+empty width+w0 width+op=-1 width+op=6",
        2: "op=-1 op=6 op=-1+null:in op=-1+null:refs op=-1+null:mask op=-1+off8:in op=-1+empty op=6+null:in op=6+null:refs op=6+null:mask "
           "op=6+off8:in op=6+empty w0+op=-1 w0+op=6",
        3: "null:in null:refs null:mask w0+null:refs w0+null:mask null:in+off8:refs null:in+off8:mask null:refs+off8:in "
           "null:refs+off8:mask null:mask+off8:in null:mask+off8:refs",
        4: "off8:in off8:mask w0+off8:in",
    },
    "unfor_compare_widths": {
        0: "empty",
        2: "op=-1 op=6 op=-1+null:widths op=-1+null:offsets op=-1+null:pk op=-1+null:refs op=-1+null:mask op=-1+null:ef op=-1+off8:widths "
           "op=-1+empty op=6+null:widths op=6+null:offsets op=6+null:pk op=6+null:refs op=6+null:mask op=6+null:ef op=6+off8:widths "
           "op=6+empty zero:pk+op=-1 zero:pk+op=6",
        3: "null:widths null:offsets null:pk null:refs null:mask null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:widths "
           "null:offsets+off8:pk null:pk+off8:refs null:pk+off8:offsets null:refs+off8:mask null:refs+off8:pk null:mask+off8:refs "
           "null:mask+off8:ef zero:pk+null:widths zero:pk+null:offsets zero:pk+null:refs zero:pk+null:mask",
        4: "off8:pk off8:mask null:ef+off8:mask zero:pk+off8:mask",
    },
    "unfor_compare_range": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:refs width+null:mask_in width+null:mask width+off8:in width+empty width+w0 width+cb=-1 "
           "width+cb=3",
        2: "cb=-1 cb=3 cb=-1+null:in cb=-1+null:refs cb=-1+null:mask_in cb=-1+null:mask cb=-1+off8:in cb=-1+empty cb=3+null:in "
           "cb=3+null:refs cb=3+null:mask_in cb=3+null:mask cb=3+off8:in cb=3+empty w0+cb=-1 w0+cb=3",
        3: "null:in null:refs null:mask_in null:mask w0+null:refs w0+null:mask_in w0+null:mask null:in+off8:refs null:in+off8:mask "
           "null:refs+off8:in null:refs+off8:mask_in null:mask_in+off8:refs null:mask_in+off8:mask null:mask+off8:in "
           "null:mask+off8:mask_in",
        4: "off8:in off8:mask_in off8:mask w0+off8:in",
    },
    "unfor_compare_range_widths": {
        0: "empty",
        2: "cb=-1 cb=3 cb=-1+null:widths cb=-1+null:offsets cb=-1+null:pk cb=-1+null:refs cb=-1+null:mask_in cb=-1+null:mask "
           "cb=-1+null:ef cb=-1+off8:widths cb=-1+empty cb=3+null:widths cb=3+null:offsets cb=3+null:pk cb=3+null:refs cb=3+null:mask_in "
           "cb=3+null:mask cb=3+null:ef cb=3+off8:widths cb=3+empty zero:pk+cb=-1 zero:pk+cb=3",
        3: "null:widths null:offsets null:pk null:refs null:mask_in null:mask null:widths+off8:ef null:widths+off8:offsets "
           "null:offsets+off8:widths null:offsets+off8:pk null:pk+off8:refs null:pk+off8:offsets null:refs+off8:mask_in null:refs+off8:pk "
           "null:mask_in+off8:refs null:mask_in+off8:mask null:mask+off8:ef null:mask+off8:mask_in zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:refs zero:pk+null:mask_in zero:pk+null:mask",
        4: "off8:pk off8:mask_in off8:mask null:ef+off8:mask zero:pk+off8:mask_in zero:pk+off8:mask",
    },
    "unfor_select": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:refs width+null:mask width+null:out_offsets width+null:out width+null:ef width+off8:in "
           "width+empty width+w0 zero:out+width",
        3: "null:in null:refs null:mask null:out_offsets null:out w0+null:refs w0+null:mask w0+null:out_offsets w0+null:out "
           "null:in+off8:refs null:in+off8:ef null:refs+off8:in null:refs+off8:mask null:mask+off8:refs null:mask+off8:out_offsets "
           "null:out_offsets+off8:out null:out_offsets+off8:mask null:out+off8:ef null:out+off8:out_offsets zero:out+null:in "
           "zero:out+null:refs zero:out+null:mask zero:out+null:out_offsets",
        4: "off8:in off8:mask off8:out w0+off8:in null:ef+off8:in null:ef+off8:out zero:out+off8:in zero:out+off8:mask",
    },
    "unfor_select_widths": {
        0: "empty",
        3: "null:widths null:offsets null:pk null:refs null:mask null:out_offsets null:out null:widths+off8:ef null:widths+off8:offsets "
           "null:offsets+off8:widths null:offsets+off8:pk null:pk+off8:refs null:pk+off8:offsets null:refs+off8:mask null:refs+off8:pk "
           "null:mask+off8:refs null:mask+off8:out_offsets null:out_offsets+off8:out null:out_offsets+off8:mask null:out+off8:ef "
           "null:out+off8:out_offsets zero:pk+null:widths zero:pk+null:offsets zero:pk+null:refs zero:pk+null:mask "
           "zero:pk+null:out_offsets zero:pk+null:out zero:out+null:widths zero:out+null:offsets zero:out+null:pk zero:out+null:refs "
           "zero:out+null:mask zero:out+null:out_offsets",
        4: "off8:pk off8:mask off8:out null:ef+off8:out zero:pk+off8:mask zero:pk+off8:out zero:out+off8:pk zero:out+off8:mask",
    },
    "unfor_aggregate": {
        0: "empty w0+empty",
        1: "width width+null:in width+null:refs width+null:mask width+null:aggs width+null:ef width+off8:in width+empty width+w0",
        3: "null:in null:refs null:aggs w0+null:refs w0+null:aggs null:in+off8:refs null:in+off8:ef null:refs+off8:in null:refs+off8:mask "
           "null:aggs+off8:ef null:aggs+off8:mask",
        4: "off8:in off8:mask off8:aggs w0+off8:in null:mask+off8:aggs null:ef+off8:in null:ef+off8:aggs",
    },
    "unfor_aggregate_widths": {
        0: "empty",
        3: "null:widths null:offsets null:pk null:refs null:aggs null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:widths "
           "null:offsets+off8:pk null:pk+off8:refs null:pk+off8:offsets null:refs+off8:mask null:refs+off8:pk null:aggs+off8:ef "
           "null:aggs+off8:mask zero:pk+null:widths zero:pk+null:offsets zero:pk+null:refs zero:pk+null:aggs",
        4: "off8:pk off8:mask off8:aggs null:mask+off8:aggs null:ef+off8:aggs zero:pk+off8:mask zero:pk+off8:aggs",
    },
    "unfor_aggregate_by": {
        1: "width width+empty width+null:in width+null:refs width+null:keys width+null:k_refs width+null:mask width+null:result "
           "width+null:ef width+off8:in width+off8:result widthk widthk+empty widthk+null:in widthk+null:result widthk+off8:in "
           "widthk+off8:result width+widthk w0+width w0+widthk w0k+width w0k+widthk n=0+width n=0+widthk",
        3: "empty w0+empty w0k+empty n=0+empty null:in null:refs null:keys null:k_refs null:result null:in+off8:ef null:in+off8:refs "
           "null:in+off8:result null:refs+off8:in null:refs+off8:keys null:refs+off8:result null:keys+off8:refs null:keys+off8:k_refs "
           "null:keys+off8:result null:k_refs+off8:keys null:k_refs+off8:mask null:k_refs+off8:result null:result+off8:mask "
           "null:result+off8:ef w0+null:refs w0+null:keys w0+null:k_refs w0+null:result w0+null:in+null:result w0+off8:in+null:result "
           "w0k+null:in w0k+null:refs w0k+null:k_refs w0k+null:result w0k+null:keys+null:in w0k+off8:keys+null:in "
           "w0k+null:keys+null:result w0k+off8:keys+null:result n=0+null:result n=0+off8:in+null:result n=0+off8:refs+null:result "
           "n=0+off8:keys+null:result n=0+off8:mask+null:result",
        4: "off8:in off8:keys off8:mask off8:result null:mask+off8:result null:ef+off8:result null:ef+off8:in w0+off8:in w0+off8:keys "
           "w0+off8:mask w0+off8:result w0+null:in+off8:result w0+off8:in+off8:result w0k+off8:in w0k+off8:keys w0k+off8:mask "
           "w0k+off8:result w0k+null:keys+off8:in w0k+off8:keys+off8:in w0k+null:keys+off8:result w0k+off8:keys+off8:result "
           "n=0+off8:result n=0+null:in+off8:result n=0+off8:in+off8:result n=0+null:refs+off8:result n=0+off8:refs+off8:result "
           "n=0+null:keys+off8:result n=0+off8:keys+off8:result n=0+null:mask+off8:result n=0+off8:mask+off8:result",
    },
    "unfor_aggregate_by_widths": {
        3: "empty zero:pk+empty zero:keys+empty n=0+empty null:widths null:offsets null:pk null:refs null:k_widths null:k_offsets "
           "null:keys null:k_refs null:result null:widths+off8:ef null:widths+off8:offsets null:widths+off8:result "
           "null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:result null:pk+off8:offsets null:pk+off8:refs "
           "null:pk+off8:result null:refs+off8:pk null:refs+off8:k_widths null:refs+off8:result null:k_widths+off8:refs "
           "null:k_widths+off8:k_offsets null:k_widths+off8:result null:k_offsets+off8:k_widths null:k_offsets+off8:keys "
           "null:k_offsets+off8:result null:keys+off8:k_offsets null:keys+off8:k_refs null:keys+off8:result null:k_refs+off8:keys "
           "null:k_refs+off8:mask null:k_refs+off8:result null:result+off8:mask null:result+off8:ef zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:refs zero:pk+null:result zero:keys+null:k_widths zero:keys+null:k_offsets "
           "zero:keys+null:k_refs zero:keys+null:result n=0+null:result n=0+off8:pk+null:result n=0+off8:refs+null:result "
           "n=0+off8:keys+null:result n=0+off8:mask+null:result",
        4: "off8:pk off8:keys off8:mask off8:result null:mask+off8:result null:ef+off8:result zero:pk+off8:keys zero:pk+off8:mask "
           "zero:pk+off8:result zero:keys+off8:pk zero:keys+off8:mask zero:keys+off8:result n=0+off8:result n=0+null:pk+off8:result "
           "n=0+off8:pk+off8:result n=0+null:refs+off8:result n=0+off8:refs+off8:result n=0+null:keys+off8:result "
           "n=0+off8:keys+off8:result n=0+null:mask+off8:result n=0+off8:mask+off8:result",
    },
    "unfor_compare_columns": {
        0: "empty w0+empty w0b+empty cb=0+empty n=0+empty n=0+null:in n=0+null:mask n=0+off8:in n=0+off8:mask",
        1: "width width+empty width+null:in width+null:refs width+null:b width+null:b_refs width+null:mask_in width+null:mask "
           "width+off8:in width+off8:mask widthb widthb+empty widthb+null:in widthb+null:mask widthb+off8:in widthb+off8:mask "
           "width+widthb width+op=6 width+cb=3 widthb+op=6 widthb+cb=3 w0+width w0+widthb w0b+width w0b+widthb cb=0+width cb=0+widthb "
           "n=0+width n=0+widthb",
        2: "op=6 op=6+empty op=6+null:in op=-1 op=-1+empty op=-1+null:in op=6+null:mask op=6+off8:in op=6+off8:mask cb=3 cb=3+empty "
           "cb=3+null:in cb=-1 cb=-1+empty cb=-1+null:in cb=3+null:mask cb=3+off8:in cb=3+off8:mask op=6+cb=3 w0+op=6 w0+cb=3 w0b+op=6 "
           "w0b+cb=3 cb=0+op=6 n=0+op=6 n=0+cb=3",
        3: "null:in null:refs null:b null:b_refs null:mask_in null:mask null:in+off8:mask null:in+off8:refs null:refs+off8:in "
           "null:refs+off8:b null:refs+off8:mask null:b+off8:refs null:b+off8:b_refs null:b+off8:mask null:b_refs+off8:b "
           "null:b_refs+off8:mask_in null:b_refs+off8:mask null:mask_in+off8:b_refs null:mask_in+off8:mask null:mask+off8:mask_in "
           "null:mask+off8:in w0+null:refs w0+null:b w0+null:b_refs w0+null:mask_in w0+null:mask w0+null:in+null:mask "
           "w0+off8:in+null:mask w0b+null:in w0b+null:refs w0b+null:b_refs w0b+null:mask_in w0b+null:mask w0b+null:b+null:in "
           "w0b+off8:b+null:in w0b+null:b+null:mask w0b+off8:b+null:mask cb=0+null:in cb=0+null:refs cb=0+null:b cb=0+null:b_refs "
           "cb=0+null:mask cb=0+null:mask_in+null:in cb=0+off8:mask_in+null:in cb=0+null:mask_in+null:mask cb=0+off8:mask_in+null:mask",
        4: "off8:in off8:b off8:mask_in off8:mask w0+off8:in w0+off8:b w0+off8:mask_in w0+off8:mask w0+null:in+off8:mask "
           "w0+off8:in+off8:mask w0b+off8:in w0b+off8:b w0b+off8:mask_in w0b+off8:mask w0b+null:b+off8:in w0b+off8:b+off8:in "
           "w0b+null:b+off8:mask w0b+off8:b+off8:mask cb=0+off8:in cb=0+off8:b cb=0+off8:mask cb=0+null:mask_in+off8:in "
           "cb=0+off8:mask_in+off8:in cb=0+null:mask_in+off8:mask cb=0+off8:mask_in+off8:mask",
    },
    "unfor_compare_columns_widths": {
        0: "empty zero:pk+empty zero:b+empty cb=0+empty n=0+empty n=0+null:pk n=0+null:mask n=0+off8:pk n=0+off8:mask",
        2: "op=6 op=6+empty op=6+null:pk op=-1 op=-1+empty op=-1+null:pk op=6+null:widths op=6+null:offsets op=6+null:refs "
           "op=6+null:b_widths op=6+null:b_offsets op=6+null:b op=6+null:b_refs op=6+null:mask_in op=6+null:mask op=6+null:ef "
           "op=6+off8:pk op=6+off8:mask cb=3 cb=3+empty cb=3+null:pk cb=-1 cb=-1+empty cb=-1+null:pk cb=3+null:mask cb=3+off8:pk "
           "cb=3+off8:mask op=6+cb=3 zero:pk+op=6 zero:pk+cb=3 zero:b+op=6 zero:b+cb=3 cb=0+op=6 n=0+op=6 n=0+cb=3",
        3: "null:widths null:offsets null:pk null:refs null:b_widths null:b_offsets null:b null:b_refs null:mask_in null:mask "
           "null:widths+off8:ef null:widths+off8:offsets null:widths+off8:mask null:offsets+off8:widths null:offsets+off8:pk "
           "null:offsets+off8:mask null:pk+off8:offsets null:pk+off8:refs null:pk+off8:mask null:refs+off8:pk null:refs+off8:b_widths "
           "null:refs+off8:mask null:b_widths+off8:refs null:b_widths+off8:b_offsets null:b_widths+off8:mask "
           "null:b_offsets+off8:b_widths null:b_offsets+off8:b null:b_offsets+off8:mask null:b+off8:b_offsets null:b+off8:b_refs "
           "null:b+off8:mask null:b_refs+off8:b null:b_refs+off8:mask_in null:b_refs+off8:mask null:mask_in+off8:b_refs "
           "null:mask_in+off8:mask null:mask+off8:mask_in null:mask+off8:ef zero:pk+null:widths zero:pk+null:offsets zero:pk+null:refs "
           "zero:pk+null:mask zero:b+null:b_widths zero:b+null:b_offsets zero:b+null:b_refs zero:b+null:mask cb=0+null:widths "
           "cb=0+null:offsets cb=0+null:pk cb=0+null:refs cb=0+null:b_widths cb=0+null:b_offsets cb=0+null:b cb=0+null:b_refs "
           "cb=0+null:mask cb=0+null:mask_in+null:pk cb=0+off8:mask_in+null:pk cb=0+null:mask_in+null:mask cb=0+off8:mask_in+null:mask",
        4: "off8:pk off8:b off8:mask_in off8:mask null:ef+off8:mask zero:pk+off8:b zero:pk+off8:mask_in zero:pk+off8:mask zero:b+off8:pk "
           "zero:b+off8:mask_in zero:b+off8:mask cb=0+off8:pk cb=0+off8:b cb=0+off8:mask cb=0+null:mask_in+off8:pk "
           "cb=0+off8:mask_in+off8:pk cb=0+null:mask_in+off8:mask cb=0+off8:mask_in+off8:mask",
    },
    "unfor_aggregate_columns": {
        0: "empty w0+empty w0b+empty n=0+empty n=0+null:in n=0+null:aggs n=0+off8:in n=0+off8:aggs",
        1: "width width+empty width+null:in width+null:aggs width+off8:in width+off8:aggs widthb widthb+empty widthb+null:in "
           "widthb+null:aggs widthb+off8:in widthb+off8:aggs ex=3+width ex=3+widthb width+widthb w0+width w0+widthb w0b+width w0b+widthb "
           "n=0+width n=0+widthb",
        2: "ex=3 ex=3+empty ex=3+null:in ex=-1 ex=-1+empty ex=-1+null:in ex=3+null:refs ex=3+null:b ex=3+null:b_refs ex=3+null:mask "
           "ex=3+null:aggs ex=3+null:ef ex=3+off8:in ex=3+off8:aggs w0+ex=3 w0b+ex=3 n=0+ex=3",
        3: "null:in null:refs null:b null:b_refs null:aggs null:in+off8:ef null:in+off8:refs null:in+off8:aggs null:refs+off8:in "
           "null:refs+off8:b null:refs+off8:aggs null:b+off8:refs null:b+off8:b_refs null:b+off8:aggs null:b_refs+off8:b "
           "null:b_refs+off8:mask null:b_refs+off8:aggs null:aggs+off8:mask null:aggs+off8:ef w0+null:refs w0+null:b w0+null:b_refs "
           "w0+null:aggs w0+null:in+null:aggs w0+off8:in+null:aggs w0b+null:in w0b+null:refs w0b+null:b_refs w0b+null:aggs "
           "w0b+null:b+null:in w0b+off8:b+null:in w0b+null:b+null:aggs w0b+off8:b+null:aggs",
        4: "off8:in off8:b off8:mask off8:aggs null:mask+off8:aggs null:ef+off8:aggs null:ef+off8:in w0+off8:in w0+off8:b w0+off8:mask "
           "w0+off8:aggs w0+null:in+off8:aggs w0+off8:in+off8:aggs w0b+off8:in w0b+off8:b w0b+off8:mask w0b+off8:aggs w0b+null:b+off8:in "
           "w0b+off8:b+off8:in w0b+null:b+off8:aggs w0b+off8:b+off8:aggs",
    },
    "unfor_aggregate_columns_widths": {
        0: "empty zero:pk+empty zero:b+empty n=0+empty n=0+null:pk n=0+null:aggs n=0+off8:pk n=0+off8:aggs",
        2: "ex=3 ex=3+empty ex=3+null:pk ex=-1 ex=-1+empty ex=-1+null:pk ex=3+null:widths ex=3+null:offsets ex=3+null:refs "
           "ex=3+null:b_widths ex=3+null:b_offsets ex=3+null:b ex=3+null:b_refs ex=3+null:mask ex=3+null:aggs ex=3+null:ef ex=3+off8:pk "
           "ex=3+off8:aggs zero:pk+ex=3 zero:b+ex=3 n=0+ex=3",
        3: "null:widths null:offsets null:pk null:refs null:b_widths null:b_offsets null:b null:b_refs null:aggs null:widths+off8:ef "
           "null:widths+off8:offsets null:widths+off8:aggs null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:aggs "
           "null:pk+off8:offsets null:pk+off8:refs null:pk+off8:aggs null:refs+off8:pk null:refs+off8:b_widths null:refs+off8:aggs "
           "null:b_widths+off8:refs null:b_widths+off8:b_offsets null:b_widths+off8:aggs null:b_offsets+off8:b_widths "
           "null:b_offsets+off8:b null:b_offsets+off8:aggs null:b+off8:b_offsets null:b+off8:b_refs null:b+off8:aggs null:b_refs+off8:b "
           "null:b_refs+off8:mask null:b_refs+off8:aggs null:aggs+off8:mask null:aggs+off8:ef zero:pk+null:widths zero:pk+null:offsets "
           "zero:pk+null:refs zero:pk+null:aggs zero:b+null:b_widths zero:b+null:b_offsets zero:b+null:b_refs zero:b+null:aggs",
        4: "off8:pk off8:b off8:mask off8:aggs null:mask+off8:aggs null:ef+off8:aggs zero:pk+off8:b zero:pk+off8:mask zero:pk+off8:aggs "
           "zero:b+off8:pk zero:b+off8:mask zero:b+off8:aggs",
    },
    "unfor_compare_in": {
        0: "empty w0+empty sb=0+empty cb=0+empty n=0+empty n=0+null:in n=0+null:mask n=0+off8:in n=0+off8:mask",
        1: "width width+empty width+null:in width+null:refs width+null:set_words width+null:mask_in width+null:mask width+off8:in "
           "width+off8:mask width+sb=over width+neg=2 width+cb=3 w0+width sb=0+width cb=0+width n=0+width",
        2: "sb=over sb=over+empty sb=over+null:in sb=over+null:mask sb=over+off8:in sb=over+off8:mask neg=2 neg=2+empty neg=2+null:in "
           "neg=-1 neg=-1+empty neg=-1+null:in neg=2+null:mask neg=2+off8:in neg=2+off8:mask cb=3 cb=3+empty cb=3+null:in cb=-1 "
           "cb=-1+empty cb=-1+null:in cb=3+null:mask cb=3+off8:in cb=3+off8:mask sb=over+neg=2 sb=over+cb=3 neg=2+cb=3 w0+sb=over "
           "w0+neg=2 w0+cb=3 sb=0+neg=2 sb=0+cb=3 cb=0+sb=over cb=0+neg=2 n=0+sb=over n=0+neg=2 n=0+cb=3",
        3: "null:in null:refs null:set_words null:mask_in null:mask null:in+off8:mask null:in+off8:refs null:refs+off8:in "
           "null:refs+off8:set_words null:refs+off8:mask null:set_words+off8:refs null:set_words+off8:mask_in null:set_words+off8:mask "
           "null:mask_in+off8:set_words null:mask_in+off8:mask null:mask+off8:mask_in null:mask+off8:in w0+null:refs w0+null:set_words "
           "w0+null:mask_in w0+null:mask w0+null:in+null:mask w0+off8:in+null:mask sb=0+null:in sb=0+null:refs sb=0+null:mask_in "
           "sb=0+null:mask sb=0+null:set_words+null:in sb=0+off8:set_words+null:in sb=0+null:set_words+null:mask "
           "sb=0+off8:set_words+null:mask cb=0+null:in cb=0+null:refs cb=0+null:set_words cb=0+null:mask cb=0+null:mask_in+null:in "
           "cb=0+off8:mask_in+null:in cb=0+null:mask_in+null:mask cb=0+off8:mask_in+null:mask",
        4: "off8:in off8:set_words off8:mask_in off8:mask w0+off8:in w0+off8:set_words w0+off8:mask_in w0+off8:mask w0+null:in+off8:mask "
           "w0+off8:in+off8:mask sb=0+off8:in sb=0+off8:mask_in sb=0+off8:mask sb=0+null:set_words+off8:in sb=0+off8:set_words+off8:in "
           "sb=0+null:set_words+off8:mask sb=0+off8:set_words+off8:mask cb=0+off8:in cb=0+off8:set_words cb=0+off8:mask "
           "cb=0+null:mask_in+off8:in cb=0+off8:mask_in+off8:in cb=0+null:mask_in+off8:mask cb=0+off8:mask_in+off8:mask",
    },
    "unfor_compare_in_widths": {
        0: "empty zero:pk+empty sb=0+empty cb=0+empty n=0+empty n=0+null:pk n=0+null:mask n=0+off8:pk n=0+off8:mask",
        2: "sb=over sb=over+empty sb=over+null:pk sb=over+null:widths sb=over+null:offsets sb=over+null:refs sb=over+null:set_words "
           "sb=over+null:mask_in sb=over+null:mask sb=over+null:ef sb=over+off8:pk sb=over+off8:mask neg=2 neg=2+empty neg=2+null:pk "
           "neg=-1 neg=-1+empty neg=-1+null:pk neg=2+null:mask neg=2+off8:pk neg=2+off8:mask cb=3 cb=3+empty cb=3+null:pk cb=-1 "
           "cb=-1+empty cb=-1+null:pk cb=3+null:mask cb=3+off8:pk cb=3+off8:mask sb=over+neg=2 sb=over+cb=3 neg=2+cb=3 zero:pk+sb=over "
           "zero:pk+neg=2 zero:pk+cb=3 sb=0+neg=2 sb=0+cb=3 cb=0+sb=over cb=0+neg=2 n=0+sb=over n=0+neg=2 n=0+cb=3",
        3: "null:widths null:offsets null:pk null:refs null:set_words null:mask_in null:mask null:widths+off8:ef "
           "null:widths+off8:offsets null:widths+off8:mask null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:mask "
           "null:pk+off8:offsets null:pk+off8:refs null:pk+off8:mask null:refs+off8:pk null:refs+off8:set_words null:refs+off8:mask "
           "null:set_words+off8:refs null:set_words+off8:mask_in null:set_words+off8:mask null:mask_in+off8:set_words "
           "null:mask_in+off8:mask null:mask+off8:mask_in null:mask+off8:ef zero:pk+null:widths zero:pk+null:offsets zero:pk+null:refs "
           "zero:pk+null:mask sb=0+null:widths sb=0+null:offsets sb=0+null:pk sb=0+null:refs sb=0+null:mask_in sb=0+null:mask "
           "sb=0+null:set_words+null:pk sb=0+off8:set_words+null:pk sb=0+null:set_words+null:mask sb=0+off8:set_words+null:mask "
           "cb=0+null:widths cb=0+null:offsets cb=0+null:pk cb=0+null:refs cb=0+null:set_words cb=0+null:mask cb=0+null:mask_in+null:pk "
           "cb=0+off8:mask_in+null:pk cb=0+null:mask_in+null:mask cb=0+off8:mask_in+null:mask",
        4: "off8:pk off8:set_words off8:mask_in off8:mask null:ef+off8:mask zero:pk+off8:set_words zero:pk+off8:mask_in "
           "zero:pk+off8:mask sb=0+off8:pk sb=0+off8:mask_in sb=0+off8:mask sb=0+null:set_words+off8:pk sb=0+off8:set_words+off8:pk "
           "sb=0+null:set_words+off8:mask sb=0+off8:set_words+off8:mask cb=0+off8:pk cb=0+off8:set_words cb=0+off8:mask "
           "cb=0+null:mask_in+off8:pk cb=0+off8:mask_in+off8:pk cb=0+null:mask_in+off8:mask cb=0+off8:mask_in+off8:mask",
    },
    "unfor_aggregate_by_columns": {
        1: "width width+empty width+null:in width+null:result width+off8:in width+off8:result widthb widthb+empty widthb+null:in "
           "widthb+null:result widthb+off8:in widthb+off8:result widthk widthk+empty widthk+null:in widthk+null:result widthk+off8:in "
           "widthk+off8:result ex=3+width ex=3+widthb ex=3+widthk width+widthb width+widthk widthb+widthk w0+width w0+widthb w0+widthk "
           "w0b+width w0b+widthb w0b+widthk w0k+width w0k+widthb w0k+widthk n=0+width n=0+widthb n=0+widthk",
        2: "ex=3 ex=3+empty ex=3+null:in ex=-1 ex=-1+empty ex=-1+null:in ex=3+null:refs ex=3+null:b ex=3+null:b_refs ex=3+null:keys "
           "ex=3+null:k_refs ex=3+null:mask ex=3+null:result ex=3+null:ef ex=3+off8:in ex=3+off8:result w0+ex=3 w0b+ex=3 w0k+ex=3 "
           "n=0+ex=3",
        3: "empty w0+empty w0b+empty w0k+empty n=0+empty null:in null:refs null:b null:b_refs null:keys null:k_refs null:result "
           "null:in+off8:ef null:in+off8:refs null:in+off8:result null:refs+off8:in null:refs+off8:b null:refs+off8:result "
           "null:b+off8:refs null:b+off8:b_refs null:b+off8:result null:b_refs+off8:b null:b_refs+off8:keys null:b_refs+off8:result "
           "null:keys+off8:b_refs null:keys+off8:k_refs null:keys+off8:result null:k_refs+off8:keys null:k_refs+off8:mask "
           "null:k_refs+off8:result null:result+off8:mask null:result+off8:ef w0+null:refs w0+null:b w0+null:b_refs w0+null:keys "
           "w0+null:k_refs w0+null:result w0+null:in+null:result w0+off8:in+null:result w0b+null:in w0b+null:refs w0b+null:b_refs "
           "w0b+null:keys w0b+null:k_refs w0b+null:result w0b+null:b+null:in w0b+off8:b+null:in w0b+null:b+null:result "
           "w0b+off8:b+null:result w0k+null:in w0k+null:refs w0k+null:b w0k+null:b_refs w0k+null:k_refs w0k+null:result "
           "w0k+null:keys+null:in w0k+off8:keys+null:in w0k+null:keys+null:result w0k+off8:keys+null:result n=0+null:result "
           "n=0+off8:in+null:result n=0+off8:refs+null:result n=0+off8:keys+null:result n=0+off8:mask+null:result",
        4: "off8:in off8:b off8:keys off8:mask off8:result null:mask+off8:result null:ef+off8:result null:ef+off8:in w0+off8:in "
           "w0+off8:b w0+off8:keys w0+off8:mask w0+off8:result w0+null:in+off8:result w0+off8:in+off8:result w0b+off8:in w0b+off8:b "
           "w0b+off8:keys w0b+off8:mask w0b+off8:result w0b+null:b+off8:in w0b+off8:b+off8:in w0b+null:b+off8:result "
           "w0b+off8:b+off8:result w0k+off8:in w0k+off8:b w0k+off8:keys w0k+off8:mask w0k+off8:result w0k+null:keys+off8:in "
           "w0k+off8:keys+off8:in w0k+null:keys+off8:result w0k+off8:keys+off8:result n=0+off8:result n=0+null:in+off8:result "
           "n=0+off8:in+off8:result n=0+null:refs+off8:result n=0+off8:refs+off8:result n=0+null:keys+off8:result "
           "n=0+off8:keys+off8:result n=0+null:mask+off8:result n=0+off8:mask+off8:result",
    },
    "unfor_aggregate_by_columns_widths": {
        2: "ex=3 ex=3+empty ex=3+null:pk ex=-1 ex=-1+empty ex=-1+null:pk ex=3+null:widths ex=3+null:offsets ex=3+null:refs "
           "ex=3+null:b_widths ex=3+null:b_offsets ex=3+null:b ex=3+null:b_refs ex=3+null:k_widths ex=3+null:k_offsets ex=3+null:keys "
           "ex=3+null:k_refs ex=3+null:mask ex=3+null:result ex=3+null:ef ex=3+off8:pk ex=3+off8:result zero:pk+ex=3 zero:b+ex=3 "
           "zero:keys+ex=3 n=0+ex=3",
        3: "empty zero:pk+empty zero:b+empty zero:keys+empty n=0+empty null:widths null:offsets null:pk null:refs null:b_widths "
           "null:b_offsets null:b null:b_refs null:k_widths null:k_offsets null:keys null:k_refs null:result null:widths+off8:ef "
           "null:widths+off8:offsets null:widths+off8:result null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:result "
           "null:pk+off8:offsets null:pk+off8:refs null:pk+off8:result null:refs+off8:pk null:refs+off8:b_widths null:refs+off8:result "
           "null:b_widths+off8:refs null:b_widths+off8:b_offsets null:b_widths+off8:result null:b_offsets+off8:b_widths "
           "null:b_offsets+off8:b null:b_offsets+off8:result null:b+off8:b_offsets null:b+off8:b_refs null:b+off8:result "
           "null:b_refs+off8:b null:b_refs+off8:k_widths null:b_refs+off8:result null:k_widths+off8:b_refs null:k_widths+off8:k_offsets "
           "null:k_widths+off8:result null:k_offsets+off8:k_widths null:k_offsets+off8:keys null:k_offsets+off8:result "
           "null:keys+off8:k_offsets null:keys+off8:k_refs null:keys+off8:result null:k_refs+off8:keys null:k_refs+off8:mask "
           "null:k_refs+off8:result null:result+off8:mask null:result+off8:ef zero:pk+null:widths zero:pk+null:offsets zero:pk+null:refs "
           "zero:pk+null:result zero:b+null:b_widths zero:b+null:b_offsets zero:b+null:b_refs zero:b+null:result zero:keys+null:k_widths "
           "zero:keys+null:k_offsets zero:keys+null:k_refs zero:keys+null:result n=0+null:result n=0+off8:pk+null:result "
           "n=0+off8:refs+null:result n=0+off8:keys+null:result n=0+off8:mask+null:result",
        4: "off8:pk off8:b off8:keys off8:mask off8:result null:mask+off8:result null:ef+off8:result zero:pk+off8:b zero:pk+off8:keys "
           "zero:pk+off8:mask zero:pk+off8:result zero:b+off8:pk zero:b+off8:keys zero:b+off8:mask zero:b+off8:result zero:keys+off8:pk "
           "zero:keys+off8:b zero:keys+off8:mask zero:keys+off8:result n=0+off8:result n=0+null:pk+off8:result n=0+off8:pk+off8:result "
           "n=0+null:refs+off8:result n=0+off8:refs+off8:result n=0+null:keys+off8:result n=0+off8:keys+off8:result "
           "n=0+null:mask+off8:result n=0+off8:mask+off8:result",
    },
    "unfor_set_build": {
        0: "empty w0+empty n=0+empty sb=0+empty n=0+null:in n=0+null:set_words n=0+off8:in n=0+off8:set_words",
        1: "width width+empty width+null:in width+null:refs width+null:mask width+null:set_words width+null:stats width+off8:in "
           "width+off8:set_words width+sb=over w0+width n=0+width sb=0+width",
        2: "sb=over sb=over+empty sb=over+null:in sb=over+null:set_words sb=over+off8:in sb=over+off8:set_words w0+sb=over n=0+sb=over",
        3: "null:in null:refs null:set_words null:in+off8:stats null:in+off8:refs null:in+off8:set_words null:refs+off8:in "
           "null:refs+off8:mask null:refs+off8:set_words null:set_words+off8:mask null:set_words+off8:stats w0+null:refs "
           "w0+null:set_words w0+null:in+null:set_words w0+off8:in+null:set_words sb=0+null:in sb=0+null:refs "
           "sb=0+null:set_words+null:in sb=0+off8:set_words+null:in",
        4: "off8:in off8:mask off8:set_words off8:stats null:mask+off8:set_words null:stats+off8:set_words null:stats+off8:in w0+off8:in "
           "w0+off8:mask w0+off8:set_words w0+off8:stats w0+null:in+off8:set_words w0+off8:in+off8:set_words sb=0+off8:in sb=0+off8:mask "
           "sb=0+off8:stats sb=0+null:set_words+off8:in sb=0+off8:set_words+off8:in",
    },
    "unfor_set_build_widths": {
        0: "empty zero:pk+empty n=0+empty sb=0+empty n=0+null:pk n=0+null:set_words n=0+off8:pk n=0+off8:set_words",
        2: "sb=over sb=over+empty sb=over+null:pk sb=over+null:widths sb=over+null:offsets sb=over+null:refs sb=over+null:mask "
           "sb=over+null:set_words sb=over+null:stats sb=over+null:ef sb=over+off8:pk sb=over+off8:set_words zero:pk+sb=over n=0+sb=over",
        3: "null:widths null:offsets null:pk null:refs null:set_words null:widths+off8:ef null:widths+off8:offsets "
           "null:widths+off8:set_words null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:set_words null:pk+off8:offsets "
           "null:pk+off8:refs null:pk+off8:set_words null:refs+off8:pk null:refs+off8:mask null:refs+off8:set_words "
           "null:set_words+off8:mask null:set_words+off8:stats zero:pk+null:widths zero:pk+null:offsets zero:pk+null:refs "
           "zero:pk+null:set_words sb=0+null:widths sb=0+null:offsets sb=0+null:pk sb=0+null:refs sb=0+null:set_words+null:pk "
           "sb=0+off8:set_words+null:pk",
        4: "off8:pk off8:mask off8:set_words off8:stats null:mask+off8:set_words null:stats+off8:set_words null:ef+off8:stats "
           "null:ef+off8:set_words zero:pk+off8:mask zero:pk+off8:set_words zero:pk+off8:stats sb=0+off8:pk sb=0+off8:mask "
           "sb=0+off8:stats sb=0+null:set_words+off8:pk sb=0+off8:set_words+off8:pk",
    },
    "unfor_aggregate_by_window": {
        0: "empty w0+empty w0k+empty n=0+empty ng=0+empty n=0+null:in n=0+null:counts n=0+off8:in n=0+off8:counts",
        1: "width width+empty width+null:in width+null:refs width+null:keys width+null:k_refs width+null:mask width+null:counts "
           "width+null:sums width+null:mins width+null:maxs width+null:stats width+off8:in width+off8:counts widthk widthk+empty "
           "widthk+null:in widthk+null:counts widthk+off8:in widthk+off8:counts width+widthk width+ng=over widthk+ng=over w0+width "
           "w0+widthk w0k+width w0k+widthk n=0+width n=0+widthk ng=0+width ng=0+widthk",
        2: "ng=over ng=over+empty ng=over+null:in ng=over+null:counts ng=over+off8:in ng=over+off8:counts w0+ng=over w0k+ng=over "
           "n=0+ng=over",
        3: "null:in null:refs null:keys null:k_refs null:in+off8:stats null:in+off8:refs null:in+off8:counts null:refs+off8:in "
           "null:refs+off8:keys null:refs+off8:counts null:keys+off8:refs null:keys+off8:k_refs null:keys+off8:counts "
           "null:k_refs+off8:keys null:k_refs+off8:mask null:k_refs+off8:counts w0+null:refs w0+null:keys w0+null:k_refs w0k+null:in "
           "w0k+null:refs w0k+null:k_refs w0k+null:keys+null:in w0k+off8:keys+null:in ng=0+null:in ng=0+null:refs ng=0+null:keys "
           "ng=0+null:k_refs ng=0+null:counts+null:in ng=0+off8:counts+null:in ng=0+null:sums+null:in ng=0+off8:sums+null:in "
           "ng=0+null:mins+null:in ng=0+off8:mins+null:in ng=0+null:maxs+null:in ng=0+off8:maxs+null:in",
        4: "off8:in off8:keys off8:mask off8:counts off8:sums off8:mins off8:maxs off8:stats null:mask+off8:counts null:counts+off8:mask "
           "null:counts+off8:sums null:sums+off8:counts null:sums+off8:mins null:mins+off8:sums null:mins+off8:maxs "
           "null:mins+off8:counts null:maxs+off8:mins null:maxs+off8:stats null:maxs+off8:counts null:stats+off8:maxs null:stats+off8:in "
           "null:stats+off8:counts w0+off8:in w0+off8:keys w0+off8:mask w0+off8:counts w0+off8:sums w0+off8:mins w0+off8:maxs "
           "w0+off8:stats w0+off8:in+null:counts w0+null:in+off8:counts w0+off8:in+off8:counts w0k+off8:in w0k+off8:keys w0k+off8:mask "
           "w0k+off8:counts w0k+off8:sums w0k+off8:mins w0k+off8:maxs w0k+off8:stats w0k+null:keys+off8:in w0k+off8:keys+off8:in "
           "w0k+off8:keys+null:counts w0k+null:keys+off8:counts w0k+off8:keys+off8:counts ng=0+off8:in ng=0+off8:keys ng=0+off8:mask "
           "ng=0+off8:stats ng=0+null:counts+off8:in ng=0+off8:counts+off8:in ng=0+null:sums+off8:in ng=0+off8:sums+off8:in "
           "ng=0+null:mins+off8:in ng=0+off8:mins+off8:in ng=0+null:maxs+off8:in ng=0+off8:maxs+off8:in",
    },
    "unfor_aggregate_by_window_widths": {
        0: "empty zero:pk+empty zero:keys+empty n=0+empty ng=0+empty n=0+null:pk n=0+null:counts n=0+off8:pk n=0+off8:counts",
        2: "ng=over ng=over+empty ng=over+null:pk ng=over+null:widths ng=over+null:offsets ng=over+null:refs ng=over+null:k_widths "
           "ng=over+null:k_offsets ng=over+null:keys ng=over+null:k_refs ng=over+null:mask ng=over+null:counts ng=over+null:sums "
           "ng=over+null:mins ng=over+null:maxs ng=over+null:stats ng=over+null:ef ng=over+off8:pk ng=over+off8:counts zero:pk+ng=over "
           "zero:keys+ng=over n=0+ng=over",
        3: "null:widths null:offsets null:pk null:refs null:k_widths null:k_offsets null:keys null:k_refs null:widths+off8:ef "
           "null:widths+off8:offsets null:widths+off8:counts null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:counts "
           "null:pk+off8:offsets null:pk+off8:refs null:pk+off8:counts null:refs+off8:pk null:refs+off8:k_widths null:refs+off8:counts "
           "null:k_widths+off8:refs null:k_widths+off8:k_offsets null:k_widths+off8:counts null:k_offsets+off8:k_widths "
           "null:k_offsets+off8:keys null:k_offsets+off8:counts null:keys+off8:k_offsets null:keys+off8:k_refs null:keys+off8:counts "
           "null:k_refs+off8:keys null:k_refs+off8:mask null:k_refs+off8:counts zero:pk+null:widths zero:pk+null:offsets "
           "zero:pk+null:refs zero:keys+null:k_widths zero:keys+null:k_offsets zero:keys+null:k_refs ng=0+null:widths ng=0+null:offsets "
           "ng=0+null:pk ng=0+null:refs ng=0+null:k_widths ng=0+null:k_offsets ng=0+null:keys ng=0+null:k_refs ng=0+null:counts+null:pk "
           "ng=0+off8:counts+null:pk ng=0+null:sums+null:pk ng=0+off8:sums+null:pk ng=0+null:mins+null:pk ng=0+off8:mins+null:pk "
           "ng=0+null:maxs+null:pk ng=0+off8:maxs+null:pk",
        4: "off8:pk off8:keys off8:mask off8:counts off8:sums off8:mins off8:maxs off8:stats null:mask+off8:counts null:counts+off8:mask "
           "null:counts+off8:sums null:sums+off8:counts null:sums+off8:mins null:mins+off8:sums null:mins+off8:maxs "
           "null:mins+off8:counts null:maxs+off8:mins null:maxs+off8:stats null:maxs+off8:counts null:stats+off8:maxs "
           "null:stats+off8:counts null:ef+off8:stats null:ef+off8:counts zero:pk+off8:keys zero:pk+off8:mask zero:pk+off8:counts "
           "zero:pk+off8:sums zero:pk+off8:mins zero:pk+off8:maxs zero:pk+off8:stats zero:keys+off8:pk zero:keys+off8:mask "
           "zero:keys+off8:counts zero:keys+off8:sums zero:keys+off8:mins zero:keys+off8:maxs zero:keys+off8:stats ng=0+off8:pk "
           "ng=0+off8:keys ng=0+off8:mask ng=0+off8:stats ng=0+null:counts+off8:pk ng=0+off8:counts+off8:pk ng=0+null:sums+off8:pk "
           "ng=0+off8:sums+off8:pk ng=0+null:mins+off8:pk ng=0+off8:mins+off8:pk ng=0+null:maxs+off8:pk ng=0+off8:maxs+off8:pk",
    },
    "unfor_lookup": {
        0: "empty w0+empty n=0+empty ns=0+empty n=0+null:in n=0+null:out n=0+off8:in n=0+off8:out",
        1: "width width+empty width+null:in width+null:refs width+null:mask width+null:table width+null:present width+null:out "
           "width+null:hit_mask width+null:stats width+off8:in width+off8:out width+ns=over w0+width n=0+width ns=0+width",
        2: "ns=over ns=over+empty ns=over+null:in ns=over+null:out ns=over+off8:in ns=over+off8:out w0+ns=over n=0+ns=over",
        3: "null:in null:refs null:table null:out null:in+off8:stats null:in+off8:refs null:in+off8:out null:refs+off8:in "
           "null:refs+off8:mask null:refs+off8:out null:table+off8:mask null:table+off8:present null:table+off8:out "
           "null:out+off8:present null:out+off8:hit_mask w0+null:refs w0+null:table w0+null:out w0+null:in+null:out w0+off8:in+null:out "
           "ns=0+null:in ns=0+null:refs ns=0+null:out ns=0+null:table+null:in ns=0+off8:table+null:in ns=0+null:table+null:out "
           "ns=0+off8:table+null:out ns=0+null:present+null:in ns=0+off8:present+null:in ns=0+null:present+null:out "
           "ns=0+off8:present+null:out",
        4: "off8:in off8:mask off8:table off8:present off8:out off8:hit_mask off8:stats null:mask+off8:table null:mask+off8:out "
           "null:present+off8:table null:present+off8:out null:hit_mask+off8:out null:hit_mask+off8:stats null:stats+off8:hit_mask "
           "null:stats+off8:in null:stats+off8:out w0+off8:in w0+off8:mask w0+off8:table w0+off8:present w0+off8:out w0+off8:hit_mask "
           "w0+off8:stats w0+null:in+off8:out w0+off8:in+off8:out ns=0+off8:in ns=0+off8:mask ns=0+off8:out ns=0+off8:hit_mask "
           "ns=0+off8:stats ns=0+null:table+off8:in ns=0+off8:table+off8:in ns=0+null:table+off8:out ns=0+off8:table+off8:out "
           "ns=0+null:present+off8:in ns=0+off8:present+off8:in ns=0+null:present+off8:out ns=0+off8:present+off8:out",
    },
    "unfor_lookup_widths": {
        0: "empty zero:pk+empty n=0+empty ns=0+empty n=0+null:pk n=0+null:out n=0+off8:pk n=0+off8:out",
        2: "ns=over ns=over+empty ns=over+null:pk ns=over+null:widths ns=over+null:offsets ns=over+null:refs ns=over+null:mask "
           "ns=over+null:table ns=over+null:present ns=over+null:out ns=over+null:hit_mask ns=over+null:stats ns=over+null:ef "
           "ns=over+off8:pk ns=over+off8:out zero:pk+ns=over n=0+ns=over",
        3: "null:widths null:offsets null:pk null:refs null:table null:out null:widths+off8:ef null:widths+off8:offsets "
           "null:widths+off8:out null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:out null:pk+off8:offsets "
           "null:pk+off8:refs null:pk+off8:out null:refs+off8:pk null:refs+off8:mask null:refs+off8:out null:table+off8:mask "
           "null:table+off8:present null:table+off8:out null:out+off8:present null:out+off8:hit_mask zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:refs zero:pk+null:out ns=0+null:widths ns=0+null:offsets ns=0+null:pk ns=0+null:refs "
           "ns=0+null:out ns=0+null:table+null:pk ns=0+off8:table+null:pk ns=0+null:table+null:out ns=0+off8:table+null:out "
           "ns=0+null:present+null:pk ns=0+off8:present+null:pk ns=0+null:present+null:out ns=0+off8:present+null:out",
        4: "off8:pk off8:mask off8:table off8:present off8:out off8:hit_mask off8:stats null:mask+off8:table null:mask+off8:out "
           "null:present+off8:table null:present+off8:out null:hit_mask+off8:out null:hit_mask+off8:stats null:stats+off8:hit_mask "
           "null:stats+off8:out null:ef+off8:stats null:ef+off8:out zero:pk+off8:mask zero:pk+off8:table zero:pk+off8:present "
           "zero:pk+off8:out zero:pk+off8:hit_mask zero:pk+off8:stats ns=0+off8:pk ns=0+off8:mask ns=0+off8:out ns=0+off8:hit_mask "
           "ns=0+off8:stats ns=0+null:table+off8:pk ns=0+off8:table+off8:pk ns=0+null:table+off8:out ns=0+off8:table+off8:out "
           "ns=0+null:present+off8:pk ns=0+off8:present+off8:pk ns=0+null:present+off8:out ns=0+off8:present+off8:out",
    },
    "unfor_lookup_u8": {
        0: "empty w0+empty n=0+empty ns=0+empty n=0+null:in n=0+null:out n=0+off8:in n=0+off8:out",
        1: "width width+empty width+null:in width+null:refs width+null:mask width+null:table width+null:present width+null:out "
           "width+null:hit_mask width+null:stats width+off8:in width+off8:out width+ns=over w0+width n=0+width ns=0+width",
        2: "ns=over ns=over+empty ns=over+null:in ns=over+null:out ns=over+off8:in ns=over+off8:out w0+ns=over n=0+ns=over",
        3: "null:in null:refs null:table null:out null:in+off8:stats null:in+off8:refs null:in+off8:out null:refs+off8:in "
           "null:refs+off8:mask null:refs+off8:out null:table+off8:mask null:table+off8:present null:table+off8:out "
           "null:out+off8:present null:out+off8:hit_mask w0+null:refs w0+null:table w0+null:out w0+null:in+null:out w0+off8:in+null:out "
           "ns=0+null:in ns=0+null:refs ns=0+null:out ns=0+null:table+null:in ns=0+off8:table+null:in ns=0+null:table+null:out "
           "ns=0+off8:table+null:out ns=0+null:present+null:in ns=0+off8:present+null:in ns=0+null:present+null:out "
           "ns=0+off8:present+null:out",
        4: "off8:in off8:mask off8:table off8:present off8:out off8:hit_mask off8:stats null:mask+off8:table null:mask+off8:out "
           "null:present+off8:table null:present+off8:out null:hit_mask+off8:out null:hit_mask+off8:stats null:stats+off8:hit_mask "
           "null:stats+off8:in null:stats+off8:out w0+off8:in w0+off8:mask w0+off8:table w0+off8:present w0+off8:out w0+off8:hit_mask "
           "w0+off8:stats w0+null:in+off8:out w0+off8:in+off8:out ns=0+off8:in ns=0+off8:mask ns=0+off8:out ns=0+off8:hit_mask "
           "ns=0+off8:stats ns=0+null:table+off8:in ns=0+off8:table+off8:in ns=0+null:table+off8:out ns=0+off8:table+off8:out "
           "ns=0+null:present+off8:in ns=0+off8:present+off8:in ns=0+null:present+off8:out ns=0+off8:present+off8:out",
    },
    "unfor_lookup_u8_widths": {
        0: "empty zero:pk+empty n=0+empty ns=0+empty n=0+null:pk n=0+null:out n=0+off8:pk n=0+off8:out",
        2: "ns=over ns=over+empty ns=over+null:pk ns=over+null:widths ns=over+null:offsets ns=over+null:refs ns=over+null:mask "
           "ns=over+null:table ns=over+null:present ns=over+null:out ns=over+null:hit_mask ns=over+null:stats ns=over+null:ef "
           "ns=over+off8:pk ns=over+off8:out zero:pk+ns=over n=0+ns=over",
        3: "null:widths null:offsets null:pk null:refs null:table null:out null:widths+off8:ef null:widths+off8:offsets "
           "null:widths+off8:out null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:out null:pk+off8:offsets "
           "null:pk+off8:refs null:pk+off8:out null:refs+off8:pk null:refs+off8:mask null:refs+off8:out null:table+off8:mask "
           "null:table+off8:present null:table+off8:out null:out+off8:present null:out+off8:hit_mask zero:pk+null:widths "
           "zero:pk+null:offsets zero:pk+null:refs zero:pk+null:out ns=0+null:widths ns=0+null:offsets ns=0+null:pk ns=0+null:refs "
           "ns=0+null:out ns=0+null:table+null:pk ns=0+off8:table+null:pk ns=0+null:table+null:out ns=0+off8:table+null:out "
           "ns=0+null:present+null:pk ns=0+off8:present+null:pk ns=0+null:present+null:out ns=0+off8:present+null:out",
        4: "off8:pk off8:mask off8:table off8:present off8:out off8:hit_mask off8:stats null:mask+off8:table null:mask+off8:out "
           "null:present+off8:table null:present+off8:out null:hit_mask+off8:out null:hit_mask+off8:stats null:stats+off8:hit_mask "
           "null:stats+off8:out null:ef+off8:stats null:ef+off8:out zero:pk+off8:mask zero:pk+off8:table zero:pk+off8:present "
           "zero:pk+off8:out zero:pk+off8:hit_mask zero:pk+off8:stats ns=0+off8:pk ns=0+off8:mask ns=0+off8:out ns=0+off8:hit_mask "
           "ns=0+off8:stats ns=0+null:table+off8:pk ns=0+off8:table+off8:pk ns=0+null:table+off8:out ns=0+off8:table+off8:out "
           "ns=0+null:present+off8:pk ns=0+off8:present+off8:pk ns=0+null:present+off8:out ns=0+off8:present+off8:out",
    },
    "unfor_aggregate_by_lookup": {
        1: "width width+empty width+null:in width+null:refs width+null:keys width+null:k_refs width+null:mask width+null:table "
           "width+null:present width+null:result width+null:stats width+null:ef width+off8:in width+off8:result widthk widthk+empty "
           "widthk+null:in widthk+null:result widthk+off8:in widthk+off8:result width+widthk width+ns=over widthk+ns=over w0+width "
           "w0+widthk w0k+width w0k+widthk n=0+width n=0+widthk ns=0+width ns=0+widthk",
        2: "ns=over ns=over+empty ns=over+null:in ns=over+null:result ns=over+off8:in ns=over+off8:result w0+ns=over w0k+ns=over "
           "n=0+ns=over",
        3: "empty w0+empty w0k+empty n=0+empty ns=0+empty null:in null:refs null:keys null:k_refs null:table null:result null:in+off8:ef "
           "null:in+off8:refs null:in+off8:result null:refs+off8:in null:refs+off8:keys null:refs+off8:result null:keys+off8:refs "
           "null:keys+off8:k_refs null:keys+off8:result null:k_refs+off8:keys null:k_refs+off8:mask null:k_refs+off8:result "
           "null:table+off8:mask null:table+off8:present null:table+off8:result null:result+off8:present null:result+off8:stats "
           "w0+null:refs w0+null:keys w0+null:k_refs w0+null:table w0+null:result w0+null:in+null:result w0+off8:in+null:result "
           "w0k+null:in w0k+null:refs w0k+null:k_refs w0k+null:table w0k+null:result w0k+null:keys+null:in w0k+off8:keys+null:in "
           "w0k+null:keys+null:result w0k+off8:keys+null:result n=0+null:result ns=0+null:in ns=0+null:refs ns=0+null:keys "
           "ns=0+null:k_refs ns=0+null:result ns=0+null:table+null:in ns=0+off8:table+null:in ns=0+null:table+null:result "
           "ns=0+off8:table+null:result ns=0+null:present+null:in ns=0+off8:present+null:in ns=0+null:present+null:result "
           "ns=0+off8:present+null:result n=0+off8:in+null:result n=0+off8:refs+null:result n=0+off8:keys+null:result "
           "n=0+off8:mask+null:result",
        4: "off8:in off8:keys off8:mask off8:table off8:present off8:result off8:stats null:mask+off8:table null:mask+off8:result "
           "null:present+off8:table null:present+off8:result null:stats+off8:result null:ef+off8:stats null:ef+off8:in "
           "null:ef+off8:result w0+off8:in w0+off8:keys w0+off8:mask w0+off8:table w0+off8:present w0+off8:result w0+off8:stats "
           "w0+null:in+off8:result w0+off8:in+off8:result w0k+off8:in w0k+off8:keys w0k+off8:mask w0k+off8:table w0k+off8:present "
           "w0k+off8:result w0k+off8:stats w0k+null:keys+off8:in w0k+off8:keys+off8:in w0k+null:keys+off8:result "
           "w0k+off8:keys+off8:result n=0+off8:result ns=0+off8:in ns=0+off8:keys ns=0+off8:mask ns=0+off8:result ns=0+off8:stats "
           "ns=0+null:table+off8:in ns=0+off8:table+off8:in ns=0+null:table+off8:result ns=0+off8:table+off8:result "
           "ns=0+null:present+off8:in ns=0+off8:present+off8:in ns=0+null:present+off8:result ns=0+off8:present+off8:result "
           "n=0+null:in+off8:result n=0+off8:in+off8:result n=0+null:refs+off8:result n=0+off8:refs+off8:result "
           "n=0+null:keys+off8:result n=0+off8:keys+off8:result n=0+null:mask+off8:result n=0+off8:mask+off8:result",
    },
    "unfor_aggregate_by_lookup_widths": {
        2: "ns=over ns=over+empty ns=over+null:pk ns=over+null:widths ns=over+null:offsets ns=over+null:refs ns=over+null:k_widths "
           "ns=over+null:k_offsets ns=over+null:keys ns=over+null:k_refs ns=over+null:mask ns=over+null:table ns=over+null:present "
           "ns=over+null:result ns=over+null:stats ns=over+null:ef ns=over+off8:pk ns=over+off8:result zero:pk+ns=over zero:keys+ns=over "
           "n=0+ns=over",
        3: "empty zero:pk+empty zero:keys+empty n=0+empty ns=0+empty null:widths null:offsets null:pk null:refs null:k_widths "
           "null:k_offsets null:keys null:k_refs null:table null:result null:widths+off8:ef null:widths+off8:offsets "
           "null:widths+off8:result null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:result null:pk+off8:offsets "
           "null:pk+off8:refs null:pk+off8:result null:refs+off8:pk null:refs+off8:k_widths null:refs+off8:result "
           "null:k_widths+off8:refs null:k_widths+off8:k_offsets null:k_widths+off8:result null:k_offsets+off8:k_widths "
           "null:k_offsets+off8:keys null:k_offsets+off8:result null:keys+off8:k_offsets null:keys+off8:k_refs null:keys+off8:result "
           "null:k_refs+off8:keys null:k_refs+off8:mask null:k_refs+off8:result null:table+off8:mask null:table+off8:present "
           "null:table+off8:result null:result+off8:present null:result+off8:stats zero:pk+null:widths zero:pk+null:offsets "
           "zero:pk+null:refs zero:pk+null:result zero:keys+null:k_widths zero:keys+null:k_offsets zero:keys+null:k_refs "
           "zero:keys+null:result n=0+null:result ns=0+null:widths ns=0+null:offsets ns=0+null:pk ns=0+null:refs ns=0+null:k_widths "
           "ns=0+null:k_offsets ns=0+null:keys ns=0+null:k_refs ns=0+null:result ns=0+null:table+null:pk ns=0+off8:table+null:pk "
           "ns=0+null:table+null:result ns=0+off8:table+null:result ns=0+null:present+null:pk ns=0+off8:present+null:pk "
           "ns=0+null:present+null:result ns=0+off8:present+null:result n=0+off8:pk+null:result n=0+off8:refs+null:result "
           "n=0+off8:keys+null:result n=0+off8:mask+null:result",
        4: "off8:pk off8:keys off8:mask off8:table off8:present off8:result off8:stats null:mask+off8:table null:mask+off8:result "
           "null:present+off8:table null:present+off8:result null:stats+off8:result null:ef+off8:stats null:ef+off8:result "
           "zero:pk+off8:keys zero:pk+off8:mask zero:pk+off8:table zero:pk+off8:present zero:pk+off8:result zero:pk+off8:stats "
           "zero:keys+off8:pk zero:keys+off8:mask zero:keys+off8:table zero:keys+off8:present zero:keys+off8:result zero:keys+off8:stats "
           "n=0+off8:result ns=0+off8:pk ns=0+off8:keys ns=0+off8:mask ns=0+off8:result ns=0+off8:stats ns=0+null:table+off8:pk "
           "ns=0+off8:table+off8:pk ns=0+null:table+off8:result ns=0+off8:table+off8:result ns=0+null:present+off8:pk "
           "ns=0+off8:present+off8:pk ns=0+null:present+off8:result ns=0+off8:present+off8:result n=0+null:pk+off8:result "
           "n=0+off8:pk+off8:result n=0+null:refs+off8:result n=0+off8:refs+off8:result n=0+null:keys+off8:result "
           "n=0+off8:keys+off8:result n=0+null:mask+off8:result n=0+off8:mask+off8:result",
    },
    "undelta_compare_range": {
        0: "empty w0+empty cb=0+empty n=0+empty n=0+null:in n=0+null:mask n=0+off8:in n=0+off8:mask",
        1: "width width+empty width+null:in width+null:bases width+null:mask_in width+null:mask width+off8:in width+off8:mask width+cb=3 "
           "w0+width cb=0+width n=0+width",
        2: "cb=3 cb=3+empty cb=3+null:in cb=-1 cb=-1+empty cb=-1+null:in cb=3+null:mask cb=3+off8:in cb=3+off8:mask w0+cb=3 n=0+cb=3",
        3: "null:in null:bases null:mask_in null:mask null:in+off8:mask null:in+off8:bases null:bases+off8:in null:bases+off8:mask_in "
           "null:bases+off8:mask null:mask_in+off8:bases null:mask_in+off8:mask null:mask+off8:mask_in null:mask+off8:in w0+null:bases "
           "w0+null:mask_in w0+null:mask w0+null:in+null:mask w0+off8:in+null:mask cb=0+null:in cb=0+null:bases cb=0+null:mask "
           "cb=0+null:mask_in+null:in cb=0+off8:mask_in+null:in cb=0+null:mask_in+null:mask cb=0+off8:mask_in+null:mask",
        4: "off8:in off8:bases off8:mask_in off8:mask w0+off8:in w0+off8:bases w0+off8:mask_in w0+off8:mask w0+null:in+off8:mask "
           "w0+off8:in+off8:mask cb=0+off8:in cb=0+off8:bases cb=0+off8:mask cb=0+null:mask_in+off8:in cb=0+off8:mask_in+off8:in "
           "cb=0+null:mask_in+off8:mask cb=0+off8:mask_in+off8:mask",
    },
    "undelta_compare_range_widths": {
        0: "empty zero:pk+empty cb=0+empty n=0+empty n=0+null:pk n=0+null:mask n=0+off8:pk n=0+off8:mask",
        2: "cb=3 cb=3+empty cb=3+null:pk cb=-1 cb=-1+empty cb=-1+null:pk cb=3+null:widths cb=3+null:offsets cb=3+null:bases "
           "cb=3+null:mask_in cb=3+null:mask cb=3+null:ef cb=3+off8:pk cb=3+off8:mask zero:pk+cb=3 n=0+cb=3",
        3: "null:widths null:offsets null:pk null:bases null:mask_in null:mask null:widths+off8:ef null:widths+off8:offsets "
           "null:widths+off8:mask null:offsets+off8:widths null:offsets+off8:pk null:offsets+off8:mask null:pk+off8:offsets "
           "null:pk+off8:bases null:pk+off8:mask null:bases+off8:pk null:bases+off8:mask_in null:bases+off8:mask null:mask_in+off8:bases "
           "null:mask_in+off8:mask null:mask+off8:mask_in null:mask+off8:ef zero:pk+null:widths zero:pk+null:offsets zero:pk+null:bases "
           "zero:pk+null:mask cb=0+null:widths cb=0+null:offsets cb=0+null:pk cb=0+null:bases cb=0+null:mask cb=0+null:mask_in+null:pk "
           "cb=0+off8:mask_in+null:pk cb=0+null:mask_in+null:mask cb=0+off8:mask_in+null:mask",
        4: "off8:pk off8:bases off8:mask_in off8:mask null:ef+off8:mask zero:pk+off8:bases zero:pk+off8:mask_in zero:pk+off8:mask "
           "cb=0+off8:pk cb=0+off8:bases cb=0+off8:mask cb=0+null:mask_in+off8:pk cb=0+off8:mask_in+off8:pk cb=0+null:mask_in+off8:mask "
           "cb=0+off8:mask_in+off8:mask",
    },
    "fl_widths_to_offsets": {
        0: "empty",
        1: "type=12 type=12+null:widths type=12+null:offsets type=12+null:total type=12+null:ef type=12+off8:widths type=12+empty",
        3: "null:widths null:offsets null:widths+off8:ef null:widths+off8:offsets null:offsets+off8:total null:offsets+off8:widths",
    },
    "fl_mask_offsets": {
        0: "empty",
        3: "null:mask null:out_offsets null:mask+off8:total null:mask+off8:out_offsets null:out_offsets+off8:total "
           "null:out_offsets+off8:mask",
        4: "off8:mask null:total+off8:mask",
    },
    "fl_aggregate_reduce": {
        3: "null:aggs null:result empty null:aggs+off8:result null:result+off8:aggs",
        4: "off8:aggs off8:result",
    },
    "fl_fill_random": {
        0: "empty",
        3: "null:dst n=60+null:dst",
        4: "n=60 n=60+off8:dst",
    },
    "fl_mixed_plan_create": {
        0: "n=0 n=0+null:widths",
        1: "type=12 type=12+off8:widths n=0+type=12 badwidths badwidths+type=12",
        3: "null:widths null:plan empty type=12+null:widths type=12+null:plan type=12+empty null:widths+off8:plan null:plan+off8:widths "
           "badwidths+null:plan",
    },
}
# the statuses every entry point is pinned at (0: its empty call)
SHAPE = {
    "pack": "0134",
    "unpack": "0134",
    "unpack_single": "013",
    "for_pack": "0134",
    "unfor_pack": "0134",
    "delta": "034",
    "undelta": "034",
    "undelta_pack": "0134",
    "transpose": "034",
    "untranspose": "034",
    "undelta_pack_untranspose": "0134",
    "transpose_delta_pack": "0134",
    "unpack_block_sums": "0134",
    "block_min_max": "034",
    "unpack_compare": "01234",
    "unpack_mixed": "013",
    "pack_mixed": "013",
    "unpack_widths": "034",
    "pack_widths": "034",
    "unpack_single_widths": "03",
    "unfor_pack_widths": "034",
    "for_pack_widths": "034",
    "undelta_pack_widths": "034",
    "undelta_pack_untranspose_widths": "034",
    "transpose_delta_pack_widths": "034",
    "for_widths": "03",
    "unpack_batch": "023",
    "pack_batch": "023",
    "unfor_pack_batch": "023",
    "for_pack_batch": "023",
    "undelta_pack_batch": "023",
    "transpose_delta_pack_batch": "023",
    "pack_host": "13",
    "unpack_host": "13",
    "unpack_single_host": "123",
    "for_pack_host": "13",
    "unfor_pack_host": "13",
    "delta_host": "3",
    "undelta_host": "3",
    "undelta_pack_host": "13",
    "transpose_host": "3",
    "untranspose_host": "3",
    "unfor_compare": "01234",
    "unfor_compare_widths": "0234",
    "unfor_compare_range": "01234",
    "unfor_compare_range_widths": "0234",
    "unfor_select": "0134",
    "unfor_select_widths": "034",
    "unfor_aggregate": "0134",
    "unfor_aggregate_widths": "034",
    "unfor_aggregate_by": "134",                # the three aggregate_by* launch their init kernel for an empty column too: no 0
    "unfor_aggregate_by_widths": "34",
    "unfor_compare_columns": "01234",
    "unfor_compare_columns_widths": "0234",
    "unfor_aggregate_columns": "01234",
    "unfor_aggregate_columns_widths": "0234",
    "unfor_compare_in": "01234",
    "unfor_compare_in_widths": "0234",
    "unfor_aggregate_by_columns": "1234",
    "unfor_aggregate_by_columns_widths": "234",
    "unfor_set_build": "01234",
    "unfor_set_build_widths": "0234",
    "unfor_aggregate_by_window": "01234",
    "unfor_aggregate_by_window_widths": "0234",
    "unfor_lookup": "01234",
    "unfor_lookup_widths": "0234",
    "unfor_lookup_u8": "01234",
    "unfor_lookup_u8_widths": "0234",
    "unfor_aggregate_by_lookup": "1234",
    "unfor_aggregate_by_lookup_widths": "234",
    "undelta_compare_range": "01234",
    "undelta_compare_range_widths": "0234",
    "fl_widths_to_offsets": "013",
    "fl_mask_offsets": "034",
    "fl_aggregate_reduce": "34",
    "fl_fill_random": "034",
    "fl_mixed_plan_create": "013",
}
N_CASES = 3549                                              # 1138 recorded at 1fd1295, 2411 at 7eb97a5


@pytest.fixture(scope="module")
def calls(lib):
    c = Calls(lib)
    yield c
    c.close()


def test_the_table_covers_every_entry_point_and_status():
    """a row pruned away, or an entry point the table never learnt of, fails here instead of leaving that entry point unpinned"""
    from fastlanes_amd import _lib
    assert {name[len("fl_{ty}_"):] for _, name, _, _ in _lib._SIGNATURES if "{ty}" in name} == set(PER_TYPE)
    assert {name[len("fl_{vty}_"):] for _, name, _, _ in _lib._SIGNATURES if "{vty}" in name} == set(PER_VALUE_TYPE)
    assert list(TABLE) == list(PER_TYPE) + list(PER_VALUE_TYPE) + list(PLAIN)
    present = {entry: set() for entry in TABLE}
    for entry, _, status in rows(TABLE):
        present[entry].add(status)
    assert {entry: "".join(map(str, sorted(s))) for entry, s in present.items()} == SHAPE
    assert all(s <= {0, 1, 2, 3, 4} for s in present.values())        # nothing that got as far as the HIP runtime
    assert len(rows(TABLE)) == N_CASES


def test_every_refusal_is_the_recorded_one(lib, calls):
    wrong = []
    try:
        for policy in POLICIES:
            lib.fl_internal_set_kernel_policy(policy)
            assert lib.fl_internal_get_kernel_policy() == policy
            for entry, case, want in rows(TABLE):
                for ty in TYS:
                    if (got := calls(entry, case, ty)) != want:
                        wrong.append((entry, case, ty, policy, got, want))
    finally:
        lib.fl_internal_set_kernel_policy(0)
    assert not wrong, wrong[:20]
