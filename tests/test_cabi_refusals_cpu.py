"""CPU: the refusal matrix of the C ABI.  Every entry point that validates its arguments -- the 42 per-type ones of FL_DECLARE_TYPE, the
eight consumers of a FoR-packed column, fl_widths_to_offsets, fl_mask_offsets, fl_aggregate_reduce, fl_fill_random and
fl_mixed_plan_create -- is called for all four element types and under kernel policy 0, 1 and 2 (the uniform-width entry points take
another path, with another order of checks, under each) with calls that are refused before anything is launched, and must answer
what it answered at 1fd1295.

The literal table below was recorded from that commit's library on a machine without a GPU, where a call that gets past validation
answers FL_ERR_HIP; such calls were pruned, so every call kept here ends in FL_ERR_WIDTH, FL_ERR_INDEX, FL_ERR_NULL or FL_ERR_ALIGN
(or in FL_OK, for an empty call) before it reaches the device, and none launches a kernel on the made-up pointers.  A case is a
well-formed call -- every pointer a distinct 16-byte-aligned address inside one zeroed buffer, width 3, one block, packed_bytes to
match, a valid op / combine -- with one or two faults, joined by "+":
    null:X     pointer X is NULL                      off8:X    pointer X moved by 8 bytes
    width      width = T + 1                          w0        width = 0: only beside a fault, where it moves the checks
    op=V / cb=V    the compare op / the mask combine set to V
    mb         max_blocks = 2^30 + 1                  empty     the count that makes the call empty is 0 and every pointer NULL
    zero:X     X is NULL and its byte count (packed_bytes, out_len) is 0: allowed, so kept only beside a fault that is refused
    index      unpack_single_host: index = 1024       plan=other    a plan of another element type
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


def arguments(spec, case, ty, base, plans):
    """the argument list of one call: the well-formed one of `spec` with the faults of `case`"""
    faults = dict(f.replace("=", ":").partition(":")[::2] for f in case.split("+"))     # kind -> what it names, or the value it sets
    empty = "empty" in faults
    args, slot = [], 0
    for tok in spec.split():
        if tok[0] == "*":
            slot += 1
            name, p = tok[1:], base + slot * SLOT
            if empty or faults.get("null") == name or faults.get("zero") == name:
                p = None
            elif faults.get("off8") == name:
                p += 8
            elif name == "widths" and "badwidths" in faults:
                p = base                                    # slot 0 holds 0xff: a width no type has
            args.append(p)
        elif tok == "w":
            args.append(TYPE_BITS[ty] + 1 if "width" in faults else 0 if "w0" in faults else 3)
        elif tok in ("n", "n64"):
            args.append(0 if empty else int(faults["n"]) if "n" in faults else 64 if tok == "n64" else 1)
        elif tok == "pb":
            args.append(0 if faults.get("zero") in ("pk", "in") else 384)
        elif tok == "ol":
            args.append(0 if faults.get("zero") == "out" else 1024)
        elif tok in ("op", "cb"):
            args.append(int(faults[tok]) if tok in faults else 1)
        elif tok == "mb":
            args.append((1 << 30) + 1 if "mb" in faults else 1)
        elif tok == "q":
            args.append(1024 if "index" in faults else 0)
        elif tok == "tb":
            args.append(int(faults["type"]) if "type" in faults else TYPE_BITS[ty])
        elif tok == "plan":
            args.append(None if faults.get("null") == "plan" else plans[TYS[(TYS.index(ty) + 1) % 4] if "plan" in faults else ty])
        else:
            args.append({"one": 1, "k": 0, "i0": 0, "seed": 1, "s": None}[tok])
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
        args = arguments(PLAIN[entry] if plain else PER_TYPE[entry], case, ty, self.base, self.plans)
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
    "fl_widths_to_offsets": "013",
    "fl_mask_offsets": "034",
    "fl_aggregate_reduce": "34",
    "fl_fill_random": "034",
    "fl_mixed_plan_create": "013",
}
N_CASES = 1138


@pytest.fixture(scope="module")
def calls(lib):
    c = Calls(lib)
    yield c
    c.close()


def test_the_table_covers_every_entry_point_and_status():
    """a row pruned away, or an entry point the table never learnt of, fails here instead of leaving that entry point unpinned"""
    from fastlanes_amd import _lib
    assert {name[len("fl_{ty}_"):] for _, name, _, _ in _lib._SIGNATURES if "{ty}" in name} == set(PER_TYPE)
    assert list(TABLE) == list(PER_TYPE) + list(PLAIN)
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
