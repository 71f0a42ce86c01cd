"""CPU: unfor_aggregate_columns / unfor_aggregate_columns_widths (COUNT / SUM / MIN / MAX of a * b, a + b or a - b between two FoR-packed
columns of one element type under a selection mask) -- the header declares and the library exports them for every element type
through a macro of their own, the Python table agrees with the header, every refusal needs no GPU, the Python forms validate before
anything is loaded, and the plain integer part the kernel shares with the host (fastlanes_amd/csrc/fl_expr_map.hpp, compiled here with
g++) -- expr_apply, the route, the constant block -- agrees with Python's integers mod 2^64."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)

FORMS = ("unfor_aggregate_columns", "unfor_aggregate_columns_widths")
MUL, ADD, SUB = 0, 1, 2
M64 = 2 ** 64
PY = {MUL: lambda x, y: (x * y) % M64, ADD: lambda x, y: (x + y) % M64, SUB: lambda x, y: (x - y) % M64}
IDENTITY = (0, 0, M64 - 1, 0)
ROUTE_IDENTITY, ROUTE_CONSTANT, ROUTE_A, ROUTE_B, ROUTE_BOTH = range(5)


def header_prototypes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from gen_rust_ffi import prototypes
    finally:
        sys.path.pop(0)
    return {name: (ret, args) for name, ret, args in prototypes()}


def test_header_declares_and_library_exports_the_eight_symbols(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_AGGREGATE_COLUMNS(T, S)")[1].split("FL_DECLARE_AGGREGATE_COLUMNS(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_AGGREGATE_COLUMNS({CT[ty]}, {ty})" in text
    assert "typedef enum fl_expr { FL_EXPR_MUL = 0, FL_EXPR_ADD = 1, FL_EXPR_SUB = 2 } fl_expr;" in text
    doc = text.split("typedef enum fl_expr")[0].rsplit("/*", 1)[1]
    assert "UNSIGNED" in doc and "two's-complement" in doc                # how a negative difference is ordered is stated
    for scope in ("signed (sign-extending) columns", "different element types", "Delta columns", "grouping", "the host tier"):
        assert scope in doc, scope
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.aggregate_columns_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.select_symbols(),
                  fastlanes_amd.aggregate_symbols(), fastlanes_amd.for_compare_range_symbols(), fastlanes_amd.aggregate_by_symbols(),
                  fastlanes_amd.for_compare_columns_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"aggregate_columns_symbols", "unfor_aggregate_columns_widths"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.FoR, "unfor_aggregate_columns")


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: a pointer is c_void_p, `unsigned` c_uint, size_t c_size_t, int c_int; the
    two columns in unfor_compare_columns' order behind `expr`, the tail unfor_aggregate's"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("AGGREGATE_COLUMNS")}
    assert len(rows) == 8
    names = {FORMS[0]: "expr width_a a a_references a_reference_stride width_b b b_references b_reference_stride mask n_blocks "
                       "block_aggs err_flag stream",
             FORMS[1]: "expr a_widths a_offsets a_packed a_packed_bytes a_references a_reference_stride b_widths b_offsets b_packed "
                       "b_packed_bytes b_references b_reference_stride mask n_blocks block_aggs err_flag stream"}
    for ty in TYPE_BITS:
        for form in FORMS:
            name = f"fl_{ty}_{form}"
            ret, args = protos[name]
            restype, argtypes = rows[name]
            assert ret == "int" and restype is ctypes.c_int
            assert [a for _, a in args] == names[form].split(), name
            assert len(args) == len(argtypes), name
            for (ctype, arg), at in zip(args, argtypes):
                want = ctypes.c_void_p if "*" in ctype else {"unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "int": ctypes.c_int}[ctype]
                assert at is want, (name, arg, ctype)
            types = dict((a, c) for c, a in args)
            for col in ("a", "b"):                                         # both columns are of the element type
                assert types[f"{col}_references"] == f"const {CT[ty]} *"
                assert types[col if form == FORMS[0] else f"{col}_packed"] == f"const {CT[ty]} *"
            assert types["block_aggs"] == "void *" and types["mask"] == "const uint32_t *"
            assert getattr(lib, name).argtypes == argtypes
    # the tail is unfor_aggregate's, the two columns unfor_compare_columns'
    for ty in TYPE_BITS:
        tail = [a for _, a in protos[f"fl_{ty}_unfor_aggregate"][1]][-5:]
        cols = [a for _, a in protos[f"fl_{ty}_unfor_compare_columns"][1]][:8]
        mine = [a for _, a in protos[f"fl_{ty}_unfor_aggregate_columns"][1]]
        assert mine[1:9] == cols and mine[-5:] == tail


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before any device call (no call here reaches a kernel): either width, expr, the empty column, the
    pointers of both columns and the slots, alignment of both columns, the mask and the slots."""
    buf = np.zeros(8192, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    A, AR, B, BR, MK, G, AW, AO, BW, BO = (p + 4096 * i for i in range(10))
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_aggregate_columns")
        g = getattr(lib, f"fl_{ty}_unfor_aggregate_columns_widths")

        def uni(ex=MUL, wa=3, a=A, ar=AR, wb=5, b=B, br=BR, mk=MK, n=1, aggs=G):
            return f(ex, wa, a, ar, 1, wb, b, br, 1, mk, n, aggs, None, None)

        def mix(ex=MUL, aw=AW, ao=AO, a=A, ab=384, ar=AR, bw=BW, bo=BO, b=B, bb=384, br=BR, mk=MK, n=1, aggs=G):
            return g(ex, aw, ao, a, ab, ar, 1, bw, bo, b, bb, br, 1, mk, n, aggs, None, None)

        # FL_ERR_WIDTH: either width, also for an empty column and in front of every other refusal
        for n in (1, 0):
            assert uni(wa=T + 1, n=n) == 1 and uni(wb=T + 1, n=n) == 1 and uni(wa=T + 1, wb=T + 1, n=n) == 1
            assert uni(wa=T + 1, ex=9, n=n) == 1 and uni(wb=T + 1, aggs=None, n=n) == 1
        assert uni(wa=T, wb=T, aggs=None) == 3                              # the widest widths are not refused as widths
        # FL_ERR_INDEX: expr outside fl_expr, also for an empty column and in front of the NULL checks
        for n in (1, 0):
            for ex in (-1, 3, 99):
                assert uni(ex=ex, n=n) == 2 and mix(ex=ex, n=n) == 2
        assert uni(ex=3, aggs=None) == 2 and mix(ex=-1, a=None) == 2
        for ex in (MUL, ADD, SUB):
            for mk in (MK, None):                                           # mask == NULL is accepted: the refusal is the OTHER pointer's
                # n_blocks == 0: nothing to do, whatever the pointers
                assert f(ex, 3, None, None, 0, 5, None, None, 0, None, 0, None, None, None) == 0
                assert g(ex, None, None, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, None, None, None) == 0
                # FL_ERR_NULL: each required pointer of both columns, and the slots
                for name in ("a", "ar", "b", "br", "aggs"):
                    assert uni(**{name: None}, ex=ex, mk=mk) == 3, (ty, name)
                for name in ("aw", "ao", "a", "ar", "bw", "bo", "b", "br", "aggs"):
                    assert mix(**{name: None}, ex=ex, mk=mk) == 3, (ty, name)
                # FL_ERR_ALIGN: either packed column and the slots at + 8 bytes (so a NULL mask got past the NULL checks)
                for name, at in (("a", A), ("b", B), ("aggs", G)):
                    assert uni(**{name: at + 8}, ex=ex, mk=mk) == 4 and mix(**{name: at + 8}, ex=ex, mk=mk) == 4, (ty, name)
                assert uni(a=None, b=B + 8, ex=ex, mk=mk) == 3              # NULL is answered before alignment
            assert uni(ex=ex, mk=MK + 4) == 4 and mix(ex=ex, mk=MK + 8) == 4   # ... and the mask
        # a column's packed pointer may be NULL only when no byte of it can be read: width 0 / no packed bytes are accepted as far as
        # the next refusal (here: the misaligned slots); with bytes to read it is required
        assert uni(wa=0, a=None, aggs=G + 8) == 4 and uni(wb=0, b=None, aggs=G + 8) == 4 and uni(wa=0, a=None, wb=0, b=None, aggs=G + 8) == 4
        assert mix(a=None, ab=0, aggs=G + 8) == 4 and mix(b=None, bb=0, aggs=G + 8) == 4 and mix(a=None, ab=0, b=None, bb=0, aggs=G + 8) == 4
        assert mix(a=None) == 3 and mix(b=None) == 3 and uni(wa=1, a=None) == 3 and uni(wb=1, b=None) == 3


def test_python_forms_refuse_before_loading_anything():
    import torch
    import fastlanes_amd as fl
    w, o = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    w2, o2 = np.zeros(2, np.uint8), np.zeros(2, np.uint64)
    col, ref = np.zeros(96, np.uint32), np.zeros(1, np.uint32)
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    # device tier only: host (numpy) input and CPU tensors
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_columns(3, col, 0, "*", 3, col, 0)
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_columns(3, tcol, 0, "*", 3, tcol, 0)
    with pytest.raises(TypeError):
        fl.unfor_aggregate_columns_widths(w, o, col, ref, "*", w, o, col, ref)
    with pytest.raises(TypeError):
        fl.unfor_aggregate_columns_widths(tw, to, tcol, tref, "*", tw, to, tcol, tref)
    # unequal block counts: 96 u32 at width 3 are one block, 192 are two; one width per block
    with pytest.raises(ValueError, match="blocks"):
        fl.FoR.unfor_aggregate_columns(3, col, 0, "*", 3, np.zeros(192, np.uint32), 0)
    with pytest.raises(ValueError, match="blocks"):
        fl.FoR.unfor_aggregate_columns(0, np.zeros(0, np.uint32), 0, "*", 3, col, 0, n_blocks=2)
    with pytest.raises(ValueError, match="blocks"):
        fl.unfor_aggregate_columns_widths(w, o, col, ref, "*", w2, o2, col, ref)
    # mixed element types
    with pytest.raises(TypeError, match="one element type"):
        fl.FoR.unfor_aggregate_columns(3, col, 0, "*", 3, np.zeros(96, np.uint16), 0)
    with pytest.raises(TypeError, match="one element type"):
        fl.unfor_aggregate_columns_widths(w, o, col, ref, "*", w, o, np.zeros(96, np.uint64), np.zeros(1, np.uint64))
    # an unknown expr, in front of everything else
    for bad in ("/", "**", "mul", 0, None, "<"):
        with pytest.raises(ValueError, match="expr"):
            fl.FoR.unfor_aggregate_columns(3, col, 0, bad, 3, col, 0)
        with pytest.raises(ValueError, match="expr"):
            fl.unfor_aggregate_columns_widths(w, o, col, ref, bad, w, o, col, ref)
    assert fl.FoR.EXPR == {"*": MUL, "+": ADD, "-": SUB}
    # a width > T of either column: FL_ERR_WIDTH, as the library answers
    for wa, wb in ((33, 3), (3, 33)):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.FoR.unfor_aggregate_columns(wa, col, 0, "*", wb, col, 0)
        assert ei.value.status == 1


SHIM = r"""
#include "fl_expr_map.hpp"
#include <stddef.h>
extern "C" void expr_apply_n(int expr, size_t n, const uint64_t* x, const uint64_t* y, uint64_t* out)
{
    for (size_t i = 0; i < n; ++i) out[i] = fl::expr_apply(expr, x[i], y[i]);
}
extern "C" int expr_valid_of(int expr) { return fl::expr_valid(expr) ? 1 : 0; }
extern "C" int expr_route_of(unsigned count, unsigned wa, unsigned wb) { return (int)fl::expr_route(count, wa, wb); }
extern "C" void expr_constant_block_of(int expr, unsigned count, uint64_t ra, uint64_t rb, uint64_t* out)
{
    const fl::BlockAggregate g = fl::expr_constant_block(expr, count, ra, rb);
    out[0] = g.count; out[1] = g.sum; out[2] = g.min; out[3] = g.max;
}
extern "C" int expr_enum_values() { return fl::EXPR_MUL | fl::EXPR_ADD << 4 | fl::EXPR_SUB << 8; }
extern "C" int expr_route_values()
{
    return fl::EXPR_IDENTITY | fl::EXPR_CONSTANT << 4 | fl::EXPR_DECODE_A << 8 | fl::EXPR_DECODE_B << 12 | fl::EXPR_DECODE_BOTH << 16;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "expr_map", SHIM)
    P = ctypes.c_void_p
    so.expr_apply_n.argtypes = [ctypes.c_int, ctypes.c_size_t, P, P, P]
    so.expr_apply_n.restype = None
    so.expr_route_of.argtypes = [ctypes.c_uint] * 3
    so.expr_constant_block_of.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_uint64, ctypes.c_uint64, P]
    so.expr_constant_block_of.restype = None
    return so


def corners(T):
    return [0, 1, 2, 2 ** (T - 1) - 1, 2 ** (T - 1), 2 ** (T - 1) + 1, 2 ** T - 2, 2 ** T - 1]


def test_header_compiles_without_hip_and_matches_the_public_enum(shim):
    assert shim.expr_enum_values() == MUL | ADD << 4 | SUB << 8
    assert shim.expr_route_values() == ROUTE_IDENTITY | ROUTE_CONSTANT << 4 | ROUTE_A << 8 | ROUTE_B << 12 | ROUTE_BOTH << 16
    assert [shim.expr_valid_of(e) for e in (-1, 0, 1, 2, 3, 99)] == [0, 1, 1, 1, 0, 0]


@pytest.mark.parametrize("ty", list(TYPE_BITS))
def test_expr_apply_at_the_corners_of_every_type(shim, ty):
    """every pair of corner values of the type, zero-extended, under the three ops, against Python integers mod 2^64: products and
    sums of u8 / u16 / u32 are exact (below 2^64), u64 wraps, a - b with a < b is the two's-complement pattern"""
    T = TYPE_BITS[ty]
    c = corners(T)
    assert {0, 1, 2 ** (T - 1), 2 ** T - 1} <= set(c)
    xs = np.array([x for x in c for _ in c], dtype=np.uint64)
    ys = np.array([y for _ in c for y in c], dtype=np.uint64)
    for ex in (MUL, ADD, SUB):
        out = np.empty(xs.size, np.uint64)
        shim.expr_apply_n(ex, xs.size, xs.ctypes.data, ys.ctypes.data, out.ctypes.data)
        exact = wrapped = below = 0
        for x, y, got in zip(xs.tolist(), ys.tolist(), out.tolist()):
            true = {MUL: x * y, ADD: x + y, SUB: x - y}[ex]
            assert got == PY[ex](x, y) == true % M64, (ty, ex, x, y)
            exact += 0 <= true < M64
            wrapped += true >= M64
            below += true < 0
            if ex == SUB and x < y and T < 64:                             # (a u64 difference need not fit int64: it wraps)
                assert got >= 2 ** 63 and got - M64 == x - y                # the pattern of the negative difference, read as int64
            if T < 64 and ex != SUB:
                assert got == true                                          # widened BEFORE the operation: nothing is lost
        assert exact > 0
        assert (wrapped > 0) == (T == 64 and ex != SUB), (ty, ex)           # only u64 products and sums wrap
        assert (below > 0) == (ex == SUB)                                   # pairs with a < b occur under SUB


def test_route_table(shim):
    """(count = 0 / > 0) x (wa = 0 / > 0) x (wb = 0 / > 0): an empty mask reads nothing whatever the widths, two width-0 sides are a
    constant, one width-0 side is never fetched"""
    for wa in (0, 1, 7, 64):
        for wb in (0, 1, 7, 64):
            assert shim.expr_route_of(0, wa, wb) == ROUTE_IDENTITY
            for count in (1, 5, 1024):
                want = ROUTE_CONSTANT if wa == 0 and wb == 0 else ROUTE_A if wb == 0 else ROUTE_B if wa == 0 else ROUTE_BOTH
                assert shim.expr_route_of(count, wa, wb) == want, (count, wa, wb)
    assert {shim.expr_route_of(c, wa, wb) for c in (0, 3) for wa in (0, 9) for wb in (0, 9)} == set(range(5))


def test_constant_block(shim):
    """count rows of ra o rb: {count, count * (ra o rb) mod 2^64, ra o rb, ra o rb}; no rows: the identity"""
    out = np.empty(4, np.uint64)
    refs = [0, 1, 255, 65535, 2 ** 32 - 1, 2 ** 63, M64 - 1, 0x123456789ABCDEF]
    seen_wrap = False
    for ex in (MUL, ADD, SUB):
        for ra in refs:
            for rb in refs:
                v = PY[ex](ra, rb)
                for count in (0, 1, 2, 1023, 1024):
                    shim.expr_constant_block_of(ex, count, ra, rb, out.ctypes.data)
                    want = IDENTITY if count == 0 else (count, (count * v) % M64, v, v)
                    assert tuple(out.tolist()) == want, (ex, ra, rb, count)
                    seen_wrap |= count * v >= M64
    assert seen_wrap


def test_cpp_mirror_declares_both_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the two new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint16_t;
void (*const uniform)(fl_expr, std::size_t, const T*, const T*, std::size_t, std::size_t, const T*, const T*, std::size_t, const std::uint32_t*,
                      std::size_t, fl_block_aggregate*, std::uint32_t*, void*) = &fastlanes::FoR<T>::unfor_aggregate_columns_device;
void (*const mixed)(fl_expr, const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const std::uint8_t*,
                    const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const std::uint32_t*, std::size_t,
                    fl_block_aggregate*, std::uint32_t*, void*) = &fastlanes::unfor_aggregate_columns_widths_device<T>;
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
