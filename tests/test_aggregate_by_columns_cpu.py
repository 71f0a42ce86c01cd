"""CPU: unfor_aggregate_by_columns / unfor_aggregate_by_columns_widths (COUNT / SUM / MIN / MAX of a * b, a + b or a - b between two
FoR-packed columns of one element type, grouped by a FoR-packed u8 key column) -- the header declares and the library exports them for
every value type through a macro of their own, the Python table agrees with the header, every refusal needs no GPU, the Python forms
validate before anything is loaded, the route the kernel shares with the host (fastlanes_amd/csrc/fl_aggregate_by_columns_map.hpp,
compiled here with g++) is exhaustive, and the C++ mirror declares both forms."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)

FORMS = ("unfor_aggregate_by_columns", "unfor_aggregate_by_columns_widths")
MUL, ADD, SUB = 0, 1, 2
SKIP, ONE_KEY, DECODE = 0, 1, 2
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
    body = text.split("#define FL_DECLARE_AGGREGATE_BY_COLUMNS(T, S)")[1].split("FL_DECLARE_AGGREGATE_BY_COLUMNS(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_AGGREGATE_BY_COLUMNS({CT[ty]}, {ty})" in text
    doc = text.split("#define FL_DECLARE_AGGREGATE_BY_COLUMNS(T, S)")[0].rsplit("/*", 1)[1]
    assert "UNSIGNED" in doc and "two's-complement" in doc and "c * SUM(a) - SUM(a * b)" in doc
    for scope in ("keys wider than u8", "a second key column", "more than one expression per launch", "three-column products",
                  "constants inside", "signed (sign-extending) columns", "Delta columns", "the host tier"):
        assert scope in doc.split("Out of scope:")[1], scope
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.aggregate_by_columns_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.select_symbols(),
                  fastlanes_amd.aggregate_symbols(), fastlanes_amd.for_compare_range_symbols(), fastlanes_amd.aggregate_by_symbols(),
                  fastlanes_amd.for_compare_columns_symbols(), fastlanes_amd.aggregate_columns_symbols(), fastlanes_amd.for_compare_in_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"aggregate_by_columns_symbols", "unfor_aggregate_by_columns_widths"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.FoR, "unfor_aggregate_by_columns")


def test_build_checks_the_new_symbol_list():
    assert "aggregate_by_columns_symbols()" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: a pointer is c_void_p, `unsigned` c_uint, size_t c_size_t, int c_int; `expr`
    and the two value columns as unfor_aggregate_columns has them, the key column and the tail as unfor_aggregate_by"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("AGGREGATE_BY_COLUMNS")}
    assert len(rows) == 8
    for ty in TYPE_BITS:
        for form, columns, by in zip(FORMS, ("unfor_aggregate_columns", "unfor_aggregate_columns_widths"),
                                     ("unfor_aggregate_by", "unfor_aggregate_by_widths")):
            name = f"fl_{ty}_{form}"
            ret, args = protos[name]
            restype, argtypes = rows[name]
            assert ret == "int" and restype is ctypes.c_int
            lead = [a for _, a in protos[f"fl_{ty}_{columns}"][1]]
            lead = lead[:lead.index("mask")]                                # expr, column a, column b
            tail = [a for _, a in protos[f"fl_{ty}_{by}"][1]]
            tail = tail[tail.index("key_width" if form == FORMS[0] else "key_widths"):]   # the key column, mask, n_blocks, result, err_flag, stream
            assert [a for _, a in args] == lead + tail, name
            assert len(args) == len(argtypes) == (18 if form == FORMS[0] else 24), name
            for (ctype, arg), at in zip(args, argtypes):
                want = ctypes.c_void_p if "*" in ctype else {"unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "int": ctypes.c_int}[ctype]
                assert at is want, (name, arg, ctype)
            types = dict((a, c) for c, a in args)
            for col in ("a", "b"):                                         # both value columns are of the element type, the keys u8
                assert types[f"{col}_references"] == f"const {CT[ty]} *"
                assert types[col if form == FORMS[0] else f"{col}_packed"] == f"const {CT[ty]} *"
            assert types["keys"] == "const uint8_t *" and types["key_references"] == "const uint8_t *"
            assert types["result"] == "void *" and types["mask"] == "const uint32_t *" and types["expr"] == "int"
            assert getattr(lib, name).argtypes == argtypes


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before any device call (no call here reaches a kernel), in the parents' order: the three widths -- also
    for an empty column -- then expr, then NULL (`result` also for an empty column: every call writes it), then alignment."""
    buf = np.zeros(16 * 512, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    A, AR, B, BR, K, KR, MK, RES, AW, AO, BW, BO, KW, KO = (p + 4096 * i for i in range(14))
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_aggregate_by_columns")
        g = getattr(lib, f"fl_{ty}_unfor_aggregate_by_columns_widths")

        def uni(ex=MUL, wa=3, a=A, ar=AR, wb=5, b=B, br=BR, kw=3, k=K, kr=KR, mk=MK, n=1, res=RES):
            return f(ex, wa, a, ar, 1, wb, b, br, 1, kw, k, kr, 1, mk, n, res, None, None)

        def mix(ex=MUL, aw=AW, ao=AO, a=A, ab=384, ar=AR, bw=BW, bo=BO, b=B, bb=384, br=BR, kw=KW, ko=KO, k=K, kb=384, kr=KR, mk=MK, n=1,
                res=RES):
            return g(ex, aw, ao, a, ab, ar, 1, bw, bo, b, bb, br, 1, kw, ko, k, kb, kr, 1, mk, n, res, None, None)

        # FL_ERR_WIDTH: each of the three widths, also for an empty column and in front of every other refusal
        for n in (1, 0):
            assert uni(wa=T + 1, n=n) == 1 and uni(wb=T + 1, n=n) == 1 and uni(kw=9, n=n) == 1 and uni(wa=T + 1, wb=T + 1, kw=9, n=n) == 1
            assert uni(wa=T + 1, ex=9, n=n) == 1 and uni(wb=T + 1, res=None, n=n) == 1 and uni(kw=9, ex=-1, res=None, n=n) == 1
        assert uni(kw=9, k=K + 8) == 1
        assert uni(wa=T, wb=T, kw=8, res=None) == 3                        # the widest widths are not refused as widths
        # FL_ERR_INDEX: expr outside fl_expr, also for an empty column and in front of the NULL checks
        for n in (1, 0):
            for ex in (-1, 3, 99):
                assert uni(ex=ex, n=n) == 2 and mix(ex=ex, n=n) == 2
        assert uni(ex=3, res=None) == 2 and mix(ex=-1, a=None) == 2 and mix(ex=3, res=None, n=0) == 2
        for ex in (MUL, ADD, SUB):
            for mk in (MK, None):                                           # mask == NULL is accepted: the refusal is the OTHER pointer's
                # FL_ERR_NULL: each required pointer of the three columns; `result` also for an empty column
                for name in ("a", "ar", "b", "br", "k", "kr", "res"):
                    assert uni(**{name: None}, ex=ex, mk=mk) == 3, (ty, name)
                for name in ("aw", "ao", "a", "ar", "bw", "bo", "b", "br", "kw", "ko", "k", "kr", "res"):
                    assert mix(**{name: None}, ex=ex, mk=mk) == 3, (ty, name)
                assert uni(res=None, n=0, ex=ex, mk=mk) == 3 and mix(res=None, n=0, ex=ex, mk=mk) == 3
                # FL_ERR_ALIGN: each packed column, the keys and the result at + 8 bytes (so a NULL mask got past the NULL checks)
                for name, at in (("a", A), ("b", B), ("k", K), ("res", RES)):
                    assert uni(**{name: at + 8}, ex=ex, mk=mk) == 4 and mix(**{name: at + 8}, ex=ex, mk=mk) == 4, (ty, name)
                assert uni(res=RES + 8, n=0, ex=ex, mk=mk) == 4 and mix(res=RES + 8, n=0, ex=ex, mk=mk) == 4
                assert uni(a=None, b=B + 8, ex=ex, mk=mk) == 3 and uni(k=None, res=RES + 8, ex=ex, mk=mk) == 3   # NULL is answered before alignment
            assert uni(ex=ex, mk=MK + 4) == 4 and mix(ex=ex, mk=MK + 8) == 4   # ... and the mask
        # an empty column looks at `result` alone: the other pointers may be anything (here: misaligned)
        assert uni(a=A + 8, b=B + 8, k=K + 8, mk=MK + 8, n=0, res=RES + 8) == 4
        # a packed pointer may be NULL only when no byte of it can be read: width 0 / no packed bytes are accepted as far as the next
        # refusal (here: the misaligned result); with bytes to read it is required
        assert uni(wa=0, a=None, res=RES + 8) == 4 and uni(wb=0, b=None, res=RES + 8) == 4 and uni(kw=0, k=None, res=RES + 8) == 4
        assert uni(wa=0, a=None, wb=0, b=None, kw=0, k=None, res=RES + 8) == 4
        assert mix(a=None, ab=0, res=RES + 8) == 4 and mix(b=None, bb=0, res=RES + 8) == 4 and mix(k=None, kb=0, res=RES + 8) == 4
        assert mix(a=None) == 3 and mix(b=None) == 3 and mix(k=None) == 3
        assert uni(wa=1, a=None) == 3 and uni(wb=1, b=None) == 3 and uni(kw=1, k=None) == 3


def test_python_forms_refuse_before_loading_anything():
    import torch
    import fastlanes_amd as fl
    w, o = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    w2, o2 = np.zeros(2, np.uint8), np.zeros(2, np.uint64)
    col, ref = np.zeros(96, np.uint32), np.zeros(1, np.uint32)
    keys, kref = np.zeros(384, np.uint8), np.zeros(1, np.uint8)
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    tkeys = torch.zeros(384, dtype=torch.uint8)
    # device tier only: host (numpy) input and CPU tensors
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by_columns(3, col, 0, "*", 3, col, 0, 3, keys, 0)
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by_columns(3, tcol, 0, "*", 3, tcol, 0, 3, tkeys, 0)
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_columns_widths(w, o, col, ref, "*", w, o, col, ref, w, o, keys, kref)
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_columns_widths(tw, to, tcol, tref, "*", tw, to, tcol, tref, tw, to, tkeys, tw)
    # unequal block counts: 96 u32 at width 3 are one block, 192 are two; 384 key bytes at width 3 are one block; one width per block
    with pytest.raises(ValueError, match="blocks"):
        fl.FoR.unfor_aggregate_by_columns(3, col, 0, "*", 3, np.zeros(192, np.uint32), 0, 3, keys, 0)
    with pytest.raises(ValueError, match="blocks"):
        fl.FoR.unfor_aggregate_by_columns(3, col, 0, "*", 3, col, 0, 3, np.zeros(768, np.uint8), 0)
    with pytest.raises(ValueError, match="blocks"):
        fl.FoR.unfor_aggregate_by_columns(0, np.zeros(0, np.uint32), 0, "*", 0, np.zeros(0, np.uint32), 0, 3, keys, 0, n_blocks=2)
    with pytest.raises(ValueError, match="blocks"):
        fl.unfor_aggregate_by_columns_widths(w, o, col, ref, "*", w2, o2, col, ref, w, o, keys, kref)
    with pytest.raises(ValueError, match="blocks"):
        fl.unfor_aggregate_by_columns_widths(w, o, col, ref, "*", w, o, col, ref, w2, o2, keys, kref)
    # mixed element types
    with pytest.raises(TypeError, match="one element type"):
        fl.FoR.unfor_aggregate_by_columns(3, col, 0, "*", 3, np.zeros(96, np.uint16), 0, 3, keys, 0)
    with pytest.raises(TypeError, match="one element type"):
        fl.unfor_aggregate_by_columns_widths(w, o, col, ref, "*", w, o, np.zeros(96, np.uint64), np.zeros(1, np.uint64), w, o, keys, kref)
    # an unknown expr, in front of everything else
    for bad in ("/", "**", "mul", 0, None, "<"):
        with pytest.raises(ValueError, match="expr"):
            fl.FoR.unfor_aggregate_by_columns(3, col, 0, bad, 3, col, 0, 3, keys, 0)
        with pytest.raises(ValueError, match="expr"):
            fl.unfor_aggregate_by_columns_widths(w, o, col, ref, bad, w2, o2, col, ref, w, o, keys, kref)
    assert fl.FoR.EXPR == {"*": MUL, "+": ADD, "-": SUB}
    # a width > T of a value column or > 8 of the key column: FL_ERR_WIDTH, as the library answers
    for wa, wb, kw in ((33, 3, 3), (3, 33, 3), (3, 3, 9)):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.FoR.unfor_aggregate_by_columns(wa, col, 0, "*", wb, col, 0, kw, keys, 0)
        assert ei.value.status == 1


SHIM = r"""
#include "fl_aggregate_by_columns_map.hpp"
extern "C" int route_by(int mask_empty, int ok, unsigned kw, unsigned wa, unsigned wb)
{
    return (int)fl::aggregate_by_columns_route(mask_empty != 0, ok != 0, kw, wa, wb).by;
}
extern "C" int route_expr(int mask_empty, int ok, unsigned kw, unsigned wa, unsigned wb)
{
    return (int)fl::aggregate_by_columns_route(mask_empty != 0, ok != 0, kw, wa, wb).expr;
}
extern "C" int route_reads(int mask_empty, int ok, unsigned kw, unsigned wa, unsigned wb)
{
    const fl::AggregateByColumnsRoute r = fl::aggregate_by_columns_route(mask_empty != 0, ok != 0, kw, wa, wb);
    return (fl::aggregate_by_columns_reads_keys(r) ? 1 : 0) | (fl::aggregate_by_columns_reads_a(r) ? 2 : 0) | (fl::aggregate_by_columns_reads_b(r) ? 4 : 0);
}
extern "C" int parents_by(int mask_empty, int ok, unsigned kw) { return (int)fl::aggregate_by_route(mask_empty != 0, ok != 0, kw); }
extern "C" int parents_expr(unsigned count, unsigned wa, unsigned wb) { return (int)fl::expr_route(count, wa, wb); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory, "aggregate_by_columns_map", SHIM)


def test_route_is_exhaustive(shim):
    """(mask empty?, the three checks ok?, key width 0..8, wa in {0, 1, T}, wb in {0, 1, T}) -> the route, its expression sub-route
    and which of the three columns it requests bytes of; written out here, and equal to the two parents' rules composed"""
    seen = set()
    for T in TYPE_BITS.values():
        for empty in (0, 1):
            for ok in (0, 1):
                for kw in range(9):
                    for wa in (0, 1, T):
                        for wb in (0, 1, T):
                            at = (empty, ok, kw, wa, wb)
                            by, ex, reads = shim.route_by(*at), shim.route_expr(*at), shim.route_reads(*at)
                            want = SKIP if empty or not ok else ONE_KEY if kw == 0 else DECODE
                            assert by == want == shim.parents_by(empty, ok, kw), at
                            if want == SKIP:
                                assert ex == ROUTE_IDENTITY and reads == 0, at       # nothing is read, nothing is contributed
                                continue
                            want_ex = ROUTE_CONSTANT if wa == 0 and wb == 0 else ROUTE_A if wb == 0 else ROUTE_B if wa == 0 else ROUTE_BOTH
                            assert ex == want_ex == shim.parents_expr(1, wa, wb), at
                            assert reads == (1 if want == DECODE else 0) | (2 if wa else 0) | (4 if wb else 0), at
                            seen.add((by, ex))
    assert seen == {(by, ex) for by in (ONE_KEY, DECODE) for ex in (ROUTE_CONSTANT, ROUTE_A, ROUTE_B, ROUTE_BOTH)}


def test_map_header_has_no_hip_dependency_and_restates_neither_parent():
    text = open(os.path.join(ROOT, "fastlanes_amd", "csrc", "fl_aggregate_by_columns_map.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in code.lower() and "__device__" not in code
    assert "aggregate_by_route(" in code and "expr_route(" in code and "aggregate_by_reads_keys(" in code
    assert '#include "fl_aggregate_by_map.hpp"' in code and '#include "fl_expr_map.hpp"' in code
    assert "key_width == 0" not in code and "wa == 0" not in code          # the parents' conditions are called, not copied


def test_cpp_mirror_declares_both_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the two new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint16_t;
using K = std::uint8_t;
void (*const uniform)(fl_expr, std::size_t, const T*, const T*, std::size_t, std::size_t, const T*, const T*, std::size_t, std::size_t, const K*,
                      const K*, std::size_t, const std::uint32_t*, std::size_t, fl_block_aggregate*, std::uint32_t*, void*)
    = &fastlanes::FoR<T>::unfor_aggregate_by_columns_device;
void (*const mixed)(fl_expr, const K*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const K*, const std::uint64_t*,
                    const T*, std::size_t, const T*, std::size_t, const K*, const std::uint64_t*, const K*, std::size_t, const K*, std::size_t,
                    const std::uint32_t*, std::size_t, fl_block_aggregate*, std::uint32_t*, void*)
    = &fastlanes::unfor_aggregate_by_columns_widths_device<T>;
auto abi_uniform = fastlanes::detail::Abi<T>::unfor_aggregate_by_columns;
auto abi_mixed = fastlanes::detail::Abi<T>::unfor_aggregate_by_columns_widths;
int main() { return uniform && mixed && abi_uniform && abi_mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
