"""CPU: unfor_compare_columns / unfor_compare_columns_widths (a <op> b between two FoR-packed columns of one element type, chained
through a mask) -- the header declares and the library exports them for every element type through a macro of their own, the Python
table agrees with the header, every refusal needs no GPU, the Python mirror validates before any launch, and the decision rule the
kernel and the host share (fastlanes_amd/csrc/fl_columns_decide.hpp, compiled here with g++) is EXACT: exhaustively at a 4-bit model
type against brute force over every value pair, and on a seeded sample of the real widths against a big-integer restatement."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)
from columns_data import ALL, EACH, NONE, OPS, PY, columns_verdict

FORMS = ("unfor_compare_columns", "unfor_compare_columns_widths")
NEW, AND, OR = 0, 1, 2


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
    body = text.split("#define FL_DECLARE_FOR_COMPARE_COLUMNS(T, S)")[1].split("FL_DECLARE_FOR_COMPARE_COLUMNS(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_FOR_COMPARE_COLUMNS({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.for_compare_columns_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.select_symbols(),
                  fastlanes_amd.aggregate_symbols(), fastlanes_amd.for_compare_range_symbols(), fastlanes_amd.aggregate_by_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"for_compare_columns_symbols", "unfor_compare_columns_widths"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.FoR, "unfor_compare_columns")


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: a pointer is c_void_p, `unsigned` c_uint, size_t c_size_t, int c_int"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("FOR_COMPARE_COLUMNS")}
    assert len(rows) == 8
    names = {FORMS[0]: "width_a a a_references a_reference_stride width_b b b_references b_reference_stride op is_signed combine mask_in "
                       "n_blocks mask stream",
             FORMS[1]: "a_widths a_offsets a_packed a_packed_bytes a_references a_reference_stride b_widths b_offsets b_packed "
                       "b_packed_bytes b_references b_reference_stride op is_signed combine mask_in n_blocks mask err_flag stream"}
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
            assert getattr(lib, name).argtypes == argtypes


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), in the order of unfor_compare_range: either width, op /
    combine, the empty column, mask_in, the other pointers, alignment."""
    buf = np.zeros(8192, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    A, AR, B, BR, MI, M, AW, AO, BW, BO = (p + 4096 * i for i in range(10))
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_compare_columns")
        g = getattr(lib, f"fl_{ty}_unfor_compare_columns_widths")

        def uni(wa=3, a=A, ar=AR, wb=5, b=B, br=BR, op=2, sg=0, cb=NEW, mi=MI, n=1, m=M):
            return f(wa, a, ar, 1, wb, b, br, 1, op, sg, cb, mi, n, m, None)

        def mix(aw=AW, ao=AO, a=A, ab=384, ar=AR, bw=BW, bo=BO, b=B, bb=384, br=BR, op=2, sg=0, cb=NEW, mi=MI, n=1, m=M):
            return g(aw, ao, a, ab, ar, 1, bw, bo, b, bb, br, 1, op, sg, cb, mi, n, m, None, None)

        # FL_ERR_WIDTH: either width, also for an empty column and in front of every other refusal
        for n in (1, 0):
            assert uni(wa=T + 1, n=n) == 1 and uni(wb=T + 1, n=n) == 1 and uni(wa=T + 1, wb=T + 1, n=n) == 1
            assert uni(wa=T + 1, op=9, n=n) == 1 and uni(wb=T + 1, cb=7, n=n) == 1 and uni(wb=T + 1, m=None, n=n) == 1
        assert uni(wa=T, wb=T, m=None) == 3                                 # the widest widths are not refused as widths
        # FL_ERR_INDEX: op outside fl_cmp, combine outside fl_mask_combine, also for an empty column
        for n in (1, 0):
            for op in (-1, 6, 99):
                assert uni(op=op, n=n) == 2 and mix(op=op, n=n) == 2
            for cb in (-1, 3, 99):
                assert uni(cb=cb, n=n) == 2 and mix(cb=cb, n=n) == 2
        assert uni(op=6, m=None) == 2 and mix(cb=3, a=None) == 2            # ... in front of the NULL checks
        for sg in (0, 1):
            for cb in (NEW, AND, OR):
                # n_blocks == 0: nothing to do, whatever the pointers
                assert f(3, None, None, 0, 5, None, None, 0, 2, sg, cb, None, 0, None, None) == 0
                assert g(None, None, None, 0, None, 0, None, None, None, 0, None, 0, 2, sg, cb, None, 0, None, None, None) == 0
                # FL_ERR_NULL: each required pointer, under every combiner
                for name in ("a", "ar", "b", "br", "m"):
                    assert uni(**{name: None}, sg=sg, cb=cb) == 3, (ty, name)
                for name in ("aw", "ao", "a", "ar", "bw", "bo", "b", "br", "m"):
                    assert mix(**{name: None}, sg=sg, cb=cb) == 3, (ty, name)
                # FL_ERR_ALIGN: either packed column and the mask at + 8 bytes
                for name, at in (("a", A), ("b", B), ("m", M)):
                    assert uni(**{name: at + 8}, sg=sg, cb=cb) == 4 and mix(**{name: at + 8}, sg=sg, cb=cb) == 4, (ty, name)
                assert uni(a=None, b=B + 8, sg=sg, cb=cb) == 3              # NULL is answered before alignment
        # mask_in: required and aligned under AND / OR, ignored under NEW
        for cb in (AND, OR):
            assert uni(cb=cb, mi=None) == 3 and mix(cb=cb, mi=None) == 3
            assert uni(cb=cb, mi=MI + 4) == 4 and mix(cb=cb, mi=MI + 8) == 4
            assert uni(cb=cb, mi=None, m=M + 8) == 3                        # ... and answered before alignment
        assert uni(cb=NEW, mi=None, m=None) == 3 and uni(cb=NEW, mi=None, m=M + 8) == 4   # got past mask_in to the next refusal
        assert uni(cb=NEW, mi=MI + 4, m=M + 8) == 4 and mix(cb=NEW, mi=None, m=M + 8) == 4
        # a column's packed pointer may be NULL only when no byte of it can be read: width 0 / no packed bytes are accepted as far as
        # the next refusal (here: the misaligned mask); with bytes to read it is required
        assert uni(wa=0, a=None, m=M + 8) == 4 and uni(wb=0, b=None, m=M + 8) == 4 and uni(wa=0, a=None, wb=0, b=None, m=M + 8) == 4
        assert mix(a=None, ab=0, m=M + 8) == 4 and mix(b=None, bb=0, m=M + 8) == 4 and mix(a=None, ab=0, b=None, bb=0, m=M + 8) == 4
        assert mix(a=None) == 3 and mix(b=None) == 3 and uni(wa=1, a=None) == 3 and uni(wb=1, b=None) == 3


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    w, o = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref, tmask = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(32, dtype=torch.int32)
    # device tier only: numpy arrays and CPU tensors
    with pytest.raises(TypeError):
        fl.FoR.unfor_compare_columns(3, np.zeros(96, dtype=np.uint32), 0, "<", 3, np.zeros(96, dtype=np.uint32), 0)
    with pytest.raises(TypeError):
        fl.FoR.unfor_compare_columns(3, tcol, 0, "<", 3, tcol, 0)
    with pytest.raises(TypeError):
        fl.unfor_compare_columns_widths(w, o, np.zeros(96, np.uint32), np.zeros(1, np.uint32), "<", w, o, np.zeros(96, np.uint32), np.zeros(1, np.uint32))
    with pytest.raises(TypeError):
        fl.unfor_compare_columns_widths(tw, to, tcol, tref, "<", tw, to, tcol, tref)
    # a combine that is none of the three, and a combine without the mask so far
    for bad in ("xor", "AND", 1, None):
        with pytest.raises(ValueError):
            fl.FoR.unfor_compare_columns(3, tcol, 0, "<", 3, tcol, 0, mask=tmask, combine=bad)
        with pytest.raises(ValueError):
            fl.unfor_compare_columns_widths(tw, to, tcol, tref, "<", tw, to, tcol, tref, mask=tmask, combine=bad)
    for cb in ("and", "or"):
        with pytest.raises(ValueError):
            fl.FoR.unfor_compare_columns(3, tcol, 0, "<", 3, tcol, 0, combine=cb)
        with pytest.raises(ValueError):
            fl.unfor_compare_columns_widths(tw, to, tcol, tref, "<", tw, to, tcol, tref, combine=cb)
    # a mask that does not hold 32 words per block
    for words in (0, 31, 33, 64):
        with pytest.raises(ValueError):
            fl.unfor_compare_columns_widths(tw, to, tcol, tref, "<", tw, to, tcol, tref, mask=torch.zeros(words, dtype=torch.int32), combine="and")


SHIM = r"""
#include "fl_columns_decide.hpp"
#include <stddef.h>
// the array form: query i = (op[i], is_signed[i], ref_a[i], wa[i], ref_b[i], wb[i]) -> the verdict of the whole rule
extern "C" void columns_decide_n(unsigned type_bits, size_t n, const int* op, const uint8_t* is_signed, const uint64_t* ref_a, const uint8_t* wa,
                                 const uint64_t* ref_b, const uint8_t* wb, int* verdict)
{
    for (size_t i = 0; i < n; ++i) verdict[i] = fl::columns_decide(type_bits, op[i], is_signed[i] != 0, ref_a[i], wa[i], ref_b[i], wb[i]);
}
// the op reduction, applied to one value pair as the kernel applies it: invert ^ (swap ? base(y, x) : base(x, y))
extern "C" int columns_relation_holds(int op, uint64_t x, uint64_t y)
{
    const fl::ColumnsRelation r = fl::columns_relation(op);
    const uint64_t p = r.swap ? y : x, q = r.swap ? x : y;
    return (int)((r.is_eq ? p == q : p < q) != r.invert);
}
extern "C" int columns_relation_fields(int op) { const fl::ColumnsRelation r = fl::columns_relation(op); return r.is_eq | r.swap << 1 | r.invert << 2; }
extern "C" uint64_t columns_bias_of(unsigned type_bits, int is_signed) { return fl::columns_bias(type_bits, is_signed != 0); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "columns_decide", SHIM)
    P = ctypes.c_void_p
    so.columns_decide_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 7
    so.columns_decide_n.restype = None
    so.columns_relation_holds.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64]
    so.columns_bias_of.argtypes = [ctypes.c_uint, ctypes.c_int]
    so.columns_bias_of.restype = ctypes.c_uint64
    return so


def decide(shim, T, op, signed, ra, wa, rb, wb):
    op = np.array(op, dtype=np.int32)
    signed, wa, wb = (np.array(x, dtype=np.uint8) for x in (signed, wa, wb))
    ra, rb = (np.array(x, dtype=np.uint64) for x in (ra, rb))
    v = np.empty(op.size, np.int32)
    shim.columns_decide_n(T, op.size, *(x.ctypes.data for x in (op, signed, ra, wa, rb, wb, v)))
    return v


def test_op_reduction_returns_the_six_truth_tables(shim):
    """base relation + swap + invert, applied to value pairs around every edge of u64, is the op itself; == / != never swap"""
    M = 2 ** 64 - 1
    edge = [0, 1, 2, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, M - 1, M]
    for code, op in enumerate(OPS):
        for x in edge:
            for y in edge:
                assert shim.columns_relation_holds(code, x, y) == int(PY[op](x, y)), (op, x, y)
    fields = [shim.columns_relation_fields(code) for code in range(6)]
    assert fields == [1, 1 | 4, 0, 2 | 4, 2, 4]                            # is_eq | swap << 1 | invert << 2
    for T in (4, 8, 16, 32, 64):
        assert shim.columns_bias_of(T, 0) == 0 and shim.columns_bias_of(T, 1) == 1 << (T - 1)


def brute_force_verdict(T, op, signed, ra, wa, rb, wb):
    """from the definition: every value pair of the two blocks' ranges, compared in the order domain"""
    N = 1 << T
    bias = N >> 1 if signed else 0
    va = (ra + bias + np.arange(1 << wa)) % N
    vb = (rb + bias + np.arange(1 << wb)) % N
    hit = PY[op](va[:, None], vb[None, :])
    return ALL if hit.all() else NONE if not hit.any() else EACH


def test_decision_rule_is_exact_at_four_bits(shim):
    """every (r_a, W_a, r_b, W_b, op, signed) of a 4-bit model type: ALL iff every value pair satisfies the predicate, NONE iff none
    does -- the header's rule, and the restatement the GPU test and the sampled test below use"""
    T = 4
    q = [(op, sg, ra, wa, rb, wb) for op in range(6) for sg in (0, 1) for ra in range(16) for wa in range(T + 1) for rb in range(16)
         for wb in range(T + 1)]
    assert len(q) == 76800
    got = decide(shim, T, *([x[j] for x in q] for j in range(6)))
    seen = set()
    for i, (op, sg, ra, wa, rb, wb) in enumerate(q):
        want = brute_force_verdict(T, OPS[op], sg, ra, wa, rb, wb)
        assert int(got[i]) == want, ("header", OPS[op], sg, ra, wa, rb, wb, int(got[i]), want)
        assert columns_verdict(T, OPS[op], bool(sg), ra, wa, rb, wb) == want, ("restatement", OPS[op], sg, ra, wa, rb, wb)
        seen.add((op, want))
    assert seen == {(op, v) for op in range(6) for v in (EACH, ALL, NONE)}


@pytest.mark.parametrize("T", [8, 16, 32, 64])
def test_decision_rule_on_a_seeded_sample(shim, T):
    """at least 10^5 cases per width against the big-integer restatement: ranges that wrap, W = T, W = 0 on either and on both sides,
    references at 0, M, 2^(T-1) - 1 and 2^(T-1), and ranges that touch in exactly one value"""
    N = 1 << T
    M, H = N - 1, N >> 1
    rng = random.Random(12000 + T)                                         # Python integers: the bounds pass 2^63
    n = 100_800
    special = [0, M, H - 1, H]
    q = []
    counts = dict(wraps=0, full=0, zero_a=0, zero_b=0, zero_both=0, touch=0, special=0)
    for i in range(n):
        wa = [0, T, 1, T - 1][i % 7] if i % 7 < 4 else rng.randint(0, T)
        wb = [0, T, T // 2][(i // 7) % 5] if (i // 7) % 5 < 3 else rng.randint(0, T)
        ra = special[i % 4] if i % 3 == 0 else rng.randint(0, M)
        span_a, span_b = (1 << wa) - 1, (1 << wb) - 1
        kind = i % 11
        if kind == 0:
            rb = (ra + span_a) % N                                          # b starts at a's last value: they touch in one value
        elif kind == 1:
            rb = (ra - span_b) % N                                          # b ends at a's first value
        elif kind == 2:
            rb = (ra + span_a + 1) % N                                      # just apart
        elif kind == 3:
            rb = (ra - span_b - 1) % N
        elif kind == 4:
            rb = special[(i // 11) % 4]
        elif kind < 8:
            rb = (ra + rng.randint(-span_b - 2, span_a + 2)) % N      # overlapping or nearly
        else:
            rb = rng.randint(0, M)
        op, sg = i % 6, (i // 6) % 2
        bias = H if sg else 0
        counts["wraps"] += ((ra + bias) % N) + span_a > M or ((rb + bias) % N) + span_b > M
        counts["full"] += wa == T or wb == T
        counts["zero_a"] += wa == 0 and wb != 0
        counts["zero_b"] += wb == 0 and wa != 0
        counts["zero_both"] += wa == 0 and wb == 0
        counts["touch"] += kind in (0, 1) and 0 < wa < T and 0 < wb < T
        counts["special"] += ra in special or rb in special
        q.append((op, sg, ra, wa, rb, wb))
    assert len(q) >= 100_000 and all(c > 1000 for c in counts.values()), counts
    got = decide(shim, T, *([x[j] for x in q] for j in range(6)))
    seen = set()
    for i, (op, sg, ra, wa, rb, wb) in enumerate(q):
        want = columns_verdict(T, OPS[op], bool(sg), ra, wa, rb, wb)
        assert int(got[i]) == want, (T, OPS[op], sg, ra, wa, rb, wb, int(got[i]), want)
        seen.add((op, want))
    assert seen == {(op, v) for op in range(6) for v in (EACH, ALL, NONE)}


def test_cpp_mirror_declares_both_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the two new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint16_t;
void (*const uniform)(std::size_t, const T*, const T*, std::size_t, std::size_t, const T*, const T*, std::size_t, fl_cmp, bool, fl_mask_combine,
                      const std::uint32_t*, std::size_t, std::uint32_t*, void*) = &fastlanes::FoR<T>::unfor_compare_columns_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const std::uint8_t*,
                    const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, fl_cmp, bool, fl_mask_combine, const std::uint32_t*,
                    std::size_t, std::uint32_t*, std::uint32_t*, void*) = &fastlanes::unfor_compare_columns_widths_device<T>;
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
