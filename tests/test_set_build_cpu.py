"""CPU: unfor_set_build / unfor_set_build_widths (the member set of the values a mask keeps of a FoR-packed column, ORed into a window's
bitmap: the build side of unfor_compare_in) -- the header declares and the library exports them for every element type through a macro
of their own, the Python table agrees with the header, every refusal needs no GPU and is unfor_compare_in's, fl.column_window agrees
with a numpy enumeration, and the block decisions the kernel and the host share (fastlanes_amd/csrc/fl_set_build_map.hpp, compiled
here with g++) are SOUND: exhaustively at a 4-bit model type against brute force over the values a block can hold, and on a seeded
sample of the real types against a restatement in Python integers."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)

FORMS = ("unfor_set_build", "unfor_set_build_widths")
SKIP, OUTSIDE, ONE_BIT, EACH = 0, 1, 2, 3


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
    body = text.split("#define FL_DECLARE_SET_BUILD(T, S)")[1].split("FL_DECLARE_SET_BUILD(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_SET_BUILD({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.set_build_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_in_symbols(), fastlanes_amd.aggregate_by_columns_symbols(),
                  fastlanes_amd.aggregate_by_symbols(), fastlanes_amd.select_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"set_build_symbols", "unfor_set_build_widths", "column_window"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.FoR, "unfor_set_build")


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: a pointer is c_void_p, `unsigned` c_uint, size_t c_size_t, uint64_t
    c_uint64, the element type its own scalar; the column's arguments are unfor_compare_in's"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("SET_BUILD")}
    assert len(rows) == 8
    for ty in TYPE_BITS:
        for form in FORMS:
            name = f"fl_{ty}_{form}"
            ret, args = protos[name]
            restype, argtypes = rows[name]
            assert ret == "int" and restype is ctypes.c_int
            in_args = [a for _, a in protos[name.replace("set_build", "compare_in")][1]]
            head = in_args[:in_args.index("set_lo")]
            tail = ["stream"] if form == "unfor_set_build" else ["err_flag", "stream"]
            assert [a for _, a in args] == head + ["mask", "n_blocks", "set_lo", "set_bits", "set_words", "stats"] + tail, name
            assert len(args) == len(argtypes), name
            scalars = {"unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64, CT[ty]: _lib.CTYPE[ty]}
            for (ctype, arg), at in zip(args, argtypes):
                assert at is (ctypes.c_void_p if "*" in ctype else scalars[ctype]), (name, arg, ctype)
            types = dict((a, c) for c, a in args)
            assert types["set_lo"] == CT[ty] and types["set_bits"] == "uint64_t" and types["set_words"] == "uint32_t *"
            assert types["stats"] == "uint64_t *" and types["mask"] == "const uint32_t *"
            assert getattr(lib, name).argtypes == argtypes


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), with unfor_compare_in's statuses for the same faults:
    the width; set_bits above min(2^T, 2^32) (FL_ERR_INDEX); the empty column; set_words and the column's pointers (FL_ERR_NULL);
    alignment, set_words and stats included.  mask and stats may be NULL."""
    buf = np.zeros(8192, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    A, AR, MK, SW, W, O, ST = (p + 4096 * i for i in range(7))
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_set_build")
        g = getattr(lib, f"fl_{ty}_unfor_set_build_widths")
        top = min(1 << T, 1 << 32)

        def uni(w=3, a=A, ar=AR, mk=MK, n=1, lo=5, sb=40, sw=SW, st=ST):
            return f(w, a, ar, 1, mk, n, lo, sb, sw, st, None)

        def mix(w=W, o=O, a=A, ab=384, ar=AR, mk=MK, n=1, lo=5, sb=40, sw=SW, st=ST):
            return g(w, o, a, ab, ar, 1, mk, n, lo, sb, sw, st, None, None)

        # FL_ERR_WIDTH: also for an empty column and in front of every other refusal
        for n in (1, 0):
            assert uni(w=T + 1, n=n) == 1 and uni(w=T + 1, sb=top + 1, n=n) == 1 and uni(w=T + 1, sw=None, n=n) == 1
        assert uni(w=T, sw=None) == 3                                       # the widest width is not refused as a width
        # FL_ERR_INDEX: set_bits above min(2^T, 2^32); also for an empty column, and in front of the NULL checks
        for n in (1, 0):
            for sb in (top + 1, top + 32, 1 << 33, 2 ** 64 - 1):
                assert uni(sb=sb, n=n) == 2 and mix(sb=sb, n=n) == 2, (ty, sb)
        assert uni(sb=top + 1, sw=None) == 2 and mix(sb=top + 1, a=None) == 2
        assert uni(sb=top, sw=None) == 3 and mix(sb=top, sw=None) == 3      # the largest window is not refused
        # n_blocks == 0: nothing to do, whatever the pointers
        assert f(3, None, None, 0, None, 0, 5, 40, None, None, None) == 0
        assert g(None, None, None, 0, None, 0, None, 0, 5, 40, None, None, None, None) == 0
        # FL_ERR_NULL: each required pointer; set_words with set_bits > 0
        for name in ("a", "ar", "sw"):
            assert uni(**{name: None}) == 3, (ty, name)
        for name in ("w", "o", "a", "ar", "sw"):
            assert mix(**{name: None}) == 3, (ty, name)
        # FL_ERR_ALIGN: the packed column, the mask, set_words and stats off a 16-byte boundary
        for name, at in (("a", A), ("mk", MK), ("sw", SW), ("st", ST)):
            for d in (4, 8):
                assert uni(**{name: at + d}) == 4 and mix(**{name: at + d}) == 4, (ty, name, d)
        assert uni(a=None, sw=SW + 8) == 3 and uni(sw=None, mk=MK + 8) == 3   # NULL is answered before alignment
        # mask and stats may be NULL: the call gets past them to the next refusal
        assert uni(mk=None, st=None, sw=SW + 8) == 4 and mix(mk=None, st=None, a=A + 8) == 4
        # the empty window: set_words is not touched, so neither NULL nor a misaligned pointer is refused -- as far as the next refusal
        assert uni(sb=0, sw=None, a=None) == 3 and uni(sb=0, sw=None, mk=MK + 8) == 4 and uni(sb=0, sw=SW + 4, mk=MK + 8) == 4
        assert mix(sb=0, sw=None, ar=None) == 3 and mix(sb=0, sw=SW + 4, st=ST + 8) == 4
        # the packed pointer may be NULL only when no byte of it can be read
        assert uni(w=0, a=None, mk=MK + 8) == 4 and mix(a=None, ab=0, mk=MK + 8) == 4
        assert mix(a=None) == 3 and uni(w=1, a=None) == 3


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    w, o = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError):                                          # device tier only: numpy arrays and CPU tensors
        fl.FoR.unfor_set_build(3, np.zeros(96, dtype=np.uint32), 0, 0, 40)
    with pytest.raises(TypeError):
        fl.FoR.unfor_set_build(3, tcol, 0, 0, 40)
    with pytest.raises(TypeError):
        fl.unfor_set_build_widths(w, o, np.zeros(96, np.uint32), np.zeros(1, np.uint32), 0, 40)
    with pytest.raises(TypeError):
        fl.unfor_set_build_widths(tw, to, tcol, tref, 0, 40)


# ---- column_window ---------------------------------------------------------------------------------------------------------------------
def enumerate_window(T, widths, refs, signed):
    """brute force: every value every block can hold, ranked in the chosen order; None when a block's range passes the order's end"""
    N, sign = 1 << T, (1 << (T - 1)) if signed else 0
    ranks = []
    for w, r in zip(widths, refs):
        start = (int(r) % N) ^ sign
        if start + (1 << int(w)) - 1 > N - 1:
            return None
        ranks += [start, start + (1 << int(w)) - 1]
    return (min(ranks) ^ sign, max(ranks) - min(ranks) + 1)


def test_column_window_against_enumeration():
    import torch
    import fastlanes_amd as fl
    rng = random.Random(71000)
    seen = dict(ok=0, wraps=0, signed_ok=0)
    for ty, T in TYPE_BITS.items():
        N = 1 << T
        dt = np.dtype(f"u{T // 8}")
        for i in range(300):
            n = rng.choice([1, 2, 5, 40])
            signed = bool(i % 2)
            centre = rng.choice([0, N - 1, N // 2, N // 2 - 1, rng.randrange(N)])
            widths = [rng.choice([0, 0, 1, 3, min(T, 11)]) for _ in range(n)]
            refs = [(centre + rng.randrange(-3000, 3000)) % N for _ in range(n)]
            if i % 7 == 0:
                widths[0] = T
                refs[0] = rng.choice([0, 1 << (T - 1), 5])
            want = enumerate_window(T, widths, refs, signed)
            args = (np.array(widths, dtype=np.uint8), np.array(refs, dtype=np.uint64).astype(dt))
            if i % 3 == 0:                                                  # torch tensors (here: on the CPU) take the same path
                args = (torch.from_numpy(args[0]), torch.from_numpy(args[1].view(f"i{T // 8}")))
            if want is None or want[1] > min(N, 1 << 27):
                with pytest.raises(ValueError, match="explicit window" if want is None else "max_bits"):
                    fl.column_window(ty, *args, signed=signed)
                seen["wraps"] += want is None
            else:
                assert fl.column_window(ty, *args, signed=signed) == want, (ty, widths, refs, signed)
                seen["signed_ok" if signed else "ok"] += 1
    assert all(v > 100 for v in seen.values()), seen


def test_column_window_orders_errors_and_width_zero_columns():
    import fastlanes_amd as fl
    u8, u32, u64 = np.uint8, np.uint32, np.uint64
    w = np.array([0, 3, 2], dtype=u8)
    r = np.array([5, 10, 250], dtype=u8)
    assert fl.column_window("u8", w, r) == (5, 249)                         # [5, 5], [10, 17], [250, 253]
    assert fl.column_window("u8", w, r, signed=True) == (250, 24)           # -6 .. 17: the window starts at a negative value's pattern
    # a column around 0 has no unsigned window, and one around the sign change no signed one
    with pytest.raises(ValueError, match="explicit window"):
        fl.column_window("u8", np.array([3], dtype=u8), np.array([252], dtype=u8))
    assert fl.column_window("u8", np.array([3], dtype=u8), np.array([252], dtype=u8), signed=True) == (252, 8)
    with pytest.raises(ValueError, match="explicit window"):
        fl.column_window("u8", np.array([3], dtype=u8), np.array([124], dtype=u8), signed=True)
    assert fl.column_window("u8", np.array([3], dtype=u8), np.array([124], dtype=u8)) == (124, 8)
    # u64 at both ends of both orders
    assert fl.column_window("u64", np.array([0, 3], dtype=u8), np.array([2 ** 64 - 5, 2 ** 64 - 10], dtype=u64)) == (2 ** 64 - 10, 8)
    assert fl.column_window("u64", np.array([0, 3], dtype=u8), np.array([2 ** 64 - 5, 3], dtype=u64), signed=True) == (2 ** 64 - 5, 16)
    assert fl.column_window("u64", np.array([2, 0], dtype=u8), np.array([2 ** 63 - 4, 2 ** 63 - 9], dtype=u64), signed=True) == (2 ** 63 - 9, 9)
    with pytest.raises(ValueError, match="explicit window"):
        fl.column_window("u64", np.array([3], dtype=u8), np.array([2 ** 63 - 4], dtype=u64), signed=True)
    with pytest.raises(ValueError, match="explicit window"):
        fl.column_window("u64", np.array([64], dtype=u8), np.array([1], dtype=u64))
    with pytest.raises(ValueError, match="max_bits"):                        # the whole domain of u64: no wrap, but far too large
        fl.column_window("u64", np.array([64], dtype=u8), np.array([0], dtype=u64))
    assert fl.column_window("u16", np.array([16], dtype=u8), np.array([0], dtype=np.uint16)) == (0, 65536)
    assert fl.column_window("u16", np.array([16], dtype=u8), np.array([0x8000], dtype=np.uint16), signed=True) == (0x8000, 65536)
    # max_bits: the message names the window
    wr = (np.array([0, 0], dtype=u8), np.array([7, 7 + (1 << 20)], dtype=u32))
    with pytest.raises(ValueError, match="1048577 bits"):
        fl.column_window("u32", *wr, max_bits=1 << 20)
    assert fl.column_window("u32", *wr, max_bits=(1 << 20) + 1) == (7, (1 << 20) + 1)
    with pytest.raises(ValueError, match=str(2 ** 31 + 1)):
        fl.column_window("u32", np.array([0, 0], dtype=u8), np.array([0, 2 ** 31], dtype=u32))     # the default: 2^27 bits
    with pytest.raises(ValueError, match="max_bits"):
        fl.column_window("u64", np.array([0, 0], dtype=u8), np.array([0, 2 ** 40], dtype=u64), max_bits=2 ** 50)   # never above 2^32
    # a column of width-0 blocks only; one reference for all; the empty column
    assert fl.column_window("u32", np.zeros(4, dtype=u8), np.array([900, 17, 17, 300], dtype=u32)) == (17, 884)
    assert fl.column_window("u32", np.zeros(4, dtype=u8), np.array([900], dtype=u32)) == (900, 1)
    assert fl.column_window("u32", np.array([0, 4, 2], dtype=u8), np.array([900], dtype=u32)) == (900, 16)
    assert fl.column_window("u32", np.zeros(0, dtype=u8), np.zeros(0, dtype=u32)) == (0, 0)
    # refusals
    with pytest.raises(ValueError):
        fl.column_window("u8", np.array([9], dtype=u8), np.array([0], dtype=u8))                  # a width above T
    with pytest.raises(ValueError):
        fl.column_window("u8", np.zeros(3, dtype=u8), np.zeros(2, dtype=u8))
    with pytest.raises(TypeError):
        fl.column_window("u16", np.zeros(3, dtype=u8), np.zeros(3, dtype=u8))
    with pytest.raises(ValueError):
        fl.column_window("u7", np.zeros(3, dtype=u8), np.zeros(3, dtype=u8))


# ---- the block decisions ---------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "fl_set_build_map.hpp"
#include <stddef.h>
// the array form: query i = (set_lo, set_bits, reference, width, mask_empty, precondition_ok, kept) -> the block's route, c, and what
// a DECIDED block adds to {inserted, outside}
extern "C" void set_build_route_n(unsigned type_bits, size_t n, const uint64_t* set_lo, const uint64_t* set_bits, const uint64_t* ref,
                                  const uint8_t* width, const uint8_t* mask_empty, const uint8_t* ok, const uint64_t* kept, int* route,
                                  uint64_t* c_out, uint64_t* inserted, uint64_t* outside, uint8_t* reads)
{
    for (size_t i = 0; i < n; ++i) {
        const fl::ForPredicate window = fl::set_window(type_bits, set_lo[i], set_bits[i]);
        const fl::SetBuildRoute r = fl::set_build_route(type_bits, window, mask_empty[i] != 0, ok[i] != 0, ref[i], width[i], c_out[i]);
        route[i] = r;
        inserted[i] = fl::set_build_inserted(r, kept[i]);
        outside[i] = fl::set_build_outside(r, kept[i]);
        reads[i] = fl::set_build_reads_packed(r);
    }
}
extern "C" uint64_t set_build_lds_bits(void) { return fl::SET_BUILD_LDS_BITS; }
extern "C" int set_build_lds_tier_of(uint64_t set_bits) { return fl::set_build_lds_tier(set_bits); }
extern "C" uint32_t set_build_last_word_mask_of(uint64_t set_bits) { return fl::set_build_last_word_mask(set_bits); }
extern "C" unsigned set_build_wave_lds_of(unsigned block_bytes, unsigned type_bits, int lds_tier) { return fl::set_build_wave_lds(block_bytes, type_bits, lds_tier != 0); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "set_build_map", SHIM)
    P = ctypes.c_void_p
    so.set_build_route_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 12
    so.set_build_route_n.restype = None
    so.set_build_lds_bits.restype = ctypes.c_uint64
    so.set_build_lds_tier_of.argtypes = [ctypes.c_uint64]
    so.set_build_last_word_mask_of.argtypes = [ctypes.c_uint64]
    so.set_build_last_word_mask_of.restype = ctypes.c_uint32
    so.set_build_wave_lds_of.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_int]
    so.set_build_wave_lds_of.restype = ctypes.c_uint
    return so


def routes(shim, T, lo, bits, ref, width, empty, ok, kept):
    lo, bits, ref, kept = (np.array(x, dtype=np.uint64) for x in (lo, bits, ref, kept))
    width, empty, ok = (np.array(x, dtype=np.uint8) for x in (width, empty, ok))
    n = lo.size
    route, c, ins, out, reads = np.empty(n, np.int32), np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint8)
    shim.set_build_route_n(T, n, *(x.ctypes.data for x in (lo, bits, ref, width, empty, ok, kept, route, c, ins, out, reads)))
    return route, c, ins, out, reads


def test_limits_of_the_header(shim):
    assert shim.set_build_lds_bits() == 65536                               # 8 KiB: the whole domain of u8 and u16
    assert [shim.set_build_lds_tier_of(b) for b in (0, 1, 2048, 65536, 65537, 2 ** 32)] == [1, 1, 1, 1, 0, 0]
    assert [shim.set_build_last_word_mask_of(b) for b in (1, 31, 32, 33, 64, 65537, 2 ** 32)] == [1, 0x7FFFFFFF, 0xFFFFFFFF, 1, 0xFFFFFFFF, 1, 0xFFFFFFFF]
    # image + private bitmap per wavefront: u8 1 KiB + 32 B, u16 2 + 8 KiB, u32 4 + 8 KiB, u64 8 + 8 KiB <= the 17 KiB unfor_aggregate_by ships with
    assert [shim.set_build_wave_lds_of(128 * T, T, 1) for T in (8, 16, 32, 64)] == [1024 + 32, 2048 + 8192, 4096 + 8192, 8192 + 8192]
    assert [shim.set_build_wave_lds_of(128 * T, T, 0) for T in (32, 64)] == [4096, 8192]


def test_routes_are_sound_at_four_bits(shim):
    """every (set_lo, set_bits, reference, width, mask in {empty, one bit, full}) of a 4-bit model type, against brute force over the
    values the block CAN hold: an OUTSIDE block can insert nothing, a ONE_BIT block inserts exactly bit c, and exactly the blocks
    that may hold values on both sides of the window's edge -- or several inside it -- are decoded"""
    T, N = 4, 16
    q = []
    for lo in range(N):
        for bits in range(N + 1):
            for ref in range(N):
                for w in range(T + 1):
                    for kept in (0, 1, 1024):
                        for ok in (1, 0):
                            q.append((lo, bits, ref, w, kept == 0, ok, kept))
    assert len(q) == 16 * 17 * 16 * 5 * 3 * 2
    route, c, ins, out, reads = routes(shim, T, *([x[j] for x in q] for j in range(7)))
    seen = set()
    for i, (lo, bits, ref, w, empty, ok, kept) in enumerate(q):
        window = {(lo + j) % N for j in range(bits)}
        vals = {(ref + f) % N for f in range(1 << w)}
        index = {(v - lo) % N for v in vals if v in window}                 # the bits the block can set
        r = int(route[i])
        what = (lo, bits, ref, w, empty, ok)
        assert int(c[i]) == (ref - lo) % N
        assert int(reads[i]) == (r == EACH)
        if empty or not ok:
            assert r == SKIP and int(ins[i]) == int(out[i]) == 0, ("an empty mask or a failed check must contribute nothing", what)
        elif not index:
            assert r == OUTSIDE and (int(ins[i]), int(out[i])) == (0, kept), ("OUTSIDE: nothing can be inserted", what)
        elif w == 0:
            assert r == ONE_BIT and index == {int(c[i])} and int(c[i]) < bits and (int(ins[i]), int(out[i])) == (kept, 0), ("ONE_BIT: exactly bit c", what)
        else:
            assert r == EACH and int(ins[i]) == int(out[i]) == 0, ("left to the decode", what)
        if r == OUTSIDE:
            assert not (vals & window), ("OUTSIDE claimed", what)
        seen.add((r, w == 0, bits == 0, bits == N))
    assert {(SKIP, True, True, False), (OUTSIDE, True, True, False), (OUTSIDE, False, False, False), (ONE_BIT, True, False, True),
            (ONE_BIT, True, False, False), (EACH, False, False, True), (EACH, False, False, False)} <= seen
    assert not any(r == EACH and z for r, z, _, _ in seen) and not any(r in (ONE_BIT, EACH) and e for r, _, e, _ in seen)


@pytest.mark.parametrize("T", [8, 16, 32, 64])
def test_routes_on_a_seeded_sample(shim, T):
    """10^5 cases per real type against a restatement in Python integers: the block's indices {(c + f) mod 2^T} meet the window
    [0, set_bits - 1] iff c lies inside it or c + 2^W - 1 passes 2^T; windows of 0, 1, 31 .. 33, 65535 .. 65537 and the largest
    number of bits, references at both ends of the window and of the domain, widths 0 and T, empty masks and failed checks"""
    N = 1 << T
    top = min(N, 1 << 32)
    rng = random.Random(72000 + T)
    sizes = [b for b in (0, 1, 2, 31, 32, 33, 255, 256, 2048, 65535, 65536, 65537, top - 1, top) if b <= top]
    q, want = [], []
    counts = dict(skip=0, outside=0, one_bit=0, each=0, wraps=0)
    for i in range(100_000):
        bits = sizes[i % len(sizes)] if i % 3 else rng.randint(0, top)
        lo = [0, N - 1, N >> 1, (N - bits) % N][i % 4] if i % 5 == 0 else rng.randrange(N)
        w = [0, T, 1, T - 1, 0][i % 11] if i % 11 < 5 else rng.randint(0, T)
        span = (1 << w) - 1
        kind = i % 7
        if kind == 0:
            ref = (lo + bits) % N                                           # the first value behind the window
        elif kind == 1:
            ref = (lo - span - 1) % N                                       # the block ends just in front of the window
        elif kind == 2:
            ref = (lo - span) % N                                           # ... or on its first value
        elif kind == 3:
            ref = (lo + max(bits, 1) - 1) % N                               # the window's last value
        elif kind == 4:
            ref = (lo + rng.randint(0, max(bits, 1) - 1)) % N               # inside
        else:
            ref = rng.randrange(N)
        empty, ok = i % 13 == 0, i % 17 != 0
        kept = 0 if empty else rng.randint(1, 1024)
        c = (ref - lo) % N
        if empty or not ok:
            r = SKIP
        elif bits == 0 or not (c <= bits - 1 or c + span >= N):
            r = OUTSIDE
        elif w == 0:
            r = ONE_BIT
        else:
            r = EACH
        counts[("skip", "outside", "one_bit", "each")[r]] += 1
        counts["wraps"] += lo + bits > N
        q.append((lo, bits, ref, w, empty, ok, kept))
        want.append((r, c, kept if r == ONE_BIT else 0, kept if r == OUTSIDE else 0))
    assert all(v > 500 for v in counts.values()), counts
    route, c, ins, out, reads = routes(shim, T, *([x[j] for x in q] for j in range(7)))
    for i in range(len(q)):
        assert (int(route[i]), int(c[i]), int(ins[i]), int(out[i])) == want[i], (T, q[i], want[i])


def test_cpp_mirror_declares_both_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the two new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint16_t;
void (*const uniform)(std::size_t, const T*, const T*, std::size_t, const std::uint32_t*, std::size_t, T, std::uint64_t, std::uint32_t*,
                      std::uint64_t*, void*) = &fastlanes::FoR<T>::unfor_set_build_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const std::uint32_t*, std::size_t,
                    T, std::uint64_t, std::uint32_t*, std::uint64_t*, std::uint32_t*, void*) = &fastlanes::unfor_set_build_widths_device<T>;
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
