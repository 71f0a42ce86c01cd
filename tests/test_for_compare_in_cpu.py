"""CPU: unfor_compare_in / unfor_compare_in_widths (set membership over a FoR-packed column: a window of the value domain plus a
bitmap, chained through a mask) -- the header declares and the library exports them for every element type through a macro of their
own, the Python table agrees with the header, every refusal needs no GPU, the Python mirror validates before any launch, member_set
finds the tightest cyclic window, and the block decisions the kernel and the host share (fastlanes_amd/csrc/fl_set_decide.hpp, compiled
here with g++) are SOUND: exhaustively at a 4-bit model type against brute force over every bitmap bit, and on a seeded sample of the
real types against a restatement in Python integers."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)

FORMS = ("unfor_compare_in", "unfor_compare_in_widths")
NEW, AND, OR = 0, 1, 2
EACH, ALL, NONE = 0, 1, 2


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
    body = text.split("#define FL_DECLARE_FOR_COMPARE_IN(T, S)")[1].split("FL_DECLARE_FOR_COMPARE_IN(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_FOR_COMPARE_IN({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.for_compare_in_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.select_symbols(),
                  fastlanes_amd.aggregate_symbols(), fastlanes_amd.for_compare_range_symbols(), fastlanes_amd.aggregate_by_symbols(),
                  fastlanes_amd.for_compare_columns_symbols(), fastlanes_amd.aggregate_columns_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"for_compare_in_symbols", "unfor_compare_in_widths", "member_set", "MemberSet"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.FoR, "unfor_compare_in")


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: a pointer is c_void_p, `unsigned` c_uint, size_t c_size_t, int c_int,
    uint64_t c_uint64, the element type its own scalar; the argument list is unfor_compare_range's with (lo, hi) replaced"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("FOR_COMPARE_IN")}
    assert len(rows) == 8
    for ty in TYPE_BITS:
        for form in FORMS:
            name = f"fl_{ty}_{form}"
            ret, args = protos[name]
            restype, argtypes = rows[name]
            assert ret == "int" and restype is ctypes.c_int
            rng_args = [a for _, a in protos[name.replace("compare_in", "compare_range")][1]]
            i = rng_args.index("lo")
            assert rng_args[i:i + 2] == ["lo", "hi"]
            assert [a for _, a in args] == rng_args[:i] + ["set_lo", "set_bits", "set_words", "negate"] + rng_args[i + 2:], name
            assert len(args) == len(argtypes), name
            scalars = {"unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64, CT[ty]: _lib.CTYPE[ty]}
            for (ctype, arg), at in zip(args, argtypes):
                assert at is (ctypes.c_void_p if "*" in ctype else scalars[ctype]), (name, arg, ctype)
            types = dict((a, c) for c, a in args)
            assert types["set_lo"] == CT[ty] and types["set_bits"] == "uint64_t" and types["set_words"] == "const uint32_t *"
            assert getattr(lib, name).argtypes == argtypes


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), in the order of unfor_compare_range with the set's own
    checks beside their kind: the width; combine, negate, set_bits (FL_ERR_INDEX); the empty column; mask_in, set_words and the other
    pointers (FL_ERR_NULL); alignment, set_words included."""
    buf = np.zeros(8192, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    A, AR, MI, M, W, O, SW = (p + 4096 * i for i in range(7))
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_compare_in")
        g = getattr(lib, f"fl_{ty}_unfor_compare_in_widths")
        top = min(1 << T, 1 << 32)

        def uni(w=3, a=A, ar=AR, lo=5, sb=40, sw=SW, ng=0, cb=NEW, mi=MI, n=1, m=M):
            return f(w, a, ar, 1, lo, sb, sw, ng, cb, mi, n, m, None)

        def mix(w=W, o=O, a=A, ab=384, ar=AR, lo=5, sb=40, sw=SW, ng=0, cb=NEW, mi=MI, n=1, m=M):
            return g(w, o, a, ab, ar, 1, lo, sb, sw, ng, cb, mi, n, m, None, None)

        # FL_ERR_WIDTH: also for an empty column and in front of every other refusal
        for n in (1, 0):
            assert uni(w=T + 1, n=n) == 1 and uni(w=T + 1, cb=7, n=n) == 1 and uni(w=T + 1, sb=top + 1, n=n) == 1 and uni(w=T + 1, m=None, n=n) == 1
        assert uni(w=T, m=None) == 3                                        # the widest width is not refused as a width
        # FL_ERR_INDEX: combine outside fl_mask_combine, negate outside {0, 1}, set_bits above min(2^T, 2^32); also for an empty column
        for n in (1, 0):
            for cb in (-1, 3, 99):
                assert uni(cb=cb, n=n) == 2 and mix(cb=cb, n=n) == 2
            for ng in (-1, 2, 99):
                assert uni(ng=ng, n=n) == 2 and mix(ng=ng, n=n) == 2
            for sb in (top + 1, top + 32, 1 << 33, 2 ** 64 - 1):
                assert uni(sb=sb, n=n) == 2 and mix(sb=sb, n=n) == 2, (ty, sb)
        assert uni(cb=3, m=None) == 2 and mix(ng=2, a=None) == 2 and uni(sb=top + 1, sw=None) == 2   # ... in front of the NULL checks
        assert uni(sb=top, m=None) == 3 and mix(sb=top, m=None) == 3        # the largest window is not refused
        for ng in (0, 1):
            for cb in (NEW, AND, OR):
                # n_blocks == 0: nothing to do, whatever the pointers
                assert f(3, None, None, 0, 5, 40, None, ng, cb, None, 0, None, None) == 0
                assert g(None, None, None, 0, None, 0, 5, 40, None, ng, cb, None, 0, None, None, None) == 0
                # FL_ERR_NULL: each required pointer, under every combiner; set_words with set_bits > 0
                for name in ("a", "ar", "m", "sw"):
                    assert uni(**{name: None}, ng=ng, cb=cb) == 3, (ty, name)
                for name in ("w", "o", "a", "ar", "m", "sw"):
                    assert mix(**{name: None}, ng=ng, cb=cb) == 3, (ty, name)
                # FL_ERR_ALIGN: the packed column, the mask and set_words off a 16-byte boundary
                for name, at in (("a", A), ("m", M), ("sw", SW)):
                    for d in (4, 8):
                        assert uni(**{name: at + d}, ng=ng, cb=cb) == 4 and mix(**{name: at + d}, ng=ng, cb=cb) == 4, (ty, name, d)
                assert uni(a=None, sw=SW + 8, ng=ng, cb=cb) == 3 and uni(sw=None, m=M + 8, ng=ng, cb=cb) == 3   # NULL is answered before alignment
        # the empty set: set_words is not read, so neither NULL nor a misaligned pointer is refused -- as far as the next refusal
        assert uni(sb=0, sw=None, m=None) == 3 and uni(sb=0, sw=None, m=M + 8) == 4 and uni(sb=0, sw=SW + 4, m=M + 8) == 4
        assert mix(sb=0, sw=None, m=None) == 3 and mix(sb=0, sw=SW + 4, m=M + 8) == 4
        # mask_in: required and aligned under AND / OR, ignored under NEW
        for cb in (AND, OR):
            assert uni(cb=cb, mi=None) == 3 and mix(cb=cb, mi=None) == 3
            assert uni(cb=cb, mi=MI + 4) == 4 and mix(cb=cb, mi=MI + 8) == 4
            assert uni(cb=cb, mi=None, m=M + 8) == 3                        # ... and answered before alignment
        assert uni(cb=NEW, mi=None, m=None) == 3 and uni(cb=NEW, mi=None, m=M + 8) == 4   # got past mask_in to the next refusal
        assert uni(cb=NEW, mi=MI + 4, m=M + 8) == 4 and mix(cb=NEW, mi=None, m=M + 8) == 4
        # the packed pointer may be NULL only when no byte of it can be read
        assert uni(w=0, a=None, m=M + 8) == 4 and mix(a=None, ab=0, m=M + 8) == 4
        assert mix(a=None) == 3 and uni(w=1, a=None) == 3


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    w, o = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref, tmask = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(32, dtype=torch.int32)
    # device tier only: numpy arrays and CPU tensors
    with pytest.raises(TypeError):
        fl.FoR.unfor_compare_in(3, np.zeros(96, dtype=np.uint32), 0, [1, 2])
    with pytest.raises(TypeError):
        fl.FoR.unfor_compare_in(3, tcol, 0, [1, 2])
    with pytest.raises(TypeError):
        fl.unfor_compare_in_widths(w, o, np.zeros(96, np.uint32), np.zeros(1, np.uint32), [1, 2])
    with pytest.raises(TypeError):
        fl.unfor_compare_in_widths(tw, to, tcol, tref, [1, 2])
    # a combine that is none of the three, and a combine without the mask so far
    for bad in ("xor", "AND", 1, None):
        with pytest.raises(ValueError):
            fl.FoR.unfor_compare_in(3, tcol, 0, [1, 2], mask=tmask, combine=bad)
        with pytest.raises(ValueError):
            fl.unfor_compare_in_widths(tw, to, tcol, tref, [1, 2], mask=tmask, combine=bad)
    for cb in ("and", "or"):
        with pytest.raises(ValueError):
            fl.FoR.unfor_compare_in(3, tcol, 0, [1, 2], combine=cb)
        with pytest.raises(ValueError):
            fl.unfor_compare_in_widths(tw, to, tcol, tref, [1, 2], combine=cb)
    # a mask that does not hold 32 words per block
    for words in (0, 31, 33, 64):
        with pytest.raises(ValueError):
            fl.unfor_compare_in_widths(tw, to, tcol, tref, [1, 2], mask=torch.zeros(words, dtype=torch.int32), combine="and")
        with pytest.raises(ValueError):
            fl.FoR.unfor_compare_in(3, tcol, 0, [1, 2], mask=torch.zeros(words, dtype=torch.int32), combine="or")


# ---- member_set ----------------------------------------------------------------------------------------------------------------------
def tightest_window(patterns, N):
    """brute force over all N rotations: (lo, bits) of the smallest window from lo that holds every pattern; ties: the smallest lo"""
    best = None
    for lo in range(N):
        bits = max((p - lo) % N for p in patterns) + 1
        if best is None or bits < best[1]:
            best = (lo, bits)
    return best


def check_bitmap(ms, patterns, N):
    assert ms.words.dtype == np.uint32 and ms.words.size == (ms.bits + 31) // 32
    bits = np.unpackbits(ms.words.view(np.uint8), bitorder="little")
    assert int(bits.sum()) == len(patterns)                                # one bit per member, nothing past `bits`
    assert all(bits[(p - ms.lo) % N] for p in patterns) and not bits[ms.bits:].any()


def test_member_set_is_the_tightest_window_of_every_sampled_u8_subset():
    import fastlanes_amd as fl
    rng = random.Random(51000)
    subsets = [{5}, {0}, {255}, {0, 128}, {64, 192}, {0, 255}, {255, 0, 1}, {10, 11, 12, 200}, set(range(256)), set(range(0, 256, 2)),
               {0, 85, 170}, {3, 88, 173}, set(range(100, 256)) | set(range(0, 20))]
    for i in range(400):
        k = rng.choice([1, 2, 3, 4, 7, 16, 50, 128, 200, 255])
        base = rng.sample(range(256), k)
        if i % 3 == 0:                                                      # clustered: a short window somewhere on the cycle
            start = rng.randrange(256)
            base = [(start + v % 40) % 256 for v in base]
        subsets.append(set(base))
    seen_wrap = seen_tie = 0
    for s in subsets:
        ms = fl.member_set("u8", sorted(s))
        lo, bits = tightest_window(s, 256)
        assert (ms.ty, ms.lo, ms.bits) == ("u8", lo, bits), (sorted(s), ms)
        check_bitmap(ms, s, 256)
        seen_wrap += lo + bits > 256
        seen_tie += sum(max((p - l) % 256 for p in s) + 1 == bits for l in range(256)) > 1
    assert seen_wrap > 20 and seen_tie >= 4
    assert tuple(fl.member_set("u8", [0, 128]))[1:3] == (0, 129) and tuple(fl.member_set("u8", [192, 64]))[1:3] == (64, 129)   # the tie rule


def test_member_set_signed_empty_inputs_and_refusals():
    import torch
    import fastlanes_amd as fl
    ms = fl.member_set("u32", [-1, 0, 1], signed=True)                      # around 0: the window wraps, 3 bits -- not 2^32
    assert (ms.lo, ms.bits) == (2 ** 32 - 1, 3) and ms.words.tolist() == [7]
    ms = fl.member_set("u64", [3, -2], signed=True)
    assert (ms.lo, ms.bits) == (2 ** 64 - 2, 6) and ms.words.tolist() == [0b100001]
    ms = fl.member_set("u16", np.array([-3, 7, 7, -3], dtype=np.int16), signed=True)        # duplicates are fine
    assert (ms.lo, ms.bits) == (65533, 11) and ms.words.tolist() == [1 | 1 << 10]
    assert (fl.member_set("u64", [2 ** 64 - 1, 3]).lo, fl.member_set("u64", np.array([2 ** 64 - 1, 3], dtype=np.uint64)).bits) == (2 ** 64 - 1, 5)
    ty, lo, bits, words = fl.member_set("u16", torch.tensor([3, 9, 40]))   # a (CPU) tensor of members; the result unpacks
    assert (ty, lo, bits) == ("u16", 3, 38) and words.tolist() == [1 | 1 << 6, 1 << 5]
    for ty in TYPE_BITS:
        e = fl.member_set(ty, [])
        assert (e.lo, e.bits, e.words.size) == (0, 0, 0)
    full = fl.member_set("u16", range(65536))
    assert (full.lo, full.bits) == (0, 65536) and (full.words == 0xFFFFFFFF).all()
    # max_bits: the message names the window
    with pytest.raises(ValueError, match="1048577 bits"):
        fl.member_set("u32", [7, 7 + (1 << 20)], max_bits=1 << 20)
    assert fl.member_set("u32", [7, 7 + (1 << 20) - 1], max_bits=1 << 20).bits == 1 << 20
    with pytest.raises(ValueError, match=str(2 ** 31 + 1)):
        fl.member_set("u32", [0, 2 ** 31])                                  # the default: 2^27 bits
    with pytest.raises(ValueError, match=str(2 ** 63 + 1)):
        fl.member_set("u64", [0, 2 ** 63], max_bits=2 ** 40)                # never above 2^32, whatever max_bits says
    # members outside the element type
    for ty, members, signed in (("u8", [256], False), ("u8", [-1], False), ("u8", [128], True), ("u8", [-129], True), ("u16", np.array([70000]), False),
                                ("u32", np.array([-1]), False)):
        with pytest.raises(ValueError):
            fl.member_set(ty, members, signed=signed)
    with pytest.raises(TypeError):
        fl.member_set("u8", np.array([1.0]))
    with pytest.raises(ValueError):
        fl.member_set("u7", [1])


# ---- the block decisions ---------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "fl_set_decide.hpp"
#include <stddef.h>
// the array form: query i = (set_lo, set_bits, the bitmap word that holds bit c, reference, width, negate) -> the block's verdict as the
// kernel reaches it: set_block_decide, the probe of a width-0 block, negate; and c
extern "C" void set_decide_n(unsigned type_bits, size_t n, const uint64_t* set_lo, const uint64_t* set_bits, const uint32_t* word, const uint64_t* ref,
                             const uint8_t* width, const uint8_t* negate, int* verdict, uint64_t* c_out)
{
    for (size_t i = 0; i < n; ++i) {
        const fl::ForPredicate window = fl::set_window(type_bits, set_lo[i], set_bits[i]);
        int v = fl::set_block_decide(type_bits, window, ref[i], width[i], c_out[i]);
        if (v == fl::SET_PROBE) v = fl::set_probe_verdict(word[i], c_out[i]);
        verdict[i] = fl::set_hit_verdict(v, negate[i] != 0);
    }
}
extern "C" int set_member_of(unsigned type_bits, uint64_t set_lo, uint64_t set_bits, const uint32_t* words, uint64_t v)
{
    return fl::set_member(type_bits, fl::set_window(type_bits, set_lo, set_bits), words, v);
}
extern "C" uint64_t set_max_bits_of(unsigned type_bits) { return fl::set_max_bits(type_bits); }
extern "C" uint64_t set_word_count_of(uint64_t set_bits) { return fl::set_word_count(set_bits); }
extern "C" uint64_t set_register_bits(void) { return fl::SET_REGISTER_BITS; }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "set_decide", SHIM)
    P = ctypes.c_void_p
    so.set_decide_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 8
    so.set_decide_n.restype = None
    so.set_member_of.argtypes = [ctypes.c_uint, ctypes.c_uint64, ctypes.c_uint64, P, ctypes.c_uint64]
    for name, args in (("set_max_bits_of", [ctypes.c_uint]), ("set_word_count_of", [ctypes.c_uint64]), ("set_register_bits", [])):
        getattr(so, name).argtypes = args
        getattr(so, name).restype = ctypes.c_uint64
    return so


def decide(shim, T, lo, bits, word, ref, width, negate):
    lo, bits, ref = (np.array(x, dtype=np.uint64) for x in (lo, bits, ref))
    word = np.array(word, dtype=np.uint32)
    width, negate = (np.array(x, dtype=np.uint8) for x in (width, negate))
    v, c = np.empty(lo.size, np.int32), np.empty(lo.size, np.uint64)
    shim.set_decide_n(T, lo.size, *(x.ctypes.data for x in (lo, bits, word, ref, width, negate, v, c)))
    return v, c


def test_limits_of_the_header(shim):
    assert [shim.set_max_bits_of(T) for T in (4, 8, 16, 32, 64)] == [16, 256, 65536, 2 ** 32, 2 ** 32]
    assert [shim.set_word_count_of(b) for b in (0, 1, 32, 33, 2048, 2049, 2 ** 32)] == [0, 1, 1, 2, 64, 65, 2 ** 27]
    assert shim.set_register_bits() == 2048                                 # 64 lanes x 32 bits


def test_block_decisions_are_sound_at_four_bits(shim):
    """every (set_lo, set_bits, bitmap of a seeded sample, reference, width, negate) of a 4-bit model type, against brute force over
    the values the block CAN hold: ALL / NONE is claimed only when it is true of every one of them; a block outside the window and a
    width-0 block are always decided; a window that covers every value decides nothing by itself."""
    T, N = 4, 16
    rng = random.Random(52000)
    q = []
    for lo in range(N):
        for bits in range(N + 1):
            maps = {0, 0xFFFF, (1 << bits) - 1, 0xFFFF & ~((1 << bits) - 1)} | {rng.randrange(1 << 16) for _ in range(4)}
            for bitmap in sorted(maps):                                     # bits at positions >= `bits`: garbage, to be ignored
                for ref in range(N):
                    for w in range(T + 1):
                        for negate in (0, 1):
                            q.append((lo, bits, bitmap, ref, w, negate))
    assert len(q) > 250_000
    got, c = decide(shim, T, *([x[j] for x in q] for j in range(6)))
    seen = set()
    words = (ctypes.c_uint32 * 1)()
    for i, (lo, bits, bitmap, ref, w, negate) in enumerate(q):
        members = {(lo + j) % N for j in range(bits) if bitmap >> j & 1}
        window = {(lo + j) % N for j in range(bits)}
        vals = {(ref + f) % N for f in range(1 << w)}
        hit = {(v in members) != bool(negate) for v in vals}
        v = int(got[i])
        assert int(c[i]) == (ref - lo) % N
        assert v in (EACH, ALL, NONE)
        if v == ALL:
            assert hit == {True}, ("ALL claimed", lo, bits, bin(bitmap), ref, w, negate)
        if v == NONE:
            assert hit == {False}, ("NONE claimed", lo, bits, bin(bitmap), ref, w, negate)
        if not (vals & window) or w == 0:
            assert v != EACH, ("left open", lo, bits, bin(bitmap), ref, w, negate)
        if bits == N and w > 0:
            assert v == EACH, ("the full window decided a block", lo, bitmap, ref, w, negate)
        seen.add((negate, v, w == 0))
        if i % 97 == 0:                                                     # member(v) of the definition, for every value
            words[0] = bitmap
            for x in range(N):
                assert shim.set_member_of(T, lo, bits, words, x) == int(x in members)
    # a width-0 block is decided either way; a wider one only as "outside the window": a miss, all hits under negate
    assert seen == {(ng, v, True) for ng in (0, 1) for v in (ALL, NONE)} | {(0, NONE, False), (1, ALL, False), (0, EACH, False), (1, EACH, False)}


@pytest.mark.parametrize("T", [8, 16, 32, 64])
def test_block_decisions_on_a_seeded_sample(shim, T):
    """10^5 cases per real type against a restatement in Python integers: the block's indices {(c + f) mod 2^T} meet the window
    [0, set_bits - 1] iff c lies inside it or c + 2^W - 1 passes 2^T; windows of 0, 1, 31 .. 33, 2048, 2049, 65536 and the largest
    number of bits, references at both ends of the window and of the domain, widths 0 and T"""
    N = 1 << T
    top = min(N, 1 << 32)
    rng = random.Random(53000 + T)
    sizes = [b for b in (0, 1, 2, 31, 32, 33, 255, 256, 2047, 2048, 2049, 65535, 65536, top - 1, top) if b <= top]
    q, want = [], []
    counts = dict(outside=0, probe_hit=0, probe_miss=0, each=0, wraps=0, full=0)
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
        word, negate = rng.getrandbits(32), (i // 7) % 2
        c = (ref - lo) % N
        if bits == 0 or not (c <= bits - 1 or c + span >= N):
            member = NONE
            counts["outside"] += 1
        elif w == 0:
            member = ALL if word >> (c & 31) & 1 else NONE
            counts["probe_hit" if member == ALL else "probe_miss"] += 1
        else:
            member = EACH
            counts["each"] += 1
        counts["wraps"] += lo + bits > N
        counts["full"] += bits == N
        q.append((lo, bits, word, ref, w, negate))
        want.append(member if member == EACH or not negate else (NONE if member == ALL else ALL))
    assert all(v > 500 for k, v in counts.items() if k != "full" or T <= 32), counts
    got, c = decide(shim, T, *([x[j] for x in q] for j in range(6)))
    for i, (lo, bits, word, ref, w, negate) in enumerate(q):
        assert int(got[i]) == want[i] and int(c[i]) == (ref - lo) % N, (T, lo, bits, hex(word), ref, w, negate, int(got[i]), want[i])


def test_cpp_mirror_declares_both_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the two new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint16_t;
void (*const uniform)(std::size_t, const T*, const T*, std::size_t, T, std::uint64_t, const std::uint32_t*, bool, fl_mask_combine,
                      const std::uint32_t*, std::size_t, std::uint32_t*, void*) = &fastlanes::FoR<T>::unfor_compare_in_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, T, std::uint64_t,
                    const std::uint32_t*, bool, fl_mask_combine, const std::uint32_t*, std::size_t, std::uint32_t*, std::uint32_t*,
                    void*) = &fastlanes::unfor_compare_in_widths_device<T>;
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
