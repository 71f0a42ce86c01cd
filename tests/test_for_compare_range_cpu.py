"""CPU: unfor_compare_range / unfor_compare_range_widths (interval predicates chained through a mask) -- the header declares and the
library exports them for every element type through a macro of their own, their argument checks need no GPU, the Python mirror
validates before any launch, the interval arithmetic the kernel runs (for_range_predicate + for_compare_decide of
fastlanes_amd/csrc/fl_for_decide.hpp, compiled here for the host) agrees with the definition -- exhaustively for u8, at the edge
bounds for u16 / u32 / u64 -- and predicate_interval gives the interval of every comparison, signed ones included."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)

OPS = ("==", "!=", "<", "<=", ">", ">=")            # fl_cmp 0..5
EACH, ALL, NONE = 0, 1, 2
NEW, AND, OR = 0, 1, 2


def test_header_declares_and_library_exports_the_eight_symbols(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_FOR_COMPARE_RANGE(T, S)")[1].split("FL_DECLARE_FOR_COMPARE_RANGE(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == ["unfor_compare_range", "unfor_compare_range_widths"]
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_FOR_COMPARE_RANGE({CT[ty]}, {ty})" in text
    assert "typedef enum fl_mask_combine { FL_MASK_NEW = 0, FL_MASK_AND = 1, FL_MASK_OR = 2 } fl_mask_combine;" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in ("unfor_compare_range", "unfor_compare_range_widths")]
    assert len(want) == 8 and sorted(fastlanes_amd.for_compare_range_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.select_symbols(),
                  fastlanes_amd.aggregate_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert "for_compare_range_symbols" in fastlanes_amd.__all__


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), in the siblings' order: width, combine, the empty
    column, NULL pointers, alignment."""
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_compare_range")
        g = getattr(lib, f"fl_{ty}_unfor_compare_range_widths")
        # f(width, in, refs, stride, lo, hi, combine, mask_in, n, mask, stream)
        # g(widths, offsets, packed, packed_bytes, refs, stride, lo, hi, combine, mask_in, n, mask, err, stream)
        for cb in (NEW, AND, OR):
            # empty column: nothing to do, whatever the pointers
            assert f(3, None, None, 0, 1, 2, cb, None, 0, None, None) == 0
            assert g(None, None, None, 0, None, 0, 1, 2, cb, None, 0, None, None, None) == 0
            # FL_ERR_WIDTH (uniform form), also ahead of the empty-column return and of a bad combine
            assert f(T + 1, p, p, 1, 1, 2, cb, p, 1, p, None) == 1
            assert f(T + 1, p, p, 1, 1, 2, cb, p, 0, p, None) == 1
        assert f(T + 1, p, p, 1, 1, 2, 7, p, 0, p, None) == 1
        # FL_ERR_INDEX: combine outside fl_mask_combine, also for an empty column
        for cb in (-1, 3, 99):
            assert f(3, p, p, 1, 1, 2, cb, p, 1, p, None) == 2
            assert f(3, p, p, 1, 1, 2, cb, p, 0, p, None) == 2
            assert g(p, p, p, 128, p, 1, 1, 2, cb, p, 1, p, None, None) == 2
            assert g(p, p, p, 128, p, 1, 1, 2, cb, p, 0, p, None, None) == 2
        # FL_ERR_NULL: mask_in with AND / OR
        for cb in (AND, OR):
            assert f(3, p, p, 1, 1, 2, cb, None, 1, p, None) == 3
            assert g(p, p, p, 128, p, 1, 1, 2, cb, None, 1, p, None, None) == 3
        # FL_ERR_NULL: references, mask, data, widths, offsets -- under every combiner
        for cb in (NEW, AND, OR):
            assert f(3, p, None, 1, 1, 2, cb, p, 1, p, None) == 3
            assert f(3, p, p, 1, 1, 2, cb, p, 1, None, None) == 3
            assert f(3, None, p, 1, 1, 2, cb, p, 1, p, None) == 3          # W > 0 reads data
            assert g(None, p, p, 128, p, 1, 1, 2, cb, p, 1, p, None, None) == 3
            assert g(p, None, p, 128, p, 1, 1, 2, cb, p, 1, p, None, None) == 3
            assert g(p, p, None, 128, p, 1, 1, 2, cb, p, 1, p, None, None) == 3   # packed bytes to read
            assert g(p, p, p, 128, None, 1, 1, 2, cb, p, 1, p, None, None) == 3
            assert g(p, p, p, 128, p, 1, 1, 2, cb, p, 1, None, None, None) == 3
            # FL_ERR_ALIGN: 16-byte packed column and mask
            assert f(3, p + 8, p, 1, 1, 2, cb, p, 1, p, None) == 4
            assert f(3, p, p, 1, 1, 2, cb, p, 1, p + 4, None) == 4
            assert g(p, p, p + 8, 128, p, 1, 1, 2, cb, p, 1, p, None, None) == 4
            assert g(p, p, p, 128, p, 1, 1, 2, cb, p, 1, p + 8, None, None) == 4
        # ... and mask_in under AND / OR; under NEW it is ignored, so a misaligned one is no alignment error
        for cb in (AND, OR):
            assert f(3, p, p, 1, 1, 2, cb, p + 4, 1, p, None) == 4
            assert g(p, p, p, 128, p, 1, 1, 2, cb, p + 8, 1, p, None, None) == 4
        # NEW with mask_in == NULL (or anything else) is accepted: every remaining refusal is about another argument
        assert f(3, p, p, 1, 1, 2, NEW, None, 1, None, None) == 3           # got past mask_in to the NULL mask
        assert f(3, p, p, 1, 1, 2, NEW, None, 1, p + 4, None) == 4          # ... and to the misaligned mask
        assert f(3, p, p, 1, 1, 2, NEW, p + 4, 1, p + 4, None) == 4
        assert g(p, p, p, 128, p, 1, 1, 2, NEW, None, 1, p + 8, None, None) == 4


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    w, o = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref, tmask = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(32, dtype=torch.int32)
    # device tier only: numpy arrays and CPU tensors
    with pytest.raises(TypeError):
        fl.FoR.unfor_compare_range(3, np.zeros(96, dtype=np.uint32), 0, 1, 2)
    with pytest.raises(TypeError):
        fl.FoR.unfor_compare_range(3, tcol, 0, 1, 2)
    with pytest.raises(TypeError):
        fl.FoR.unfor_compare_range(3, tcol, 0, 1, 2, mask=tmask, combine="and")
    with pytest.raises(TypeError):
        fl.unfor_compare_range_widths(w, o, np.zeros(96, np.uint32), np.zeros(1, np.uint32), 1, 2)
    with pytest.raises(TypeError):
        fl.unfor_compare_range_widths(tw, to, tcol, tref, 1, 2)
    with pytest.raises(TypeError):
        fl.unfor_compare_range_widths(tw, to, tcol, tref, 1, 2, mask=tmask, combine="or")
    # a combine that is none of the three, and a combine without the mask so far
    for bad in ("xor", "AND", 1, None):
        with pytest.raises(ValueError):
            fl.FoR.unfor_compare_range(3, tcol, 0, 1, 2, mask=tmask, combine=bad)
        with pytest.raises(ValueError):
            fl.unfor_compare_range_widths(tw, to, tcol, tref, 1, 2, mask=tmask, combine=bad)
    for cb in ("and", "or"):
        with pytest.raises(ValueError):
            fl.FoR.unfor_compare_range(3, tcol, 0, 1, 2, combine=cb)
        with pytest.raises(ValueError):
            fl.unfor_compare_range_widths(tw, to, tcol, tref, 1, 2, combine=cb)
    # a mask that does not hold 32 words per block
    for words in (0, 31, 33, 64):
        with pytest.raises(ValueError):
            fl.unfor_compare_range_widths(tw, to, tcol, tref, 1, 2, mask=torch.zeros(words, dtype=torch.int32), combine="and")
        with pytest.raises(ValueError):
            fl.FoR.unfor_compare_range(3, tcol, 0, 1, 2, mask=torch.zeros(words, dtype=torch.int32), combine="or")
    assert {"unfor_compare_range_widths", "predicate_interval"} <= set(fl.__all__) and hasattr(fl.FoR, "unfor_compare_range")


SHIM = r"""
#include "fl_for_decide.hpp"
#include <stddef.h>
#include <string.h>
// the array form: query i = (lo[i], hi[i], reference[i], width[i])
extern "C" void for_range_decide_n(unsigned type_bits, size_t n, const uint64_t* lo, const uint64_t* hi, const uint64_t* reference,
                                   const uint8_t* width, uint64_t* a, uint64_t* c, uint64_t* s, int* none, int* verdict)
{
    for (size_t i = 0; i < n; ++i) {
        const fl::ForPredicate p = fl::for_range_predicate(type_bits, lo[i], hi[i]);
        verdict[i] = fl::for_compare_decide(type_bits, p, reference[i], width[i], c[i]);
        a[i] = p.a;
        s[i] = p.s;
        none[i] = p.none ? 1 : 0;
    }
}
// the unsigned predicates of unfor_compare, for predicate_interval to agree with
extern "C" void for_compare_predicate_n(unsigned type_bits, size_t n, const int* op, const uint64_t* k, uint64_t* a, uint64_t* s, int* none)
{
    for (size_t i = 0; i < n; ++i) {
        const fl::ForPredicate p = fl::for_compare_predicate(type_bits, op[i], k[i]);
        a[i] = p.a;
        s[i] = p.s;
        none[i] = p.none ? 1 : 0;
    }
}
// u8, every (lo, hi, reference, W): 256^3 x 9 queries against the DEFINITION hit(f) = ((f + r - lo) mod 256) <= ((hi - lo) mod 256),
// written out here without the helper's c / s.  Returns the number of disagreements; the first one goes to bad[0..4] =
// (lo, hi, reference, W, what: 1 verdict, 2 the per-element form ((f + c) mod 256) <= s, 3 the predicate itself).
extern "C" long for_range_u8_exhaustive(int* bad)
{
    long wrong = 0;
    for (unsigned lo = 0; lo < 256; ++lo)
        for (unsigned hi = 0; hi < 256; ++hi) {
            const fl::ForPredicate p = fl::for_range_predicate(8, lo, hi);
            const unsigned len = (hi - lo) & 255u;
            for (unsigned r = 0; r < 256; ++r) {
                unsigned char hit[256], model[256];
                uint64_t c0;
                fl::for_compare_decide(8, p, r, 0, c0);           // c does not depend on W (checked below)
                for (unsigned f = 0; f < 256; ++f) hit[f] = (unsigned char)((((f + r) - lo) & 255u) <= len);
                for (unsigned f = 0; f < 256; ++f) model[f] = (unsigned char)((((f + (unsigned)c0) & 255u) <= (unsigned)p.s));
                const bool same = memcmp(hit, model, 256) == 0;   // the per-element form, for every field value
                unsigned every = 0, some = 0;                     // prefix lengths: hit[0 .. every) all set, hit[0 .. some) all clear
                while (every < 256 && hit[every]) ++every;
                while (some < 256 && !hit[some]) ++some;
                for (unsigned w = 0; w <= 8; ++w) {
                    const unsigned fields = 1u << w;
                    const int want = every >= fields ? fl::FOR_CMP_ALL : some >= fields ? fl::FOR_CMP_NONE : fl::FOR_CMP_EACH;
                    uint64_t c;
                    const int got = fl::for_compare_decide(8, p, r, w, c);
                    int what = 0;
                    if (p.none || p.a != lo || p.s != len) what = 3;
                    else if (got != want) what = 1;
                    else if (c != c0 || !same) what = 2;
                    if (what) {
                        if (!wrong) { bad[0] = (int)lo; bad[1] = (int)hi; bad[2] = (int)r; bad[3] = (int)w; bad[4] = what; }
                        ++wrong;
                    }
                }
            }
        }
    return wrong;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "for_range_decide", SHIM, opt="-O3")
    P = ctypes.c_void_p
    lib.for_range_decide_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 9
    lib.for_range_decide_n.restype = None
    lib.for_compare_predicate_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 5
    lib.for_compare_predicate_n.restype = None
    lib.for_range_u8_exhaustive.argtypes = [P]
    lib.for_range_u8_exhaustive.restype = ctypes.c_long
    return lib


def range_decide(shim, T, lo, hi, r, w):
    lo, hi, r = (np.array(x, dtype=np.uint64) for x in (lo, hi, r))
    w = np.array(w, dtype=np.uint8)
    n = lo.size
    a, c, s = (np.empty(n, np.uint64) for _ in range(3))
    none, v = np.empty(n, np.int32), np.empty(n, np.int32)
    shim.for_range_decide_n(T, n, *(x.ctypes.data for x in (lo, hi, r, w, a, c, s, none, v)))
    return a, c, s, none, v


def test_range_decide_u8_exhaustive(shim):
    """Every (lo, hi, reference, W) of u8: the verdict is ALL exactly when every field value f < 2^W hits, NONE exactly when none
    does, EACH otherwise -- and ((f + c) mod 2^T) <= s equals the definition for every f, whatever the verdict."""
    bad = np.zeros(5, np.int32)
    wrong = shim.for_range_u8_exhaustive(bad.ctypes.data)
    assert wrong == 0, (wrong, dict(zip(("lo", "hi", "reference", "W", "what"), bad.tolist())))
    # the shim's own reading of the definition, against numpy, on a few intervals (plain, wrapping, single value, full)
    v = np.arange(256)
    for lo, hi, want in ((10, 20, (v >= 10) & (v <= 20)), (200, 5, (v >= 200) | (v <= 5)), (7, 7, v == 7), (9, 8, v >= 0), (0, 255, v >= 0)):
        a, c, s, none, verdict = range_decide(shim, 8, [lo], [hi], [0], [8])
        assert not none[0] and np.array_equal(((v - int(a[0])) & 255) <= int(s[0]), want), (lo, hi)
        assert verdict[0] == (ALL if want.all() else EACH)


@pytest.mark.parametrize("ty", ["u16", "u32", "u64"])
def test_range_decide_at_the_edges(shim, ty):
    """lo, hi in {0, 1, M-1, M, 2^(T-1)-1, 2^(T-1), r-1, r, r+2^W-1, r+2^W} for references near 0, near M, in the middle, and every
    interesting width.  Membership of (f + r) mod 2^T in the cyclic interval changes only where it crosses lo, passes hi or wraps, so
    evaluating the definition at f = 0, 2^W - 1 and on both sides of those crossings decides ALL / NONE / EACH independently of the
    helper."""
    T = TYPE_BITS[ty]
    N = 1 << T
    M = N - 1
    rng = np.random.default_rng(5150 + T)
    q = []
    for r in (0, 1, M, M - 3, 1 << (T - 1), (1 << (T - 1)) - 2, int(rng.integers(0, M, dtype=np.uint64, endpoint=True))):
        for W in (0, 1, 2, T // 2, T - 1, T):
            span = (1 << W) - 1
            bounds = [0, 1, M - 1, M, (1 << (T - 1)) - 1, 1 << (T - 1), (r - 1) % N, r, (r + span) % N, (r + span + 1) % N]
            q += [(lo, hi, r, W) for lo in bounds for hi in bounds]
    a, c, s, none, v = range_decide(shim, T, *([x[j] for x in q] for j in range(4)))
    seen = set()
    for i, (lo, hi, r, W) in enumerate(q):
        top = (1 << W) - 1
        length = (hi - lo) % N

        def hit(f):
            return ((f + r - lo) % N) <= length
        assert not none[i] and int(a[i]) == lo and int(s[i]) == length, (ty, lo, hi)
        points = {0, top}
        for x in ((lo - r) % N, (hi + 1 - r) % N, (-r) % N):
            points |= {y for y in (x, (x - 1) % N) if y <= top}
        outcomes = {hit(f) for f in points}
        want = ALL if outcomes == {True} else NONE if outcomes == {False} else EACH
        assert int(v[i]) == want, (ty, lo, hi, r, W)
        seen.add(want)
        if want == EACH:
            for f in points:
                assert (((f + int(c[i])) % N) <= int(s[i])) == hit(f), (ty, lo, hi, r, W, f)
    assert seen == {EACH, ALL, NONE}


def _members(T, interval, values):
    """which of `values` (bit patterns) lie in the cyclic interval; None: none of them"""
    if interval is None:
        return [False] * len(values)
    lo, hi = interval
    N = 1 << T
    assert 0 <= lo < N and 0 <= hi < N
    return [((v - lo) % N) <= ((hi - lo) % N) for v in values]


def _signed(T, v):
    return v - (1 << T) if v >> (T - 1) else v


PY = {"==": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
      ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
NP = {"==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}


def test_predicate_interval_u8_exhaustive():
    """six ops x every constant x unsigned / signed, against numpy's comparison on the uint8 / int8 view of all 256 bit patterns"""
    import fastlanes_amd as fl
    bits = np.arange(256, dtype=np.uint8)
    for signed, view, ks in ((False, bits, range(256)), (True, bits.view(np.int8), range(-128, 128))):
        for op in OPS:
            for k in ks:
                iv = fl.predicate_interval("u8", op, k, signed=signed)
                want = NP[op](view, view.dtype.type(k))
                assert (iv is None) == (not want.any()), (op, k, signed)
                assert np.array_equal(np.array(_members(8, iv, list(range(256)))), want), (op, k, signed, iv)
    with pytest.raises(ValueError):
        fl.predicate_interval("u8", "<", 128, signed=True)
    with pytest.raises(ValueError):
        fl.predicate_interval("u8", "<>", 1)
    # the documented example, and the complement rule: [hi + 1, lo - 1] unless the interval is full
    assert fl.predicate_interval("u32", "<", -5, signed=True) == (1 << 31, (1 << 32) - 6)
    for op, k in (("<", 17), (">=", 200), ("==", 0), ("!=", 255)):
        lo, hi = fl.predicate_interval("u8", op, k)
        comp = _members(8, ((hi + 1) % 256, (lo - 1) % 256), list(range(256)))
        assert comp == [not m for m in _members(8, (lo, hi), list(range(256)))]


@pytest.mark.parametrize("ty", ["u16", "u32", "u64"])
def test_predicate_interval_edge_constants(shim, ty):
    """the wider types at the edge constants, on the bit patterns around every edge, against Python's integers; and for unsigned the
    same set of satisfying values as for_compare_predicate gives unfor_compare"""
    import fastlanes_amd as fl
    T = TYPE_BITS[ty]
    N = 1 << T
    H = N >> 1
    edges = sorted({x % N for e in (0, 1, H - 1, H, H + 1, N - 2, N - 1, 12345 % N, N - 77) for x in (e - 1, e, e + 1)})
    for signed in (False, True):
        ks = sorted({_signed(T, e) for e in edges}) if signed else edges
        for op in OPS:
            for k in ks:
                iv = fl.predicate_interval(ty, op, k, signed=signed)
                want = [PY[op](_signed(T, v) if signed else v, k) for v in edges]
                assert _members(T, iv, edges) == want, (ty, op, k, signed, iv)
                below = k + H if signed else k                             # how many values are smaller than k
                n_sat = {"==": 1, "!=": N - 1, "<": below, "<=": below + 1, ">": N - below - 1, ">=": N - below}[op]
                assert (0 if iv is None else (iv[1] - iv[0]) % N + 1) == n_sat, (ty, op, k, signed, iv)
    # unsigned: the predicate unfor_compare reduces the same (op, constant) to
    q = [(o, k) for o in range(6) for k in edges]
    op, k = np.array([x[0] for x in q], np.int32), np.array([x[1] for x in q], np.uint64)
    a, s, none = np.empty(len(q), np.uint64), np.empty(len(q), np.uint64), np.empty(len(q), np.int32)
    shim.for_compare_predicate_n(T, len(q), *(x.ctypes.data for x in (op, k, a, s, none)))
    for i, (o, kk) in enumerate(q):
        iv = fl.predicate_interval(ty, OPS[o], kk)
        assert (iv is None) == bool(none[i]), (ty, OPS[o], kk)
        if iv is not None:
            assert (iv[1] - iv[0]) % N == int(s[i]) and (int(s[i]) == N - 1 or iv[0] == int(a[i])), (ty, OPS[o], kk, iv)


def test_cpp_mirror_declares_both_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the two new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint32_t;
void (*const uniform)(std::size_t, const T*, const T*, std::size_t, T, T, fl_mask_combine, const std::uint32_t*, std::size_t, std::uint32_t*,
                      void*) = &fastlanes::FoR<T>::unfor_compare_range_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, T, T, fl_mask_combine,
                    const std::uint32_t*, std::size_t, std::uint32_t*, std::uint32_t*, void*) = &fastlanes::unfor_compare_range_widths_device<T>;
static_assert(FL_MASK_NEW == 0 && FL_MASK_AND == 1 && FL_MASK_OR == 2, "fl_mask_combine");
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
