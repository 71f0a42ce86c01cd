"""CPU: undelta_compare_range / undelta_compare_range_widths (interval predicates over Delta-packed columns, chained through a mask).
  * the block decision of fastlanes_amd/csrc/fl_delta_decide.hpp, compiled here for the host, is SOUND -- exhaustively over the 8-bit
    domain, at the wrap and saturation edges for u16 / u32 / u64 -- and not vacuous (the verdict counts are pinned);
  * the routes of fl_delta_compare_range_map.hpp keep their order, and its group placement is lane_base;
  * a numpy model of the group placement (no value is untransposed) equals the oracle's untranspose(undelta_pack(..)) for all four types;
  * the header declares and the library exports the eight symbols through a macro of their own, their argument checks need no GPU, the
    Python mirror validates before any launch, the C++ mirror compiles."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import delta_compare_range_data as dd
from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)
from datagen import values
from oracle_lib import lanes, packed_len

EACH, ALL, NONE, BASES = 0, 1, 2, 3
NEW, AND, OR = 0, 1, 2

SHIM = r"""
#include "fl_delta_compare_range_map.hpp"
#include <stddef.h>
// What the kernel does with a block: the interval -> the predicate, c_l = (base_l - a) mod 2^T, cmin / cmax over the lanes, the verdict
extern "C" void delta_decide_n(unsigned type_bits, size_t n, size_t n_lanes, const uint64_t* lo, const uint64_t* hi, const uint64_t* bases,
                               const uint8_t* width, uint64_t* cmin, uint64_t* cmax, uint64_t* reach, int* verdict)
{
    const uint64_t M = fl::type_max(type_bits);
    for (size_t i = 0; i < n; ++i) {
        const fl::ForPredicate p = fl::for_range_predicate(type_bits, lo[i], hi[i]);
        uint64_t mn = ~0ull, mx = 0;
        for (size_t l = 0; l < n_lanes; ++l) {
            const uint64_t c = (bases[i * n_lanes + l] - p.a) & M;
            mn = c < mn ? c : mn;
            mx = c > mx ? c : mx;
        }
        cmin[i] = mn;
        cmax[i] = mx;
        reach[i] = fl::delta_reach(type_bits, width[i]);
        verdict[i] = fl::delta_compare_decide(type_bits, p, mn, mx, width[i]);
    }
}
// u8, a = 0 (the rule only sees c = base - a), every s, every W in 0..8, every cmin <= cmax.  Lane l's values are c_l + k for k = the
// sum of 1 .. 8 deltas of [0, 2^W - 1]; c_l may be ANY value of [cmin, cmax] and k any value of [0, reach], reach = 8 (2^W - 1), so the
// sums the verdict must hold for are every integer x of [cmin, cmax + reach], judged by the definition (x mod 256) <= s.
// counts[verdict] += 1; returns the number of unsound verdicts, the first one in bad[0..3] = (s, W, cmin, cmax).
extern "C" long delta_decide_u8_exhaustive(long* counts, int* bad)
{
    long wrong = 0;
    for (unsigned s = 0; s < 256; ++s) {
        const fl::ForPredicate p = fl::for_range_predicate(8, 0, s);
        for (unsigned w = 0; w <= 8; ++w) {
            const unsigned reach = 8u * ((1u << w) - 1u);
            for (unsigned cmin = 0; cmin < 256; ++cmin)
                for (unsigned cmax = cmin; cmax < 256; ++cmax) {
                    const int v = fl::delta_compare_decide(8, p, cmin, cmax, w);
                    ++counts[v];
                    bool sound = true;
                    if (v == fl::DELTA_CMP_ALL || v == fl::DELTA_CMP_NONE) {
                        const unsigned last = cmax + reach < cmin + 255u ? cmax + reach : cmin + 255u;   // 256 consecutive x cover every residue
                        for (unsigned x = cmin; x <= last && sound; ++x) sound = ((x & 255u) <= s) == (v == fl::DELTA_CMP_ALL);
                    } else if (v == fl::DELTA_CMP_BASES) {
                        sound = w == 0;
                    } else {
                        sound = v == fl::DELTA_CMP_EACH && w != 0;
                    }
                    if (!sound) {
                        if (!wrong) { bad[0] = (int)s; bad[1] = (int)w; bad[2] = (int)cmin; bad[3] = (int)cmax; }
                        ++wrong;
                    }
                }
        }
    }
    return wrong;
}
extern "C" int delta_route(unsigned type_bits, uint64_t lo, uint64_t hi, int ok, int live, uint64_t cmin, uint64_t cmax, unsigned width)
{
    return fl::delta_range_route(type_bits, fl::for_range_predicate(type_bits, lo, hi), ok != 0, live != 0, cmin, cmax, width);
}
extern "C" int delta_route_reads(int route) { return (fl::delta_range_reads_bases((fl::DeltaRangeRoute)route) ? 1 : 0) | (fl::delta_range_reads_packed((fl::DeltaRangeRoute)route) ? 2 : 0); }
extern "C" unsigned delta_group_bit_of(unsigned l) { return fl::delta_group_bit(l); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "delta_decide", SHIM, opt="-O3")
    P = ctypes.c_void_p
    so.delta_decide_n.argtypes = [ctypes.c_uint, ctypes.c_size_t, ctypes.c_size_t] + [P] * 8
    so.delta_decide_n.restype = None
    so.delta_decide_u8_exhaustive.argtypes = [P, P]
    so.delta_decide_u8_exhaustive.restype = ctypes.c_long
    so.delta_route.argtypes = [ctypes.c_uint, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint]
    so.delta_route.restype = ctypes.c_int
    so.delta_route_reads.argtypes = [ctypes.c_int]
    so.delta_route_reads.restype = ctypes.c_int
    so.delta_group_bit_of.argtypes = [ctypes.c_uint]
    so.delta_group_bit_of.restype = ctypes.c_uint
    return so


def decide(shim, T, queries):
    """queries: [(lo, hi, bases, W)] -> (cmin, cmax, reach, verdict) arrays"""
    n, L = len(queries), len(queries[0][2])
    lo, hi = (np.array([q[j] for q in queries], dtype=np.uint64) for j in (0, 1))
    bases = np.array([q[2] for q in queries], dtype=np.uint64).reshape(-1)
    w = np.array([q[3] for q in queries], dtype=np.uint8)
    cmin, cmax, reach = (np.empty(n, np.uint64) for _ in range(3))
    v = np.empty(n, np.int32)
    shim.delta_decide_n(T, n, L, *(x.ctypes.data for x in (lo, hi, bases, w, cmin, cmax, reach, v)))
    return cmin, cmax, reach, v


# ---- 1. the decision is sound, exhaustively over the 8-bit domain ------------------------------------------------------------------
# every (s, W, cmin <= cmax): 256 * 9 * 32896 cases.  The counts are pinned so that a rule that decides nothing (or everything) fails;
# they are those of the rule as the header's comment states it, counted apart from the header in exact integers (numpy).
U8_CASES = 256 * 9 * (256 * 257 // 2)
U8_COUNTS = {EACH: 54356072, ALL: 9468108, NONE: 9172044, BASES: 2796160}


def test_decision_is_sound_for_every_8_bit_case_and_not_vacuous(shim):
    counts = np.zeros(4, dtype=np.int64)
    bad = np.zeros(4, dtype=np.int32)
    wrong = shim.delta_decide_u8_exhaustive(counts.ctypes.data, bad.ctypes.data)
    assert wrong == 0, (wrong, dict(zip(("s", "W", "cmin", "cmax"), bad.tolist())))
    assert int(counts.sum()) == U8_CASES
    assert dict(enumerate(counts.tolist())) == U8_COUNTS


def test_decision_is_translation_invariant(shim):
    """(bases + t, lo + t, hi + t) decides as (bases, lo, hi) does: the rule sees only c_l = base_l - lo and s = hi - lo"""
    rng = np.random.default_rng(4100)

    def below(n):
        return int.from_bytes(rng.bytes(9), "little") % n

    for ty, T in TYPE_BITS.items():
        N, L = 1 << T, lanes(ty)
        qs, moved = [], []
        for k in range(300):
            w = below(T + 1) if k % 2 else below(4)
            centre, spread = below(N), 1 << below(T)
            bases = [(centre + below(spread)) % N for _ in range(L)]
            lo = (centre - below(4 * spread)) % N
            hi = (lo + below(min(N, 8 * spread + 2 * T * (1 << w)))) % N
            t = below(N)
            qs.append((lo, hi, bases, w))
            moved.append(((lo + t) % N, (hi + t) % N, [(b + t) % N for b in bases], w))
        a, b = decide(shim, T, qs), decide(shim, T, moved)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), ty
        assert set(a[3].tolist()) == {EACH, ALL, NONE, BASES}, (ty, set(a[3].tolist()))


# ---- 2. the wider types at the wrap and saturation edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("ty", ["u16", "u32", "u64"])
def test_decision_at_the_wrap_and_saturation_edges(shim, ty):
    """reach just below, at and above s - cmax (ALL) and M - cmax (NONE), bases on both sides of s and of the wrap, widths whose reach
    approaches and passes 2^T (u64: W >= 59 saturates the 64-bit reach) -- against the rule in Python's exact integers"""
    T = TYPE_BITS[ty]
    N = 1 << T
    M = N - 1
    L = lanes(ty)
    widths = sorted({0, 1, 2, T // 2, T - 6, T - 5, T - 4, T - 3, T - 2, T - 1, T})
    qs = []
    for w in widths:
        reach = T * ((1 << w) - 1)
        for lo in (0, 7, N >> 1, M - 2):
            for gap in (-2, -1, 0, 1, 2):
                for spread in (0, 1, 5):
                    # ALL edge: cmax + reach = s + gap
                    for s in (reach + spread + 9, M - 1, (M >> 1) + 3):
                        cmax = s + gap - reach
                        if 0 <= cmax - spread and cmax <= M and s <= M:
                            cs = [cmax - spread] + [cmax] * (L - 1)
                            qs.append((lo, (lo + s) % N, [(c + lo) % N for c in cs], w))
                    # NONE edge: cmax + reach = M + gap, cmin on both sides of s
                    cmax = M + gap - reach
                    if spread <= cmax <= M:
                        for s in (cmax - spread - 1, cmax - spread, 0, 3):
                            if 0 <= s < M:
                                cs = [cmax] + [cmax - spread] * (L - 1)
                                qs.append((lo, (lo + s) % N, [(c + lo) % N for c in cs], w))
        # the full interval, a single value, bases that straddle the wrap
        qs.append((5, 4, [0, M] * (L // 2), w))
        qs.append((9, 9, [9] * L, w))
        qs.append((M, 1, [M, 0] * (L // 2), w))
    cmin, cmax, reach, v = decide(shim, T, qs)
    seen = set()
    for i, (lo, hi, bases, w) in enumerate(qs):
        want = dd.verdict_of(T, lo, hi, bases, w)
        assert int(v[i]) == want, (ty, lo, hi, bases[:2], w, int(v[i]), want)
        mn, mx, exact = dd.bases_range(T, lo, bases, w)
        assert (int(cmin[i]), int(cmax[i]), int(reach[i])) == (mn, mx, min(exact, (1 << 64) - 1)), (ty, i)
        seen.add(want)
    assert seen == {EACH, ALL, NONE, BASES}
    if ty == "u64":                                                         # 64 (2^W - 1) passes 2^64 - 1 from W = 59 on
        for w in range(56, 65):
            r = int(decide(shim, 64, [(0, 1, [0] * L, w)])[2][0])
            assert r == min(64 * ((1 << w) - 1), (1 << 64) - 1) and (r == (1 << 64) - 1) == (w >= 59), w


def test_routes_keep_their_order_and_the_groups_tile_the_mask(shim):
    SKIP_, KEEP_, ALL_, NONE_, BASES_, EACH_ = range(6)
    for T in (8, 16, 32, 64):
        M = (1 << T) - 1
        for w in (0, 3, T):
            # (lo, hi, cmin, cmax) for the four verdicts at width w
            decided = {ALL_: (0, M, 1, 2), NONE_: (0, 0, 1, 1) if w == 0 else (7, 6 - 1, 0, 0)}
            for ok in (0, 1):
                for live in (0, 1):
                    r = shim.delta_route(T, 5, 4, ok, live, 1, 2, w)       # the full interval: ALL whenever the decision is reached
                    assert r == (SKIP_ if not ok else KEEP_ if not live else ALL_), (T, w, ok, live)
            assert shim.delta_route(T, 0, 0, 1, 1, 1, 1, 0) == NONE_
            assert shim.delta_route(T, 0, 0, 1, 1, 0, 1, 0) == BASES_      # width 0 with mixed bases
            assert shim.delta_route(T, 0, 0, 1, 1, 0, 1, 1) == EACH_
            assert decided
    assert [shim.delta_route_reads(r) for r in range(6)] == [0, 0, 1, 1, 1, 3]   # bit 0: bases needed, bit 1: packed bytes requested
    for ty, T in TYPE_BITS.items():
        bits = [shim.delta_group_bit_of(l) for l in range(1024 // T)]
        assert bits == [dd.lane_base(l) for l in range(1024 // T)]
        assert sorted(bits) == list(range(0, 1024, T)), ty                 # a permutation of {0, T, 2T, ..}: T-bit aligned groups


# ---- 3. the placement model against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", list(TYPE_BITS))
def test_group_placement_model_equals_untranspose_of_undelta_pack(oracle, ty):
    """Summing each lane's chain and placing its T verdicts at lane_base(l) gives the mask of the untransposed decoded block: random
    packed bytes and bases (the values wrap), every interesting width, plain / wrapping / single-value intervals"""
    T = TYPE_BITS[ty]
    N = 1 << T
    L = lanes(ty)
    rng = np.random.default_rng(4200 + T)
    for w in sorted({0, 1, 3, T // 2, T - 1, T}):
        pk = values(ty, packed_len(ty, w), 4300 + 64 * T + w)
        bases = values(ty, L, 4400 + 64 * T + w)
        vals = oracle.untranspose(ty, oracle.undelta_pack(ty, w, pk, bases))
        v0, v1 = int(vals[int(rng.integers(0, 1024))]), int(vals[int(rng.integers(0, 1024))])
        for lo, hi in ((v0, v1), (v1, v0), (v0, v0), (int(bases[3]), (int(bases[3]) + (N >> 2)) % N), (0, N >> 1)):
            got = dd.placement_model(ty, w, pk, bases, lo, hi)
            assert np.array_equal(got, dd.want_mask(vals, lo, hi)), (ty, w, lo, hi)
    # a sorted block: ONE row's verdict flips at each end of the interval
    v, widths, blocks, bases = dd.sorted_column(oracle, ty, 3, 4500 + T)
    for b, (w, pk) in enumerate(blocks):
        vb = v[b * 1024:(b + 1) * 1024]
        for r in dd.edge_rows(ty)[::3]:
            lo, hi = int(vb[r]), int(vb[min(r + T // 8, 1023)])
            assert np.array_equal(dd.placement_model(ty, w, pk, bases[b * L:(b + 1) * L], lo, hi), dd.want_mask(vb, lo, hi)), (ty, b, r)


def test_the_definitions_own_decision_is_sound_on_random_blocks(oracle):
    """tests/delta_compare_range_data.py: verdict_of (what the GPU tests count routes with) never claims ALL / NONE / BASES wrongly"""
    for ty, T in TYPE_BITS.items():
        N, L = 1 << T, lanes(ty)
        rng = np.random.default_rng(4600 + T)
        seen = set()
        for k in range(60):
            w = [0, 1, 2, 3][k % 4]
            pk = values(ty, packed_len(ty, w), 4700 + k)
            b0 = int(rng.integers(0, N, dtype=np.uint64))
            bases = np.array([(b0 + int(x)) % N for x in rng.integers(0, 3 if k % 3 else 1, size=L)], dtype=pk.dtype)
            vals = oracle.untranspose(ty, oracle.undelta_pack(ty, w, pk, bases))
            reach = T * ((1 << w) - 1)
            for lo, hi in ((b0, (b0 + reach + 2) % N), ((b0 + reach + 3) % N, (b0 - 1) % N), (b0 + 1, (b0 + 1 + reach // 2) % N), (b0, b0)):
                lo %= N
                v = dd.verdict_of(T, lo, hi, bases, w)
                hits = dd.hit_bits(vals, lo, hi)
                seen.add(v)
                if v == ALL:
                    assert hits.all(), (ty, k)
                elif v == NONE:
                    assert not hits.any(), (ty, k)
                elif v == BASES:
                    assert w == 0 and np.array_equal(vals, oracle.untranspose(ty, np.tile(bases, T))), (ty, k)
        assert seen == {EACH, ALL, NONE, BASES}, (ty, seen)


# ---- 4. exports, refusals, mirrors -------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_eight_symbols(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_DELTA_COMPARE_RANGE(T, S)")[1].split("FL_DECLARE_DELTA_COMPARE_RANGE(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == list(dd.FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_DELTA_COMPARE_RANGE({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in dd.FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.delta_compare_range_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.for_compare_range_symbols(),
                  fastlanes_amd.select_symbols(), fastlanes_amd.aggregate_symbols(), fastlanes_amd.aggregate_by_lookup_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"delta_compare_range_symbols", "undelta_compare_range_widths"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.Delta, "undelta_compare_range")


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), in unfor_compare_range's order: width, combine, the
    empty column, NULL pointers, alignment -- `bases` among the required and the 16-byte aligned pointers."""
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_undelta_compare_range")
        g = getattr(lib, f"fl_{ty}_undelta_compare_range_widths")
        # f(width, in, bases, lo, hi, combine, mask_in, n, mask, stream)
        # g(widths, offsets, packed, packed_bytes, bases, lo, hi, combine, mask_in, n, mask, err, stream)
        for cb in (NEW, AND, OR):
            assert f(3, None, None, 1, 2, cb, None, 0, None, None) == 0
            assert g(None, None, None, 0, None, 1, 2, cb, None, 0, None, None, None) == 0
            assert f(T + 1, p, p, 1, 2, cb, p, 1, p, None) == 1
            assert f(T + 1, p, p, 1, 2, cb, p, 0, p, None) == 1
        assert f(T + 1, p, p, 1, 2, 7, p, 0, p, None) == 1                  # the width ahead of a bad combine
        for cb in (-1, 3, 99):
            assert f(3, p, p, 1, 2, cb, p, 1, p, None) == 2
            assert f(3, p, p, 1, 2, cb, p, 0, p, None) == 2
            assert g(p, p, p, 128, p, 1, 2, cb, p, 1, p, None, None) == 2
            assert g(p, p, p, 128, p, 1, 2, cb, p, 0, p, None, None) == 2
        for cb in (AND, OR):
            assert f(3, p, p, 1, 2, cb, None, 1, p, None) == 3
            assert g(p, p, p, 128, p, 1, 2, cb, None, 1, p, None, None) == 3
        for cb in (NEW, AND, OR):
            assert f(3, p, None, 1, 2, cb, p, 1, p, None) == 3             # bases
            assert f(3, p, p, 1, 2, cb, p, 1, None, None) == 3             # mask
            assert f(3, None, p, 1, 2, cb, p, 1, p, None) == 3             # W > 0 reads data
            assert f(0, None, p, 1, 2, cb, p, 1, p + 4, None) == 4         # W = 0 needs none: on to the misaligned mask
            assert g(None, p, p, 128, p, 1, 2, cb, p, 1, p, None, None) == 3
            assert g(p, None, p, 128, p, 1, 2, cb, p, 1, p, None, None) == 3
            assert g(p, p, None, 128, p, 1, 2, cb, p, 1, p, None, None) == 3
            assert g(p, p, p, 128, None, 1, 2, cb, p, 1, p, None, None) == 3
            assert g(p, p, p, 128, p, 1, 2, cb, p, 1, None, None, None) == 3
            assert f(3, p + 8, p, 1, 2, cb, p, 1, p, None) == 4
            assert f(3, p, p + 8, 1, 2, cb, p, 1, p, None) == 4            # bases are read as 16-byte cells
            assert f(3, p, p, 1, 2, cb, p, 1, p + 4, None) == 4
            assert g(p, p, p + 8, 128, p, 1, 2, cb, p, 1, p, None, None) == 4
            assert g(p, p, p, 128, p + 8, 1, 2, cb, p, 1, p, None, None) == 4
            assert g(p, p, p, 128, p, 1, 2, cb, p, 1, p + 8, None, None) == 4
        for cb in (AND, OR):
            assert f(3, p, p, 1, 2, cb, p + 4, 1, p, None) == 4
            assert g(p, p, p, 128, p, 1, 2, cb, p + 8, 1, p, None, None) == 4
        # NEW ignores mask_in: NULL or misaligned, every remaining refusal is about another argument
        assert f(3, p, p, 1, 2, NEW, None, 1, None, None) == 3
        assert f(3, p, p, 1, 2, NEW, p + 4, 1, p + 4, None) == 4
        assert g(p, p, p, 128, p, 1, 2, NEW, None, 1, p + 8, None, None) == 4


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tbase, tmask = torch.zeros(96, dtype=torch.int32), torch.zeros(32, dtype=torch.int32), torch.zeros(32, dtype=torch.int32)
    with pytest.raises(TypeError):
        fl.Delta.undelta_compare_range(3, np.zeros(96, dtype=np.uint32), np.zeros(32, dtype=np.uint32), 1, 2)
    with pytest.raises(TypeError):
        fl.Delta.undelta_compare_range(3, tcol, tbase, 1, 2)
    with pytest.raises(TypeError):
        fl.undelta_compare_range_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(32, np.uint32), 1, 2)
    with pytest.raises(TypeError):
        fl.undelta_compare_range_widths(tw, to, tcol, tbase, 1, 2, mask=tmask, combine="or")
    for bad in ("xor", "AND", 1, None):
        with pytest.raises(ValueError):
            fl.Delta.undelta_compare_range(3, tcol, tbase, 1, 2, mask=tmask, combine=bad)
        with pytest.raises(ValueError):
            fl.undelta_compare_range_widths(tw, to, tcol, tbase, 1, 2, mask=tmask, combine=bad)
    for cb in ("and", "or"):
        with pytest.raises(ValueError):
            fl.Delta.undelta_compare_range(3, tcol, tbase, 1, 2, combine=cb)
        with pytest.raises(ValueError):
            fl.undelta_compare_range_widths(tw, to, tcol, tbase, 1, 2, combine=cb)
    for words in (0, 31, 33, 64):
        with pytest.raises(ValueError):
            fl.undelta_compare_range_widths(tw, to, tcol, tbase, 1, 2, mask=torch.zeros(words, dtype=torch.int32), combine="and")


def test_cpp_mirror_declares_both_forms(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint32_t;
void (*const uniform)(std::size_t, const T*, const T*, T, T, fl_mask_combine, const std::uint32_t*, std::size_t, std::uint32_t*, void*) =
    &fastlanes::Delta<T>::undelta_compare_range_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, T, T, fl_mask_combine, const std::uint32_t*,
                    std::size_t, std::uint32_t*, std::uint32_t*, void*) = &fastlanes::undelta_compare_range_widths_device<T>;
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
