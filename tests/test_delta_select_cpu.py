"""CPU: undelta_select / undelta_select_widths (the rows a mask keeps of a Delta-packed column, compacted in original row order).
  * the routes of fastlanes_amd/csrc/fl_delta_select_map.hpp, compiled here for the host, keep their order SKIP > EMPTY > BOUNDS > BASES >
    EACH, and its landing of every (FastLanes lane l, row r) equals the definition -- the mask bits of the block below original row
    lane_base(l) + r -- for all four types under empty, full, one-bit, one-bit-clear, run and random masks, every landing in [0, count)
    hit exactly once;
  * a numpy lane-group model of the select (chains summed along their rows, each kept row written straight to its landing, no value
    untransposed) equals the definition's run over the oracle's untranspose(undelta_pack(..));
  * the header declares and the library exports the eight symbols through a macro of their own, every refusal is returned without a GPU
    and in order, the Python mirror validates before any launch, the C++ mirror compiles."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import delta_compare_range_data as dd
import delta_select_data as ds
from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)
from datagen import values
from oracle_lib import lanes, packed_len

SHIM = r"""
#include "fl_delta_select_map.hpp"
extern "C" int dsel_route(int ok, int empty, int inside, unsigned width) { return fl::delta_select_route(ok != 0, empty != 0, inside != 0, width); }
extern "C" int dsel_route_does(int route)
{
    const fl::DeltaSelectRoute r = (fl::DeltaSelectRoute)route;
    return (fl::delta_select_reads_bases(r) ? 1 : 0) | (fl::delta_select_reads_packed(r) ? 2 : 0) | (fl::delta_select_writes(r) ? 4 : 0);
}
// landing[l * type_bits + r] of every (FastLanes lane, row) of the block, kept or not; returns the block's count
extern "C" unsigned dsel_landings(unsigned type_bits, const uint32_t* mask, unsigned* landing)
{
    unsigned scan[32];
    const unsigned count = fl::delta_select_scan_words(mask, scan);
    for (unsigned l = 0; l < 1024u / type_bits; ++l)
        for (unsigned r = 0; r < type_bits; ++r) landing[l * type_bits + r] = fl::delta_select_block_landing(type_bits, mask, scan, l, r);
    return count;
}
extern "C" unsigned dsel_group_bit(unsigned l) { return fl::delta_group_bit(l); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "delta_select", SHIM)
    so.dsel_route.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    so.dsel_route.restype = ctypes.c_int
    so.dsel_route_does.argtypes = [ctypes.c_int]
    so.dsel_route_does.restype = ctypes.c_int
    so.dsel_landings.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    so.dsel_landings.restype = ctypes.c_uint
    so.dsel_group_bit.argtypes = [ctypes.c_uint]
    so.dsel_group_bit.restype = ctypes.c_uint
    return so


# ---- 1. the routes and the landing map ----------------------------------------------------------------------------------------------
def test_routes_keep_their_order(shim):
    for T in TYPE_BITS.values():
        for w in (0, 1, T // 2, T):
            for ok in (0, 1):
                for empty in (0, 1):
                    for inside in (0, 1):
                        mask_block = np.zeros(32, np.int32) if empty else np.ones(32, np.int32)
                        assert shim.dsel_route(ok, empty, inside, w) == ds.route_of(bool(ok), mask_block, bool(inside), w), (T, w, ok, empty, inside)
            assert shim.dsel_route(0, 1, 0, w) == ds.SKIP                   # SKIP ahead of everything
            assert shim.dsel_route(1, 1, 0, w) == ds.EMPTY                  # EMPTY ahead of BOUNDS: an empty block has no run to place
            assert shim.dsel_route(1, 0, 0, w) == ds.BOUNDS                 # BOUNDS ahead of BASES and EACH
            assert shim.dsel_route(1, 0, 1, w) == (ds.BASES if w == 0 else ds.EACH)
    assert (ds.SKIP, ds.EMPTY, ds.BOUNDS, ds.BASES, ds.EACH) == (0, 1, 2, 3, 4)
    # bit 0: bases used, bit 1: packed bytes requested, bit 2: a run stored
    assert [shim.dsel_route_does(r) for r in range(5)] == [0, 0, 0, 5, 7]
    for ty, T in TYPE_BITS.items():
        assert [shim.dsel_group_bit(l) for l in range(1024 // T)] == [dd.lane_base(l) for l in range(1024 // T)], ty


def landing_masks(ty):
    """(name, bool[1024]) of every mask the landing map is checked under"""
    T = TYPE_BITS[ty]
    R = T // 8
    rng = np.random.default_rng(6100 + T)
    yield "empty", np.zeros(1024, bool)
    yield "full", np.ones(1024, bool)
    for r in dd.edge_rows(ty):
        one = np.zeros(1024, bool)
        one[r] = True
        yield f"bit {r}", one
        yield f"all but bit {r}", ~one
    # runs [r0, r1] that cross an R-piece, a T-group, a 32-bit word and a 64-row boundary
    for r0, r1 in ((R - 1, R), (T - 1, T), (31, 32), (63, 64), (3 * T + R - 1, 3 * T + R), (5 * T - 2, 5 * T + 1), (95, 96), (127, 129),
                   (447, 449), (511, 512), (R, 1024 - R - 1), (T // 2, 64 + T // 2), (1, 1022), (960 - 1, 960 + T)):
        run = np.zeros(1024, bool)
        run[r0:r1 + 1] = True
        yield f"rows {r0}..{r1}", run
        yield f"all but rows {r0}..{r1}", ~run
    for k in range(4):
        yield f"random 2 % #{k}", rng.random(1024) < 0.02
        yield f"random 50 % #{k}", rng.random(1024) < 0.5


@pytest.mark.parametrize("ty", list(TYPE_BITS))
def test_landing_of_every_row_equals_the_definition(shim, ty):
    T = TYPE_BITS[ty]
    L = 1024 // T
    position = np.array([dd.lane_base(l) + r for l in range(L) for r in range(T)])
    assert sorted(position) == list(range(1024))                            # the chains tile the block
    seen = 0
    for name, bits in landing_masks(ty):
        words = np.packbits(bits, bitorder="little").view(np.uint32).copy()
        got = np.zeros(1024, dtype=np.uint32)
        count = shim.dsel_landings(T, words.ctypes.data, got.ctypes.data)
        assert count == int(bits.sum()), (ty, name)
        below = np.concatenate([[0], np.cumsum(bits)])                      # rank(p) = the mask bits below original row p
        assert np.array_equal(got, below[position]), (ty, name)
        assert got[0] == ds.landing_of(bits, dd.lane_base(0)) and got[-1] == ds.landing_of(bits, dd.lane_base(L - 1) + T - 1)
        kept = got[bits[position]]
        assert sorted(kept.tolist()) == list(range(count)), (ty, name)      # every landing in [0, count) is hit exactly once
        seen += 1
    assert seen >= 2 + 2 * len(dd.edge_rows(ty)) + 28 + 8


# ---- 2. the lane-group model against the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", list(TYPE_BITS))
def test_lane_group_model_equals_the_definition(oracle, ty):
    """widths 0, 1, T/2 and T, random packed bytes and bases (the chains wrap), random masks, sparse ones, one-bit ones, runs, full"""
    T = TYPE_BITS[ty]
    L = lanes(ty)
    rng = np.random.default_rng(6200 + T)
    for w in (0, 1, T // 2, T):
        pk = values(ty, packed_len(ty, w), 6300 + 64 * T + w)
        bases = values(ty, L, 6400 + 64 * T + w)
        vals = oracle.untranspose(ty, oracle.undelta_pack(ty, w, pk, bases))
        masks = [rng.integers(0, 1 << 32, size=32, dtype=np.uint64).astype(np.uint32).view(np.int32),
                 np.packbits(rng.random(1024) < 0.02, bitorder="little").view(np.int32), np.full(32, -1, np.int32), np.zeros(32, np.int32)]
        masks += [ds.rows_mask(1, 0, r, r) for r in (0, T - 1, T, 519, 1023)]
        masks += [ds.rows_mask(1, 0, r0, r1) for r0, r1 in ((T - 1, T), (31, 64), (500, 530))]
        for k, m in enumerate(masks):
            got = ds.lane_group_model(ty, w, pk, bases, m)
            want, _ = ds.want_run(vals, m)
            assert got.dtype == want.dtype and np.array_equal(got, want), (ty, w, k)


# ---- 3. exports, refusals, mirrors -------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_eight_symbols(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_DELTA_SELECT(T, S)")[1].split("FL_DECLARE_DELTA_SELECT(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == list(ds.FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_DELTA_SELECT({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in ds.FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.delta_select_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.select_symbols(), fastlanes_amd.aggregate_symbols(),
                  fastlanes_amd.delta_compare_range_symbols(), fastlanes_amd.delta_aggregate_symbols(), fastlanes_amd.for_compare_symbols(),
                  fastlanes_amd.for_compare_range_symbols(), fastlanes_amd.aggregate_by_symbols(), fastlanes_amd.aggregate_columns_symbols(),
                  fastlanes_amd.lookup_symbols(), fastlanes_amd.set_build_symbols(), fastlanes_amd.for_compare_columns_symbols(),
                  fastlanes_amd.for_compare_in_symbols(), fastlanes_amd.aggregate_by_columns_symbols(), fastlanes_amd.aggregate_by_window_symbols(),
                  fastlanes_amd.aggregate_by_lookup_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"delta_select_symbols", "undelta_select_widths"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.Delta, "undelta_select")
    import __graft_entry__ as ge
    import inspect
    assert "delta_select_symbols()" in inspect.getsource(ge.build)            # the build's symbol check includes them


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), in unfor_select's order: width, the empty column, NULL
    pointers, alignment -- `bases` among the required and the 16-byte aligned pointers, `out` NULL allowed with out_len == 0, `err_flag`
    optional."""
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_undelta_select")
        g = getattr(lib, f"fl_{ty}_undelta_select_widths")
        # f(width, in, bases, mask, out_offsets, out, out_len, n, err, stream)
        # g(widths, offsets, packed, packed_bytes, bases, mask, out_offsets, out, out_len, n, err, stream)
        assert f(3, None, None, None, None, None, 0, 0, None, None) == 0    # the empty column: nothing else is looked at
        assert f(T, p + 8, p + 8, p + 4, p + 4, p + 8, 5, 0, None, None) == 0
        assert g(None, None, None, 0, None, None, None, None, 0, 0, None, None) == 0
        assert f(T + 1, p, p, p, p, p, 8, 1, None, None) == 1               # width > T
        assert f(T + 1, p, p, p, p, p, 8, 0, None, None) == 1               # ... also for an empty column
        assert f(T + 1, None, None, None, None, None, 0, 1, None, None) == 1   # ... ahead of the NULL pointers
        assert f(T + 1, p + 8, p, p, p, p, 8, 1, None, None) == 1           # ... and of the alignment
        assert f(3, p, None, p, p, p, 8, 1, None, None) == 3                # bases
        assert f(3, p, p, None, p, p, 8, 1, None, None) == 3                # mask
        assert f(3, p, p, p, None, p, 8, 1, None, None) == 3                # out_offsets
        assert f(3, p, p, p, p, None, 8, 1, None, None) == 3                # out, with out_len > 0
        assert f(3, None, p, p, p, p, 8, 1, None, None) == 3                # W > 0 reads data
        assert f(3, None, p + 8, p, p, p, 8, 1, None, None) == 3            # NULL ahead of alignment
        assert f(3, p, p, None, p, p + 8, 8, 1, None, None) == 3
        assert f(0, None, p, p, p, p + 8, 8, 1, None, None) == 4            # W = 0 needs no data: on to the misaligned output
        assert f(0, None, None, p, p, p, 8, 1, None, None) == 3             # ... but its bases
        assert f(3, p, p + 8, p, p, None, 0, 1, None, None) == 4            # out == NULL with out_len == 0 is allowed: on to the bases' alignment
        assert f(3, p, p, p + 4, p, None, 0, 1, None, None) == 4
        assert g(None, p, p, 128, p, p, p, p, 8, 1, None, None) == 3
        assert g(p, None, p, 128, p, p, p, p, 8, 1, None, None) == 3
        assert g(p, p, None, 128, p, p, p, p, 8, 1, None, None) == 3        # packed_bytes > 0: bytes can be read
        assert g(p, p, p, 128, None, p, p, p, 8, 1, None, None) == 3
        assert g(p, p, p, 128, p, None, p, p, 8, 1, None, None) == 3
        assert g(p, p, p, 128, p, p, None, p, 8, 1, None, None) == 3
        assert g(p, p, p, 128, p, p, p, None, 8, 1, None, None) == 3
        assert g(p, p, None, 0, p, p, p, p + 8, 8, 1, None, None) == 4      # packed_bytes == 0: no byte can be read, on to the output
        assert g(p, p, None, 0, None, p, p, p, 8, 1, None, None) == 3
        assert g(p, p, p, 128, p + 8, p, p, None, 0, 1, None, None) == 4    # out == NULL with out_len == 0
        assert f(3, p + 8, p, p, p, p, 8, 1, None, None) == 4
        assert f(3, p, p + 8, p, p, p, 8, 1, None, None) == 4               # bases are read as 16-byte cells
        assert f(3, p, p, p + 4, p, p, 8, 1, None, None) == 4
        assert f(3, p, p, p, p, p + 8, 8, 1, None, None) == 4
        assert g(p, p, p + 8, 128, p, p, p, p, 8, 1, None, None) == 4
        assert g(p, p, p, 128, p + 8, p, p, p, 8, 1, None, None) == 4
        assert g(p, p, p, 128, p, p + 8, p, p, 8, 1, None, None) == 4
        assert g(p, p, p, 128, p, p, p, p + 16 + 8, 8, 1, None, None) == 4


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tbase, tmask = torch.zeros(96, dtype=torch.int32), torch.zeros(32, dtype=torch.int32), torch.zeros(32, dtype=torch.int32)
    nmask = np.zeros(32, dtype=np.int32)
    with pytest.raises(TypeError):
        fl.Delta.undelta_select(3, np.zeros(96, dtype=np.uint32), np.zeros(32, dtype=np.uint32), nmask)
    with pytest.raises(TypeError):
        fl.Delta.undelta_select(3, tcol, tbase, tmask)
    with pytest.raises(TypeError):
        fl.undelta_select_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(32, np.uint32), nmask)
    with pytest.raises(TypeError):
        fl.undelta_select_widths(tw, to, tcol, tbase, tmask)
    with pytest.raises(TypeError):
        fl.Delta.undelta_select(0, np.zeros(0, dtype=np.uint32), np.zeros(32, dtype=np.uint32), nmask, n_blocks=1)


def test_cpp_mirror_declares_both_forms(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint16_t;
void (*const uniform)(std::size_t, const T*, const T*, const std::uint32_t*, const std::uint64_t*, T*, std::size_t, std::size_t, std::uint32_t*,
                      void*) = &fastlanes::Delta<T>::undelta_select_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, const std::uint32_t*, const std::uint64_t*, T*,
                    std::size_t, std::size_t, std::uint32_t*, void*) = &fastlanes::undelta_select_widths_device<T>;
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
