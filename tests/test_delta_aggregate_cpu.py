"""CPU: undelta_aggregate / undelta_aggregate_widths (COUNT / SUM / MIN / MAX of a Delta-packed column under a mask).
  * the routes of fastlanes_amd/csrc/fl_delta_aggregate_map.hpp, compiled here for the host, keep their order SKIP > IDENTITY > BASES > EACH,
    and its width-0 block equals the definition in Python's exact integers for all four types;
  * a numpy lane-group model of the aggregate (chains summed along their rows, row r of lane l governed by mask bit lane_base(l) + r, no
    value untransposed) equals the definition's slot over the oracle's untranspose(undelta_pack(..));
  * the header declares and the library exports the eight symbols through a macro of their own, every refusal is returned without a GPU
    and in order, the Python mirror validates before any launch, the C++ mirror compiles."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import delta_aggregate_data as da
from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)
from datagen import values
from delta_compare_range_data import incoming_mask
from oracle_lib import TYPES, lanes, packed_len

SHIM = r"""
#include "fl_delta_aggregate_map.hpp"
extern "C" int dagg_route(int ok, int empty, unsigned width) { return fl::delta_aggregate_route(ok != 0, empty != 0, width); }
extern "C" int dagg_route_reads(int route)
{
    return (fl::delta_aggregate_reads_bases((fl::DeltaAggregateRoute)route) ? 1 : 0) | (fl::delta_aggregate_reads_packed((fl::DeltaAggregateRoute)route) ? 2 : 0);
}
extern "C" void dagg_bases_block(unsigned type_bits, const uint64_t* bases, const unsigned* p, uint64_t* out)
{
    const fl::BlockAggregate g = fl::delta_aggregate_bases_block(type_bits, bases, p);
    out[0] = g.count; out[1] = g.sum; out[2] = g.min; out[3] = g.max;
}
extern "C" unsigned dagg_group_bit(unsigned l) { return fl::delta_group_bit(l); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "delta_aggregate", SHIM)
    so.dagg_route.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    so.dagg_route.restype = ctypes.c_int
    so.dagg_route_reads.argtypes = [ctypes.c_int]
    so.dagg_route_reads.restype = ctypes.c_int
    so.dagg_bases_block.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    so.dagg_bases_block.restype = None
    so.dagg_group_bit.argtypes = [ctypes.c_uint]
    so.dagg_group_bit.restype = ctypes.c_uint
    return so


def bases_block(shim, T, bases, p):
    b = np.array([int(x) for x in bases], dtype=np.uint64)
    q = np.array(p, dtype=np.uint32)
    out = np.empty(4, dtype=np.uint64)
    shim.dagg_bases_block(T, b.ctypes.data, q.ctypes.data, out.ctypes.data)
    return [int(x) for x in out]


# ---- 1. the routes and the width-0 block ---------------------------------------------------------------------------------------------
def test_routes_keep_their_order(shim):
    for T in TYPE_BITS.values():
        for w in (0, 1, T // 2, T):
            for ok in (0, 1):
                for empty in (0, 1):
                    mask_block = np.zeros(32, np.int32) if empty else np.ones(32, np.int32)
                    want = da.route_of(bool(ok), mask_block, w)
                    assert shim.dagg_route(ok, empty, w) == want, (T, w, ok, empty)
            assert shim.dagg_route(0, 1, w) == da.SKIP                      # SKIP ahead of IDENTITY
            assert shim.dagg_route(1, 1, w) == da.IDENTITY_ROUTE            # IDENTITY ahead of BASES and EACH
            assert shim.dagg_route(1, 0, w) == (da.BASES if w == 0 else da.EACH)
    assert (da.SKIP, da.IDENTITY_ROUTE, da.BASES, da.EACH) == (0, 1, 2, 3)
    assert [shim.dagg_route_reads(r) for r in range(4)] == [0, 0, 1, 3]       # bit 0: bases used, bit 1: packed bytes requested
    for ty, T in TYPE_BITS.items():
        assert [shim.dagg_group_bit(l) for l in range(1024 // T)] == [da.lane_base(l) for l in range(1024 // T)], ty


@pytest.mark.parametrize("ty", list(TYPE_BITS))
def test_bases_block_equals_the_definition(shim, oracle, ty):
    """random bases and group popcounts with some groups empty; the one-nonempty-group case; no group kept; every row kept; and the
    whole width-0 block against the oracle's untranspose(undelta_pack::<0>(..)) under a mask"""
    T = TYPE_BITS[ty]
    L = lanes(ty)
    rng = np.random.default_rng(5100 + T)
    for k in range(40):
        bases = values(ty, L, 5200 + 64 * T + k)
        p = rng.integers(0, T + 1, size=L)
        p[rng.random(L) < 0.4] = 0
        if k == 0:
            p[:] = 0
        if k == 1:
            p[:] = T
        assert bases_block(shim, T, bases, p) == da.bases_block(T, bases, p), (ty, k)
    for l in (0, 1, L // 2, L - 1):                                         # ONE group kept: min = max = its base, sum = p * base
        for k in (1, T // 2, T):
            bases = values(ty, L, 5300 + l)
            p = np.zeros(L, dtype=np.int64)
            p[l] = k
            b = int(bases[l])
            assert bases_block(shim, T, bases, p) == [k, (k * b) % (1 << 64), b, b] == da.bases_block(T, bases, p), (ty, l, k)
    # the block itself: every chain repeats its base, the mask's groups give p
    for k, m in enumerate([None] + list(incoming_mask(12, 5400 + T).reshape(12, 32))):
        bases = values(ty, L, 5500 + 64 * T + k)
        vals = oracle.untranspose(ty, oracle.undelta_pack(ty, 0, np.zeros(0, dtype=TYPES[ty][0]), bases))
        want = [int(x) for x in da.want_slots(vals, m)[0]]
        assert bases_block(shim, T, bases, da.group_popcounts(ty, m)) == want, (ty, k)


def test_bases_block_u64_sum_wraps(shim):
    """u64 bases near 2^64: sum p_l * base_l wraps mod 2^64"""
    M = (1 << 64) - 1
    bases = [M - l for l in range(16)]
    for p in ([64] * 16, [1] + [0] * 15, [0] * 15 + [63], list(range(16)), [64, 0] * 8):
        want = da.bases_block(64, bases, p)
        assert sum(k * b for k, b in zip(p, bases)) > M or sum(p) <= 1       # the exact sum does not fit 64 bits
        assert bases_block(shim, 64, bases, p) == want, p
    assert bases_block(shim, 64, bases, [64] * 16) == [1024, (64 * sum(bases)) % (1 << 64), M - 15, M]


# ---- 2. the lane-group model against the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", list(TYPE_BITS))
def test_lane_group_model_equals_the_definition(oracle, ty):
    """widths 0, 1, T/2 and T, random packed bytes and bases (the chains wrap), random masks, sparse ones, one-bit ones and no mask"""
    T = TYPE_BITS[ty]
    L = lanes(ty)
    rng = np.random.default_rng(5600 + T)
    for w in (0, 1, T // 2, T):
        pk = values(ty, packed_len(ty, w), 5700 + 64 * T + w)
        bases = values(ty, L, 5800 + 64 * T + w)
        vals = oracle.untranspose(ty, oracle.undelta_pack(ty, w, pk, bases))
        masks = [None, rng.integers(0, 1 << 32, size=32, dtype=np.uint64).astype(np.uint32).view(np.int32),
                 np.packbits(rng.random(1024) < 0.02, bitorder="little").view(np.int32)]
        masks += [da.rows_mask(1, 0, r, r) for r in (0, T - 1, T, 519, 1023)]
        for k, m in enumerate(masks):
            got = da.lane_group_model(ty, w, pk, bases, m)
            assert np.array_equal(got, da.want_slots(vals, m)[0]), (ty, w, k)


# ---- 3. exports, refusals, mirrors -------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_eight_symbols(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_DELTA_AGGREGATE(T, S)")[1].split("FL_DECLARE_DELTA_AGGREGATE(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == list(da.FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_DELTA_AGGREGATE({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in da.FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.delta_aggregate_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.aggregate_symbols(), fastlanes_amd.delta_compare_range_symbols(),
                  fastlanes_amd.select_symbols(), fastlanes_amd.aggregate_columns_symbols(), fastlanes_amd.aggregate_by_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"delta_aggregate_symbols", "undelta_aggregate_widths"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.Delta, "undelta_aggregate")
    import __graft_entry__ as ge
    import inspect
    assert "delta_aggregate_symbols()" in inspect.getsource(ge.build)         # the build's symbol check includes them


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), in unfor_aggregate's order: width, the empty column,
    NULL pointers, alignment -- `bases` among the required and the 16-byte aligned pointers, `mask` and `err_flag` optional."""
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_undelta_aggregate")
        g = getattr(lib, f"fl_{ty}_undelta_aggregate_widths")
        # f(width, in, bases, mask, n, block_aggs, err, stream)
        # g(widths, offsets, packed, packed_bytes, bases, mask, n, block_aggs, err, stream)
        assert f(3, None, None, None, 0, None, None, None) == 0             # the empty column: nothing else is looked at
        assert f(T, p + 8, p + 8, p + 4, 0, p + 8, None, None) == 0
        assert g(None, None, None, 0, None, None, 0, None, None, None) == 0
        assert f(T + 1, p, p, p, 1, p, None, None) == 1                     # width > T
        assert f(T + 1, p, p, p, 0, p, None, None) == 1                     # ... also for an empty column
        assert f(T + 1, None, None, None, 1, None, None, None) == 1         # ... ahead of the NULL pointers
        assert f(T + 1, p + 8, p, p, 1, p, None, None) == 1                 # ... and of the alignment
        for mask in (None, p):
            assert f(3, p, None, mask, 1, p, None, None) == 3               # bases
            assert f(3, p, p, mask, 1, None, None, None) == 3               # block_aggs
            assert f(3, None, p, mask, 1, p, None, None) == 3               # W > 0 reads data
            assert f(3, None, p + 8, mask, 1, p, None, None) == 3           # NULL ahead of alignment
            assert f(0, None, p, mask, 1, p + 8, None, None) == 4           # W = 0 needs none: on to the misaligned slots
            assert f(0, None, None, mask, 1, p, None, None) == 3            # ... but its bases
            assert g(None, p, p, 128, p, mask, 1, p, None, None) == 3
            assert g(p, None, p, 128, p, mask, 1, p, None, None) == 3
            assert g(p, p, None, 128, p, mask, 1, p, None, None) == 3       # packed_bytes > 0: bytes can be read
            assert g(p, p, p, 128, None, mask, 1, p, None, None) == 3
            assert g(p, p, p, 128, p, mask, 1, None, None, None) == 3
            assert g(p, p, None, 0, p, mask, 1, p + 8, None, None) == 4     # packed_bytes == 0: no byte can be read, on to the slots
            assert g(p, p, None, 0, None, mask, 1, p, None, None) == 3
            assert f(3, p + 8, p, mask, 1, p, None, None) == 4
            assert f(3, p, p + 8, mask, 1, p, None, None) == 4              # bases are read as 16-byte cells
            assert f(3, p, p, mask, 1, p + 8, None, None) == 4
            assert g(p, p, p + 8, 128, p, mask, 1, p, None, None) == 4
            assert g(p, p, p, 128, p + 8, mask, 1, p, None, None) == 4
            assert g(p, p, p, 128, p, mask, 1, p + 16 + 8, None, None) == 4
        assert f(3, p, p, p + 4, 1, p, None, None) == 4                     # the mask, when there is one
        assert g(p, p, p, 128, p, p + 8, 1, p, None, None) == 4


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tbase, tmask = torch.zeros(96, dtype=torch.int32), torch.zeros(32, dtype=torch.int32), torch.zeros(32, dtype=torch.int32)
    with pytest.raises(TypeError):
        fl.Delta.undelta_aggregate(3, np.zeros(96, dtype=np.uint32), np.zeros(32, dtype=np.uint32))
    with pytest.raises(TypeError):
        fl.Delta.undelta_aggregate(3, tcol, tbase)
    with pytest.raises(TypeError):
        fl.undelta_aggregate_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(32, np.uint32))
    with pytest.raises(TypeError):
        fl.undelta_aggregate_widths(tw, to, tcol, tbase, mask=tmask)
    with pytest.raises(TypeError):
        fl.Delta.undelta_aggregate(0, np.zeros(0, dtype=np.uint32), np.zeros(32, dtype=np.uint32), n_blocks=1)


def test_cpp_mirror_declares_both_forms(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint16_t;
void (*const uniform)(std::size_t, const T*, const T*, const std::uint32_t*, std::size_t, fl_block_aggregate*, std::uint32_t*, void*) =
    &fastlanes::Delta<T>::undelta_aggregate_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, const std::uint32_t*, std::size_t,
                    fl_block_aggregate*, std::uint32_t*, void*) = &fastlanes::undelta_aggregate_widths_device<T>;
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
