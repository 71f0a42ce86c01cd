"""CPU: unfor_aggregate / unfor_aggregate_widths / aggregate_reduce (COUNT / SUM / MIN / MAX of a FoR-packed column under a selection
mask) -- the header declares and the library exports them for every element type, their argument checks need no GPU, the Python mirror
validates before any launch, and the arithmetic the kernels share with the host (fastlanes_amd/csrc/fl_aggregate_map.hpp, compiled here
with g++) -- combine / identity and the no-decode answer of an empty mask or a width-0 block -- agrees with numpy and with brute force."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)

IDENTITY = (0, 0, 2 ** 64 - 1, 0)


def test_header_declares_and_library_exports_the_nine_symbols(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_AGGREGATE(T, S)")[1].split("FL_DECLARE_AGGREGATE(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == ["unfor_aggregate", "unfor_aggregate_widths"]
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_AGGREGATE({CT[ty]}, {ty})" in text
    assert "FL_DECLARE_AGGREGATE_REDUCE(aggregate_reduce)" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in ("unfor_aggregate", "unfor_aggregate_widths")] + ["fl_aggregate_reduce"]
    assert len(want) == 9 and sorted(fastlanes_amd.aggregate_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.select_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s


def test_block_aggregate_is_32_bytes(tmp_path):
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include "fastlanes_amd.h"\n'
                   "int main(void) { return sizeof(fl_block_aggregate) == 32 && sizeof(((fl_block_aggregate *)0)->max) == 8 ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel)."""
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    red = lib.fl_aggregate_reduce
    # (block_aggs, n, result, stream)
    assert red(None, 1, p, None) == 3 and red(p, 1, None, None) == 3 and red(None, 0, None, None) == 3   # the result is always written
    assert red(p + 8, 1, p, None) == 4 and red(p, 1, p + 8, None) == 4
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_aggregate")
        g = getattr(lib, f"fl_{ty}_unfor_aggregate_widths")
        # (width, in, refs, stride, mask, n, block_aggs, err, stream)
        assert f(3, None, None, 0, None, 0, None, None, None) == 0         # an empty column
        # (widths, offsets, packed, packed_bytes, refs, stride, mask, n, block_aggs, err, stream)
        assert g(None, None, None, 0, None, 0, None, 0, None, None, None) == 0
        assert f(T + 1, p, p, 1, p, 1, p, None, None) == 1                 # FL_ERR_WIDTH
        assert f(T + 1, p, p, 1, p, 0, p, None, None) == 1                 # ... before the empty-column return, as unfor_select
        # FL_ERR_NULL: references, block_aggs, data, widths, offsets -- with and without a mask (mask == NULL is accepted: the
        # refusal below is the OTHER pointer's)
        for mask in (p, None):
            assert f(3, p, None, 1, mask, 1, p, None, None) == 3
            assert f(3, p, p, 1, mask, 1, None, None, None) == 3
            assert f(3, None, p, 1, mask, 1, p, None, None) == 3           # W > 0 reads data
            assert g(None, p, p, 128, p, 1, mask, 1, p, None, None) == 3
            assert g(p, None, p, 128, p, 1, mask, 1, p, None, None) == 3
            assert g(p, p, None, 128, p, 1, mask, 1, p, None, None) == 3   # packed_bytes > 0 reads data
            assert g(p, p, p, 128, None, 1, mask, 1, p, None, None) == 3
            assert g(p, p, p, 128, p, 1, mask, 1, None, None, None) == 3
            # FL_ERR_ALIGN: 16-byte packed column and block_aggs (so a NULL mask got past the NULL checks)
            assert f(3, p + 8, p, 1, mask, 1, p, None, None) == 4
            assert f(3, p, p, 1, mask, 1, p + 8, None, None) == 4
            assert g(p, p, p + 8, 128, p, 1, mask, 1, p, None, None) == 4
            assert g(p, p, p, 128, p, 1, mask, 1, p + 8, None, None) == 4
        assert f(3, p, p, 1, p + 4, 1, p, None, None) == 4                 # ... and mask
        assert g(p, p, p, 128, p, 1, p + 4, 1, p, None, None) == 4


def test_python_mirror_validates_on_cpu_tensors():
    import torch
    import fastlanes_amd as fl
    with pytest.raises(TypeError):
        fl.aggregate_reduce(np.zeros(4, np.uint64))                        # device tier only
    with pytest.raises(TypeError):
        fl.aggregate_reduce(torch.zeros(4, dtype=torch.int64))             # a CPU tensor
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate(3, np.zeros(96, dtype=np.uint32), 0)
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate(3, torch.zeros(96, dtype=torch.int32), 0, torch.zeros(32, dtype=torch.int32))
    with pytest.raises(TypeError):
        fl.unfor_aggregate_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(1, np.uint32))
    with pytest.raises(TypeError):
        fl.unfor_aggregate_widths(torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(96, dtype=torch.int32),
                                  torch.zeros(1, dtype=torch.int32), torch.zeros(32, dtype=torch.int32))
    assert {"unfor_aggregate_widths", "aggregate_reduce", "aggregate_symbols"} <= set(fl.__all__) and hasattr(fl.FoR, "unfor_aggregate")


SHIM = r"""
#include "fl_aggregate_map.hpp"
#include <stddef.h>
// slots[n][4] folded left to right from the identity
extern "C" void agg_fold(const uint64_t* slots, size_t n, uint64_t* out)
{
    fl::BlockAggregate g = fl::aggregate_identity();
    for (size_t i = 0; i < n; ++i) g = fl::aggregate_combine(g, fl::BlockAggregate{slots[4 * i], slots[4 * i + 1], slots[4 * i + 2], slots[4 * i + 3]});
    out[0] = g.count; out[1] = g.sum; out[2] = g.min; out[3] = g.max;
}
// what the kernel answers without reading a packed byte; returns the route (0 identity, 1 constant, 2 decode: out untouched)
extern "C" int agg_no_decode(unsigned count, unsigned w, uint64_t ref, uint64_t* out)
{
    const fl::AggregateRoute route = fl::aggregate_route(count, w);
    if (route == fl::AGG_DECODE) return (int)route;
    const fl::BlockAggregate g = fl::aggregate_constant_block(count, ref);
    out[0] = g.count; out[1] = g.sum; out[2] = g.min; out[3] = g.max;
    return (int)route;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    s = build_shim(tmp_path_factory, "aggregate_map", SHIM)
    s.agg_fold.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    s.agg_fold.restype = None
    s.agg_no_decode.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint64, ctypes.c_void_p]
    s.agg_no_decode.restype = ctypes.c_int
    return s


def numpy_combine(slots):
    """uint64[n, 4] -> (count, sum, min, max); uint64 addition wraps"""
    if slots.shape[0] == 0:
        return IDENTITY
    return (int(slots[:, 0].sum(dtype=np.uint64)), int(slots[:, 1].sum(dtype=np.uint64)), int(slots[:, 2].min()), int(slots[:, 3].max()))


def test_combine_against_numpy(shim):
    rng = np.random.default_rng(1600)
    ident = np.array(IDENTITY, dtype=np.uint64)
    wrapped = 0
    for n in (0, 1, 2, 3, 17, 1000):
        for kind in ("random", "identities", "half", "big sums"):
            slots = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
            if kind == "identities":
                slots[:] = ident
            elif kind == "half":
                slots[rng.random(n) < 0.5] = ident
            elif kind == "big sums":
                slots[:, 1] |= np.uint64(1 << 63)                           # any two of them wrap
            out = np.zeros(4, dtype=np.uint64)
            shim.agg_fold(slots.ctypes.data, n, out.ctypes.data)
            assert tuple(int(x) for x in out) == numpy_combine(slots), (n, kind)
            if n > 1 and sum(int(x) for x in slots[:, 1]) >= 1 << 64:
                wrapped += 1
    assert wrapped >= 8                                                     # wrapping sums were really met


def brute_force(count, ref):
    """`count` kept rows of a width-0 block: every value is the reference"""
    vals = np.full(count, ref, dtype=np.uint64)
    if count == 0:
        return IDENTITY
    return (count, int(vals.sum(dtype=np.uint64)), int(vals.min()), int(vals.max()))


def no_decode(shim, count, w, ref):
    out = np.full(4, 0xDEADBEEF, dtype=np.uint64)
    route = shim.agg_no_decode(count, w, ref, out.ctypes.data)
    return route, tuple(int(x) for x in out)


def test_no_decode_shortcut_u8_exhaustive(shim):
    for ref in range(256):
        for count in (0, 1, 1023, 1024):
            route, got = no_decode(shim, count, 0, ref)                     # width 0
            assert route == (1 if count else 0) and got == brute_force(count, ref), (ref, count)
            for w in (1, 8):                                                # a width > 0 only skips the decode for an empty mask
                route, got = no_decode(shim, count, w, ref)
                if count == 0:
                    assert route == 0 and got == IDENTITY
                else:
                    assert route == 2 and got == (0xDEADBEEF,) * 4


def test_no_decode_shortcut_u64_wraps(shim):
    rng = np.random.default_rng(1601)
    refs = [0, 1, 2 ** 63, 2 ** 64 - 1, 2 ** 64 - 2, 2 ** 64 - 1023, 2 ** 64 // 1024, 2 ** 64 // 1024 + 1]
    refs += [int(x) for x in rng.integers(0, 1 << 64, size=64, dtype=np.uint64)]
    refs += [2 ** 64 - 1 - int(x) for x in rng.integers(0, 4096, size=64)]
    wrapped = 0
    for ref in refs:
        for count in (0, 1, 2, 3, 511, 1023, 1024):
            route, got = no_decode(shim, count, 0, ref)
            assert route == (1 if count else 0) and got == brute_force(count, ref), (ref, count)
            wrapped += count * ref >= 1 << 64
    assert wrapped >= 100                                                   # count * r really wrapped
