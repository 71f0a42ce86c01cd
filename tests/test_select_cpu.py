"""CPU: mask_offsets / unfor_select / unfor_select_widths (decode only the rows a selection mask keeps) -- the header declares and the
library exports them for every element type, their argument checks need no GPU, the Python mirror validates before any launch, and the
index arithmetic the kernel runs (fastlanes_amd/csrc/fl_select_map.hpp, compiled here for the host) tiles a block's 1024 mask bits
exactly once and lands every kept element where np.flatnonzero puts it."""
import ctypes
import os
import re

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)


def test_header_declares_and_library_exports_the_nine_symbols(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_SELECT(T, S)")[1].split("FL_DECLARE_SELECT(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == ["unfor_select", "unfor_select_widths"]
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_SELECT({CT[ty]}, {ty})" in text
    assert "FL_DECLARE_MASK_OFFSETS(mask_offsets)" in text
    want = ["fl_mask_offsets"] + [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in ("unfor_select", "unfor_select_widths")]
    assert len(want) == 9 and sorted(fastlanes_amd.select_symbols()) == sorted(want)
    assert not set(want) & set(fastlanes_amd.exported_symbols())          # the pinned list stays as it was
    for s in want:
        assert hasattr(lib, s), s


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel)."""
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    mo = lib.fl_mask_offsets
    assert mo(None, 0, None, None, None) == 0                              # empty column
    assert mo(None, 1, p, None, None) == 3 and mo(p, 1, None, None, None) == 3
    assert mo(p + 4, 1, p, None, None) == 4
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_select")
        g = getattr(lib, f"fl_{ty}_unfor_select_widths")
        # (width, in, refs, stride, mask, out_offsets, out, out_len, n, err, stream)
        assert f(3, None, None, 0, None, None, None, 0, 0, None, None) == 0
        assert g(None, None, None, 0, None, 0, None, None, None, 0, 0, None, None) == 0
        assert f(T + 1, p, p, 1, p, p, p, 1024, 1, None, None) == 1        # FL_ERR_WIDTH
        assert f(T + 1, p, p, 1, p, p, p, 1024, 0, None, None) == 1        # ... before the empty-column return, as unfor_compare
        # FL_ERR_NULL: references, mask, out_offsets, out, data, widths, offsets
        assert f(3, p, None, 1, p, p, p, 1024, 1, None, None) == 3
        assert f(3, p, p, 1, None, p, p, 1024, 1, None, None) == 3
        assert f(3, p, p, 1, p, None, p, 1024, 1, None, None) == 3
        assert f(3, p, p, 1, p, p, None, 1024, 1, None, None) == 3
        assert f(3, None, p, 1, p, p, p, 1024, 1, None, None) == 3         # W > 0 reads data
        assert g(None, p, p, 128, p, 1, p, p, p, 1024, 1, None, None) == 3
        assert g(p, None, p, 128, p, 1, p, p, p, 1024, 1, None, None) == 3
        assert g(p, p, None, 128, p, 1, p, p, p, 1024, 1, None, None) == 3
        assert g(p, p, p, 128, None, 1, p, p, p, 1024, 1, None, None) == 3
        assert g(p, p, p, 128, p, 1, None, p, p, 1024, 1, None, None) == 3
        assert g(p, p, p, 128, p, 1, p, None, p, 1024, 1, None, None) == 3
        assert g(p, p, p, 128, p, 1, p, p, None, 1024, 1, None, None) == 3
        # FL_ERR_ALIGN: 16-byte packed column, mask and output base
        assert f(3, p + 8, p, 1, p, p, p, 1024, 1, None, None) == 4
        assert f(3, p, p, 1, p + 4, p, p, 1024, 1, None, None) == 4
        assert f(3, p, p, 1, p, p, p + 8, 1024, 1, None, None) == 4
        assert g(p, p, p + 8, 128, p, 1, p, p, p, 1024, 1, None, None) == 4
        assert g(p, p, p, 128, p, 1, p + 8, p, p, 1024, 1, None, None) == 4
        assert g(p, p, p, 128, p, 1, p, p, p + 8, 1024, 1, None, None) == 4


def test_python_mirror_validates_on_cpu_tensors():
    import torch
    import fastlanes_amd as fl
    mask_np = np.zeros(32, np.uint32)
    with pytest.raises(TypeError):
        fl.mask_offsets(mask_np)                                           # device tier only
    with pytest.raises(TypeError):
        fl.mask_offsets(torch.zeros(32, dtype=torch.int32))                # a CPU tensor
    with pytest.raises(TypeError):
        fl.FoR.unfor_select(3, np.zeros(96, dtype=np.uint32), 0, mask_np)
    with pytest.raises(TypeError):
        fl.FoR.unfor_select(3, torch.zeros(96, dtype=torch.int32), 0, torch.zeros(32, dtype=torch.int32))
    with pytest.raises(TypeError):
        fl.unfor_select_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(1, np.uint32), mask_np)
    with pytest.raises(TypeError):
        fl.unfor_select_widths(torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(96, dtype=torch.int32),
                               torch.zeros(1, dtype=torch.int32), torch.zeros(32, dtype=torch.int32))
    assert {"mask_offsets", "unfor_select_widths"} <= set(fl.__all__) and hasattr(fl.FoR, "unfor_select")


SHIM = r"""
#include "fl_select_map.hpp"
#include <stddef.h>
// One block as a 64-lane wavefront runs it (fl_select.hpp), lane by lane on the host: every lane cuts its slices out of the mask words,
// packs its per-group counts, the packed words are scanned inclusively over the lanes, and every kept element is landed.
//   owner[i]  += 1 for every index i some lane's slice covers (slices must tile 0..1023 exactly once)
//   order[]    = the indices in (group, lane, element) order (must be 0..1023 ascending: index order)
//   run[p]     = the index that lands at position p;  returns the block's count (-1: a landing position outside [0, count))
template <unsigned SZ> static int run_block(const uint32_t* mask, int* owner, int* order, int* run)
{
    using M = fl::SelectMap<SZ>;
    uint32_t slice[64][M::GROUPS];
    uint64_t mine[64], incl[64];
    int n_order = 0;
    for (unsigned k = 0; k < M::GROUPS; ++k)
        for (unsigned l = 0; l < 64; ++l)
            for (unsigned e = 0; e < M::N; ++e) {
                owner[M::first_bit(k, l) + e] += 1;
                order[n_order++] = (int)(M::first_bit(k, l) + e);
            }
    for (unsigned l = 0; l < 64; ++l) {
        mine[l] = 0;
        for (unsigned k = 0; k < M::GROUPS; ++k) {
            slice[l][k] = M::slice(mask[M::mask_word(k, l)], k, l);
            mine[l] |= M::pack_count((unsigned)__builtin_popcount(slice[l][k]), k);
        }
        incl[l] = (l ? incl[l - 1] : 0) + mine[l];
        if (M::SCAN_BITS == 32) incl[l] &= 0xffffffffull;                   // the kernel scans a 32-bit word for u8 / u16
    }
    const uint64_t totals = incl[63];
    const int count = (int)M::group_base(totals, M::GROUPS);
    for (unsigned l = 0; l < 64; ++l)
        for (unsigned k = 0; k < M::GROUPS; ++k)
            for (unsigned e = 0; e < M::N; ++e)
                if ((slice[l][k] >> e) & 1u) {
                    const unsigned at = M::landing(totals, incl[l] - mine[l], k, slice[l][k], e);
                    if (at >= (unsigned)count) return -1;
                    run[at] = (int)(M::first_bit(k, l) + e);
                }
    return count;
}
extern "C" int select_map_block(unsigned sz, const uint32_t* mask, int* owner, int* order, int* run)
{
    switch (sz) {
    case 1: return run_block<1>(mask, owner, order, run);
    case 2: return run_block<2>(mask, owner, order, run);
    case 4: return run_block<4>(mask, owner, order, run);
    case 8: return run_block<8>(mask, owner, order, run);
    default: return -2;
    }
}
"""


@pytest.fixture(scope="module")
def select_map(tmp_path_factory):
    shim = build_shim(tmp_path_factory, "select_map", SHIM)
    shim.select_map_block.argtypes = [ctypes.c_uint] + [ctypes.c_void_p] * 4
    shim.select_map_block.restype = ctypes.c_int

    def run(sz, mask_bits):
        words = np.packbits(np.asarray(mask_bits, dtype=np.uint8), bitorder="little").view(np.uint32).copy()
        assert words.size == 32
        owner, order, out = np.zeros(1024, np.int32), np.full(1024, -1, np.int32), np.full(1024, -1, np.int32)
        count = shim.select_map_block(sz, words.ctypes.data, owner.ctypes.data, order.ctypes.data, out.ctypes.data)
        return count, owner, order, out
    return run


@pytest.mark.parametrize("ty", list(TYPE_BITS))
def test_select_map_tiles_the_mask_and_lands_in_index_order(select_map, ty):
    sz = TYPE_BITS[ty] // 8
    rng = np.random.default_rng(1400 + sz)
    masks = [np.zeros(1024, bool), np.ones(1024, bool), np.arange(1024) % 2 == 1]
    for i in (0, 31, 32, 1022, 1023):
        m = np.zeros(1024, bool)
        m[i] = True
        masks.append(m)
    for density in (1 / 1024, 0.01, 0.1, 0.5, 0.9):
        masks += [rng.random(1024) < density for _ in range(40)]
    # one whole 1-KiB group kept and nothing else; everything but one group: the group bases
    ge = 1024 // sz
    for k in range(sz):
        m = np.zeros(1024, bool)
        m[k * ge:(k + 1) * ge] = True
        masks += [m, ~m]
    for m in masks:
        count, owner, order, run = select_map(sz, m)
        assert (owner == 1).all()                                          # the slices tile the 1024 bits exactly once ...
        assert (order == np.arange(1024)).all()                            # ... in index order over (group, lane, element)
        want = np.flatnonzero(m)
        assert count == want.size
        assert (run[:count] == want).all() and (run[count:] == -1).all()
