"""CPU: unfor_aggregate_by / unfor_aggregate_by_widths (COUNT / SUM / MIN / MAX of a FoR-packed column grouped by a FoR-packed u8 key
column) -- the header declares and the library exports them for every value type, the Python table agrees with the header, their
argument checks need no GPU, the routes and the key-byte address map the kernel shares with the host
(fastlanes_amd/csrc/fl_aggregate_by_map.hpp, compiled here with g++) are exhaustive / a bijection, and the numpy reference the GPU test
compares against gives a hand-written answer."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)
from group_data import expected_groups

IDENTITY = (0, 0, 2 ** 64 - 1, 0)
FORMS = ("unfor_aggregate_by", "unfor_aggregate_by_widths")


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
    body = text.split("#define FL_DECLARE_AGGREGATE_BY(T, S)")[1].split("FL_DECLARE_AGGREGATE_BY(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_AGGREGATE_BY({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.aggregate_by_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.select_symbols(),
                  fastlanes_amd.aggregate_symbols(), fastlanes_amd.for_compare_range_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: a pointer is c_void_p, `unsigned` c_uint, size_t c_size_t; int comes back"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("AGGREGATE_BY")}
    assert len(rows) == 8
    names = {"unfor_aggregate_by": "width in references reference_stride key_width keys key_references key_reference_stride mask n_blocks "
                                   "result err_flag stream",
             "unfor_aggregate_by_widths": "widths offsets packed packed_bytes references reference_stride key_widths key_offsets keys "
                                          "keys_bytes key_references key_reference_stride mask n_blocks result err_flag stream"}
    for ty in TYPE_BITS:
        for form in FORMS:
            name = f"fl_{ty}_{form}"
            ret, args = protos[name]
            restype, argtypes = rows[name]
            assert ret == "int" and restype is ctypes.c_int
            assert [a for _, a in args] == names[form].split(), name
            assert len(args) == len(argtypes), name
            for (ctype, arg), at in zip(args, argtypes):
                want = ctypes.c_void_p if "*" in ctype else {"unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t}[ctype]
                assert at is want, (name, arg, ctype)
            # the value column's pointers are of the value type, the key column's of uint8_t
            types = dict((a, c) for c, a in args)
            assert types["references"] == f"const {CT[ty]} *" and types["keys"] == "const uint8_t *" and types["key_references"] == "const uint8_t *"
            assert types["in" if form == FORMS[0] else "packed"] == f"const {CT[ty]} *"
            assert getattr(lib, name).argtypes == argtypes


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel): width first -- also for an empty column -- then NULL,
    then alignment."""
    buf = np.zeros(8192, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    V, R, K, KR, M, RES, W, O, KW, KO = (p + 4096 * i for i in range(10))
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_aggregate_by")
        g = getattr(lib, f"fl_{ty}_unfor_aggregate_by_widths")

        def uni(width=3, v=V, r=R, kw=3, k=K, kr=KR, m=M, n=1, res=RES):
            return f(width, v, r, 1, kw, k, kr, 1, m, n, res, None, None)

        def mix(w=W, o=O, v=V, pb=384, r=R, kw=KW, ko=KO, k=K, kb=384, kr=KR, m=M, n=1, res=RES):
            return g(w, o, v, pb, r, 1, kw, ko, k, kb, kr, 1, m, n, res, None, None)

        # FL_ERR_WIDTH: either width, also with n_blocks = 0, and in front of every other refusal
        for n in (1, 0):
            assert uni(width=T + 1, n=n) == 1 and uni(kw=9, n=n) == 1 and uni(width=T + 1, kw=9, n=n) == 1
        assert uni(width=T + 1, res=None) == 1 and uni(kw=9, k=K + 8) == 1
        assert uni(width=T, kw=8, res=None) == 3                           # the widest widths are not refused as widths
        # FL_ERR_NULL: each required pointer; `result` also for an empty column (every call writes it); mask == NULL is accepted
        for m in (M, None):
            assert uni(v=None, m=m) == 3 and uni(r=None, m=m) == 3 and uni(k=None, m=m) == 3 and uni(kr=None, m=m) == 3
            assert uni(res=None, m=m) == 3 and uni(res=None, n=0, m=m) == 3
            for name in ("w", "o", "v", "r", "kw", "ko", "k", "kr", "res"):
                assert mix(**{name: None}, m=m) == 3, (ty, name)
            assert mix(res=None, n=0, m=m) == 3
            # FL_ERR_ALIGN: in / packed, keys, result at + 8 bytes (a NULL mask got past the NULL checks)
            assert uni(v=V + 8, m=m) == 4 and uni(k=K + 8, m=m) == 4 and uni(res=RES + 8, m=m) == 4
            assert mix(v=V + 8, m=m) == 4 and mix(k=K + 8, m=m) == 4 and mix(res=RES + 8, m=m) == 4
            assert uni(res=RES + 8, n=0, m=m) == 4 and mix(res=RES + 8, n=0, m=m) == 4
        assert uni(m=M + 8) == 4 and mix(m=M + 8) == 4                     # ... and mask
        assert uni(v=None, k=K + 8) == 3                                   # NULL is answered before alignment
        # a packed pointer may be NULL only when no byte of it can be read: width 0 / no packed bytes are accepted as far as the next
        # refusal (here: the misaligned result)
        assert uni(width=0, v=None, res=RES + 8) == 4 and uni(kw=0, k=None, res=RES + 8) == 4
        assert mix(v=None, pb=0, res=RES + 8) == 4 and mix(k=None, kb=0, res=RES + 8) == 4
        assert mix(v=None) == 3 and mix(k=None) == 3                       # ... with bytes to read they are required


def test_python_mirror_validates_on_cpu_tensors():
    import torch
    import fastlanes_amd as fl
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by(3, np.zeros(96, dtype=np.uint32), 0, 3, np.zeros(384, dtype=np.uint8), 0)       # device tier only
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by(3, torch.zeros(96, dtype=torch.int32), 0, 3, torch.zeros(384, dtype=torch.uint8), 0)   # CPU tensors
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(1, np.uint32),
                                     np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(384, np.uint8), np.zeros(1, np.uint8))
    assert {"unfor_aggregate_by_widths", "aggregate_by_symbols"} <= set(fl.__all__) and hasattr(fl.FoR, "unfor_aggregate_by")


SHIM = r"""
#include "fl_aggregate_by_map.hpp"
extern "C" int by_route(int mask_empty, int ok, unsigned key_width) { return (int)fl::aggregate_by_route(mask_empty != 0, ok != 0, key_width); }
extern "C" int by_reads_keys(int route) { return fl::aggregate_by_reads_keys((fl::AggregateByRoute)route) ? 1 : 0; }
extern "C" int by_reads_values(int route, unsigned value_width) { return fl::aggregate_by_reads_values((fl::AggregateByRoute)route, value_width) ? 1 : 0; }
extern "C" unsigned by_key_store(unsigned lane) { return fl::aggregate_by_key_store(lane); }
extern "C" unsigned by_key_byte(unsigned sz, unsigned k, unsigned lane, unsigned e)
{
    return sz == 1 ? fl::aggregate_by_key_byte<1>(k, lane, e) : sz == 2 ? fl::aggregate_by_key_byte<2>(k, lane, e)
         : sz == 4 ? fl::aggregate_by_key_byte<4>(k, lane, e) : fl::aggregate_by_key_byte<8>(k, lane, e);
}
extern "C" unsigned by_first_bit(unsigned sz, unsigned k, unsigned lane)
{
    return sz == 1 ? fl::SelectMap<1>::first_bit(k, lane) : sz == 2 ? fl::SelectMap<2>::first_bit(k, lane)
         : sz == 4 ? fl::SelectMap<4>::first_bit(k, lane) : fl::SelectMap<8>::first_bit(k, lane);
}
extern "C" unsigned by_wave_lds(unsigned value_block_bytes) { return fl::aggregate_by_wave_lds(value_block_bytes); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory, "aggregate_by_map", SHIM)


def test_route_is_exhaustive(shim):
    """(mask empty?, key width 0..8, value width 0 / > 0, precondition ok?) -> the route and what it reads"""
    SKIP, ONE_KEY, DECODE = 0, 1, 2
    seen = set()
    for empty in (0, 1):
        for ok in (0, 1):
            for kw in range(9):
                route = shim.by_route(empty, ok, kw)
                want = SKIP if empty or not ok else ONE_KEY if kw == 0 else DECODE
                assert route == want, (empty, ok, kw)
                assert shim.by_reads_keys(route) == (route == DECODE)       # no key byte unless both columns are decoded
                for vw in (0, 1, 64):
                    assert shim.by_reads_values(route, vw) == (route != SKIP and vw > 0), (empty, ok, kw, vw)
                    seen.add((route, bool(vw)))
    assert seen == {(r, v) for r in (SKIP, ONE_KEY, DECODE) for v in (False, True)}


@pytest.mark.parametrize("sz", [1, 2, 4, 8])
def test_key_byte_map_is_a_bijection_onto_the_key_area(shim, sz):
    n = 16 // sz
    hit = np.zeros(1024, int)
    for k in range(sz):
        for lane in range(64):
            first = shim.by_first_bit(sz, k, lane)
            assert first % n == 0                                           # one aligned read of n bytes
            for e in range(n):
                at = shim.by_key_byte(sz, k, lane, e)
                assert at == first + e
                hit[at] += 1
    assert (hit == 1).all()
    # the key block's own decode stores lane l's 16 keys at 16 l: a u8 block's index order, one cell per lane, the whole area
    assert [shim.by_key_store(lane) for lane in range(64)] == list(range(0, 1024, 16))
    assert [shim.by_key_store(lane) for lane in range(64)] == [shim.by_first_bit(1, 0, lane) for lane in range(64)]


def test_lds_budget(shim):
    """value image + 1 KiB of keys + the 8-KiB table: at most 17 KiB for a single-wave workgroup"""
    assert [shim.by_wave_lds(128 * T) for T in TYPE_BITS.values()] == [10 * 1024, 11 * 1024, 13 * 1024, 17 * 1024]


def test_numpy_reference_on_a_hand_written_example():
    """two blocks, seven interesting rows; everything else is value 0 under key 0 and masked out"""
    vals = np.zeros(2048, dtype=np.uint64)
    keys = np.zeros(2048, dtype=np.uint8)
    bits = np.zeros(2048, bool)
    rows = [(0, 0, 5, 2 ** 64 - 1, True), (0, 1, 5, 3, True), (0, 1023, 255, 7, True), (1, 0, 5, 10, True), (1, 7, 255, 99, False),
            (1, 8, 0, 2 ** 63, True), (1, 9, 0, 2 ** 63, True)]
    for b, i, key, v, kept in rows:
        vals[b * 1024 + i], keys[b * 1024 + i], bits[b * 1024 + i] = v, key, kept
    got = expected_groups(vals, keys, bits)
    assert got.dtype == np.uint64 and got.shape == (256, 4)
    want = {0: (2, 0, 2 ** 63, 2 ** 63),                                    # 2^63 + 2^63 wraps to 0
            5: (3, 12, 3, 2 ** 64 - 1),                                     # (2^64 - 1) + 3 + 10 = 12 mod 2^64
            255: (1, 7, 7, 7)}                                              # the masked-out 99 does not count
    for g in range(256):
        assert tuple(int(x) for x in got[g]) == want.get(g, IDENTITY), g
    # no mask: every row, the zeros under key 0 included
    full = expected_groups(vals, keys, None)
    assert tuple(int(x) for x in full[0]) == (2048 - 5, 0, 0, 2 ** 63) and tuple(int(x) for x in full[255]) == (2, 106, 7, 99)
    assert int(full[:, 0].sum()) == 2048
    # a block taken out (a device check failed): block 1 contributes nothing
    part = expected_groups(vals, keys, bits, without=(1,))
    assert tuple(int(x) for x in part[5]) == (2, 2, 3, 2 ** 64 - 1) and tuple(int(x) for x in part[0]) == IDENTITY
    # narrow value types are zero-extended
    assert tuple(int(x) for x in expected_groups(np.full(1024, 255, np.uint8), np.full(1024, 9, np.uint8), None)[9]) == (1024, 261120, 255, 255)
