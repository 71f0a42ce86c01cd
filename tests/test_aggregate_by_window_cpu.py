"""CPU: unfor_aggregate_by_window / unfor_aggregate_by_window_widths (COUNT / SUM / MIN / MAX of a FoR-packed value column grouped by a
FoR-packed key column of the same type inside a dense window of the key domain) -- the header declares and the library exports them for
every element type through a macro of their own, the Python table agrees with the header, every refusal needs no GPU under each kernel
policy, the Python mirror validates before any launch, the C++ mirror compiles, and the block decisions the kernel and the host share
(fastlanes_amd/csrc/fl_aggregate_by_window_map.hpp, compiled here with g++) are SOUND: exhaustively at a 4-bit model type against brute
force over the keys a block can hold, and on a seeded sample of the real types against a restatement in Python integers."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)

FORMS = ("unfor_aggregate_by_window", "unfor_aggregate_by_window_widths")
SKIP, OUTSIDE, ONE_GROUP, EACH = 0, 1, 2, 3
TAIL = ["mask", "n_blocks", "key_lo", "n_groups", "counts", "sums", "mins", "maxs", "stats"]


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
    body = text.split("#define FL_DECLARE_AGGREGATE_BY_WINDOW(T, S)")[1].split("FL_DECLARE_AGGREGATE_BY_WINDOW(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_AGGREGATE_BY_WINDOW({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.aggregate_by_window_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_symbols(), fastlanes_amd.select_symbols(), fastlanes_amd.aggregate_symbols(),
                  fastlanes_amd.for_compare_range_symbols(), fastlanes_amd.aggregate_by_symbols(), fastlanes_amd.for_compare_columns_symbols(),
                  fastlanes_amd.aggregate_columns_symbols(), fastlanes_amd.for_compare_in_symbols(), fastlanes_amd.aggregate_by_columns_symbols(),
                  fastlanes_amd.set_build_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    internal = open(os.path.join(ROOT, "include", "fastlanes_amd_internal.h")).read()
    assert "aggregate_by_window" not in internal                            # no internal symbol is added
    for s in want:
        assert hasattr(lib, s), s
    assert {"aggregate_by_window_symbols", "unfor_aggregate_by_window_widths", "GroupTable"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.FoR, "unfor_aggregate_by_window")


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: a pointer is c_void_p, `unsigned` c_uint, size_t c_size_t, uint64_t
    c_uint64, the element type its own scalar; the two columns' arguments are unfor_aggregate_by's, the key column of type T"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("AGGREGATE_BY_WINDOW")}
    assert len(rows) == 8
    for ty in TYPE_BITS:
        for form in FORMS:
            name = f"fl_{ty}_{form}"
            ret, args = protos[name]
            restype, argtypes = rows[name]
            assert ret == "int" and restype is ctypes.c_int
            by_args = [a for _, a in protos[name.replace("_by_window", "_by")][1]]
            head = by_args[:by_args.index("mask")]
            tail = ["stream"] if form == "unfor_aggregate_by_window" else ["err_flag", "stream"]
            assert [a for _, a in args] == head + TAIL + tail, name
            assert len(args) == len(argtypes), name
            scalars = {"unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64, CT[ty]: _lib.CTYPE[ty]}
            for (ctype, arg), at in zip(args, argtypes):
                assert at is (ctypes.c_void_p if "*" in ctype else scalars[ctype]), (name, arg, ctype)
            types = dict((a, c) for c, a in args)
            assert types["key_lo"] == CT[ty] and types["n_groups"] == "uint64_t" and types["mask"] == "const uint32_t *"
            assert types["keys"] == types["key_references"] == f"const {CT[ty]} *"
            assert all(types[a] == "uint64_t *" for a in ("counts", "sums", "mins", "maxs", "stats"))
            assert getattr(lib, name).argtypes == argtypes


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), under each kernel policy: either width (FL_ERR_WIDTH,
    also for an empty column); n_groups above min(2^T, 2^32) (FL_ERR_INDEX); the empty column; the columns' pointers (FL_ERR_NULL);
    alignment of the packed columns, the mask, the four arrays and stats.  The mask, the four arrays and stats may be NULL."""
    buf = np.zeros(8192, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    A, AR, K, KR, MK, W, O, KW, KO, CN, SM, MN, MX, ST = (p + 4096 * i for i in range(14))
    try:
        for policy in (0, 1, 2):
            lib.fl_internal_set_kernel_policy(policy)
            for ty, T in TYPE_BITS.items():
                f = getattr(lib, f"fl_{ty}_unfor_aggregate_by_window")
                g = getattr(lib, f"fl_{ty}_unfor_aggregate_by_window_widths")
                top = min(1 << T, 1 << 32)

                def uni(w=3, a=A, ar=AR, kw=2, k=K, kr=KR, mk=MK, n=1, lo=5, ng=40, cn=CN, sm=SM, mn=MN, mx=MX, st=ST):
                    return f(w, a, ar, 1, kw, k, kr, 1, mk, n, lo, ng, cn, sm, mn, mx, st, None)

                def mix(w=W, o=O, a=A, ab=384, ar=AR, kw=KW, ko=KO, k=K, kb=256, kr=KR, mk=MK, n=1, lo=5, ng=40, cn=CN, sm=SM, mn=MN, mx=MX, st=ST):
                    return g(w, o, a, ab, ar, 1, kw, ko, k, kb, kr, 1, mk, n, lo, ng, cn, sm, mn, mx, st, None, None)

                # FL_ERR_WIDTH: either column, also for an empty column and in front of every other refusal
                for n in (1, 0):
                    assert uni(w=T + 1, n=n) == 1 and uni(kw=T + 1, n=n) == 1 and uni(kw=T + 1, ng=top + 1, n=n) == 1 and uni(w=T + 1, a=None, n=n) == 1
                assert uni(w=T, kw=T, a=None) == 3                              # the widest widths are not refused as widths
                # FL_ERR_INDEX: n_groups above min(2^T, 2^32); also for an empty column, and in front of the NULL checks
                for n in (1, 0):
                    for ng in (top + 1, top + 32, 1 << 33, 2 ** 64 - 1):
                        assert uni(ng=ng, n=n) == 2 and mix(ng=ng, n=n) == 2, (ty, ng)
                assert uni(ng=top + 1, a=None) == 2 and mix(ng=top + 1, k=None) == 2
                assert uni(ng=top, a=None) == 3 and mix(ng=top, kr=None) == 3   # the largest window is not refused
                # n_blocks == 0: nothing to do, whatever the pointers
                assert f(3, None, None, 0, 2, None, None, 0, None, 0, 5, 40, None, None, None, None, None, None) == 0
                assert g(None, None, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, 5, 40, None, None, None, None, None, None, None) == 0
                # FL_ERR_NULL: each required pointer of either column
                for name in ("a", "ar", "k", "kr"):
                    assert uni(**{name: None}) == 3, (ty, name)
                for name in ("w", "o", "a", "ar", "kw", "ko", "k", "kr"):
                    assert mix(**{name: None}) == 3, (ty, name)
                # FL_ERR_ALIGN: the packed columns, the mask, the four arrays and stats off a 16-byte boundary
                for name, at in (("a", A), ("k", K), ("mk", MK), ("cn", CN), ("sm", SM), ("mn", MN), ("mx", MX), ("st", ST)):
                    for d in (4, 8):
                        assert uni(**{name: at + d}) == 4 and mix(**{name: at + d}) == 4, (ty, name, d)
                assert uni(a=None, cn=CN + 8) == 3 and uni(kr=None, mk=MK + 8) == 3   # NULL is answered before alignment
                # the mask, each array and stats may be NULL: the call gets past them to the next refusal
                assert uni(mk=None, st=None, cn=None, sm=None, mn=None, mx=None, k=K + 8) == 4
                assert mix(mk=None, st=None, cn=None, sm=None, mn=None, mx=None, a=A + 8) == 4
                for name in ("cn", "sm", "mn", "mx"):
                    assert uni(**{name: None}, st=ST + 8) == 4 and mix(**{name: None}, st=ST + 8) == 4
                # the empty window: the arrays are not touched, so a misaligned one is not refused -- as far as the next refusal
                assert uni(ng=0, cn=CN + 4, sm=SM + 8, a=None) == 3 and uni(ng=0, cn=CN + 4, mk=MK + 8) == 4 and mix(ng=0, mx=MX + 4, st=ST + 8) == 4
                # a packed pointer may be NULL only when no byte of it can be read
                assert uni(w=0, a=None, mk=MK + 8) == 4 and uni(kw=0, k=None, mk=MK + 8) == 4
                assert mix(a=None, ab=0, mk=MK + 8) == 4 and mix(k=None, kb=0, mk=MK + 8) == 4
                assert mix(a=None) == 3 and mix(k=None) == 3 and uni(w=1, a=None) == 3 and uni(kw=1, k=None) == 3
    finally:
        lib.fl_internal_set_kernel_policy(0)


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    w, o = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    ncol, nref = np.zeros(96, np.uint32), np.zeros(1, np.uint32)
    # device tier only: numpy arrays and CPU tensors
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by_window(3, ncol, 0, 3, ncol, 0, 0, 40)
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by_window(3, tcol, 0, 3, tcol, 0, 0, 40)
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_window_widths(w, o, ncol, nref, w, o, ncol, nref, 0, 40)
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_window_widths(tw, to, tcol, tref, tw, to, tcol, tref, 0, 40)
    # the key column has the value column's type
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_window_widths(tw, to, tcol, tref, tw, to, torch.zeros(96, dtype=torch.int16), torch.zeros(1, dtype=torch.int16), 0, 40)
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by_window(3, tcol, 0, 3, torch.zeros(192, dtype=torch.uint8), 0, 0, 40)
    # what: a tuple of distinct names out of count, sum, min, max -- judged before anything else
    for what, error in (("count", TypeError), (("count", "mean"), ValueError), (("sum", "sum"), ValueError), (None, TypeError)):
        with pytest.raises(error):
            fl.unfor_aggregate_by_window_widths(tw, to, tcol, tref, tw, to, tcol, tref, 0, 40, what=what)
        with pytest.raises(error):
            fl.FoR.unfor_aggregate_by_window(3, tcol, 0, 3, tcol, 0, 0, 40, what=what)
    # packed=None is the COUNT-only form
    for what in (("count", "sum"), ("sum",), (), ("count", "min")):
        with pytest.raises(ValueError, match="COUNT-only"):
            fl.unfor_aggregate_by_window_widths(None, None, None, None, tw, to, tcol, tref, 0, 40, what=what)
        with pytest.raises(ValueError, match="COUNT-only"):
            fl.FoR.unfor_aggregate_by_window(None, None, None, 3, tcol, 0, 0, 40, what=what)
    with pytest.raises(ValueError, match="COUNT-only"):
        fl.unfor_aggregate_by_window_widths(None, None, None, None, tw, to, tcol, tref, 0, 40)       # the default names "sum"
    # the table: n_groups within [0, min(2^T, 2^32)]; into= another ty, lo, n_groups or set of arrays (ValueError), not a table (TypeError)
    from fastlanes_amd.codec import _group_table_target, _window_what
    assert _window_what(["max", "count"]) == ("count", "max") and _window_what(()) == ()
    cpu = torch.device("cpu")
    for ty, T in TYPE_BITS.items():
        top = min(1 << T, 1 << 32)
        for ng in (-1, top + 1):
            with pytest.raises(ValueError, match="n_groups"):
                _group_table_target(ty, 0, ng, ("count",), None, cpu)
    t = _group_table_target("u32", -1, 300, ("count", "sum"), None, cpu)      # lo is taken mod 2^T; fresh arrays hold the identities
    assert isinstance(t, fl.GroupTable) and (t.ty, t.lo, t.n_groups) == ("u32", 2 ** 32 - 1, 300) and t.what() == ("count", "sum")
    assert t.mins is None and t.maxs is None and t.counts.dtype == torch.int64 and t.counts.numel() == 300 and not t.counts.any() and not t.sums.any()
    full = _group_table_target("u8", 7, 5, ("count", "sum", "min", "max"), None, cpu)
    assert full.mins.tolist() == [-1] * 5 and full.maxs.tolist() == [0] * 5 and list(full)[:3] == ["u8", 7, 5]
    for args in (("u16", -1, 300, ("count", "sum")), ("u32", 5, 300, ("count", "sum")), ("u32", -1, 301, ("count", "sum")),
                 ("u32", -1, 300, ("count",)), ("u32", -1, 300, ("count", "sum", "min"))):
        with pytest.raises(ValueError):
            _group_table_target(*args, t, cpu)
    with pytest.raises(TypeError):
        _group_table_target("u32", -1, 300, ("count", "sum"), t.counts, cpu)
    with pytest.raises(TypeError):                                           # a table whose arrays are not on a device
        _group_table_target("u32", -1, 300, ("count", "sum"), t, cpu)


# ---- the block decisions ---------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "fl_aggregate_by_window_map.hpp"
#include <stddef.h>
// the array form: query i = (key_lo, n_groups, key reference, key width, value width, need_values, mask_empty, precondition_ok, kept)
// -> the block's route, c, what a DECIDED block adds to {inside, outside}, and which columns it reads
extern "C" void window_route_n(unsigned type_bits, size_t n, const uint64_t* key_lo, const uint64_t* n_groups, const uint64_t* ref,
                               const uint8_t* key_width, const uint8_t* value_width, const uint8_t* need_values, const uint8_t* mask_empty,
                               const uint8_t* ok, const uint64_t* kept, int* route, uint64_t* c_out, uint64_t* inside, uint64_t* outside,
                               uint8_t* reads_keys, uint8_t* reads_values)
{
    for (size_t i = 0; i < n; ++i) {
        const fl::ForPredicate window = fl::set_window(type_bits, key_lo[i], n_groups[i]);
        const fl::AggregateByWindowRoute r =
            fl::aggregate_by_window_route(type_bits, window, mask_empty[i] != 0, ok[i] != 0, ref[i], key_width[i], c_out[i]);
        route[i] = r;
        inside[i] = fl::aggregate_by_window_inside(r, kept[i]);
        outside[i] = fl::aggregate_by_window_outside(r, kept[i]);
        reads_keys[i] = fl::aggregate_by_window_reads_keys(r);
        reads_values[i] = fl::aggregate_by_window_reads_values(r, value_width[i], need_values[i] != 0);
    }
}
extern "C" uint64_t window_lds_groups(void) { return fl::AGGREGATE_BY_WINDOW_LDS_GROUPS; }
extern "C" int window_lds_tier_of(uint64_t n_groups) { return fl::aggregate_by_window_lds_tier(n_groups); }
extern "C" uint64_t window_max_groups_of(unsigned type_bits) { return fl::aggregate_by_window_max_groups(type_bits); }
extern "C" unsigned window_wave_lds_of(unsigned block_bytes, int lds_tier) { return fl::aggregate_by_window_wave_lds(block_bytes, lds_tier != 0); }
extern "C" unsigned window_slot_bytes(void) { return (unsigned)sizeof(fl::BlockAggregate); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "aggregate_by_window_map", SHIM)
    P = ctypes.c_void_p
    so.window_route_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 15
    so.window_route_n.restype = None
    so.window_lds_groups.restype = ctypes.c_uint64
    so.window_lds_tier_of.argtypes = [ctypes.c_uint64]
    so.window_max_groups_of.argtypes = [ctypes.c_uint]
    so.window_max_groups_of.restype = ctypes.c_uint64
    so.window_wave_lds_of.argtypes = [ctypes.c_uint, ctypes.c_int]
    so.window_wave_lds_of.restype = ctypes.c_uint
    so.window_slot_bytes.restype = ctypes.c_uint
    return so


def routes(shim, T, lo, groups, ref, kw, vw, need, empty, ok, kept):
    lo, groups, ref, kept = (np.array(x, dtype=np.uint64) for x in (lo, groups, ref, kept))
    kw, vw, need, empty, ok = (np.array(x, dtype=np.uint8) for x in (kw, vw, need, empty, ok))
    n = lo.size
    route, c, ins, out = np.empty(n, np.int32), np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint64)
    rk, rv = np.empty(n, np.uint8), np.empty(n, np.uint8)
    shim.window_route_n(T, n, *(x.ctypes.data for x in (lo, groups, ref, kw, vw, need, empty, ok, kept, route, c, ins, out, rk, rv)))
    return route, c, ins, out, rk, rv


def test_tiers_and_lds_bytes(shim):
    assert shim.window_lds_groups() == 256 and shim.window_slot_bytes() == 32      # the 8 KiB table unfor_aggregate_by ships with
    assert [shim.window_lds_tier_of(g) for g in (0, 1, 256, 257, 2 ** 32)] == [1, 1, 1, 0, 0]
    assert [shim.window_max_groups_of(T) for T in (8, 16, 32, 64)] == [256, 65536, 2 ** 32, 2 ** 32]
    # per wavefront: the block's image (128 * T bytes) and, in the LDS tier, the table: 9 / 10 / 12 / 16 KiB for u8 / u16 / u32 / u64
    assert [shim.window_wave_lds_of(128 * T, 1) for T in (8, 16, 32, 64)] == [1024 + 8192, 2048 + 8192, 4096 + 8192, 8192 + 8192]
    assert [shim.window_wave_lds_of(128 * T, 0) for T in (16, 32, 64)] == [2048, 4096, 8192]


def test_routes_are_sound_at_four_bits(shim):
    """every (key_lo, n_groups, key reference, key width, mask in {empty, one bit, full}, failed check) of a 4-bit model type, against
    brute force over the keys the block CAN hold: an OUTSIDE block can update no slot (every kept row is outside), a ONE_GROUP block
    updates exactly slot c with every kept row, and exactly the blocks that may hold keys on both sides of the window's edge -- or
    several inside it -- are decoded; the value column is requested only by a block that updates something, only when an array
    needs values, and never at width 0"""
    T, N = 4, 16
    q = []
    for lo in range(N):
        for groups in range(N + 1):
            for ref in range(N):
                for w in range(T + 1):
                    for kept in (0, 1, 1024):
                        for ok in (1, 0):
                            q.append((lo, groups, ref, w, (lo + ref + w) % (T + 1), (lo + groups + ref) % 2, kept == 0, ok, kept))
    assert len(q) == 16 * 17 * 16 * 5 * 3 * 2
    route, c, ins, out, rk, rv = routes(shim, T, *([x[j] for x in q] for j in range(9)))
    seen = set()
    for i, (lo, groups, ref, w, vw, need, empty, ok, kept) in enumerate(q):
        window = {(lo + j) % N for j in range(groups)}
        keys = {(ref + f) % N for f in range(1 << w)}
        slots = {(k - lo) % N for k in keys if k in window}                 # the slots the block can update
        r = int(route[i])
        what = (lo, groups, ref, w, empty, ok)
        assert int(c[i]) == (ref - lo) % N
        assert int(rk[i]) == (r == EACH)
        assert int(rv[i]) == (r in (ONE_GROUP, EACH) and bool(need) and vw != 0), what
        if empty or not ok:
            assert r == SKIP and int(ins[i]) == int(out[i]) == 0, ("an empty mask or a failed check must contribute nothing", what)
        elif not slots:
            assert r == OUTSIDE and (int(ins[i]), int(out[i])) == (0, kept), ("OUTSIDE: no slot can be updated", what)
        elif w == 0:
            assert r == ONE_GROUP and slots == {int(c[i])} and int(c[i]) < groups and (int(ins[i]), int(out[i])) == (kept, 0), ("ONE_GROUP: exactly slot c", what)
        else:
            assert r == EACH and int(ins[i]) == int(out[i]) == 0, ("left to the decode", what)
        if r == OUTSIDE:
            assert not (keys & window), ("OUTSIDE claimed", what)
        seen.add((r, w == 0, groups == 0, groups == N))
    assert {(SKIP, True, True, False), (OUTSIDE, True, True, False), (OUTSIDE, False, False, False), (ONE_GROUP, True, False, True),
            (ONE_GROUP, True, False, False), (EACH, False, False, True), (EACH, False, False, False)} <= seen
    assert not any(r == EACH and z for r, z, _, _ in seen) and not any(r in (ONE_GROUP, EACH) and e for r, _, e, _ in seen)


@pytest.mark.parametrize("T", [8, 16, 32, 64])
def test_routes_on_a_seeded_sample(shim, T):
    """10^5 cases per real type against a restatement in Python integers: the block's slots {(c + f) mod 2^T} meet the window
    [0, n_groups - 1] iff c lies inside it or c + 2^KW - 1 passes 2^T; windows of 0, 1, 255 .. 257, 65535 .. 65537 and the largest
    number of groups, key references at both ends of the window and of the domain, key widths 0 and T, empty masks, failed checks"""
    N = 1 << T
    top = min(N, 1 << 32)
    rng = random.Random(98000 + T)
    sizes = [g for g in (0, 1, 2, 31, 32, 255, 256, 257, 2048, 65535, 65536, 65537, top - 1, top) if g <= top]
    q, want = [], []
    counts = dict(skip=0, outside=0, one_group=0, each=0, wraps=0, values=0)
    for i in range(100_000):
        groups = sizes[i % len(sizes)] if i % 3 else rng.randint(0, top)
        lo = [0, N - 1, N >> 1, (N - groups) % N][i % 4] if i % 5 == 0 else rng.randrange(N)
        w = [0, T, 1, T - 1, 0][i % 11] if i % 11 < 5 else rng.randint(0, T)
        vw, need = rng.choice([0, 0, 1, T, rng.randint(0, T)]), i % 3 != 1
        span = (1 << w) - 1
        kind = i % 7
        if kind == 0:
            ref = (lo + groups) % N                                         # the first key behind the window
        elif kind == 1:
            ref = (lo - span - 1) % N                                       # the block ends just in front of the window
        elif kind == 2:
            ref = (lo - span) % N                                           # ... or on its first key
        elif kind == 3:
            ref = (lo + max(groups, 1) - 1) % N                             # the window's last key
        elif kind == 4:
            ref = (lo + rng.randint(0, max(groups, 1) - 1)) % N             # inside
        else:
            ref = rng.randrange(N)
        empty, ok = i % 13 == 0, i % 17 != 0
        kept = 0 if empty else rng.randint(1, 1024)
        c = (ref - lo) % N
        if empty or not ok:
            r = SKIP
        elif groups == 0 or not (c <= groups - 1 or c + span >= N):
            r = OUTSIDE
        elif w == 0:
            r = ONE_GROUP
        else:
            r = EACH
        reads_values = r in (ONE_GROUP, EACH) and need and vw != 0
        counts[("skip", "outside", "one_group", "each")[r]] += 1
        counts["wraps"] += lo + groups > N
        counts["values"] += reads_values
        q.append((lo, groups, ref, w, vw, need, empty, ok, kept))
        want.append((r, c, kept if r == ONE_GROUP else 0, kept if r == OUTSIDE else 0, int(r == EACH), int(reads_values)))
    assert all(v > 500 for v in counts.values()), counts
    got = routes(shim, T, *([x[j] for x in q] for j in range(9)))
    for i in range(len(q)):
        assert tuple(int(g[i]) for g in got) == want[i], (T, q[i], want[i])


def test_cpp_mirror_declares_both_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the two new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint16_t;
using U64 = std::uint64_t;
void (*const uniform)(std::size_t, const T*, const T*, std::size_t, std::size_t, const T*, const T*, std::size_t, const std::uint32_t*, std::size_t,
                      T, U64, U64*, U64*, U64*, U64*, U64*, void*) = &fastlanes::FoR<T>::unfor_aggregate_by_window_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const std::uint8_t*, const std::uint64_t*,
                    const T*, std::size_t, const T*, std::size_t, const std::uint32_t*, std::size_t, T, U64, U64*, U64*, U64*, U64*, U64*,
                    std::uint32_t*, void*) = &fastlanes::unfor_aggregate_by_window_widths_device<T>;
int main() { return uniform && mixed ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
