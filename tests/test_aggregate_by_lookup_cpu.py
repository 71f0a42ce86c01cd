"""CPU: unfor_aggregate_by_lookup / unfor_aggregate_by_lookup_widths (GROUP BY a u8 dimension attribute fetched through a FoR-packed
key column: unfor_lookup_u8 and unfor_aggregate_by in one pass) -- the header declares and the library exports the 8 symbols through a
macro of its own, the Python table agrees with the header, every refusal needs no GPU, the Python mirror checks its arguments before
any launch, the numpy model of the definition (tests/aggregate_by_lookup_data.py) equals the chain it replaces on the GPU test's own
inputs, and the block routes the kernel and the host share (fastlanes_amd/csrc/fl_aggregate_by_lookup_map.hpp, compiled here with g++)
are SOUND: exhaustively over the 8-bit domain against the per-element definition, and on seeded samples of the 16 / 32 / 64-bit types
with windows that wrap past 2^T - 1."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from aggregate_by_lookup_data import (EACH, FORMS, MISSING, NOTHING, ONE_GROUP, RUN_OF_3, SKIP, STATS_PREFILL, code_table, expected_fused,
                                      present_words, route_masks, route_of, route_pair, routes_taken, window_lo, window_sizes)
from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)
from group_data import expected_groups
from lookup_data import ABSENT_SLOT, expected_lookup


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
    body = text.split("#define FL_DECLARE_AGGREGATE_BY_LOOKUP(T, S)")[1].split("FL_DECLARE_AGGREGATE_BY_LOOKUP(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_AGGREGATE_BY_LOOKUP({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS]
    assert len(want) == 8 and sorted(fastlanes_amd.aggregate_by_lookup_symbols()) == sorted(want)
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.lookup_symbols(), fastlanes_amd.set_build_symbols(),
                  fastlanes_amd.aggregate_by_window_symbols(), fastlanes_amd.aggregate_by_symbols(), fastlanes_amd.select_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"aggregate_by_lookup_symbols", "unfor_aggregate_by_lookup_widths"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.FoR, "unfor_aggregate_by_lookup")
    doc = text.split("#define FL_DECLARE_AGGREGATE_BY_LOOKUP(T, S)")[0].rsplit("/*", 1)[1]
    for words in ("Out of scope", "a value type different from the key type", "more than 256 groups", "several tables", "LDS\n * copy of the dimension table",
                  "sparse or hashed keys", "Delta", "host tier", "2^31 bytes"):
        assert words in doc, words
    lookup_doc = text.split("#define FL_DECLARE_LOOKUP(T, S)")[0].rsplit("/*", 1)[1]
    assert "a fused GROUP BY-through-lookup kernel" not in lookup_doc       # no longer out of the lookup's scope: it exists


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: the two columns, mask and n_blocks are unfor_aggregate_by_window's, then
    key_lo, n_slots, table, present, result, stats, err_flag, stream -- BOTH forms take err_flag, as unfor_aggregate_by's do"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("AGGREGATE_BY_LOOKUP")}
    assert len(rows) == 8
    scalars = {"unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64}
    for ty in TYPE_BITS:
        for widths in (False, True):
            name = f"fl_{ty}_{FORMS[widths]}"
            ret, args = protos[name]
            restype, argtypes = rows[name]
            assert ret == "int" and restype is ctypes.c_int
            window = [a for _, a in protos[f"fl_{ty}_unfor_aggregate_by_window{'_widths' if widths else ''}"][1]]
            head = window[:window.index("key_lo")]                          # the two columns, mask, n_blocks
            assert [a for _, a in args] == head + ["key_lo", "n_slots", "table", "present", "result", "stats", "err_flag", "stream"], name
            assert len(args) == len(argtypes), name
            types = dict((a, c) for c, a in args)
            assert types["key_lo"] == CT[ty] and types["n_slots"] == "uint64_t" and types["table"] == "const uint8_t *"
            assert types["present"] == "const uint32_t *" and types["result"] == "void *" and types["stats"] == "uint64_t *"
            assert types["keys"] == f"const {CT[ty]} *" and types["key_references"] == f"const {CT[ty]} *" and types["mask"] == "const uint32_t *"
            for (ctype, arg), at in zip(args, argtypes):
                want = ctypes.c_void_p if "*" in ctype else _lib.CTYPE[ty] if arg == "key_lo" else scalars[ctype]
                assert at is want, (name, arg, ctype)
            assert getattr(lib, name).argtypes == argtypes


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before any device work (no call here reaches a kernel), in the order of the two parents: either width
    above T (FL_ERR_WIDTH, also for an empty column); n_slots above min(2^T, 2^32) or a table of 2^31 bytes or more (FL_ERR_INDEX);
    result NULL, table NULL with n_slots > 0, a required column pointer NULL (FL_ERR_NULL); alignment of both packed columns, mask,
    present, table, result and stats (FL_ERR_ALIGN).  mask, present and stats may be NULL.  (n_blocks == 0 with a valid result is
    FL_OK and WRITES the identities: a launch, so the GPU tests hold it.)"""
    buf = np.zeros(8192, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    A, AR, K, KR, MK, TB, W, O, KW, KO, ST, PR, RES = (p + 4096 * i for i in range(13))
    for ty, T in TYPE_BITS.items():
        f, g = getattr(lib, f"fl_{ty}_{FORMS[0]}"), getattr(lib, f"fl_{ty}_{FORMS[1]}")
        top = min(1 << T, 1 << 32, (1 << 31) - 1)                           # the largest table that is not refused

        def uni(w=3, a=A, ar=AR, kw=2, k=K, kr=KR, mk=MK, n=1, lo=5, ns=40, tb=TB, pr=PR, res=RES, st=ST):
            return f(w, a, ar, 1, kw, k, kr, 1, mk, n, lo, ns, tb, pr, res, st, None, None)

        def mix(w=W, o=O, a=A, ab=384, ar=AR, kw=KW, ko=KO, k=K, kb=256, kr=KR, mk=MK, n=1, lo=5, ns=40, tb=TB, pr=PR, res=RES, st=ST):
            return g(w, o, a, ab, ar, 1, kw, ko, k, kb, kr, 1, mk, n, lo, ns, tb, pr, res, st, None, None)

        # FL_ERR_WIDTH: either width, also for an empty column and in front of every other refusal
        for n in (1, 0):
            assert uni(w=T + 1, n=n) == 1 and uni(kw=T + 1, n=n) == 1 and uni(w=T + 1, ns=top + 1, n=n) == 1 and uni(kw=T + 1, res=None, n=n) == 1
        assert uni(w=T, kw=T, res=None) == 3                                # the widest widths are not refused as widths
        # FL_ERR_INDEX: also for an empty column, and in front of the NULL checks
        for n in (1, 0):
            for ns in (top + 1, top + 32, 1 << 33, 2 ** 64 - 1):
                assert uni(ns=ns, n=n) == 2 and mix(ns=ns, n=n) == 2, (ty, ns)
        assert uni(ns=top + 1, res=None) == 2 and mix(ns=top + 1, a=None) == 2
        assert uni(ns=top, tb=None) == 3 and mix(ns=top, tb=None) == 3      # the largest table is not refused
        # FL_ERR_NULL: result is required even for an empty column (every call writes it); each required pointer; table with n_slots > 0
        assert uni(res=None, n=0) == 3 and mix(res=None, n=0) == 3
        assert f(3, None, None, 0, 2, None, None, 0, None, 0, 5, 40, None, None, None, None, None, None) == 3
        for name in ("a", "ar", "k", "kr", "tb", "res"):
            assert uni(**{name: None}) == 3, (ty, name)
        for name in ("w", "o", "a", "ar", "kw", "ko", "k", "kr", "tb", "res"):
            assert mix(**{name: None}) == 3, (ty, name)
        # FL_ERR_ALIGN: every pointer the kernel reads or writes 16 bytes at a time
        for name, at in (("a", A), ("k", K), ("mk", MK), ("pr", PR), ("tb", TB), ("res", RES), ("st", ST)):
            for d in (4, 8):
                assert uni(**{name: at + d}) == 4 and mix(**{name: at + d}) == 4, (ty, name, d)
        assert uni(res=RES + 8, n=0) == 4                                   # ... result also for an empty column
        assert uni(a=None, tb=TB + 8) == 3 and uni(res=None, mk=MK + 8) == 3 and uni(k=None, res=RES + 8) == 3  # NULL before alignment
        # mask, present and stats may be NULL: the call gets past them to the next refusal
        assert uni(mk=None, pr=None, st=None, tb=TB + 8) == 4 and mix(mk=None, pr=None, st=None, k=K + 8) == 4
        # the empty window: neither table nor present is read, so neither NULL nor a misaligned pointer is refused
        assert uni(ns=0, tb=None, a=None) == 3 and uni(ns=0, tb=None, mk=MK + 8) == 4 and uni(ns=0, tb=TB + 4, pr=PR + 4, mk=MK + 8) == 4
        assert mix(ns=0, tb=None, kr=None) == 3 and mix(ns=0, tb=TB + 4, st=ST + 8) == 4
        # a packed pointer may be NULL only when no byte of it can be read
        assert uni(w=0, a=None, mk=MK + 8) == 4 and uni(kw=0, k=None, mk=MK + 8) == 4 and mix(a=None, ab=0, mk=MK + 8) == 4
        assert mix(k=None, kb=0, mk=MK + 8) == 4 and mix(a=None) == 3 and mix(k=None) == 3 and uni(w=1, a=None) == 3 and uni(kw=1, k=None) == 3


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    table = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(TypeError):                                          # device tier only: numpy arrays and CPU tensors
        fl.FoR.unfor_aggregate_by_lookup(3, np.zeros(96, dtype=np.uint32), 0, 3, np.zeros(96, dtype=np.uint32), 0, 0, np.zeros(4, np.uint8))
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by_lookup(3, tcol, 0, 3, tcol, 0, 0, table)
    with pytest.raises(TypeError):                                          # the key column has the value column's type
        fl.FoR.unfor_aggregate_by_lookup(3, tcol, 0, 3, torch.zeros(96, dtype=torch.int16), 0, 0, table)
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_lookup_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(1, np.uint32),
                                            np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(1, np.uint32), 0,
                                            np.zeros(4, np.uint8))
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_lookup_widths(tw, to, tcol, tref, tw, to, tcol, tref, 0, table)
    with pytest.raises(TypeError):
        fl.unfor_aggregate_by_lookup_widths(tw, to, tcol, tref, tw, to, torch.zeros(96, dtype=torch.int64), tref, 0, table)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", list(TYPE_BITS))
def test_model_is_the_chain_on_the_gpu_tests_inputs(oracle, ty):
    """the model of the fused call equals what it replaces -- lookup_data.expected_lookup (the u8 codes in row order, the hits, stats)
    followed by group_data.expected_groups with the codes as keys and mask = the hits -- on the column pairs, windows, masks and
    bitmaps tests/test_gpu_aggregate_by_lookup.py runs; and the chosen columns take every route (the GPU test asserts the same)"""
    T = TYPE_BITS[ty]
    N = 1 << T
    lo = window_lo(ty)
    seen = set()
    for n in (3, 11):
        pair = route_pair(oracle, ty, n, 41000 + T + n)
        vals, keys = pair["val"]["decoded"], pair["key"]["decoded"]
        for n_slots in window_sizes(ty):
            table = code_table(n_slots, 41200 + n_slots % 1000)
            pw = present_words(n_slots, 41300 + n_slots % 1000, clear=(ABSENT_SLOT,))
            if n_slots:
                pw[0] |= 1
            for keep in route_masks(n, 41100 + n).values():
                for present in (None, pw):
                    result, stats, hit = expected_fused(ty, vals, keys, keep, lo, table, present, STATS_PREFILL)
                    _, _, lstats, codes, h = expected_lookup(oracle, ty, "u8", keys, keep, lo, table, present, 0, STATS_PREFILL)
                    assert np.array_equal(h, hit) and lstats.tolist() == stats.tolist()
                    assert np.array_equal(result, expected_groups(vals, codes, h)), (ty, n, n_slots)
                    if n == 11:
                        seen |= routes_taken(ty, pair, keep, lo, n_slots, present)
                    if n == 11 and keep is None and present is None and 2 < n_slots < N:
                        assert result[255, 0] >= 1024 and result[0, 0] > 0  # codes 255 (slot 0) and 0 (slot 2) are groups that occur
    assert seen == {"NOTHING", "MISSING", "ONE_GROUP present", "ONE_GROUP absent", "EACH"}, seen
    assert RUN_OF_3 >> 16 & 0xFF == 3


# ---- the block routes --------------------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "fl_aggregate_by_lookup_map.hpp"
#include <stddef.h>
using namespace fl;
// the array form: query i = (key_lo, n_slots, key reference, key width, mask_empty, precondition_ok) -> the block's route and c
extern "C" void aggl_route_n(unsigned type_bits, size_t n, const uint64_t* key_lo, const uint64_t* n_slots, const uint64_t* ref, const uint8_t* width,
                             const uint8_t* mask_empty, const uint8_t* ok, int* route, uint64_t* c_out)
{
    for (size_t i = 0; i < n; ++i)
        route[i] = aggregate_by_lookup_route(type_bits, set_window(type_bits, key_lo[i], n_slots[i]), mask_empty[i] != 0, ok[i] != 0, ref[i], width[i], c_out[i]);
}
// what the routes read and count: row r = route, columns = reads_keys, reads_values(w 3, present), reads_values(w 3, absent),
// reads_values(w 0, present), reads_table, decided hits / misses of 7 kept rows with the slot present, then absent
extern "C" void aggl_effects(uint64_t* out)
{
    for (int r = 0; r < 5; ++r) {
        const AggregateByLookupRoute route = (AggregateByLookupRoute)r;
        uint64_t* o = out + 9 * r;
        o[0] = aggregate_by_lookup_reads_keys(route);
        o[1] = aggregate_by_lookup_reads_values(route, 3, true);
        o[2] = aggregate_by_lookup_reads_values(route, 3, false);
        o[3] = aggregate_by_lookup_reads_values(route, 0, true);
        o[4] = aggregate_by_lookup_reads_table(route);
        o[5] = aggregate_by_lookup_decided_hits(route, 7, true);
        o[6] = aggregate_by_lookup_decided_misses(route, 7, true);
        o[7] = aggregate_by_lookup_decided_hits(route, 7, false);
        o[8] = aggregate_by_lookup_decided_misses(route, 7, false);
    }
}
extern "C" unsigned aggl_wave_lds(unsigned block_bytes) { return aggregate_by_lookup_wave_lds(block_bytes); }
// EXHAUSTIVE over the 8-bit domain: every (key_lo, n_slots 0 .. 256, key reference, key width 0 .. 8, mask empty / not, check failed /
// not) against the per-element definition -- the keys a block CAN hold are (reference + f) mod 256, f < 2^W; their slots (key -
// key_lo) mod 256.  Returns the number of violations; counts[route] = how often each route was taken; first[0 .. 5] = the first violation.
extern "C" uint64_t aggl_exhaustive_u8(uint64_t* counts, uint64_t* first)
{
    static uint16_t least[256][256][9], most[256][256][9];                  // [key_lo][reference][width]: the least / greatest slot of the block
    for (unsigned lo = 0; lo < 256; ++lo)
        for (unsigned ref = 0; ref < 256; ++ref)
            for (unsigned w = 0; w <= 8; ++w) {
                unsigned m = 256, M = 0;
                for (unsigned f = 0; f < (1u << w); ++f) {
                    const unsigned j = (((ref + f) & 255u) - lo) & 255u;
                    m = j < m ? j : m;
                    M = j > M ? j : M;
                }
                least[lo][ref][w] = (uint16_t)m;
                most[lo][ref][w] = (uint16_t)M;
            }
    uint64_t bad = 0;
    for (unsigned lo = 0; lo < 256; ++lo)
        for (unsigned slots = 0; slots <= 256; ++slots) {
            const ForPredicate window = set_window(8, lo, slots);
            for (unsigned ref = 0; ref < 256; ++ref)
                for (unsigned w = 0; w <= 8; ++w)
                    for (unsigned q = 0; q < 3; ++q) {                      // q: 0 a kept row, 1 an empty mask, 2 a failed check
                        uint64_t c = ~0ull;
                        const int r = aggregate_by_lookup_route(8, window, q == 1, q != 2, ref, w, c);
                        const bool none_inside = least[lo][ref][w] >= slots;   // no key of the block lies in the window
                        int want;
                        if (q == 2) want = AGGL_SKIP;
                        else if (q == 1) want = AGGL_NOTHING;
                        else if (none_inside) want = AGGL_MISSING;
                        else if (w == 0) want = AGGL_ONE_GROUP;
                        else want = AGGL_EACH;
                        bool ok = r == want && c == ((ref - lo) & 255u);
                        // ONE_GROUP: EVERY key of the block sits at slot c, inside the window
                        if (r == AGGL_ONE_GROUP) ok = ok && least[lo][ref][w] == c && most[lo][ref][w] == c && c < slots;
                        ++counts[r];
                        if (!ok && bad++ == 0) { first[0] = lo; first[1] = slots; first[2] = ref; first[3] = w; first[4] = q; first[5] = (uint64_t)r; }
                    }
        }
    return bad;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "aggregate_by_lookup_map", SHIM)
    P = ctypes.c_void_p
    so.aggl_route_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 8
    so.aggl_route_n.restype = None
    so.aggl_effects.argtypes = [P]
    so.aggl_effects.restype = None
    so.aggl_wave_lds.argtypes = [ctypes.c_uint]
    so.aggl_wave_lds.restype = ctypes.c_uint
    so.aggl_exhaustive_u8.argtypes = [P, P]
    so.aggl_exhaustive_u8.restype = ctypes.c_uint64
    return so


def routes(shim, T, lo, slots, ref, width, empty, ok):
    lo, slots, ref = (np.array(x, dtype=np.uint64) for x in (lo, slots, ref))
    width, empty, ok = (np.array(x, dtype=np.uint8) for x in (width, empty, ok))
    route, c = np.empty(lo.size, np.int32), np.empty(lo.size, np.uint64)
    shim.aggl_route_n(T, lo.size, *(x.ctypes.data for x in (lo, slots, ref, width, empty, ok, route, c)))
    return route, c


def test_routes_are_sound_exhaustively_over_the_8_bit_domain(shim):
    """all 256 * 257 * 256 * 9 * 3 = 455 million cases, checked inside the shim: a failed check is SKIP, an empty mask NOTHING, a block
    routed MISSING has NO key in the window, a block routed ONE_GROUP has EVERY key at slot c < n_slots, everything else -- and only
    that -- is decoded; c = (reference - key_lo) mod 2^T always"""
    counts, first = np.zeros(5, np.uint64), np.zeros(6, np.uint64)
    bad = shim.aggl_exhaustive_u8(counts.ctypes.data, first.ctypes.data)
    assert bad == 0, ("key_lo, n_slots, reference, width, case, route", first.tolist())
    total = 256 * 257 * 256 * 9
    assert int(counts.sum()) == 3 * total and int(counts[SKIP]) == total and int(counts[NOTHING]) == total
    assert all(int(counts[r]) > 0 for r in (MISSING, ONE_GROUP, EACH)) and int(counts[MISSING] + counts[ONE_GROUP] + counts[EACH]) == total
    # width 0: the reference is inside the window for `slots` of the 256 references
    assert int(counts[ONE_GROUP]) == 256 * sum(range(257))


def test_what_the_routes_read_and_count(shim):
    out = np.zeros(45, np.uint64)
    shim.aggl_effects(out.ctypes.data)
    rows = out.reshape(5, 9).tolist()
    assert rows[SKIP] == [0] * 9 and rows[NOTHING] == [0] * 9              # neither column, no table byte, nothing counted
    assert rows[MISSING] == [0, 0, 0, 0, 0, 0, 7, 0, 7]                     # misses += kept, nothing read
    assert rows[ONE_GROUP] == [0, 1, 0, 0, 1, 7, 0, 0, 7]                   # no key byte; the value block only when the slot is present
    assert rows[EACH] == [1, 1, 1, 0, 1, 0, 0, 0, 0]                        # both columns; counted per row
    for T in (8, 16, 32, 64):                                               # image + 8 KiB of groups: unfor_aggregate_by_window's LDS tier
        assert shim.aggl_wave_lds(128 * T) == 128 * T + 8192


@pytest.mark.parametrize("T", [16, 32, 64])
def test_routes_on_a_seeded_sample(shim, T):
    """3 * 10^4 cases per type against the restatement in Python integers (aggregate_by_lookup_data.route_of, which the GPU tests use to
    say which routes their columns take): windows of 0, 1, 8192, 8193 and the largest number of slots, windows that wrap past 2^T - 1,
    references at both ends of the window and of the domain, widths 0 and T"""
    ty = f"u{T}"
    N = 1 << T
    top = min(N, 1 << 32)
    rng = random.Random(41400 + T)
    sizes = [b for b in (0, 1, 2, 45, 1024, 1025, 8192, 8193, 65535, 65536, top - 1, top) if b <= top]
    q, want = [], []
    counts = dict(SKIP=0, NOTHING=0, MISSING=0, ONE_GROUP=0, EACH=0, wraps=0)
    for i in range(30_000):
        slots = sizes[i % len(sizes)] if i % 3 else rng.randint(0, top)
        lo = [0, N - 1, N >> 1, (N - slots // 2) % N][i % 4] if i % 5 else rng.randrange(N)
        w = [0, T, 1, T - 1, 0][i % 11] if i % 11 < 5 else rng.randint(0, T)
        span = (1 << w) - 1
        kind = i % 7
        if kind == 0:
            ref = (lo + slots) % N                                          # the first key behind the window
        elif kind == 1:
            ref = (lo - span - 1) % N                                       # the block ends just in front of the window
        elif kind == 2:
            ref = (lo - span) % N                                           # ... or on its first key
        elif kind == 3:
            ref = (lo + max(slots, 1) - 1) % N                              # the window's last key
        elif kind == 4:
            ref = (lo + rng.randint(0, max(slots, 1) - 1)) % N              # inside
        else:
            ref = rng.randrange(N)
        empty, ok = i % 13 == 0, i % 17 != 0
        r = route_of(ty, lo, slots, ref, w, empty, ok)
        counts[("SKIP", "NOTHING", "MISSING", "ONE_GROUP", "EACH")[r]] += 1
        counts["wraps"] += lo + slots > N
        q.append((lo, slots, ref, w, empty, ok))
        want.append((r, (ref - lo) % N))
    assert all(v > 300 for v in counts.values()), counts
    route, c = routes(shim, T, *([x[j] for x in q] for j in range(6)))
    for i in range(len(q)):
        assert (int(route[i]), int(c[i])) == want[i], (T, q[i], want[i])


def test_cpp_mirror_declares_both_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the two new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint32_t;
using U = std::uint8_t;
void (*const uniform)(std::size_t, const T*, const T*, std::size_t, std::size_t, const T*, const T*, std::size_t, const std::uint32_t*, std::size_t, T,
                      std::uint64_t, const U*, const std::uint32_t*, fl_block_aggregate*, std::uint64_t*, std::uint32_t*, void*) =
    &fastlanes::FoR<T>::unfor_aggregate_by_lookup_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const std::uint8_t*, const std::uint64_t*,
                    const T*, std::size_t, const T*, std::size_t, const std::uint32_t*, std::size_t, T, std::uint64_t, const U*, const std::uint32_t*,
                    fl_block_aggregate*, std::uint64_t*, std::uint32_t*, void*) = &fastlanes::unfor_aggregate_by_lookup_widths_device<T>;
void (*const narrow)(std::size_t, const U*, const U*, std::size_t, std::size_t, const U*, const U*, std::size_t, const std::uint32_t*, std::size_t, U,
                     std::uint64_t, const U*, const std::uint32_t*, fl_block_aggregate*, std::uint64_t*, std::uint32_t*, void*) =
    &fastlanes::FoR<U>::unfor_aggregate_by_lookup_device;
int main() { return uniform && mixed && narrow ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
