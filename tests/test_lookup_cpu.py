"""CPU: unfor_lookup / unfor_lookup_widths and their uint8-payload twins (a dimension attribute fetched through a FoR-packed key column
inside a dense window: the probe side of a payload join) -- the header declares and the library exports the 16 symbols (7 (key,
payload) pairs in two forms each, and u8's pair under its _u8 name: every element type has one surface) through two macros of their
own, the Python table agrees with the header, every refusal needs no GPU, the numpy model of the definition (tests/lookup_data.py) is
what the definition says, and the block routes and the tier function the kernel and the host share
(fastlanes_amd/csrc/fl_lookup_map.hpp, compiled here with g++) are SOUND: over every (reference, width, key_lo, n_slots) of an 8-bit
domain against the per-element definition, and on seeded samples of the 16 / 32 / 64-bit types with windows that wrap past 2^T - 1."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from cpu_support import CT, ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)
from lookup_data import ENTRIES, PAIRS, entry, expected_lookup, pack_full_width, present_words, table_of

FORMS = ("unfor_lookup", "unfor_lookup_widths")
FORMS_U8 = ("unfor_lookup_u8", "unfor_lookup_u8_widths")
SKIP, MISSING, ONE_SLOT, EACH = 0, 1, 2, 3


def header_prototypes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from gen_rust_ffi import prototypes
    finally:
        sys.path.pop(0)
    return {name: (ret, args) for name, ret, args in prototypes()}


def test_header_declares_and_library_exports_the_sixteen_symbols(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_LOOKUP(T, S)")[1].split("FL_DECLARE_LOOKUP(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == sorted(FORMS)
    body8 = text.split("#define FL_DECLARE_LOOKUP_U8(T, S)")[1].split("FL_DECLARE_LOOKUP_U8(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body8)) == sorted(FORMS_U8)
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_LOOKUP({CT[ty]}, {ty})" in text
        assert f"FL_DECLARE_LOOKUP_U8({CT[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in FORMS + FORMS_U8]
    assert len(want) == 16 and sorted(fastlanes_amd.lookup_symbols()) == sorted(want)
    assert len(PAIRS) == 7 and sorted(want) == sorted({entry(t, u, w, twin) for t, u, twin in ENTRIES for w in (True, False)})
    for other in (fastlanes_amd.exported_symbols(), fastlanes_amd.for_compare_in_symbols(), fastlanes_amd.set_build_symbols(),
                  fastlanes_amd.aggregate_by_window_symbols(), fastlanes_amd.aggregate_by_symbols(), fastlanes_amd.select_symbols()):
        assert not set(want) & set(other)                                  # the pinned lists stay as they were
    for s in want:
        assert hasattr(lib, s), s
    assert {"lookup_symbols", "unfor_lookup_widths", "full_width_column"} <= set(fastlanes_amd.__all__)
    assert hasattr(fastlanes_amd.FoR, "unfor_lookup")
    doc = text.split("#define FL_DECLARE_LOOKUP(T, S)")[0].rsplit("/*", 1)[1]
    for words in ("Out of scope", "several tables per launch", "sparse or hashed keys", "Delta", "host tier", "2^31 bytes", "fused GROUP BY"):
        assert words in doc, words


def test_python_table_agrees_with_the_header_prototypes(lib):
    """every argument of the header's prototype, in order: a pointer is c_void_p, `unsigned` c_uint, size_t c_size_t, uint64_t c_uint64,
    the key type and the payload type their own scalars; the column's arguments are unfor_set_build's"""
    from fastlanes_amd import _lib
    protos = header_prototypes()
    rows = {name: (restype, argtypes) for name, restype, argtypes in _lib._rows("LOOKUP", "LOOKUP_U8")}
    assert len(rows) == 16
    for ty, uty, twin in ENTRIES:
        for widths in (False, True):
            name = entry(ty, uty, widths, twin)
            ret, args = protos[name]
            restype, argtypes = rows[name]
            assert ret == "int" and restype is ctypes.c_int
            sb_args = [a for _, a in protos[f"fl_{ty}_unfor_set_build{'_widths' if widths else ''}"][1]]
            head = sb_args[:sb_args.index("set_lo")]                        # the column, mask, n_blocks
            tail = ["err_flag", "stream"] if widths else ["stream"]
            assert [a for _, a in args] == head + ["key_lo", "n_slots", "table", "present", "missing", "out", "hit_mask", "stats"] + tail, name
            assert len(args) == len(argtypes), name
            types = dict((a, c) for c, a in args)
            assert types["key_lo"] == CT[ty] and types["n_slots"] == "uint64_t" and types["table"] == f"const {CT[uty]} *"
            assert types["missing"] == CT[uty] and types["out"] == f"{CT[uty]} *" and types["present"] == "const uint32_t *"
            assert types["hit_mask"] == "uint32_t *" and types["stats"] == "uint64_t *" and types["mask"] == "const uint32_t *"
            scalars = {"unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t, "int": ctypes.c_int, "uint64_t": ctypes.c_uint64}
            for (ctype, arg), at in zip(args, argtypes):
                if "*" in ctype:
                    want = ctypes.c_void_p
                elif arg == "key_lo":
                    want = _lib.CTYPE[ty]
                elif arg == "missing":
                    want = _lib.CTYPE[uty]
                else:
                    want = scalars[ctype]
                assert at is want, (name, arg, ctype)
            assert getattr(lib, name).argtypes == argtypes


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel), in unfor_set_build's order: the width; n_slots above
    min(2^T, 2^32) or a table of 2^31 bytes or more (FL_ERR_INDEX); the empty column; table, out and the column's pointers
    (FL_ERR_NULL); alignment of the packed column, mask, hit_mask, present, table, out and stats.  mask, present, hit_mask and stats
    may be NULL."""
    buf = np.zeros(8192, dtype=np.uint64)
    p = buf.ctypes.data
    assert p % 16 == 0
    A, AR, MK, TB, W, O, ST, PR, OUT, HM = (p + 4096 * i for i in range(10))
    for ty, uty, twin in ENTRIES:
        T, U = TYPE_BITS[ty], TYPE_BITS[uty]
        f, g = getattr(lib, entry(ty, uty, False, twin)), getattr(lib, entry(ty, uty, True, twin))
        top = min(1 << T, 1 << 32, ((1 << 31) - 1) // (U // 8))             # the largest table that is not refused

        def uni(w=3, a=A, ar=AR, mk=MK, n=1, lo=5, ns=40, tb=TB, pr=PR, out=OUT, hm=HM, st=ST):
            return f(w, a, ar, 1, mk, n, lo, ns, tb, pr, 0, out, hm, st, None)

        def mix(w=W, o=O, a=A, ab=384, ar=AR, mk=MK, n=1, lo=5, ns=40, tb=TB, pr=PR, out=OUT, hm=HM, st=ST):
            return g(w, o, a, ab, ar, 1, mk, n, lo, ns, tb, pr, 0, out, hm, st, None, None)

        # FL_ERR_WIDTH: also for an empty column and in front of every other refusal
        for n in (1, 0):
            assert uni(w=T + 1, n=n) == 1 and uni(w=T + 1, ns=top + 1, n=n) == 1 and uni(w=T + 1, tb=None, n=n) == 1
        assert uni(w=T, tb=None) == 3                                       # the widest width is not refused as a width
        # FL_ERR_INDEX: also for an empty column, and in front of the NULL checks
        for n in (1, 0):
            for ns in (top + 1, top + 32, 1 << 33, 2 ** 64 - 1):
                assert uni(ns=ns, n=n) == 2 and mix(ns=ns, n=n) == 2, (ty, uty, ns)
        assert uni(ns=top + 1, tb=None) == 2 and mix(ns=top + 1, a=None) == 2
        assert uni(ns=top, tb=None) == 3 and mix(ns=top, tb=None) == 3      # the largest table is not refused
        if T >= 32:                                                         # the byte bound, not the slot bound, is what binds
            assert (top + 1) * (U // 8) >= 1 << 31 and top * (U // 8) < 1 << 31
        # n_blocks == 0: nothing to do, whatever the pointers
        assert f(3, None, None, 0, None, 0, 5, 40, None, None, 0, None, None, None, None) == 0
        assert g(None, None, None, 0, None, 0, None, 0, 5, 40, None, None, 0, None, None, None, None, None) == 0
        # FL_ERR_NULL: each required pointer; table with n_slots > 0; out
        for name in ("a", "ar", "tb", "out"):
            assert uni(**{name: None}) == 3, (ty, uty, name)
        for name in ("w", "o", "a", "ar", "tb", "out"):
            assert mix(**{name: None}) == 3, (ty, uty, name)
        # FL_ERR_ALIGN: every pointer the kernel reads or writes 16 bytes at a time
        for name, at in (("a", A), ("mk", MK), ("hm", HM), ("pr", PR), ("tb", TB), ("out", OUT), ("st", ST)):
            for d in (4, 8):
                assert uni(**{name: at + d}) == 4 and mix(**{name: at + d}) == 4, (ty, uty, name, d)
        assert uni(a=None, tb=TB + 8) == 3 and uni(out=None, mk=MK + 8) == 3  # NULL is answered before alignment
        # mask, present, hit_mask and stats may be NULL: the call gets past them to the next refusal
        assert uni(mk=None, pr=None, hm=None, st=None, tb=TB + 8) == 4 and mix(mk=None, pr=None, hm=None, st=None, a=A + 8) == 4
        # the empty window: neither table nor present is read, so neither NULL nor a misaligned pointer is refused
        assert uni(ns=0, tb=None, a=None) == 3 and uni(ns=0, tb=None, mk=MK + 8) == 4 and uni(ns=0, tb=TB + 4, pr=PR + 4, mk=MK + 8) == 4
        assert mix(ns=0, tb=None, ar=None) == 3 and mix(ns=0, tb=TB + 4, st=ST + 8) == 4
        # the packed pointer may be NULL only when no byte of it can be read
        assert uni(w=0, a=None, mk=MK + 8) == 4 and mix(a=None, ab=0, mk=MK + 8) == 4
        assert mix(a=None) == 3 and uni(w=1, a=None) == 3


def test_python_mirror_validates_before_any_launch():
    import torch
    import fastlanes_amd as fl
    tw, to = torch.zeros(1, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64)
    tcol, tref = torch.zeros(96, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError):                                          # device tier only: numpy arrays and CPU tensors
        fl.FoR.unfor_lookup(3, np.zeros(96, dtype=np.uint32), 0, 0, np.zeros(4, np.uint8))
    with pytest.raises(TypeError):
        fl.FoR.unfor_lookup(3, tcol, 0, 0, torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        fl.unfor_lookup_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint32), np.zeros(1, np.uint32), 0, np.zeros(4, np.uint8))
    with pytest.raises(TypeError):
        fl.unfor_lookup_widths(tw, to, tcol, tref, 0, torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        fl.full_width_column("u7", 3, "cpu")
    w, o, r = fl.full_width_column("u32", 3, "cpu")
    assert w.tolist() == [32] * 3 and o.tolist() == [0, 4096, 8192] and r.tolist() == [0] and r.dtype == torch.uint32


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def test_model_is_the_definition(oracle):
    """the numpy model against a row-by-row restatement in Python integers; pack(u8, 8, v) == v; pack(T, T, v) is a permutation that
    unpack undoes and, for u16 / u32 / u64, is NOT the identity"""
    rng = np.random.default_rng(97000)
    for ty, uty in PAIRS:
        T, U = TYPE_BITS[ty], TYPE_BITS[uty]
        N = 1 << T
        lo, n_slots = N - 20, min(50, N)
        table = table_of(uty, n_slots, 97100 + T)
        pw = present_words(n_slots, 97200 + T, clear=(0, 7))
        keys = ((rng.integers(0, 80, size=2048).astype(np.uint64) + np.uint64(lo - 10)) & np.uint64(N - 1)).astype(f"u{T // 8}")
        keep = rng.random(2048) < 0.7
        for present in (None, pw):
            out, hit_words, stats, v, h = expected_lookup(oracle, ty, uty, keys, keep, lo, table, present, (1 << U) - 1)
            for i in range(2048):
                j = (int(keys[i]) - lo) % N
                hit = bool(keep[i]) and j < n_slots and (present is None or (int(pw[j >> 5]) >> (j & 31)) & 1 == 1)
                assert bool(h[i]) == hit and int(v[i]) == (int(table[j]) if hit else (1 << U) - 1), (ty, uty, i)
            assert stats.tolist() == [int(h.sum()), int((keep & ~h).sum())]
            assert np.array_equal(np.unpackbits(hit_words.view(np.uint8), bitorder="little").astype(bool), h)
            back = np.concatenate([oracle.unpack(uty, U, blk) for blk in out.reshape(-1, out.size // 2)])
            assert np.array_equal(back, v)
    v8 = rng.integers(0, 256, size=1024).astype(np.uint8)
    assert np.array_equal(oracle.pack("u8", 8, v8), v8) and np.array_equal(pack_full_width(oracle, "u8", v8), v8)
    for ty in ("u16", "u32", "u64"):
        v = np.arange(1024).astype(f"u{TYPE_BITS[ty] // 8}")
        p = oracle.pack(ty, TYPE_BITS[ty], v)
        assert sorted(p.tolist()) == v.tolist() and not np.array_equal(p, v)


# ---- the block routes and the tier -------------------------------------------------------------------------------------------------------
SHIM = r"""
#include "fl_lookup_map.hpp"
#include <stddef.h>
// the array form: query i = (key_lo, n_slots, reference, width, mask_empty, precondition_ok, kept) -> the block's route, c, and what a
// block decided without a gather adds to the misses
extern "C" void lookup_route_n(unsigned type_bits, size_t n, const uint64_t* key_lo, const uint64_t* n_slots, const uint64_t* ref,
                               const uint8_t* width, const uint8_t* mask_empty, const uint8_t* ok, const uint64_t* kept, int* route,
                               uint64_t* c_out, uint64_t* misses, uint8_t* reads_packed, uint8_t* reads_table, uint8_t* writes)
{
    for (size_t i = 0; i < n; ++i) {
        const fl::ForPredicate window = fl::set_window(type_bits, key_lo[i], n_slots[i]);
        const fl::LookupRoute r = fl::lookup_route(type_bits, window, mask_empty[i] != 0, ok[i] != 0, ref[i], width[i], c_out[i]);
        route[i] = r;
        misses[i] = fl::lookup_decided_misses(r, kept[i]);
        reads_packed[i] = fl::lookup_reads_packed(r);
        reads_table[i] = fl::lookup_reads_table(r);
        writes[i] = fl::lookup_writes_block(r);
    }
}
extern "C" uint64_t lookup_lds_bytes(void) { return fl::LOOKUP_LDS_BYTES; }
extern "C" int lookup_tier_of(uint64_t n_slots, unsigned payload_bytes) { return fl::lookup_tier(n_slots, payload_bytes); }
extern "C" int lookup_slots_refused_of(unsigned type_bits, uint64_t n_slots, unsigned payload_bytes) { return fl::lookup_slots_refused(type_bits, n_slots, payload_bytes); }
extern "C" unsigned lookup_wave_lds_of(unsigned block_bytes, unsigned type_bits, unsigned payload_bytes, int lds_tier) { return fl::lookup_wave_lds(block_bytes, type_bits, payload_bytes, lds_tier != 0); }
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = build_shim(tmp_path_factory, "lookup_map", SHIM)
    P = ctypes.c_void_p
    so.lookup_route_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 13
    so.lookup_route_n.restype = None
    so.lookup_lds_bytes.restype = ctypes.c_uint64
    so.lookup_tier_of.argtypes = [ctypes.c_uint64, ctypes.c_uint]
    so.lookup_slots_refused_of.argtypes = [ctypes.c_uint, ctypes.c_uint64, ctypes.c_uint]
    so.lookup_wave_lds_of.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_int]
    so.lookup_wave_lds_of.restype = ctypes.c_uint
    return so


def routes(shim, T, lo, slots, ref, width, empty, ok, kept):
    lo, slots, ref, kept = (np.array(x, dtype=np.uint64) for x in (lo, slots, ref, kept))
    width, empty, ok = (np.array(x, dtype=np.uint8) for x in (width, empty, ok))
    n = lo.size
    route, c, miss = np.empty(n, np.int32), np.empty(n, np.uint64), np.empty(n, np.uint64)
    rp, rt, wr = np.empty(n, np.uint8), np.empty(n, np.uint8), np.empty(n, np.uint8)
    shim.lookup_route_n(T, n, *(x.ctypes.data for x in (lo, slots, ref, width, empty, ok, kept, route, c, miss, rp, rt, wr)))
    return route, c, miss, rp, rt, wr


def test_tier_function_at_the_boundary(shim):
    """n_slots * sizeof(U) = 8192 is the LDS tier's last table, one slot more the memory tier's first, for each U; the LDS a wavefront
    asks for is unfor_set_build's; the refusals' bounds"""
    assert shim.lookup_lds_bytes() == 8192
    for payload in (1, 2, 4, 8):
        at = 8192 // payload
        assert [shim.lookup_tier_of(s, payload) for s in (0, 1, at - 1, at, at + 1, 1 << 20)] == [0, 0, 0, 0, 1, 1], payload
    # image + private table per wavefront: u8 1 KiB + 256 B, u16 2 + 8 KiB, u32 4 + 8 KiB, u64 8 + 8 KiB: unfor_set_build's (u8: 32 B there)
    for T in (16, 32, 64):
        for payload in (1, T // 8):
            assert shim.lookup_wave_lds_of(128 * T, T, payload, 1) == 128 * T + 8192 and shim.lookup_wave_lds_of(128 * T, T, payload, 0) == 128 * T
    assert shim.lookup_wave_lds_of(1024, 8, 1, 1) == 1024 + 256
    for T, payload in ((8, 1), (16, 2), (16, 1), (32, 4), (32, 1), (64, 8), (64, 1)):
        top = min(1 << T, 1 << 32, ((1 << 31) - 1) // payload)
        assert [shim.lookup_slots_refused_of(T, s, payload) for s in (0, 1, top, top + 1, 2 ** 64 - 1)] == [0, 0, 0, 1, 1], (T, payload)


def test_routes_agree_with_the_definition_over_the_8_bit_domain(shim):
    """every (key_lo, n_slots, reference, width) of u8, with an empty and a non-empty mask and a failed check, against the per-element
    definition over the keys the block CAN hold: a MISSING block holds no key inside the window (or keeps no row), a ONE_SLOT block
    holds exactly the key of slot c, and exactly the blocks that may hold keys on both sides of the window's edge -- or several
    inside it -- are decoded"""
    T, N = 8, 256
    q = []
    for lo in list(range(0, N, 7)) + [N - 1, N - 40]:
        for slots in (0, 1, 2, 31, 32, 33, 45, 128, 255, 256):
            for ref in range(N):
                for w in range(T + 1):
                    q.append((lo, slots, ref, w, 0, 1, 1024))
                q.append((lo, slots, ref, ref % (T + 1), 1, 1, 0))
                q.append((lo, slots, ref, ref % (T + 1), 0, 0, 7))
    route, c, miss, rp, rt, wr = routes(shim, T, *([x[j] for x in q] for j in range(7)))
    seen = set()
    for i, (lo, slots, ref, w, empty, ok, kept) in enumerate(q):
        window = {(lo + j) % N for j in range(slots)}
        vals = {(ref + f) % N for f in range(1 << w)}
        inside = {(v - lo) % N for v in vals if v in window}                # the slots the block can read
        r = int(route[i])
        what = (lo, slots, ref, w, empty, ok)
        assert int(c[i]) == (ref - lo) % N
        assert int(rp[i]) == (r == EACH) and int(rt[i]) == (r in (ONE_SLOT, EACH)) and int(wr[i]) == (r != SKIP)
        if not ok:
            assert r == SKIP and int(miss[i]) == 0, ("a failed check leaves the block alone", what)
        elif empty or not inside:
            assert r == MISSING and int(miss[i]) == kept, ("MISSING: nothing can hit", what)
        elif w == 0:
            assert r == ONE_SLOT and inside == {int(c[i])} and int(c[i]) < slots and int(miss[i]) == 0, ("ONE_SLOT: exactly slot c", what)
        else:
            assert r == EACH and int(miss[i]) == 0, ("left to the decode", what)
        seen.add((r, w == 0, slots == 0, slots == N, lo + slots > N))
    assert {r for r, *_ in seen} == {SKIP, MISSING, ONE_SLOT, EACH}
    assert any(r == EACH and wraps for r, _, _, _, wraps in seen) and any(r == ONE_SLOT and full for r, _, _, full, _ in seen)
    assert not any(r == EACH and z for r, z, *_ in seen) and not any(r in (ONE_SLOT, EACH) and e for r, _, e, _, _ in seen)


@pytest.mark.parametrize("T", [16, 32, 64])
def test_routes_on_a_seeded_sample(shim, T):
    """3 * 10^4 cases per type against a restatement in Python integers: the block's slots {(c + f) mod 2^T} meet the window
    [0, n_slots - 1] iff c lies inside it or c + 2^W - 1 passes 2^T; windows of 0, 1, the tier boundaries and the largest number of
    slots, windows that wrap past 2^T - 1, references at both ends of the window and of the domain, widths 0 and T"""
    N = 1 << T
    top = min(N, 1 << 32)
    rng = random.Random(97300 + T)
    sizes = [b for b in (0, 1, 2, 45, 1024, 1025, 8192, 8193, 65535, 65536, top - 1, top) if b <= top]
    q, want = [], []
    counts = dict(skip=0, missing=0, one_slot=0, each=0, wraps=0)
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
        kept = 0 if empty else rng.randint(1, 1024)
        c = (ref - lo) % N
        if not ok:
            r = SKIP
        elif empty or slots == 0 or not (c <= slots - 1 or c + span >= N):
            r = MISSING
        elif w == 0:
            r = ONE_SLOT
        else:
            r = EACH
        counts[("skip", "missing", "one_slot", "each")[r]] += 1
        counts["wraps"] += lo + slots > N
        q.append((lo, slots, ref, w, empty, ok, kept))
        want.append((r, c, kept if r == MISSING else 0))
    assert all(v > 300 for v in counts.values()), counts
    route, c, miss, rp, rt, wr = routes(shim, T, *([x[j] for x in q] for j in range(7)))
    for i in range(len(q)):
        assert (int(route[i]), int(c[i]), int(miss[i])) == want[i], (T, q[i], want[i])


def test_cpp_mirror_declares_all_forms(tmp_path):
    """a plain C++17 translation unit that includes fastlanes_amd.hpp and takes the addresses of the four new mirror functions"""
    src = tmp_path / "mirror.cpp"
    src.write_text(r"""
#include "fastlanes_amd.hpp"
using T = std::uint32_t;
using U = std::uint8_t;
void (*const uniform)(std::size_t, const T*, const T*, std::size_t, const std::uint32_t*, std::size_t, T, std::uint64_t, const T*,
                      const std::uint32_t*, T, T*, std::uint32_t*, std::uint64_t*, void*) = &fastlanes::FoR<T>::unfor_lookup_device;
void (*const uniform8)(std::size_t, const T*, const T*, std::size_t, const std::uint32_t*, std::size_t, T, std::uint64_t, const U*,
                       const std::uint32_t*, U, U*, std::uint32_t*, std::uint64_t*, void*) = &fastlanes::FoR<T>::unfor_lookup_u8_device;
void (*const mixed)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const std::uint32_t*, std::size_t,
                    T, std::uint64_t, const T*, const std::uint32_t*, T, T*, std::uint32_t*, std::uint64_t*, std::uint32_t*, void*) =
    &fastlanes::unfor_lookup_widths_device<T>;
void (*const mixed8)(const std::uint8_t*, const std::uint64_t*, const T*, std::size_t, const T*, std::size_t, const std::uint32_t*, std::size_t,
                     T, std::uint64_t, const U*, const std::uint32_t*, U, U*, std::uint32_t*, std::uint64_t*, std::uint32_t*, void*) =
    &fastlanes::unfor_lookup_u8_widths_device<T>;
void (*const narrow)(std::size_t, const U*, const U*, std::size_t, const std::uint32_t*, std::size_t, U, std::uint64_t, const U*,
                     const std::uint32_t*, U, U*, std::uint32_t*, std::uint64_t*, void*) = &fastlanes::FoR<U>::unfor_lookup_device;
int main() { return uniform && uniform8 && mixed && mixed8 && narrow ? 0 : 1; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(tmp_path / "mirror.o")])
