"""GPU: the accepting side of the header's alignment promise -- "device pointers 16-byte aligned; 128 is only recommended", and a
mixed-width column's offsets[b] any multiple of 16 -- at every device-tier entry point: what an engine that sub-allocates its chunks
from a slab relies on.  Every buffer of every call here lies at a chosen residue mod 128 (gpu_support.placed: one raw allocation of
seeded random bytes, the payload >= 256 bytes in, >= 256 guard bytes behind it), every result is compared with the CPU oracle's
(oracle.batch / the per-block calls, numpy over them for masks and aggregates) bit for bit, and after every call every byte outside
every payload of that call -- inputs included -- must be what it was.  tests/test_support_cpu.py pins, without a GPU, that the columns
used here start blocks on all eight residues and that a decode from an address rounded to 128 bytes gives other values: a kernel that
rounds a base, sizes a descriptor or steps its reads by a 128-byte rule of its own fails here.

Entry points of include/fastlanes_amd.h that take a device data pointer, and the test that calls each with every such pointer off a
128-byte boundary (checked against the header by eye):
  test_uniform_width_families      fl_<ty>_pack, _unpack, _for_pack, _unfor_pack, _delta, _undelta, _undelta_pack,
                                   _undelta_pack_untranspose, _transpose_delta_pack, _transpose, _untranspose, _unpack_block_sums,
                                   _block_min_max, _unpack_compare
  test_mixed_width_columns         fl_<ty>_unpack_widths, _pack_widths, _unfor_pack_widths, _for_pack_widths, _undelta_pack_widths,
                                   _undelta_pack_untranspose_widths, _transpose_delta_pack_widths, _unpack_single_widths,
                                   _unpack_mixed, _pack_mixed
  test_for_consumers               fl_<ty>_unfor_compare, _unfor_compare_widths, _unfor_compare_range, _unfor_compare_range_widths,
                                   _unfor_select, _unfor_select_widths, _unfor_aggregate, _unfor_aggregate_widths, fl_mask_offsets,
                                   fl_aggregate_reduce
  test_batch_from_one_slab         fl_<ty>_unpack_batch, _pack_batch, _unfor_pack_batch, _for_pack_batch, _undelta_pack_batch (both
                                   orders), _transpose_delta_pack_batch
  test_unpack_single_two_forms     fl_<ty>_unpack_single, _unpack_single_widths
  test_encoder_metadata_steps      fl_<ty>_for_widths, fl_widths_to_offsets
Left out on purpose: fl_column_pair_alloc / fl_column_pair_free (they hand out memory, they take none), fl_fill_random (its own,
8-byte, rule is refused and accepted in test_cabi.py), fl_internal_* (measurement hooks, not part of the interface), the host tier
(host pointers of any alignment; the library stages them), fl_mixed_plan_create (a host array in, the plan's own device arrays).
Single words the Python mirror allocates itself -- its err_flag, mask_offsets' total inside a select call, the scalar a broadcast
reference is uploaded as -- stay where torch puts them; wherever a test calls the C ABI directly, those are placed too."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import gpu_support as gs
import test_gpu_aggregate as agg
import test_gpu_for_compare_range as rng_
import test_gpu_select as sel
from datagen import values
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import GUARD, POLICIES, SENTINEL, TYS, expected_blocks, placed, sentinel_of, want_mask
from oracle_lib import TYPES, lanes, load_oracle, packed_len, tbits
from test_gpu_for_consumer_shapes import SHAPES, column_masks

pytestmark = pytest.mark.gpu

N_UNIFORM = gs.UNIFORM_BLOCKS


# ---- expected values: once per (type, width) / (type, column), shared by every policy and residue ----
@functools.lru_cache(maxsize=None)
def plain_case(ty):
    """the unpacked side of the uniform-width tests: full-entropy values, references, bases, and what has no width"""
    o, n, L = load_oracle(), N_UNIFORM, lanes(ty)
    T = tbits(ty)
    c = dict(vals=values(ty, n * 1024, 35000 + T), refs=values(ty, n, 35100 + T), bases=values(ty, n * L, 35200 + T))
    c["delta"] = o.batch("delta", ty, None, c["vals"], aux=c["bases"])
    c["undelta"] = o.batch("undelta", ty, None, c["vals"], aux=c["bases"])
    c["transpose"] = o.batch("transpose", ty, None, c["vals"])
    c["untranspose"] = o.batch("untranspose", ty, None, c["vals"])
    c["transpose_delta"] = o.batch("delta", ty, None, c["transpose"], aux=c["bases"])
    c["mins"], c["maxs"] = c["vals"].reshape(n, 1024).min(axis=1), c["vals"].reshape(n, 1024).max(axis=1)
    return c


@functools.lru_cache(maxsize=None)
def uniform_case(ty, w):
    o, n, p = load_oracle(), N_UNIFORM, plain_case(ty)
    pk = gs.uniform_packed(ty, w)
    one = np.full(n, p["refs"][0], dtype=TYPES[ty][0])
    c = dict(pk=pk, unpack=o.batch("unpack", ty, w, pk, n_blocks=n), pack=o.batch("pack", ty, w, p["vals"]))
    c["for_pack 1"], c["for_pack n"] = o.batch("for_pack", ty, w, p["vals"], aux=one), o.batch("for_pack", ty, w, p["vals"], aux=p["refs"])
    c["unfor_pack 1"] = o.batch("unfor_pack", ty, w, pk, aux=one, n_blocks=n)
    c["unfor_pack n"] = o.batch("unfor_pack", ty, w, pk, aux=p["refs"], n_blocks=n)
    c["undelta_pack"] = o.batch("undelta_pack", ty, w, pk, aux=p["bases"], n_blocks=n)
    c["undelta_pack_untranspose"] = o.batch("untranspose", ty, None, c["undelta_pack"])
    c["transpose_delta_pack"] = o.batch("pack", ty, w, p["transpose_delta"])
    c["sums"] = c["unpack"].reshape(n, 1024).astype(np.uint64).sum(axis=1, dtype=np.uint64)
    return c


@functools.lru_cache(maxsize=None)
def column_case(ty, n):
    """the padded mixed-width column of n blocks (gpu_support.aligned_column_host) and the oracle's results, block by block"""
    o, L, T = load_oracle(), lanes(ty), tbits(ty)
    widths, off, col, blocks, gaps = gs.aligned_column_host(ty, n)
    c = dict(widths=widths, off=off, col=col, blocks=blocks, gaps=gaps, sizes=widths.astype(np.int64) * 128)
    c["refs"], c["bases"], c["vals"] = values(ty, n, 36000 + 64 * T + n), values(ty, n * L, 36100 + 64 * T + n), values(ty, n * 1024, 36200 + 64 * T + n)
    base = lambda b: c["bases"][b * L:(b + 1) * L]
    block = lambda b: c["vals"][b * 1024:(b + 1) * 1024]
    c["unpack"] = np.concatenate([o.unpack(ty, w, pk) for w, pk in blocks])
    c["unfor_pack"] = np.concatenate([o.unfor_pack(ty, w, pk, c["refs"][b]) for b, (w, pk) in enumerate(blocks)])
    c["undelta_pack"] = np.concatenate([o.undelta_pack(ty, w, pk, base(b)) for b, (w, pk) in enumerate(blocks)])
    c["undelta_pack_untranspose"] = o.batch("untranspose", ty, None, c["undelta_pack"])
    c["pack"] = [o.pack(ty, w, block(b)) for b, (w, _) in enumerate(blocks)]
    c["for_pack"] = [o.for_pack(ty, w, block(b), c["refs"][b]) for b, (w, _) in enumerate(blocks)]
    c["transpose_delta_pack"] = [o.pack(ty, w, o.delta(ty, o.transpose(ty, block(b)), base(b))) for b, (w, _) in enumerate(blocks)]
    return c


# ---- the calls' plumbing ----
def seeds_from(start):
    counter = itertools.count(start, 2)                                          # placed() draws a payload from seed + 1
    return lambda: next(counter)


def same(p, want, what):
    """the placed buffer's payload, as it is now, holds `want`'s bytes"""
    got = p.np()
    want = np.ascontiguousarray(want)
    assert got.nbytes == want.nbytes and np.array_equal(got.view(np.uint8), want.reshape(-1).view(np.uint8)), what


def guards(what, *bufs):
    for i, p in enumerate(bufs):
        p.check_guards((what, "buffer", i))


def cabi(fl, name, *args):
    """a device-tier C call on the current stream; the status must be FL_OK"""
    import torch
    rc = getattr(fl.load(), name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc, fl.load().fl_last_hip_error())


def zero_flag(seed):
    return placed(np.zeros(1, np.int32), "int32", 32, seed)


def flag_clear(flag, what):
    assert int(flag.t.item()) == 0, (what, "err_flag", int(flag.t.item()))


def out_of(ty, n_elems, residue, seed):
    return placed(n_elems * (tbits(ty) // 8), ty, residue, seed)


# ---- a. the uniform-width families ----
@pytest.mark.parametrize("policy", [0, 1, 2])
@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_families(fl, kernel_policy, ty, policy):
    """35 blocks (two full workgroups at 4 blocks per wavefront and a tail of 3) at the widths on both sides of the 2 * W >= T switch
    of the read route and at the ends; input at 16k, output at 16(8 - k), Delta's bases at 16((k + 2) % 7 + 1) for k = 1 .. 7;
    per-block references, mins / maxs at sizeof(T), block sums at 8."""
    kernel_policy(policy)
    T, n, esz = tbits(ty), N_UNIFORM, tbits(ty) // 8
    p = plain_case(ty)
    seed = seeds_from(40000 + 1000 * T)
    ops = list(gs.CMP)
    for wi, w in enumerate(gs.uniform_widths(ty)):
        c = uniform_case(ty, w)
        pl = packed_len(ty, w)
        op, k_cmp = ops[wi % len(ops)], int(c["unpack"][517])
        mask_want = want_mask(c["unpack"], op, k_cmp)
        for k in range(1, 8):
            rin, rout, raux = 16 * k, 16 * (8 - k), 16 * ((k + 2) % 7 + 1)
            what = (ty, policy, w, k)
            d_pk = placed(c["pk"], ty, rin, gs.packed_seed(ty, w, rin))
            d_vals = placed(p["vals"], ty, rin, seed())
            d_bases = placed(p["bases"], ty, raux, seed())
            d_refs, d_ref1 = placed(p["refs"], ty, esz, seed()), placed(p["refs"][:1], ty, esz, seed())
            assert d_pk.nbytes == 0 or d_pk.t.data_ptr() % 128 == rin
            assert d_vals.t.data_ptr() % 128 == rin and d_bases.t.data_ptr() % 128 == raux and d_refs.t.data_ptr() % 128 == esz

            def run(name, call, src, aux, n_out, *more):
                o = out_of(ty, n_out, rout, seed())
                assert o.nbytes == 0 or o.t.data_ptr() % 128 == rout
                got = call(o.t)
                assert got.data_ptr() == o.t.data_ptr() or o.nbytes == 0
                same(o, c[name] if name in c else p[name], what + (name,))
                guards(what + (name,), o, src, *([aux] if aux is not None else []), *more)

            run("pack", lambda o: fl.BitPacking.pack(w, d_vals.t, output=o), d_vals, None, n * pl)
            run("unpack", lambda o: fl.BitPacking.unpack(w, d_pk.t, output=o, n_blocks=n), d_pk, None, n * 1024)
            for tag, r in (("1", d_ref1), ("n", d_refs)):
                run("for_pack " + tag, lambda o: fl.FoR.for_pack(w, d_vals.t, r.t, output=o), d_vals, r, n * pl)
                run("unfor_pack " + tag, lambda o: fl.FoR.unfor_pack(w, d_pk.t, r.t, output=o, n_blocks=n), d_pk, r, n * 1024)
            run("undelta_pack", lambda o: fl.Delta.undelta_pack(w, d_pk.t, d_bases.t, output=o), d_pk, d_bases, n * 1024)
            run("undelta_pack_untranspose", lambda o: fl.Delta.undelta_pack_untranspose(w, d_pk.t, d_bases.t, output=o), d_pk, d_bases, n * 1024)
            run("transpose_delta_pack", lambda o: fl.Delta.transpose_delta_pack(w, d_vals.t, d_bases.t, output=o), d_vals, d_bases, n * pl)

            sums = placed(n * 8, "int64", 8, seed())
            fl.BitPacking.unpack_block_sums(w, d_pk.t, n_blocks=n, output=sums.t)
            same(sums, c["sums"], what + ("unpack_block_sums",))
            mask = placed(n * 128, "int32", rin, seed())
            fl.BitPacking.unpack_compare(w, d_pk.t, op, k_cmp, n_blocks=n, output=mask.t)
            same(mask, mask_want, what + ("unpack_compare", op))
            guards(what + ("sums, compare",), sums, mask, d_pk)

            if wi == 0:                                                         # the calls without a width: once per residue set
                run("delta", lambda o: fl.Delta.delta(d_vals.t, d_bases.t, output=o), d_vals, d_bases, n * 1024)
                run("undelta", lambda o: fl.Delta.undelta(d_vals.t, d_bases.t, output=o), d_vals, d_bases, n * 1024)
                run("transpose", lambda o: fl.Transpose.transpose(d_vals.t, output=o), d_vals, None, n * 1024)
                run("untranspose", lambda o: fl.Transpose.untranspose(d_vals.t, output=o), d_vals, None, n * 1024)
                mins, maxs = out_of(ty, n, esz, seed()), out_of(ty, n, esz, seed())
                fl.BitPacking.block_min_max(d_vals.t, output=(mins.t, maxs.t))
                same(mins, p["mins"], what + ("mins",))
                same(maxs, p["maxs"], what + ("maxs",))
                guards(what + ("block_min_max",), mins, maxs, d_vals)


# ---- b. mixed-width columns whose blocks start on every 16-byte residue ----
def column_image(out, c, blocks_want):
    """what the packed column `out` (a placed buffer the size of c's column) must hold after an encoder: its own bytes in the gaps,
    the oracle's block at every offset"""
    want = out.before()
    assert want.size == c["gaps"].size
    for o, s, pk in zip(c["off"].tolist(), c["sizes"].tolist(), blocks_want):
        assert pk.nbytes == s
        want[o:o + s] = pk.view(np.uint8)
    assert np.array_equal(want[c["gaps"]], out.before()[c["gaps"]])
    return want


def lookups(fl, ty, name, lead, idx, out, flag, what):
    cabi(fl, f"fl_{ty}_{name}", *lead, idx.t.data_ptr(), idx.t.numel(), out.t.data_ptr(), flag.t.data_ptr())
    flag_clear(flag, what)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_columns(fl, kernel_policy, ty, policy):
    """n = 2 * 4 * bpw + bpw + 1 blocks of the policy's blocks per wavefront, widths 0 .. T and random ones, 0 .. 112 bytes between
    neighbours; the column's base at 16 and at 80 mod 128: under either, blocks that hold bytes start on all eight residues."""
    kernel_policy(policy)
    n = gs.aligned_column_blocks(gs.policy_bpw(policy))
    assert n in gs.ALIGNED_COLUMN_BLOCKS
    T, esz, L = tbits(ty), tbits(ty) // 8, lanes(ty)
    c = column_case(ty, n)
    seed = seeds_from(50000 + 1000 * T + 10 * n)
    rs = np.random.default_rng(50000 + T + n)
    # every element of three blocks -- the widest, a middle one, the last -- and 257 seeded elements
    three = [int(np.argmax(c["widths"] == T)), n // 2, n - 1]
    index = np.concatenate([b * 1024 + np.arange(1024) for b in three] + [rs.integers(0, n * 1024, size=257)]).astype(np.int64)
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        rout, rbases = 16 * (8 - k), 16 * ((k + 2) % 7 + 1)
        what = (ty, policy, n, base)
        d_col = placed(c["col"], ty, base, gs.column_seed(ty, n, base))
        d_w, d_off = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", rout, seed())
        d_refs, d_bases, d_vals = placed(c["refs"], ty, esz, seed()), placed(c["bases"], ty, rbases, seed()), placed(c["vals"], ty, 16 * (k + 2), seed())
        meta = (d_w, d_off)
        assert d_col.t.data_ptr() % 128 == base and ((d_col.t.data_ptr() + c["off"]) % 128 != 0)[c["widths"] > 0].sum() >= n // 2

        def decode(name, call, *ins):
            o = out_of(ty, n * 1024, rout, seed())
            call(o.t)
            same(o, c[name], what + (name,))
            guards(what + (name,), o, d_col, *meta, *ins)

        def encode(name, call, *ins):
            o = placed(c["col"].nbytes, ty, base, seed())
            call(o.t)
            same(o, column_image(o, c, c[name]), what + (name,))                # blocks, and the gaps' bytes as they were
            guards(what + (name,), o, d_vals, *meta, *ins)

        decode("unpack", lambda o: fl.unpack_widths(d_w.t, d_off.t, d_col.t, output=o))
        encode("pack", lambda o: fl.pack_widths(d_w.t, d_off.t, d_vals.t, o))
        decode("unfor_pack", lambda o: fl.unfor_pack_widths(d_w.t, d_off.t, d_col.t, d_refs.t, output=o), d_refs)
        encode("for_pack", lambda o: fl.for_pack_widths(d_w.t, d_off.t, d_vals.t, d_refs.t, o), d_refs)
        decode("undelta_pack", lambda o: fl.undelta_pack_widths(d_w.t, d_off.t, d_col.t, d_bases.t, output=o), d_bases)
        decode("undelta_pack_untranspose", lambda o: fl.undelta_pack_widths(d_w.t, d_off.t, d_col.t, d_bases.t, output=o, untranspose=True), d_bases)
        encode("transpose_delta_pack", lambda o: fl.transpose_delta_pack_widths(d_w.t, d_off.t, d_vals.t, d_bases.t, o), d_bases)

        d_idx, got, flag = placed(index, "int64", rbases, seed()), out_of(ty, index.size, rout, seed()), zero_flag(seed())
        lead = (d_w.t.data_ptr(), d_off.t.data_ptr(), d_col.t.data_ptr(), d_col.nbytes, n)
        lookups(fl, ty, "unpack_single_widths", lead, d_idx, got, flag, what)
        same(got, c["unpack"][index], what + ("unpack_single_widths",))
        guards(what + ("unpack_single_widths",), got, d_idx, flag, d_col, *meta)

    # MixedWidthPlan lays its blocks back to back: the same blocks, without the gaps, in a buffer at 48 mod 128
    plan = fl.MixedWidthPlan(ty, c["widths"])
    try:
        d_pk = placed(np.concatenate([pk for _, pk in c["blocks"]]), ty, 48, seed())
        assert plan.packed_bytes == d_pk.nbytes and d_pk.t.data_ptr() % 128 == 48
        o = out_of(ty, n * 1024, 112, seed())
        plan.unpack(d_pk.t, output=o.t)
        same(o, c["unpack"], (ty, policy, "plan.unpack"))
        guards((ty, policy, "plan.unpack"), o, d_pk)
        d_vals, o = placed(c["vals"], ty, 112, seed()), placed(d_pk.nbytes, ty, 48, seed())
        plan.pack(d_vals.t, output=o.t)
        same(o, np.concatenate(c["pack"]), (ty, policy, "plan.pack"))
        guards((ty, policy, "plan.pack"), o, d_vals)
    finally:
        plan.close()


# ---- c. the four FoR consumers on the same padded columns ----
@pytest.mark.parametrize("policy,bpw", SHAPES)
@pytest.mark.parametrize("ty", TYS)
def test_for_consumers(fl, kernel_policy, ty, policy, bpw):
    """compare, the interval predicate (new / and / or out of place, and in place), the mask prefix sum, select and aggregate with
    its reduction: over the padded mixed-width column at both bases, and over a uniform column at W = T//2 + 1 placed the same way;
    masks at residues of their own (mask_in and mask never the same one), the select output at 16k, the slots at 16 (= 16 mod 32)."""
    kernel_policy(policy)
    assert bpw == gs.policy_bpw(policy)
    n = gs.aligned_column_blocks(bpw)
    assert n in gs.ALIGNED_COLUMN_BLOCKS
    T, esz = tbits(ty), tbits(ty) // 8
    N = 1 << T
    c = column_case(ty, n)
    seed = seeds_from(60000 + 1000 * T + 10 * n)
    wu = T // 2 + 1
    pku = gs.uniform_packed(ty, wu, n)
    valsu = load_oracle().batch("unfor_pack", ty, wu, pku, aux=c["refs"], n_blocks=n)
    bits, words = column_masks(n, 60300 + n)
    kept = int(bits.sum())
    pop = bits.reshape(n, 1024).sum(axis=1).astype(np.int64)
    lo, hi = int(c["refs"][n // 2]), (int(c["refs"][n // 2]) + (N >> 2)) % N
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        d_col, d_pku = placed(c["col"], ty, base, gs.column_seed(ty, n, base)), placed(pku, ty, base, gs.packed_seed(ty, wu, base))
        d_w, d_off = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", 16 * (8 - k), seed())
        d_refs = placed(c["refs"], ty, esz, seed())
        d_m = placed(words, "int32", 16, seed())
        assert d_col.t.data_ptr() % 128 == base == d_pku.t.data_ptr() % 128 and d_m.t.data_ptr() % 128 == 16
        forms = (("mixed", c["unfor_pack"], (d_col, d_w, d_off, d_refs)), ("uniform", valsu, (d_pku, d_refs)))
        for form, vals, ins in forms:
            what = (ty, policy, n, base, form)
            mixed = form == "mixed"
            head = (d_w.t, d_off.t, d_col.t, d_refs.t) if mixed else (wu, d_pku.t, d_refs.t)

            # unfor_compare
            m = placed(n * 128, "int32", 16 * (k + 2), seed())
            if mixed:
                fl.unfor_compare_widths(*head, "<=", lo, output=m.t)
            else:
                fl.FoR.unfor_compare(*head, "<=", lo, n_blocks=n, output=m.t)
            same(m, want_mask(vals, "<=", lo), what + ("compare",))
            guards(what + ("compare",), m, *ins)

            # unfor_compare_range: new / and / or out of place (mask_in at 16, mask at another residue), and in place
            call = fl.unfor_compare_range_widths if mixed else functools.partial(fl.FoR.unfor_compare_range, n_blocks=n)
            for j, cb in enumerate(rng_.COMBINE):
                m = placed(n * 128, "int32", {1: (64, 80, 96), 5: (32, 48, 112)}[k][j], seed())
                assert m.t.data_ptr() % 128 not in (0, 16)
                call(*head, lo, hi, output=m.t, **(dict(mask=d_m.t, combine=cb) if cb != "new" else {}))
                same(m, rng_.want_mask(vals, lo, hi, cb, words), what + ("range", cb))
                guards(what + ("range", cb), m, d_m, *ins)
            m = placed(words, "int32", 16 * (8 - k), seed())
            call(*head, lo, hi, mask=m.t, combine="and", output=m.t)
            same(m, rng_.want_mask(vals, lo, hi, "and", words), what + ("range", "and in place"))
            guards(what + ("range", "and in place"), m, *ins)

            # the mask prefix sum, then unfor_select into a buffer at 16k
            oo, total = placed(n * 8, "int64", 48, seed()), placed(8, "int64", 80, seed())
            cabi(fl, "fl_mask_offsets", d_m.t.data_ptr(), n, oo.t.data_ptr(), total.t.data_ptr())
            same(oo, np.cumsum(pop) - pop, what + ("mask_offsets",))
            same(total, np.array([kept], dtype=np.int64), what + ("mask_offsets total",))
            guards(what + ("mask_offsets",), oo, total, d_m)
            buf = placed(np.full(kept + GUARD, sentinel_of(ty), dtype=TYPES[ty][0]), ty, 16 * k, seed())
            if mixed:
                fl.unfor_select_widths(*head, d_m.t, out_offsets=oo.t, total=total.t, output=buf.t)
            else:
                fl.FoR.unfor_select(*head, d_m.t, out_offsets=oo.t, total=total.t, n_blocks=n, output=buf.t)
            sel.check_select(ty, buf.t, total.t, vals, bits, what + ("select",))
            guards(what + ("select",), buf, oo, total, d_m, *ins)

            # unfor_aggregate into slots at 16 mod 32, and the reduction of those slots into a result at 16k
            want = expected_blocks(vals, bits)
            slots = placed(np.full((n + GUARD) * 4, SENTINEL, dtype=np.uint64), "int64", 16, seed())
            if mixed:
                result, _ = fl.unfor_aggregate_widths(*head, d_m.t, block_aggs=slots.t[:n * 4])
            else:
                result, _ = fl.FoR.unfor_aggregate(*head, d_m.t, n_blocks=n, block_aggs=slots.t[:n * 4])
            agg.check_slots(slots.t, n, result, want, what + ("aggregate",))
            res = placed(32, "int64", 16 * k, seed())
            cabi(fl, "fl_aggregate_reduce", slots.t.data_ptr(), n, res.t.data_ptr())
            same(res, gs.combine(want), what + ("aggregate_reduce",))
            guards(what + ("aggregate",), slots, res, d_m, *ins)


# ---- d. a batch sub-allocated from one slab ----
COUNTS = [5, 1, 0, 9, 33, 2, 64, 3, 17, 1, 8, 4, 12, 6]


class Slab:
    """arrays laid out by gpu_support.slab_layout inside one placed buffer of random filler"""

    def __init__(self, ty, sizes, arrays, residue, seed):
        self.ty, self.esz = ty, tbits(ty) // 8
        self.sizes = [int(s) for s in sizes]
        self.starts, total = gs.slab_layout(self.sizes)
        image = np.random.default_rng(seed + 1).integers(0, 256, size=total, dtype=np.uint8)
        for s, a in zip(self.starts, arrays if arrays is not None else []):
            image[s:s + a.nbytes] = np.ascontiguousarray(a).view(np.uint8)
        self.p = placed(image, ty, residue, seed)
        self.tensors = [self.p.t[s // self.esz:(s + z) // self.esz] for s, z in zip(self.starts, self.sizes)]

    def holds(self, arrays, what):
        """every array is `arrays`' (None: whatever it was), and the filler between and around them is what it was"""
        want = self.p.before()
        for a, (s, arr) in enumerate(zip(self.starts, arrays)):
            if arr is not None:
                assert arr.nbytes == self.sizes[a], (what, a)
                want[s:s + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8)
        got = self.p.np().view(np.uint8)
        for a, (s, z) in enumerate(zip(self.starts, self.sizes)):
            assert np.array_equal(got[s:s + z], want[s:s + z]), (what, "array", a)
        assert np.array_equal(got, want), (what, "the filler between two arrays was written")
        self.p.check_guards(what)


def off_boundary(batch, seed):
    """the batch's own device arrays -- pointers, widths, block counts, references -- moved off the 128-byte boundary as well"""
    keep = []
    for name, dt, residue in (("d_packed", "int64", 16), ("d_unpacked", "int64", 48), ("d_widths", "uint8", 80), ("d_n_blocks", "int32", 112),
                              ("d_refs", "uint8", 32), ("d_bases", "int64", 96)):
        t = getattr(batch, name)
        if t is not None:
            p = placed(t.cpu().numpy(), dt, residue, seed())
            setattr(batch, name, p.t)
            keep.append(p)
    return keep


@pytest.mark.parametrize("ty", TYS)
def test_batch_from_one_slab(fl, ty):
    """14 arrays -- 0 .. 64 blocks, widths with 0 and T -- cut from one slab each for the packed side, the unpacked side and the bases:
    array a starts 16 * (a % 8) bytes behind its neighbour's end, so every residue occurs and a write past an array lands in the next
    one or in the filler between them, both of which are compared."""
    o = load_oracle()
    T, esz, L = tbits(ty), tbits(ty) // 8, lanes(ty)
    rs = np.random.default_rng(70000 + T)
    widths = [int(x) for x in rs.integers(0, T + 1, size=len(COUNTS))]
    widths[0], widths[3], widths[4], widths[6] = T, 0, T // 2, T // 2 - 1
    refs = [int(x) for x in values(ty, len(COUNTS), 70100 + T)]
    seed = seeds_from(70200 + 1000 * T)
    pk_np = [values(ty, n * packed_len(ty, w), 70300 + a) for a, (n, w) in enumerate(zip(COUNTS, widths))]
    vals_np = [values(ty, n * 1024, 70400 + a) for a, n in enumerate(COUNTS)]
    bases_np = [values(ty, n * L, 70500 + a) for a, n in enumerate(COUNTS)]
    psz, usz, bsz = [p.nbytes for p in pk_np], [v.nbytes for v in vals_np], [b.nbytes for b in bases_np]
    each = lambda f: [f(a, n, w) for a, (n, w) in enumerate(zip(COUNTS, widths))]
    ref_of = lambda a, n: np.full(n, refs[a], dtype=TYPES[ty][0])

    s_pk, s_vals, s_bases = Slab(ty, psz, pk_np, 16, seed()), Slab(ty, usz, vals_np, 48, seed()), Slab(ty, bsz, bases_np, 80, seed())
    for slab in (s_pk, s_vals, s_bases):
        held = [t for t in slab.tensors if t.numel()]
        assert all(t.data_ptr() % 16 == 0 for t in held) and sum(t.data_ptr() % 128 != 0 for t in held) >= len(held) - 2
    assert {s % 128 for s in s_vals.starts} == set(range(0, 128, 16))
    ins = (s_pk, s_vals, s_bases)

    def run(name, want, packed_side, unpacked_side, method, kw, call_kw, outs):
        batch = fl.Batch(packed_side.tensors, unpacked_side.tensors, widths, **kw)
        keep = off_boundary(batch, seed)
        getattr(batch, method)(check=True, **call_kw)
        outs.holds(want, (ty, name))
        for slab in ins:
            slab.holds([None] * len(COUNTS), (ty, name, "an input changed"))
        guards((ty, name, "the batch's own arrays"), *keep)

    decoded = lambda: Slab(ty, usz, None, 112, seed())
    encoded = lambda: Slab(ty, psz, None, 32, seed())
    out = decoded()
    run("unpack", each(lambda a, n, w: o.batch("unpack", ty, w, pk_np[a], n_blocks=n)), s_pk, out, "unpack", {}, {}, out)
    out = encoded()
    run("pack", each(lambda a, n, w: o.batch("pack", ty, w, vals_np[a])), out, s_vals, "pack", {}, {}, out)
    out = decoded()
    run("unfor_pack", each(lambda a, n, w: o.batch("unfor_pack", ty, w, pk_np[a], aux=ref_of(a, n), n_blocks=n)), s_pk, out, "unpack",
        dict(references=refs), {}, out)
    out = encoded()
    run("for_pack", each(lambda a, n, w: o.batch("for_pack", ty, w, vals_np[a], aux=ref_of(a, n))), out, s_vals, "pack", dict(references=refs), {}, out)
    undelta = each(lambda a, n, w: o.batch("undelta_pack", ty, w, pk_np[a], aux=bases_np[a], n_blocks=n))
    out = decoded()
    run("undelta_pack", undelta, s_pk, out, "undelta_pack", dict(bases=s_bases.tensors), dict(untranspose=False), out)
    out = decoded()
    run("undelta_pack, untranspose", [o.batch("untranspose", ty, None, u) for u in undelta], s_pk, out, "undelta_pack", dict(bases=s_bases.tensors),
        dict(untranspose=True), out)
    out = encoded()
    run("transpose_delta_pack", each(lambda a, n, w: o.batch("pack", ty, w, o.batch("delta", ty, None, o.batch("transpose", ty, None, vals_np[a]),
                                                                                   aux=bases_np[a]))),
        out, s_vals, "transpose_delta_pack", dict(bases=s_bases.tensors), {}, out)


# ---- e. unpack_single's two forms ----
LOOKUP_COUNTS = [1, 3, 4, 5, 1025]


@pytest.mark.parametrize("ty", TYS)
def test_unpack_single_two_forms(fl, ty):
    """The launcher takes four lookups per thread where the indices are 16-byte aligned and the result is aligned to its four-element
    store, and one per thread otherwise (and for a tail of up to three).  Indices at 8 mod 16 (one per thread for the whole vector,
    also with every index of one block); indices aligned and the result at sizeof(T) mod 128; both aligned (the vector form); the
    packed column at 16 mod 128 throughout.  Uniform widths 1, T//2 + 1, T and a padded mixed-width column of those widths."""
    o = load_oracle()
    T, esz = tbits(ty), tbits(ty) // 8
    seed = seeds_from(80000 + 1000 * T)
    rs = np.random.default_rng(80000 + T)
    places = (("indices at 8", 8, 16 * 5), ("result at sizeof(T)", 48, esz), ("both aligned", 48, 80))
    columns = []
    for w in (1, T // 2 + 1, T):
        pk = values(ty, 3 * packed_len(ty, w), 80100 + 64 * T + w)
        pl = packed_len(ty, w)
        columns.append((("uniform", w), 3, pk, [(w, pk[b * pl:(b + 1) * pl]) for b in range(3)], None))
    mw, moff, mcol, mblocks, _ = gs.mixed_column_host(ty, [1, T // 2 + 1, T, 0, T // 2 + 1, 1, T], 80200 + T, pad16=[1, 3, 0, 2, 5, 7, 4])
    assert not ((moff + 16) % 128 == 0).any() and len(set(((moff + 16) % 128)[mw > 0].tolist())) >= 5
    columns.append((("mixed",), 7, mcol, mblocks, (mw, moff)))
    for tag, nb, col, blocks, meta in columns:
        sets = [rs.integers(0, nb * 1024, size=count).astype(np.int64) for count in LOOKUP_COUNTS]
        whole = 1024 * (nb - 1) + np.arange(1024, dtype=np.int64)               # every index of the last block
        expect = lambda idx: np.array([o.unpack_single(ty, blocks[i >> 10][0], blocks[i >> 10][1], i & 1023) for i in idx.tolist()], dtype=TYPES[ty][0])
        wants = [expect(idx) for idx in sets]
        want_whole = expect(whole)
        d_col = placed(col, ty, 16, seed())
        assert d_col.t.data_ptr() % 128 == 16
        if meta is None:
            name, lead, ins = "unpack_single", (tag[1], d_col.t.data_ptr(), nb), (d_col,)
        else:
            d_w, d_off = placed(meta[0], "uint8", 96, seed()), placed(meta[1], "int64", 112, seed())
            name, lead, ins = "unpack_single_widths", (d_w.t.data_ptr(), d_off.t.data_ptr(), d_col.t.data_ptr(), d_col.nbytes, nb), (d_col, d_w, d_off)
        for place, r_idx, r_out in places:
            runs = list(zip(sets, wants)) + ([(whole, want_whole)] if r_idx == 8 else [])
            for idx, want in runs:
                what = (ty, tag, place, idx.size)
                d_idx, got, flag = placed(idx, "int64", r_idx, seed()), out_of(ty, idx.size, r_out, seed()), zero_flag(seed())
                assert d_idx.t.data_ptr() % 16 == r_idx % 16 and got.t.data_ptr() % 128 == r_out
                lookups(fl, ty, name, lead, d_idx, got, flag, what)
                same(got, want, what)
                guards(what, got, d_idx, flag, *ins)


# ---- f. the encoder's metadata steps ----
@pytest.mark.parametrize("ty", TYS)
def test_encoder_metadata_steps(fl, ty):
    """for_widths (mins, maxs at sizeof(T), the widths written at 16k) and widths_to_offsets (widths at 16k, offsets and the total at
    residues of their own) against numpy: bit length of max - min, exclusive prefix sum of 128 * W"""
    T, esz = tbits(ty), tbits(ty) // 8
    seed = seeds_from(90000 + 1000 * T)
    for n, k in ((1, 1), (37, 3), (4099, 6)):
        what = (ty, n)
        a, b = values(ty, n, 90100 + T + n), values(ty, n, 90200 + T + n)
        b[::5] >>= np.array(T - 3, dtype=b.dtype)                               # small spans among the random ones
        a[::5] >>= np.array(T - 3, dtype=a.dtype)
        a[::7] = b[::7]                                                         # constant blocks: width 0
        mins, maxs = np.minimum(a, b), np.maximum(a, b)
        want_w = np.array([int(x).bit_length() for x in (maxs - mins).tolist()], dtype=np.uint8)
        assert want_w.min() == 0 and want_w.max() <= T
        d_mins, d_maxs, d_w = placed(mins, ty, esz, seed()), placed(maxs, ty, esz, seed()), placed(n, "uint8", 16 * k, seed())
        cabi(fl, f"fl_{ty}_for_widths", d_mins.t.data_ptr(), d_maxs.t.data_ptr(), n, d_w.t.data_ptr())
        same(d_w, want_w, what + ("for_widths",))
        guards(what + ("for_widths",), d_w, d_mins, d_maxs)
        size = want_w.astype(np.int64) * 128
        d_off, d_total, flag = placed(n * 8, "int64", 16 * (8 - k), seed()), placed(8, "int64", 16 * ((k + 2) % 7 + 1), seed()), zero_flag(seed())
        cabi(fl, "fl_widths_to_offsets", T, d_w.t.data_ptr(), n, d_off.t.data_ptr(), d_total.t.data_ptr(), flag.t.data_ptr())
        flag_clear(flag, what)
        same(d_off, np.cumsum(size) - size, what + ("widths_to_offsets",))
        same(d_total, np.array([size.sum()], dtype=np.int64), what + ("total",))
        guards(what + ("widths_to_offsets",), d_off, d_total, flag, d_w)
