"""GPU: unfor_aggregate_by_columns / unfor_aggregate_by_columns_widths -- COUNT / SUM / MIN / MAX of a * b, a + b or a - b between two
FoR-packed columns of one element type, grouped by a FoR-packed u8 key column under a selection mask -- against the oracle's unfor_pack
of ALL THREE columns (ffor.rs:38-50), combined with numpy in uint64 (both values zero-extended first, the operation wrapping mod 2^64:
group_columns_data.expr) and reduced per key with group_data.expected_groups: uint64[256, 4], bit-exact.  What the cases exercise is
asserted on the reference by tests/test_group_columns_data_cpu.py."""
import ctypes

import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import GUARD, IDENTITY, SENTINEL, TDT, TYS, UNIFORM_BLOCKS, combine, mask_set, mask_words, placed, sentinel_slots, to_dev, u64_of
from group_columns_data import MIXED_BLOCKS, OPS, expected, expr, mixed_case, routed_case, value_column
from group_data import GROUPS, KEY_WIDTH, expected_groups, key_blocks, key_column

pytestmark = pytest.mark.gpu

RUN_OF_4 = 2 + 65536 * 4                        # kernel policy: wave-per-block mode, at least 4 blocks per wavefront's run
RUNS = [RUN_OF_4, 2 + 256 * 3 + 65536 * 16]     # ... and runs of 16 at 3 waves per SIMD: the policies of test_gpu_aggregate_by.py


def check_result(buf, got, want, what):
    """all 256 slots are the expected ones (so every sentinel was overwritten), the guard behind them is untouched"""
    assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (GROUPS, 4), what
    now = u64_of(buf)
    assert np.array_equal(now[:GROUPS * 4].reshape(GROUPS, 4), want), what
    assert now.size == (GROUPS + GUARD) * 4 and (now[GROUPS * 4:] == SENTINEL).all(), (what, "the guard was written")


def dev(column, broadcast=False):
    """a host column of group_columns_data.value_column / group_data.key_column -> (widths, offsets, packed, references) on the device"""
    import torch
    w, off, col, refs = column[:4]
    return torch.from_numpy(w).cuda(), torch.from_numpy(off).cuda(), to_dev(col), to_dev(refs[:1] if broadcast else refs)


def dmask(bits):
    return None if bits is None else mask_words(bits)


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_form(fl, oracle, ty):
    """THE mixed-width case (every (wa, wb) pair class, key blocks of every distribution, random wrapping per-block references): the
    three ops under the whole mask set and no mask, the result pre-filled with a sentinel and a guard behind it; one broadcast
    reference per column; once the result allocated by the call."""
    T = tbits(ty)
    n = MIXED_BLOCKS[ty]
    a, b, key, _ = mixed_case(oracle, ty, 21000 + T)
    da, db, dk = dev(a), dev(b), dev(key)
    masks = mask_set(n, np.random.default_rng(21100 + T), with_none=True)
    for op in OPS:
        for name, bits in masks.items():
            buf, slots = sentinel_slots(GROUPS)
            got = fl.unfor_aggregate_by_columns_widths(*da, op, *db, *dk, mask=dmask(bits), result=slots)
            check_result(buf, got, expected(op, a, b, key, bits), (ty, op, name))
    # the convenience path: the result allocated inside the call
    got = fl.unfor_aggregate_by_columns_widths(*da, "*", *db, *dk, mask=mask_words(masks["random 1 %"]))
    assert tuple(got.shape) == (GROUPS, 4) and np.array_equal(u64_of(got), expected("*", a, b, key, masks["random 1 %"])), (ty, "result=None")
    # one broadcast reference per column (stride 0)
    a, b, key, _ = mixed_case(oracle, ty, 21200 + T, broadcast=True)
    da, db, dk = dev(a, True), dev(b, True), dev(key, True)
    for op, name in zip(OPS, ("no mask", "random 50 %", "0xAAAAAAAA")):
        buf, slots = sentinel_slots(GROUPS)
        got = fl.unfor_aggregate_by_columns_widths(*da, op, *db, *dk, mask=dmask(masks[name]), result=slots)
        check_result(buf, got, expected(op, a, b, key, masks[name]), (ty, op, name, "broadcast"))


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_form(fl, oracle, ty):
    """35 blocks and 1 block; width pairs (0, 0), (0, T/2), (T/2, 0), (1, T), (T, T) against the key kinds clustered, two, wrapping,
    uniform and constant (key widths 0, 1, 3, 8, 8); `*` on every pair, `+` and `-` on two; per-block references, and scalar ones
    (stride 0) -- zero references among them: the plain bit-packed columns' expression."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    rng = np.random.default_rng(21300 + T)
    pairs = [(0, 0), (0, T // 2), (T // 2, 0), (1, T), (T, T)]
    kinds = ["clustered", "two", "wrapping", "uniform", "constant"]
    for n in (UNIFORM_BLOCKS, 1):
        masks = mask_set(n, rng, full=False, with_none=True)
        names = list(masks) if n > 1 else ["ones", "random 50 %", "no mask"]
        for i, ((wa, wb), kind) in enumerate(zip(pairs, kinds)):
            kw, _, kcol, krefs, keys = key_column(oracle, key_blocks(oracle, kind, n, rng))
            assert (kw == KEY_WIDTH[kind]).all()
            apk, bpk = values(ty, n * packed_len(ty, wa), 21400 + 64 * T + wa), values(ty, n * packed_len(ty, wb), 21500 + 64 * T + wb)
            ra, rb = values(ty, n, 21600 + T + i), values(ty, n, 21700 + T + i)
            va = oracle.batch("unfor_pack", ty, wa, apk, aux=ra, n_blocks=n)
            vb = oracle.batch("unfor_pack", ty, wb, bpk, aux=rb, n_blocks=n)
            dapk, dbpk, dra, drb, dk, dkr = (to_dev(x) for x in (apk, bpk, ra, rb, kcol, krefs))
            for op in OPS if i in (1, 3) else ["*"]:
                x = expr(op, va, vb)
                for name in names:
                    buf, slots = sentinel_slots(GROUPS)
                    got = fl.FoR.unfor_aggregate_by_columns(wa, dapk, dra, op, wb, dbpk, drb, KEY_WIDTH[kind], dk, dkr, mask=dmask(masks[name]),
                                                            n_blocks=n, result=slots)
                    check_result(buf, got, expected_groups(x, keys, masks[name]), (ty, n, wa, wb, kind, op, name))
            # scalar references, stride 0: 5 and 9 on the values; zero on all three columns is the plain bit-packed case
            for sa, sb, sk in ((5, 9, int(krefs[0])), (0, 0, 0)):
                pa = oracle.batch("unfor_pack", ty, wa, apk, aux=np.full(n, sa, dtype=dt), n_blocks=n)
                pb = oracle.batch("unfor_pack", ty, wb, bpk, aux=np.full(n, sb, dtype=dt), n_blocks=n)
                pkeys = key_column(oracle, [(int(KEY_WIDTH[kind]), sk, kcol[b * 128 * KEY_WIDTH[kind]:(b + 1) * 128 * KEY_WIDTH[kind]]) for b in range(n)])[4]
                if sa == 0:
                    assert np.array_equal(pa, oracle.batch("unpack", ty, wa, apk, n_blocks=n))
                got = fl.FoR.unfor_aggregate_by_columns(wa, dapk, sa, "*", wb, dbpk, sb, KEY_WIDTH[kind], dk, sk, mask=dmask(masks["random 50 %"]),
                                                        n_blocks=n)
                assert np.array_equal(u64_of(got), expected_groups(expr("*", pa, pb), pkeys, masks["random 50 %"])), (ty, n, wa, wb, kind, sa)


@pytest.mark.parametrize("ty", TYS)
def test_consistent_with_both_parents_and_deterministic(fl, oracle, ty):
    """A width-0 column b of reference 1 under `*`: unfor_aggregate_by_widths of column a, slot for slot.  Every key block of width 0
    with one reference g: slot g is aggregate_reduce of unfor_aggregate_columns_widths, every other slot the identity.  Two runs of
    one call give identical bits."""
    import torch
    T = tbits(ty)
    n = MIXED_BLOCKS[ty]
    a, b, key, _ = mixed_case(oracle, ty, 21800 + T)
    da, db, dk = dev(a), dev(b), dev(key)
    z = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    none_t = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    none_8 = torch.empty(0, dtype=torch.uint8, device="cuda:0")
    one = to_dev(np.ones(1, dtype=TYPES[ty][0]))
    g = 201
    for name, bits in mask_set(n, np.random.default_rng(21900 + T), full=False, with_none=True).items():
        dm = dmask(bits)
        first = fl.unfor_aggregate_by_columns_widths(*da, "*", *db, *dk, mask=dm)
        again = fl.unfor_aggregate_by_columns_widths(*da, "*", *db, *dk, mask=dm)
        assert torch.equal(first, again), (ty, name, "two runs differ")
        assert np.array_equal(u64_of(first), expected("*", a, b, key, bits)), (ty, name)
        by = fl.unfor_aggregate_by_widths(*da, *dk, dm)
        assert np.array_equal(u64_of(by), expected_groups(a[4], key[4], bits))          # (the yardstick itself is right)
        got = fl.unfor_aggregate_by_columns_widths(*da, "*", z, zoff, none_t, one, *dk, mask=dm)
        assert torch.equal(got, by), (ty, name, "a * 1 is not unfor_aggregate_by of a")
        for op in OPS:
            total, _ = fl.unfor_aggregate_columns_widths(*da, op, *db, mask=dm)
            got = u64_of(fl.unfor_aggregate_by_columns_widths(*da, op, *db, z, zoff, none_8, to_dev(np.full(1, g, np.uint8)), mask=dm))
            want = np.tile(IDENTITY, (GROUPS, 1))
            want[g] = u64_of(total)
            if want[g, 0] == 0:
                want[g] = IDENTITY
            assert np.array_equal(got, want), (ty, name, op, "one key")
            assert np.array_equal(combine(got), u64_of(total))


@pytest.mark.parametrize("policy", RUNS)
@pytest.mark.parametrize("ty", TYS)
def test_runs_of_mixed_routes_uneven_tail_and_idle_wavefronts(fl, oracle, kernel_policy, ty, policy):
    """A cap on the grid through the kernel policy's blocks-per-wavefront field: 35 blocks in runs of 4 are eight full runs, a tail of 3
    and 26 wavefronts of the 35-workgroup grid without a block (runs of 16: 16, 16, 3 and 32 idle).  The blocks alternate SKIP /
    ONE_KEY / DECODE; a group is fed from several runs.  Equal to the reference, and to the call without the cap."""
    T = tbits(ty)
    n = UNIFORM_BLOCKS
    run = (policy >> 16) & 0xFF
    assert n % run == 3 and -(-n // run) < n
    a, b, key, bits, routes = routed_case(oracle, ty, n, 22000 + T)
    assert set(routes[:run]) == {0, 1, 2}
    da, db, dk, dm = dev(a), dev(b), dev(key), mask_words(bits)
    plain = {op: fl.unfor_aggregate_by_columns_widths(*da, op, *db, *dk, mask=dm) for op in OPS}   # policy 0
    kernel_policy(policy)
    for op in OPS:
        want = expected(op, a, b, key, bits)
        buf, slots = sentinel_slots(GROUPS)
        check_result(buf, fl.unfor_aggregate_by_columns_widths(*da, op, *db, *dk, mask=dm, result=slots), want, (ty, policy, op))
        assert np.array_equal(u64_of(plain[op]), want), (ty, op, "policy 0")
    # no mask under the cap: the tail run (blocks 32..34) and a full one are both non-trivial
    buf, slots = sentinel_slots(GROUPS)
    check_result(buf, fl.unfor_aggregate_by_columns_widths(*da, "-", *db, *dk, result=slots), expected("-", a, b, key, None), (ty, policy, "no mask"))


def raw_widths(fl, ty, code, da, db, dk, dm, n, result):
    """The C ABI call with its own err_flag; returns the flag's value."""
    import torch
    esz = tbits(ty) // 8
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [code]
    for (w, o, col, refs), size in ((da, esz), (db, esz), (dk, 1)):
        args += [w.data_ptr(), o.data_ptr(), col.data_ptr(), col.numel() * size, refs.data_ptr(), 1]
    rc = getattr(fl.load(), f"fl_{ty}_unfor_aggregate_by_columns_widths")(*args, None if dm is None else dm.data_ptr(), n, result.data_ptr(),
                                                                         err.data_ptr(), stream)
    assert rc == 0
    return int(err.item())


@pytest.mark.parametrize("ty", TYS)
def test_device_errors_flag_and_skip_the_block(fl, oracle, ty):
    """A block failing its check in column a only (width T + 1), in column b only (outside its column), in the key column only (a
    misaligned offset; width 9): exactly that block's FL_DEVERR_* bits, the result is the reference without that block -- whichever
    column failed -- and check=True raises."""
    import torch
    T = tbits(ty)
    n = 20
    rng = np.random.default_rng(22100 + T)
    a = value_column(oracle, ty, rng.integers(1, T + 1, size=n), 22101 + T, values(ty, n, 22102 + T))
    b = value_column(oracle, ty, rng.integers(1, T + 1, size=n), 22103 + T, values(ty, n, 22104 + T))
    key = key_column(oracle, [key_blocks(oracle, ("uniform", "wrapping", "two")[blk % 3], 1, rng)[0] for blk in range(n)])
    bits = rng.random(n * 1024) < 0.4
    dm = mask_words(bits)

    def changed(column, field, blk, v):
        x = column[field].copy()
        x[blk] = v
        return column[:field] + (x,) + column[field + 1:]
    cases = [("a: width T + 1", 7, 1, 1, changed(a, 0, 7, T + 1), b, key),
             ("b: block out of bounds", 11, 8, 6, a, changed(b, 1, 11, b[1][11] + (1 << 40)), key),
             ("key: offset + 8", 5, 4, 4, a, b, changed(key, 1, 5, key[1][5] + 8)),
             ("key: width 9", 3, 1, 1, a, b, changed(key, 0, 3, 9))]
    for code, (what, blk, flag, status, a_, b_, key_) in enumerate(cases):
        op = OPS[code % 3]
        da, db, dk = dev(a_), dev(b_), dev(key_)
        for m, mbits in ((dm, bits), (None, None)):
            buf, slots = sentinel_slots(GROUPS)
            assert raw_widths(fl, ty, code % 3, da, db, dk, m, n, slots) == flag, (ty, what)
            check_result(buf, slots, expected(op, a, b, key, mbits, without=(blk,)), (ty, what))
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_aggregate_by_columns_widths(*da, op, *db, *dk, mask=dm)
        assert ei.value.status == status, (ty, what)
    # all four at once: every bit, every one of the blocks skipped
    da, db = dev(changed(a, 0, 7, T + 1)), dev(changed(b, 1, 11, b[1][11] + (1 << 40)))
    dk = dev(changed(changed(key, 1, 5, key[1][5] + 8), 0, 3, 9))
    buf, slots = sentinel_slots(GROUPS)
    assert raw_widths(fl, ty, 0, da, db, dk, dm, n, slots) == 1 | 4 | 8
    check_result(buf, slots, expected("*", a, b, key, bits, without=(3, 5, 7, 11)), (ty, "all four"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("residue", [16, 80])
@pytest.mark.parametrize("ty", TYS)
def test_buffers_at_16_byte_residues(fl, oracle, ty, residue):
    """both value columns, the keys, the mask and the result placed at a 16-byte residue off the 128-byte boundary: the result is right
    and no byte around them changes"""
    T = tbits(ty)
    n = 9
    rng = np.random.default_rng(22200 + T + residue)
    wa, wb = T // 2, T // 2 - 1
    apk, bpk = values(ty, n * packed_len(ty, wa), 22201 + T), values(ty, n * packed_len(ty, wb), 22202 + T)
    ra, rb = values(ty, n, 22203 + T), values(ty, n, 22204 + T)
    va = oracle.batch("unfor_pack", ty, wa, apk, aux=ra, n_blocks=n)
    vb = oracle.batch("unfor_pack", ty, wb, bpk, aux=rb, n_blocks=n)
    _, _, kcol, krefs, keys = key_column(oracle, key_blocks(oracle, "wrapping", n, rng))
    bits = rng.random(n * 1024) < 0.5
    seed = 22210 + 8 * T + residue
    pa, pb = placed(apk, ty, residue, seed), placed(bpk, ty, residue, seed + 1)
    pkeys = placed(kcol, "u8", residue, seed + 2)
    pmask = placed(np.packbits(bits, bitorder="little").view(np.int32), "int32", residue, seed + 3)
    pres = placed(np.full(GROUPS * 4, SENTINEL, dtype=np.uint64).view(np.int64), "int64", residue, seed + 4)
    got = fl.FoR.unfor_aggregate_by_columns(wa, pa.t, to_dev(ra), "-", wb, pb.t, to_dev(rb), 3, pkeys.t, to_dev(krefs), mask=pmask.t, result=pres.t)
    assert got.data_ptr() == pres.t.data_ptr() and got.data_ptr() % 128 == residue
    assert np.array_equal(pres.np().view(np.uint64).reshape(GROUPS, 4), expected_groups(expr("-", va, vb), keys, bits)), (ty, residue)
    for p, what in ((pa, "a"), (pb, "b"), (pkeys, "keys"), (pmask, "mask"), (pres, "result")):
        p.check_guards((ty, residue, what))
    for p in (pa, pb, pkeys, pmask):
        assert np.array_equal(p.np().view(np.uint8), p.before())


@pytest.mark.parametrize("ty", TYS)
def test_non_default_stream_and_empty_columns(fl, oracle, ty):
    import torch
    T = tbits(ty)
    n = 17
    a, b, key, bits, _ = routed_case(oracle, ty, n, 22300 + T)
    da, db, dk, dm = dev(a), dev(b), dev(key), mask_words(bits)
    s = torch.cuda.Stream()
    buf, slots = sentinel_slots(GROUPS)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = fl.unfor_aggregate_by_columns_widths(*da, "+", *db, *dk, mask=dm, result=slots, check=False)
    s.synchronize()
    check_result(buf, got, expected("+", a, b, key, bits), (ty, "stream"))
    # empty columns: 256 identities, with and without a mask
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    e8 = torch.empty(0, dtype=torch.uint8, device="cuda:0")
    e64 = torch.empty(0, dtype=torch.int64, device="cuda:0")
    ref, kref = to_dev(np.zeros(1, TYPES[ty][0])), to_dev(np.zeros(1, np.uint8))
    want = np.tile(IDENTITY, (GROUPS, 1))
    for m in (None, torch.empty(0, dtype=torch.int32, device="cuda:0")):
        buf, slots = sentinel_slots(GROUPS)
        check_result(buf, fl.FoR.unfor_aggregate_by_columns(3, empty, 0, "*", 5, empty, 0, 3, e8, 0, mask=m, result=slots), want, (ty, "uniform"))
        buf, slots = sentinel_slots(GROUPS)
        check_result(buf, fl.unfor_aggregate_by_columns_widths(e8, e64, empty, ref, "-", e8, e64, empty, ref, e8, e64, e8, kref, mask=m, result=slots),
                     want, (ty, "mixed"))


def pack_column(fl, ty, vals):
    """the library's own encoder chain: per-block minimum as the reference, for_widths, widths_to_offsets, for_pack_widths"""
    import torch
    v = np.ascontiguousarray(vals, dtype=TYPES[ty][0]).reshape(-1, 1024)
    mins, maxs = to_dev(v.min(axis=1)), to_dev(v.max(axis=1))
    widths = fl.for_widths(mins, maxs)
    offsets, total = fl.widths_to_offsets(ty, widths)
    out = torch.zeros(int(total.item()) // (tbits(ty) // 8), dtype=getattr(torch, TDT[ty]), device="cuda:0")
    fl.for_pack_widths(widths, offsets, to_dev(v.reshape(-1)), mins, out)
    return widths, offsets, out, mins


def test_q1_shape_end_to_end(fl):
    """SELECT k, COUNT(*), SUM(qty), SUM(price), SUM(price * (100 - discount)) WHERE shipdate <= cutoff GROUP BY k, k = flag * 2 +
    status: one range mask, two unfor_aggregate_by_widths launches and one unfor_aggregate_by_columns_widths launch over five columns
    packed by for_pack_widths, nothing materialised -- against numpy on the original values"""
    ty, n = "u32", 20
    rng = np.random.default_rng(22400)
    N = n * 1024
    qty = rng.integers(1, 51, size=N).astype(np.uint32)
    price = (rng.integers(90_000, 10_500_000, size=N) + np.repeat(rng.integers(0, 1 << 31, size=n), 1024)).astype(np.uint32)
    discount = rng.integers(0, 11, size=N).astype(np.uint32)
    date = np.sort(rng.integers(8000, 10600, size=N)).astype(np.uint32)          # clustered by date, as a fact table is
    k = (rng.integers(0, 3, size=N) * 2 + rng.integers(0, 2, size=N)).astype(np.uint8)
    k[:1024] = 4                                                            # a block of one key: key width 0
    cutoff = int(np.quantile(date, 0.8))
    dq, dp, dd, dt_, dkey = (pack_column(fl, t, v) for t, v in (("u32", qty), ("u32", price), ("u32", discount), ("u32", date), ("u8", k)))
    assert int(dkey[0][0].item()) == 0 and int(dkey[0].max().item()) == 3
    m = fl.unfor_compare_range_widths(*dt_, 0, cutoff)
    by_qty = u64_of(fl.unfor_aggregate_by_widths(*dq, *dkey, m))
    by_price = u64_of(fl.unfor_aggregate_by_widths(*dp, *dkey, m))
    by_pd = u64_of(fl.unfor_aggregate_by_columns_widths(*dp, "*", *dd, *dkey, mask=m))
    keep = date <= cutoff
    assert 0.5 * N < keep.sum() < N and (expr("*", price, discount)[keep] >= np.uint64(1 << 32)).any()
    for g in range(GROUPS):
        rows = keep & (k == g)
        p, d, q = (x[rows].astype(object) for x in (price, discount, qty))
        assert int(by_pd[g, 0]) == int(by_qty[g, 0]) == int(by_price[g, 0]) == int(rows.sum()), g
        if not rows.any():
            assert g > 5 and np.array_equal(by_pd[g], IDENTITY)
            continue
        assert int(by_qty[g, 1]) == int(q.sum()) and int(by_price[g, 1]) == int(p.sum()), g
        assert 100 * int(by_price[g, 1]) - int(by_pd[g, 1]) == int((p * (100 - d)).sum()), g   # sum_disc_price, in cents of cents
        assert int(by_pd[g, 2]) == int((p * d).min()) and int(by_pd[g, 3]) == int((p * d).max()), g
