"""GPU: undelta_aggregate / undelta_aggregate_widths -- COUNT / SUM / MIN / MAX per block of a DELTA-packed column over the rows a mask
keeps -- against the slots numpy builds from the oracle's untranspose(undelta_pack(..)) per block (delta.rs:47-63, transpose.rs:17-22)
and the mask's bits (bit i of word i // 32 of block b, LSB first, i = the ORIGINAL row).  Every slot buffer is prefilled with
gpu_support's sentinel, so every slot must be written; `result` is compared with the combination of the expected slots.  The
expectation and the routes a launch must take come from the definition (tests/delta_aggregate_data.py), never from the headers under
test; every comparison is bit exact."""
import numpy as np
import pytest

import delta_aggregate_data as da
import delta_compare_range_data as dd
import gpu_support as gs
from datagen import values
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TDT, TYS, mixed_column, sentinel_slots, to_dev, u64_of
from oracle_lib import TYPES, lanes, packed_len, tbits

pytestmark = pytest.mark.gpu


def check(call, n, vals, mask_words, what, skipped=()):
    """`call(mask=, block_aggs=)` -> (result, slots) into a sentinel-filled buffer: every slot, the guard behind them, the result"""
    buf, slots = sentinel_slots(n)
    dmask = None if mask_words is None else to_dev(mask_words)
    result, out = call(mask=dmask, block_aggs=slots)
    assert out.data_ptr() == slots.data_ptr()
    want = da.want_slots(vals, mask_words, skipped)
    got = u64_of(buf)
    g = got[:n * 4].reshape(n, 4)
    if not np.array_equal(g, want):
        wrong = np.argwhere(g != want)
        b, s = (int(x) for x in wrong[0])
        raise AssertionError(f"{what}: {len(wrong)} slot words differ, the first in block {b}: {gs.SLOTS[s]} is {int(g[b, s])}, not {int(want[b, s])}")
    assert (got[n * 4:] == gs.SENTINEL).all(), (what, "the guard was written")
    assert np.array_equal(u64_of(result), gs.combine(want)), (what, "result")
    return want


@pytest.mark.parametrize("ty", TYS)
def test_random_columns_every_route(fl, oracle, ty):
    """Random packed bytes (the chains wrap) under random, clustered and equal bases: every width 0..T, a ragged column of 263 blocks, and
    1 / 2 / 3 / 5 blocks; without a mask and under masks that mix random blocks with empty, full, one-bit-set and one-bit-clear ones.
    IDENTITY, BASES and EACH occur in ONE launch of the two larger columns."""
    T = tbits(ty)
    rng = np.random.default_rng(13100 + T)
    for n, widths in ((T + 1, np.arange(T + 1)), (263, rng.integers(0, T + 1, size=263)), (1, [T // 2]), (2, [3, T]), (3, [T, 0, 1]),
                      (5, [2, T - 1, 0, T, 5])):
        dw, doff, col, blocks = mixed_column(ty, widths, 13200 + n)
        bases = dd.delta_bases(ty, n, 13300 + n)
        dcol, dbases = to_dev(col), to_dev(bases)
        vals = dd.decode(oracle, ty, blocks, bases)
        call = lambda **kw: fl.undelta_aggregate_widths(dw, doff, dcol, dbases, **kw)
        check(call, n, vals, None, (ty, n, "no mask"))
        for shift in ((0, 1, 3) if n >= 10 else (0, 1, 2, 3, 4, 5)):
            m = dd.incoming_mask(n, 13400 + n, shift=shift)
            if n >= 10 and shift == 0:
                assert set(da.column_routes(widths, m)) == {da.IDENTITY_ROUTE, da.BASES, da.EACH}, (ty, n)
            check(call, n, vals, m, (ty, n, "mask", shift))


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_every_width(fl, oracle, ty):
    """Delta.undelta_aggregate over a uniform-width column of 37 blocks at every (T, W): both sides of the read route's switch, W = 0 (no
    packed bytes: BASES) and W = T among them"""
    T = tbits(ty)
    n = 37
    for w in range(T + 1):
        pk = values(ty, n * packed_len(ty, w), 13500 + 64 * T + w)
        bases = dd.delta_bases(ty, n, 13600 + 64 * T + w)
        vals = dd.decode_uniform(oracle, ty, w, pk, bases, n)
        dpk, dbases = to_dev(pk), to_dev(bases)
        call = lambda **kw: fl.Delta.undelta_aggregate(w, dpk, dbases, n_blocks=n, **kw)
        check(call, n, vals, dd.incoming_mask(n, 13700 + w, shift=w), (ty, w, "mask"))
        if w % 3 == 0 or w == T:
            check(call, n, vals, None, (ty, w, "no mask"))


@pytest.fixture(scope="module")
def sorted_columns(oracle):
    """ty -> the sorted column of 11 blocks, built once (the round trip through the oracle is asserted while it is built)"""
    return {ty: dd.sorted_column(oracle, ty, 11, 13800 + tbits(ty)) for ty in TYS}


@pytest.mark.parametrize("ty", TYS)
def test_sorted_columns_where_one_element_decides(fl, oracle, sorted_columns, ty):
    """A sorted column (strictly ascending inside a block for T >= 32): for every pair of edge rows a mask that keeps rows [r0, r1] of one
    block -- min is the value at r0, max the value at r1, count r1 - r0 + 1 -- and one-bit masks at every edge row (count 1, sum = min =
    max), which decide for the narrow types, whose values repeat.  A mask bit applied one row, one R-piece or one T-group off changes
    the answer (asserted from the definition where the block ascends strictly).  Mixed-width form; the one-bit masks also through the
    uniform form of the same blocks repacked at the widest width."""
    import torch
    T = tbits(ty)
    R = T // 8
    L = lanes(ty)
    v, widths, blocks, bases = sorted_columns[ty]
    n = len(blocks)
    off, col = dd.column_of(blocks, ty)
    dw, doff = torch.from_numpy(widths).cuda(), torch.from_numpy(off).cuda()
    dcol, dbases = to_dev(col), to_dev(bases)
    mixed = lambda **kw: fl.undelta_aggregate_widths(dw, doff, dcol, dbases, **kw)
    wmax = int(widths.max())
    upk = np.concatenate([oracle.pack(ty, wmax, oracle.delta(ty, oracle.transpose(ty, v[b * 1024:(b + 1) * 1024]), bases[b * L:(b + 1) * L]))
                          for b in range(n)])
    dupk = to_dev(upk)
    uniform = lambda **kw: fl.Delta.undelta_aggregate(wmax, dupk, dbases, **kw)
    rows = dd.edge_rows(ty)
    wide = [b for b in range(n) if widths[b] > 0]
    assert len(wide) >= 4
    moved_differs = 0
    for k, (r0, r1) in enumerate((a, b) for i, a in enumerate(rows) for b in rows[i:]):
        blk = wide[k % len(wide)]
        m = da.rows_mask(n, blk, r0, r1)
        want = check(mixed, n, v, m, (ty, "rows", blk, r0, r1))
        vb = v[blk * 1024:(blk + 1) * 1024]
        assert int(want[blk, 0]) == r1 - r0 + 1
        if T >= 32:                                                         # strictly ascending: ONE row holds each extreme
            assert (int(want[blk, 2]), int(want[blk, 3])) == (int(vb[r0]), int(vb[r1])), (ty, blk, r0, r1)
            for d in (1, R, T):                                             # the same mask 1 row, one R-piece, one T-group further on
                if r1 + d < 1024:
                    other = da.want_slots(v, da.rows_mask(n, blk, r0 + d, r1 + d))
                    assert not np.array_equal(other[blk, 1:], want[blk, 1:]), (ty, blk, r0, r1, d)
                    moved_differs += 1
    assert T < 32 or moved_differs > 100
    for k, r in enumerate(rows):
        for blk in (wide[k % len(wide)], (k * 3) % n):
            m = da.rows_mask(n, blk, r, r)
            x = int(v[blk * 1024 + r])
            for form, call in (("mixed", mixed), ("uniform", uniform)):
                want = check(call, n, v, m, (ty, form, "one bit", blk, r))
                assert [int(y) for y in want[blk]] == [1, x, x, x]


def test_u64_sums_wrap(fl, oracle):
    """u64 columns whose sums wrap mod 2^64: random values at full width (every block's exact sum passes 2^64), and width-0 blocks whose
    bases sit just below 2^64 (the BASES route's sum of p_l * base_l wraps)"""
    ty, n = "u64", 9
    dw, doff, col, blocks = mixed_column(ty, [64, 63, 64, 0, 62, 64, 0, 64, 61], 13900)
    bases = values(ty, n * 16, 13901)
    bases[3 * 16:4 * 16] = np.uint64(2 ** 64 - 1) - np.arange(16, dtype=np.uint64)
    bases[6 * 16:7 * 16] = np.uint64(2 ** 63 + 5)
    vals = dd.decode(oracle, ty, blocks, bases)
    exact = [sum(int(x) for x in vals[b * 1024:(b + 1) * 1024]) for b in range(n)]
    assert all(s >= 2 ** 64 for s in exact)
    dcol, dbases = to_dev(col), to_dev(bases)
    call = lambda **kw: fl.undelta_aggregate_widths(dw, doff, dcol, dbases, **kw)
    want = check(call, n, vals, None, (ty, "wrapping sums"))
    assert [int(x) for x in want[:, 1]] == [s % 2 ** 64 for s in exact]
    m = dd.incoming_mask(n, 13902, shift=3)                                 # blocks 3 and 6 under a one-bit-clear / a random mask
    kept = [sum(int(x) for x, k in zip(vals[b * 1024:(b + 1) * 1024], da.mask_bits(m)[b * 1024:(b + 1) * 1024]) if k) for b in (3, 6)]
    assert all(s >= 2 ** 64 for s in kept)
    check(call, n, vals, m, (ty, "wrapping sums under a mask"))


@pytest.mark.parametrize("ty", TYS)
def test_skipped_blocks_hold_the_identity_and_raise_their_bits(fl, oracle, ty):
    """A block with a width > T, one with a misaligned offset, one outside the packed column: the kernel checks them itself, err_flag holds
    the three bits, the skipped blocks' slots hold the identity, every other slot is right; check=True raises, check=False stays silent."""
    import ctypes
    import torch
    T = tbits(ty)
    esz = T // 8
    n = 40
    rng = np.random.default_rng(14000 + T)
    widths = rng.integers(1, T + 1, size=n).astype(np.uint8)
    dw, doff, col, blocks = mixed_column(ty, widths, 14001)
    bases = dd.delta_bases(ty, n, 14002)
    vals = dd.decode(oracle, ty, blocks, bases)
    off = doff.cpu().numpy()
    bad_w = widths.copy()
    bad_w[7] = T + 1
    boff = off.copy()
    boff[5] += 8
    boff[11] += 1 << 40
    dbw, dboff = torch.from_numpy(bad_w).cuda(), torch.from_numpy(boff).cuda()
    dcol, dbases = to_dev(col), to_dev(bases)
    lib = fl.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    skipped = (5, 7, 11)
    for m in (None, dd.incoming_mask(n, 14003, shift=2)):
        dm = None if m is None else to_dev(m)
        buf, slots = sentinel_slots(n)
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(lib, f"fl_{ty}_undelta_aggregate_widths")(dbw.data_ptr(), dboff.data_ptr(), dcol.data_ptr(), col.size * esz, dbases.data_ptr(),
                                                              None if dm is None else dm.data_ptr(), n, slots.data_ptr(), err.data_ptr(), stream)
        assert rc == 0
        assert int(err.item()) == 1 | 4 | 8, (ty, int(err.item()))
        got = u64_of(buf)
        assert np.array_equal(got[:n * 4].reshape(n, 4), da.want_slots(vals, m, skipped)), ty
        assert (got[n * 4:] == gs.SENTINEL).all()
        # check=False stays silent: the same slots, and the result combines the valid blocks
        check(lambda **kw: fl.undelta_aggregate_widths(dbw, dboff, dcol, dbases, check=False, **kw), n, vals, m, (ty, "check=False"), skipped)
    for status, w_, o_ in ((1, dbw, doff), (4, dw, torch.from_numpy(np.where(np.arange(n) == 5, off + 8, off)).cuda()),
                           (6, dw, torch.from_numpy(np.where(np.arange(n) == 11, off + (1 << 40), off)).cuda())):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.undelta_aggregate_widths(w_, o_, dcol, dbases)
        assert ei.value.status == status, (ty, status)


@pytest.mark.parametrize("policy", gs.POLICIES)
@pytest.mark.parametrize("ty", TYS)
def test_policies_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Every kernel policy (forced waves / blocks per wavefront / prefetch: the kernel takes a wavefront's blocks one after the other,
    whatever the shape) gives the same bits; a non-default stream; an empty column; columns of width-0 blocks with no packed bytes."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    L = lanes(ty)
    rng = np.random.default_rng(14100 + T)
    n = 131
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 14101)
    bases = dd.delta_bases(ty, n, 14102)
    vals = dd.decode(oracle, ty, blocks, bases)
    pk2 = values(ty, n * packed_len(ty, T // 2), 14103)
    vals2 = dd.decode_uniform(oracle, ty, T // 2, pk2, bases, n)
    m = dd.incoming_mask(n, 14104)
    s = torch.cuda.Stream()
    dcol, dbases, dpk2 = to_dev(col), to_dev(bases), to_dev(pk2)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        check(lambda **kw: fl.undelta_aggregate_widths(dw, doff, dcol, dbases, **kw), n, vals, m, (ty, policy, "mixed"))
        check(lambda **kw: fl.undelta_aggregate_widths(dw, doff, dcol, dbases, check=False, **kw), n, vals, None, (ty, policy, "mixed, no mask"))
        check(lambda **kw: fl.Delta.undelta_aggregate(T // 2, dpk2, dbases, **kw), n, vals2, m, (ty, policy, "uniform"))
    s.synchronize()
    # empty columns: the identity
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    ew, eo = torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0")
    for result, slots in (fl.undelta_aggregate_widths(ew, eo, empty, empty), fl.Delta.undelta_aggregate(3, empty, empty)):
        assert slots.numel() == 0 and np.array_equal(u64_of(result), gs.IDENTITY)
    # width-0 blocks, no packed bytes: lane l's T rows repeat base_l
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    vz = np.concatenate([oracle.untranspose(ty, np.tile(bases[k * L:(k + 1) * L], T)) for k in range(5)])
    for mz in (None, dd.incoming_mask(5, 14105, shift=3), dd.incoming_mask(5, 14106, shift=4)):
        check(lambda **kw: fl.undelta_aggregate_widths(z, zoff, empty, dbases[:5 * L], **kw), 5, vz, mz, (ty, policy, "width 0"))
        check(lambda **kw: fl.Delta.undelta_aggregate(0, empty, dbases[:5 * L], **kw), 5, vz, mz, (ty, policy, "uniform width 0, n_blocks from the bases"))


@pytest.mark.parametrize("ty", TYS)
def test_chain_delta_range_then_delta_aggregate(fl, oracle, sorted_columns, ty):
    """SELECT COUNT(*), SUM(ts), MIN(ts), MAX(ts) WHERE ts BETWEEN a AND b on a sorted, Delta-coded column: undelta_compare_range_widths ->
    undelta_aggregate_widths(mask=..) equals numpy, and equals unfor_aggregate_widths over the device-materialised column
    (undelta_pack_widths(.., untranspose=True) read as a full-width column, the mask given in that column's order), bit for bit."""
    import torch
    T = tbits(ty)
    v, widths, blocks, bases = sorted_columns[ty]
    n = len(blocks)
    off, col = dd.column_of(blocks, ty)
    dw, doff = torch.from_numpy(widths).cuda(), torch.from_numpy(off).cuda()
    dcol, dbases = to_dev(col), to_dev(bases)
    decoded = fl.undelta_pack_widths(dw, doff, dcol, dbases, untranspose=True)
    assert np.array_equal(gs.to_np(decoded, ty), v)
    fw, fo, fr = fl.full_width_column(ty, n, "cuda:0")
    for a, b in ((int(v[2 * 1024 + 300]), int(v[7 * 1024 + 77])), (int(v[5 * 1024 + T]), int(v[5 * 1024 + 3 * T - 1])), (int(v[1023]), int(v[1024]))):
        m = fl.undelta_compare_range_widths(dw, doff, dcol, dbases, a, b)
        words = gs.got_mask(m)
        assert np.array_equal(words, dd.want_mask(v, a, b))
        want = check(lambda **kw: fl.undelta_aggregate_widths(dw, doff, dcol, dbases, **{**kw, "mask": m}), n, v, words, (ty, a, b))
        kept = v[dd.hit_bits(v, a, b)].astype(np.uint64)
        assert kept.size and [int(x) for x in gs.combine(want)] == [kept.size, int(kept.sum(dtype=np.uint64)), int(kept.min()), int(kept.max())]
        result2, slots2 = fl.unfor_aggregate_widths(fw, fo, decoded, fr, mask=to_dev(da.in_full_width_order(ty, words)))
        assert np.array_equal(u64_of(slots2), want), (ty, a, b, "the materialising path")
        assert np.array_equal(u64_of(result2), gs.combine(want))
