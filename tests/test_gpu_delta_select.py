"""GPU: undelta_select / undelta_select_widths -- the rows a mask keeps of a DELTA-packed column, compacted in original row order --
against the oracle's untranspose(undelta_pack(..)) per block (delta.rs:47-63, transpose.rs:17-22) indexed by the mask's bits (bit i of
word i // 32 of block b, LSB first, i = the ORIGINAL row).  Every output is a sentinel-filled buffer with GUARD elements behind `total`:
`total` must be right, a skipped block's slots must still hold the sentinel, the guard must be untouched.  The expectation and the routes
a launch must take come from the definition (tests/delta_select_data.py), never from the headers under test; every comparison is bit
exact."""
import ctypes

import numpy as np
import pytest

import delta_compare_range_data as dd
import delta_select_data as ds
import gpu_support as gs
from datagen import values
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import GUARD, TDT, TYS, mixed_column, sentinel_buffer, sentinel_of, to_dev, to_np
from oracle_lib import lanes, packed_len, tbits

pytestmark = pytest.mark.gpu


def check(fl, call, ty, vals, mask_words, what, skipped=()):
    """`call(mask, out_offsets=, total=, output=)` into a sentinel-filled buffer of total + GUARD elements, out_len = total: mask_offsets'
    results against numpy, the run against vals[bits], the skipped blocks' slots and the guard still the sentinel.  Returns the run."""
    offsets, total = ds.offsets_of(mask_words)
    dm = to_dev(mask_words)
    oo, total_dev = fl.mask_offsets(dm)
    assert int(total_dev.item()) == total, (what, "total")
    assert np.array_equal(oo.cpu().numpy(), offsets), (what, "out_offsets")
    buf = sentinel_buffer(ty, total + GUARD)
    out = call(dm, out_offsets=oo, total=total_dev, output=buf[:total])
    assert out.numel() == total and (total == 0 or out.data_ptr() == buf.data_ptr())
    want, written = ds.want_run(vals, mask_words, skipped)
    want = np.where(written, want, sentinel_of(ty))
    got = to_np(buf, ty)
    if not np.array_equal(got[:total], want):
        wrong = np.flatnonzero(got[:total] != want)
        k = int(wrong[0])
        b = int(np.searchsorted(offsets, k, side="right")) - 1
        raise AssertionError(f"{what}: {wrong.size} of {total} elements differ, the first at {k} (block {b}, its kept row {k - int(offsets[b])}): "
                             f"{int(got[k])}, not {int(want[k])}")
    assert (got[total:] == sentinel_of(ty)).all(), (what, "the guard was written")
    return want


def bits_words(bits):
    return np.packbits(bits, bitorder="little").view(np.int32)


@pytest.mark.parametrize("ty", TYS)
def test_random_columns_every_route(fl, oracle, ty):
    """Random packed bytes (the chains wrap) under random, clustered and equal bases: every width 0..T, a ragged column of 263 blocks, and
    1 / 2 / 3 / 5 blocks, under masks that mix random blocks with empty, full, one-bit-set and one-bit-clear ones (EMPTY, BASES and EACH
    occur in ONE launch of the two larger columns) and under random 1 % and 50 % masks; the convenience path sizes the result itself."""
    T = tbits(ty)
    rng = np.random.default_rng(16100 + T)
    for n, widths in ((T + 1, np.arange(T + 1)), (263, rng.integers(0, T + 1, size=263)), (1, [T // 2]), (2, [3, T]), (3, [T, 0, 1]),
                      (5, [2, T - 1, 0, T, 5])):
        dw, doff, col, blocks = mixed_column(ty, widths, 16200 + n)
        bases = dd.delta_bases(ty, n, 16300 + n)
        dcol, dbases = to_dev(col), to_dev(bases)
        vals = dd.decode(oracle, ty, blocks, bases)
        call = lambda dm, **kw: fl.undelta_select_widths(dw, doff, dcol, dbases, dm, **kw)
        for shift in range(6):
            m = dd.incoming_mask(n, 16400 + n, shift=shift)
            if n == 263 or (n == T + 1 and shift == 0):                     # (the width column's one width-0 block is block 0)
                assert set(ds.column_routes(widths, m)) == {ds.EMPTY, ds.BASES, ds.EACH}, (ty, n, shift)
            check(fl, call, ty, vals, m, (ty, n, "mask", shift))
        named = gs.mask_set(n, rng, full=False)
        for name in ("random 1 %", "random 50 %"):
            m = bits_words(named[name])
            check(fl, call, ty, vals, m, (ty, n, name))
        # output=None, the offsets computed inside: one call, the result sized by the total
        got = fl.undelta_select_widths(dw, doff, dcol, dbases, to_dev(m))
        assert np.array_equal(to_np(got, ty), ds.want_run(vals, m)[0]), (ty, n, "output=None")


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_every_width(fl, oracle, ty):
    """Delta.undelta_select over a uniform-width column of 37 blocks at every (T, W): both sides of the read route's switch, W = 0 (no
    packed bytes: BASES) and W = T among them"""
    T = tbits(ty)
    n = 37
    for w in range(T + 1):
        pk = values(ty, n * packed_len(ty, w), 16500 + 64 * T + w)
        bases = dd.delta_bases(ty, n, 16600 + 64 * T + w)
        vals = dd.decode_uniform(oracle, ty, w, pk, bases, n)
        dpk, dbases = to_dev(pk), to_dev(bases)
        call = lambda dm, **kw: fl.Delta.undelta_select(w, dpk, dbases, dm, n_blocks=n, **kw)
        check(fl, call, ty, vals, dd.incoming_mask(n, 16700 + w, shift=w), (ty, w, "mask"))
        if w in (0, T // 2, T):
            got = fl.Delta.undelta_select(w, dpk, dbases, to_dev(dd.incoming_mask(n, 16800 + w)), n_blocks=n)
            assert np.array_equal(to_np(got, ty), ds.want_run(vals, dd.incoming_mask(n, 16800 + w))[0]), (ty, w, "output=None")


@pytest.fixture(scope="module")
def sorted_columns(oracle):
    """ty -> the sorted column of 11 blocks, built once (the round trip through the oracle is asserted while it is built)"""
    return {ty: dd.sorted_column(oracle, ty, 11, 16900 + tbits(ty)) for ty in TYS}


@pytest.mark.parametrize("ty", TYS)
def test_sorted_columns_keep_the_row_order(fl, oracle, sorted_columns, ty):
    """A sorted column (strictly ascending inside a block for T >= 32): for every pair of edge rows a mask that keeps rows [r0, r1] of one
    block gives exactly v[r0 .. r1], in order; one-bit masks at every edge row give the one value, through both forms (the uniform form
    over the same blocks repacked at the widest width).  The same mask one row, one R-piece or one T-group further on gives a different
    run (asserted from the definition where the block ascends strictly)."""
    import torch
    T = tbits(ty)
    R = T // 8
    L = lanes(ty)
    v, widths, blocks, bases = sorted_columns[ty]
    n = len(blocks)
    off, col = dd.column_of(blocks, ty)
    dw, doff = torch.from_numpy(widths).cuda(), torch.from_numpy(off).cuda()
    dcol, dbases = to_dev(col), to_dev(bases)
    mixed = lambda dm, **kw: fl.undelta_select_widths(dw, doff, dcol, dbases, dm, **kw)
    wmax = int(widths.max())
    upk = np.concatenate([oracle.pack(ty, wmax, oracle.delta(ty, oracle.transpose(ty, v[b * 1024:(b + 1) * 1024]), bases[b * L:(b + 1) * L]))
                          for b in range(n)])
    dupk = to_dev(upk)
    uniform = lambda dm, **kw: fl.Delta.undelta_select(wmax, dupk, dbases, dm, **kw)
    rows = dd.edge_rows(ty)
    wide = [b for b in range(n) if widths[b] > 0]
    assert len(wide) >= 4
    moved_differs = 0
    for k, (r0, r1) in enumerate((a, b) for i, a in enumerate(rows) for b in rows[i:]):
        blk = wide[k % len(wide)]
        m = ds.rows_mask(n, blk, r0, r1)
        want = check(fl, mixed, ty, v, m, (ty, "rows", blk, r0, r1))
        vb = v[blk * 1024:(blk + 1) * 1024]
        assert np.array_equal(want, vb[r0:r1 + 1])
        if T >= 32:                                                         # strictly ascending: the order is visible in the values
            assert (want[1:] > want[:-1]).all()
            for d in (1, R, T):                                             # the same mask 1 row, one R-piece, one T-group further on
                if r1 + d < 1024:
                    other, _ = ds.want_run(v, ds.rows_mask(n, blk, r0 + d, r1 + d))
                    assert not np.array_equal(other, want), (ty, blk, r0, r1, d)
                    moved_differs += 1
    assert T < 32 or moved_differs > 100
    for k, r in enumerate(rows):
        for blk in (wide[k % len(wide)], (k * 3) % n):
            m = ds.rows_mask(n, blk, r, r)
            for form, call in (("mixed", mixed), ("uniform", uniform)):
                want = check(fl, call, ty, v, m, (ty, form, "one bit", blk, r))
                assert want.tolist() == [int(v[blk * 1024 + r])]


def raw_select_widths(fl, ty, dw, doff, dcol, dbases, dm, oo, buf, out_len):
    """The C ABI call with its own err_flag; returns the flag's value."""
    import torch
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(fl.load(), f"fl_{ty}_undelta_select_widths")(dw.data_ptr(), doff.data_ptr(), dcol.data_ptr(), dcol.numel() * (tbits(ty) // 8),
                                                             dbases.data_ptr(), dm.data_ptr(), oo.data_ptr(), buf.data_ptr(), out_len, dw.numel(),
                                                             err.data_ptr(), stream)
    assert rc == 0
    return int(err.item())


@pytest.mark.parametrize("ty", TYS)
def test_skipped_blocks_keep_their_slots_and_raise_their_bits(fl, oracle, ty):
    """A block with a width > T, one with a misaligned offset, one outside the packed column: the kernel checks them itself, err_flag holds
    the three bits, the skipped blocks' output slots still hold the sentinel, every other run is right; check=True raises with the right
    status, check=False stays silent."""
    import torch
    T = tbits(ty)
    n = 40
    rng = np.random.default_rng(17000 + T)
    widths = rng.integers(1, T + 1, size=n).astype(np.uint8)
    dw, doff, col, blocks = mixed_column(ty, widths, 17001)
    bases = dd.delta_bases(ty, n, 17002)
    vals = dd.decode(oracle, ty, blocks, bases)
    off = doff.cpu().numpy()
    bad_w = widths.copy()
    bad_w[7] = T + 1
    boff = off.copy()
    boff[5] += 8
    boff[11] += 1 << 40
    dbw, dboff = torch.from_numpy(bad_w).cuda(), torch.from_numpy(boff).cuda()
    dcol, dbases = to_dev(col), to_dev(bases)
    skipped = (5, 7, 11)
    for m in (bits_words(rng.random(n * 1024) < 0.2), dd.incoming_mask(n, 17003, shift=3)):
        counts = ds.block_counts(m)
        assert all(counts[b] > 0 for b in skipped)                          # the skipped blocks own output slots
        offsets, total = ds.offsets_of(m)
        dm, doo = to_dev(m), to_dev(offsets)
        buf = sentinel_buffer(ty, total + GUARD)
        flag = raw_select_widths(fl, ty, dbw, dboff, dcol, dbases, dm, doo, buf, total)
        assert flag == 1 | 4 | 8, (ty, flag)
        want, written = ds.want_run(vals, m, skipped)
        got = to_np(buf, ty)
        assert np.array_equal(got[:total], np.where(written, want, sentinel_of(ty))), ty
        assert (got[total:] == sentinel_of(ty)).all()
        # check=False stays silent: the same output
        check(fl, lambda dm, **kw: fl.undelta_select_widths(dbw, dboff, dcol, dbases, dm, check=False, **kw), ty, vals, m, (ty, "check=False"), skipped)
    # SKIP ahead of EMPTY: the failing blocks' masks are all zero, and their bits are raised all the same; nothing of theirs is written
    quiet = m.copy().reshape(n, 32)
    quiet[list(skipped)] = 0
    quiet = quiet.reshape(-1)
    assert all(ds.block_counts(quiet)[b] == 0 for b in skipped)
    assert [ds.column_routes(bad_w, quiet, skipped)[b] for b in skipped] == [ds.SKIP] * 3
    offsets, total = ds.offsets_of(quiet)
    buf = sentinel_buffer(ty, total + GUARD)
    flag = raw_select_widths(fl, ty, dbw, dboff, dcol, dbases, to_dev(quiet), to_dev(offsets), buf, total)
    assert flag == 1 | 4 | 8, (ty, "empty masks", flag)
    got = to_np(buf, ty)
    assert np.array_equal(got[:total], ds.want_run(vals, quiet)[0]) and (got[total:] == sentinel_of(ty)).all(), (ty, "empty masks")
    dm = to_dev(m)
    for status, w_, o_ in ((1, dbw, doff), (4, dw, torch.from_numpy(np.where(np.arange(n) == 5, off + 8, off)).cuda()),
                           (6, dw, torch.from_numpy(np.where(np.arange(n) == 11, off + (1 << 40), off)).cuda())):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.undelta_select_widths(w_, o_, dcol, dbases, dm)
        assert ei.value.status == status, (ty, status)


@pytest.mark.parametrize("ty", TYS)
def test_output_bounds_never_write_outside(fl, oracle, ty):
    """out_len one short of total, and one block's out_offsets moved past out_len: FL_DEVERR_BOUNDS is raised, exactly those blocks
    write nothing, every other block is right, the guard behind `total` stays untouched -- through the mixed and the uniform form, whose
    err_flag serves this."""
    import torch
    T = tbits(ty)
    n = 53
    rng = np.random.default_rng(17100 + T)
    widths = rng.integers(0, T + 1, size=n)
    widths[[9, n - 4]] = (0, T // 2)                                        # a width-0 block and a decoded one among the refused
    dw, doff, col, blocks = mixed_column(ty, widths, 17101)
    bases = dd.delta_bases(ty, n, 17102)
    vals = dd.decode(oracle, ty, blocks, bases)
    bits = rng.random(n * 1024) < 0.3
    bits[-3 * 1024:] = False                                                # the last three blocks keep nothing: block n - 4 ends the output
    m = bits_words(bits)
    offsets, total = ds.offsets_of(m)
    last = n - 4
    dm, dcol, dbases = to_dev(m), to_dev(col), to_dev(bases)
    oo, total_dev = fl.mask_offsets(dm)
    moved = offsets.copy()
    moved[9] = total + 5                                                    # past out_len
    shifted = offsets.copy()
    shifted[last] += 3                                                      # its run would end 3 elements behind out_len
    for what, offs, out_len, refused in (("one short", offsets, total - 1, (last,)), ("moved past out_len", moved, total, (9,)),
                                         ("shifted", shifted, total, (last,))):
        assert [b for b, r in enumerate(ds.column_routes(widths, m, (), offs, out_len)) if r == ds.BOUNDS] == list(refused), what
        want, written = ds.want_run(vals, m, refused)
        want = np.where(written, want, sentinel_of(ty))
        buf = sentinel_buffer(ty, total + GUARD)
        flag = raw_select_widths(fl, ty, dw, doff, dcol, dbases, dm, to_dev(offs), buf, out_len)
        assert flag == 8, (ty, what, flag)
        got = to_np(buf, ty)
        assert np.array_equal(got[:total], want), (ty, what)
        assert (got[total:] == sentinel_of(ty)).all(), (ty, what, "the guard was written")
    # EMPTY ahead of BOUNDS: the empty blocks' offsets lie past out_len (and one at 2^63), and nothing is raised; every run is right
    stray = offsets.copy()
    stray[-3:] = (total + 1, total + 4096, 1 << 62)
    assert [ds.route_of(True, m.reshape(n, 32)[b], False, widths[b]) for b in (n - 3, n - 2, n - 1)] == [ds.EMPTY] * 3
    buf = sentinel_buffer(ty, total + GUARD)
    flag = raw_select_widths(fl, ty, dw, doff, dcol, dbases, dm, to_dev(stray), buf, total)
    assert flag == 0, (ty, "empty blocks past out_len", flag)
    got = to_np(buf, ty)
    assert np.array_equal(got[:total], ds.want_run(vals, m)[0]) and (got[total:] == sentinel_of(ty)).all(), (ty, "empty blocks past out_len")
    # the Python mirror reports it
    with pytest.raises(fl.FastLanesError) as ei:
        fl.undelta_select_widths(dw, doff, dcol, dbases, dm, out_offsets=oo, total=total_dev, output=sentinel_buffer(ty, total + GUARD)[:total - 1])
    assert ei.value.status == 6
    # the uniform form: 3 blocks, out_len right and one short
    nu, w = 3, 5
    pk = values(ty, nu * packed_len(ty, w), 17103 + T)
    ub = dd.delta_bases(ty, nu, 17104 + T)
    uvals = dd.decode_uniform(oracle, ty, w, pk, ub, nu)
    um = bits_words(rng.random(nu * 1024) < 0.3)
    uoff, utotal = ds.offsets_of(um)
    dpk, dub, dum, duoff = to_dev(pk), to_dev(ub), to_dev(um), to_dev(uoff)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for out_len, flag in ((utotal, 0), (utotal - 1, 8)):
        want, written = ds.want_run(uvals, um, (nu - 1,) if flag else ())
        buf = sentinel_buffer(ty, utotal + GUARD)
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(fl.load(), f"fl_{ty}_undelta_select")(w, dpk.data_ptr(), dub.data_ptr(), dum.data_ptr(), duoff.data_ptr(), buf.data_ptr(), out_len,
                                                           nu, err.data_ptr(), stream)
        assert rc == 0 and int(err.item()) == flag, (ty, out_len, rc, int(err.item()))
        got = to_np(buf, ty)
        assert np.array_equal(got[:utotal], np.where(written, want, sentinel_of(ty))), (ty, out_len)
        assert (got[utotal:] == sentinel_of(ty)).all(), (ty, out_len, "the guard was written")


@pytest.mark.parametrize("policy", gs.POLICIES)
@pytest.mark.parametrize("ty", TYS)
def test_policies_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Every kernel policy (forced waves / blocks per wavefront / prefetch: the kernel takes a wavefront's blocks one after the other,
    whatever the shape) gives the same bits; a non-default stream; an empty column; an all-empty mask with no output at all; columns of
    width-0 blocks with no packed bytes."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    L = lanes(ty)
    rng = np.random.default_rng(17200 + T)
    n = 131
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 17201)
    bases = dd.delta_bases(ty, n, 17202)
    vals = dd.decode(oracle, ty, blocks, bases)
    pk2 = values(ty, n * packed_len(ty, T // 2), 17203)
    vals2 = dd.decode_uniform(oracle, ty, T // 2, pk2, bases, n)
    m = dd.incoming_mask(n, 17204)
    s = torch.cuda.Stream()
    dcol, dbases, dpk2 = to_dev(col), to_dev(bases), to_dev(pk2)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        check(fl, lambda dm, **kw: fl.undelta_select_widths(dw, doff, dcol, dbases, dm, **kw), ty, vals, m, (ty, policy, "mixed"))
        check(fl, lambda dm, **kw: fl.undelta_select_widths(dw, doff, dcol, dbases, dm, check=False, **kw), ty, vals,
              bits_words(rng.random(n * 1024) < 0.5), (ty, policy, "mixed, 50 %"))
        check(fl, lambda dm, **kw: fl.Delta.undelta_select(T // 2, dpk2, dbases, dm, **kw), ty, vals2, m, (ty, policy, "uniform"))
    s.synchronize()
    # empty columns: nothing selected
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    ew, eo = torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0")
    em = torch.empty(0, dtype=torch.int32, device="cuda:0")
    for got in (fl.undelta_select_widths(ew, eo, empty, empty, em), fl.Delta.undelta_select(3, empty, empty, em)):
        assert got.numel() == 0
    # an all-empty mask: the total is 0, out == NULL with out_len == 0 is accepted and nothing is raised
    zm = torch.zeros(n * 32, dtype=torch.int32, device="cuda:0")
    assert fl.undelta_select_widths(dw, doff, dcol, dbases, zm).numel() == 0
    oo, _ = fl.mask_offsets(zm)
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(fl.load(), f"fl_{ty}_undelta_select_widths")(dw.data_ptr(), doff.data_ptr(), dcol.data_ptr(), dcol.numel() * (T // 8), dbases.data_ptr(),
                                                             zm.data_ptr(), oo.data_ptr(), None, 0, n, err.data_ptr(), stream)
    assert rc == 0 and int(err.item()) == 0
    # width-0 blocks, no packed bytes: lane l's T rows repeat base_l
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    vz = np.concatenate([oracle.untranspose(ty, np.tile(bases[k * L:(k + 1) * L], T)) for k in range(5)])
    for mz in (dd.incoming_mask(5, 17205, shift=3), dd.incoming_mask(5, 17206, shift=4), bits_words(rng.random(5 * 1024) < 0.5)):
        check(fl, lambda dm, **kw: fl.undelta_select_widths(z, zoff, empty, dbases[:5 * L], dm, **kw), ty, vz, mz, (ty, policy, "width 0"))
        check(fl, lambda dm, **kw: fl.Delta.undelta_select(0, empty, dbases[:5 * L], dm, **kw), ty, vz, mz,
              (ty, policy, "uniform width 0, n_blocks from the bases"))


@pytest.mark.parametrize("ty", TYS)
def test_chain_delta_range_then_delta_select(fl, oracle, sorted_columns, ty):
    """SELECT ts WHERE ts BETWEEN a AND b on a sorted, Delta-coded column: undelta_compare_range_widths -> undelta_select_widths(mask=..)
    equals v[hit_bits], and equals the device-materialised column (undelta_pack_widths(.., untranspose=True)) indexed by the same bits
    on the device, bit for bit."""
    import torch
    T = tbits(ty)
    v, widths, blocks, bases = sorted_columns[ty]
    n = len(blocks)
    off, col = dd.column_of(blocks, ty)
    dw, doff = torch.from_numpy(widths).cuda(), torch.from_numpy(off).cuda()
    dcol, dbases = to_dev(col), to_dev(bases)
    decoded = fl.undelta_pack_widths(dw, doff, dcol, dbases, untranspose=True)
    assert np.array_equal(to_np(decoded, ty), v)
    for a, b in ((int(v[2 * 1024 + 300]), int(v[7 * 1024 + 77])), (int(v[5 * 1024 + T]), int(v[5 * 1024 + 3 * T - 1])), (int(v[1023]), int(v[1024]))):
        m = fl.undelta_compare_range_widths(dw, doff, dcol, dbases, a, b)
        words = gs.got_mask(m)
        assert np.array_equal(words, dd.want_mask(v, a, b))
        want = check(fl, lambda dm, **kw: fl.undelta_select_widths(dw, doff, dcol, dbases, m, **kw), ty, v, words, (ty, a, b))
        hit = dd.hit_bits(v, a, b)
        assert want.size and np.array_equal(want, v[hit])
        dbits = torch.from_numpy(hit).cuda()
        indexed = decoded.view(getattr(torch, gs.SIGNED[ty]))[dbits].view(decoded.dtype)
        got = fl.undelta_select_widths(dw, doff, dcol, dbases, m)
        assert torch.equal(got.view(torch.uint8), indexed.contiguous().view(torch.uint8)), (ty, a, b, "the materialising path")
