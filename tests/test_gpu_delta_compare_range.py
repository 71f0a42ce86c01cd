"""GPU: undelta_compare_range / undelta_compare_range_widths -- interval predicates over DELTA-packed columns, chained through a mask --
against the mask numpy builds from the oracle's untranspose(undelta_pack(..)) per block (delta.rs:47-63, transpose.rs:17-22):
    hit = ((v - lo) mod 2^T) <= ((hi - lo) mod 2^T);   new: hit,  and: mask_in & hit,  or: mask_in | hit
in unfor_compare_range's layout (bit i of word i // 32 of block b, LSB first, i = the ORIGINAL row).  The expectation and the routes a
launch must take are computed from the definition (tests/delta_compare_range_data.py), never from the headers under test."""
import numpy as np
import pytest

import delta_compare_range_data as dd
from datagen import values
from oracle_lib import lanes, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TDT, TYS, got_mask, mixed_column, to_dev

pytestmark = pytest.mark.gpu

COMBINE = dd.COMBINE
PREFILL = 0x5A5A5A5A


def prefilled(n):
    import torch
    return torch.full((n * 32,), PREFILL, dtype=torch.int32, device="cuda:0")


def check_every_combiner(fl, call, n, vals, lo, hi, min_host, dmin, what):
    """`call(**kw)` -> the device mask: the three combiners out of place into a 0x5A-prefilled output (every block must be overwritten,
    the ones the incoming mask had already decided included), AND / OR in place, and NEW with a mask it must ignore"""
    for cb in COMBINE:
        want = dd.want_mask(vals, lo, hi, cb, min_host)
        args = dict(mask=dmin, combine=cb) if cb != "new" else {}
        got = got_mask(call(output=prefilled(n), **args))
        assert np.array_equal(got, want), (*what, cb, lo, hi)
        if cb != "new":
            inplace = dmin.clone()
            out = call(mask=inplace, combine=cb, output=inplace)
            assert out is inplace and np.array_equal(got_mask(inplace), want), (*what, cb, lo, hi, "in place")
            assert np.array_equal(got_mask(dmin), min_host)                  # out of place left mask_in alone
    got = got_mask(call(mask=dmin, combine="new"))
    assert np.array_equal(got, dd.want_mask(vals, lo, hi)), (*what, "new with a mask", lo, hi)


@pytest.mark.parametrize("ty", TYS)
def test_random_columns_every_route_every_combiner(fl, oracle, ty):
    """Random packed bytes (the chains wrap) under random, clustered and equal bases: every width 0..T, a ragged column of 263 blocks,
    and 1 / 2 / 3 / 5 blocks; full, wrapping, single-value intervals and bounds at each side of picked blocks' [cmin, cmax + reach]; the
    three combiners over incoming masks that mix random blocks with empty, full, one-bit-set and one-bit-clear ones (KEEP).  ALL, NONE,
    BASES and EACH occur under ONE interval of the two larger columns (the width-0 block with mixed bases is BASES), so one launch
    takes every path."""
    T = tbits(ty)
    rng = np.random.default_rng(9100 + T)
    four_routes = {}
    for n, widths in ((T + 1, np.arange(T + 1)), (263, rng.integers(0, T + 1, size=263)), (1, [T // 2]), (2, [3, T]), (3, [T, 0, 1]),
                      (5, [2, T - 1, 0, T, 5])):
        dw, doff, col, blocks = mixed_column(ty, widths, 11200 + n)
        bases = dd.delta_bases(ty, n, 11300 + n)
        dcol, dbases = to_dev(col), to_dev(bases)
        vals = dd.decode(oracle, ty, blocks, bases)
        picks = sorted({0, min(1, n - 1), min(2, n - 1), n // 3, n // 2, n - 1} | set(rng.integers(0, n, size=2).tolist()))
        ivs = dd.intervals_for(ty, widths, bases, picks)
        routes = [set(dd.column_verdicts(ty, lo, hi, bases, widths)) for lo, hi in ivs]
        four_routes[n] = any(r == {dd.EACH, dd.ALL, dd.NONE, dd.BASES} for r in routes)
        if n >= 10:                                                         # every interval that takes all four routes, and every third other
            ivs = [iv for q, (iv, r) in enumerate(zip(ivs, routes)) if len(r) == 4 or q % 3 == 0]
        else:
            ivs = ivs[::3]
        for q, (lo, hi) in enumerate(ivs):
            min_host = dd.incoming_mask(n, 11400 + n, shift=q)
            dmin = to_dev(min_host)
            if q % 4 == 0 or n < 10:
                check_every_combiner(fl, lambda **kw: fl.undelta_compare_range_widths(dw, doff, dcol, dbases, lo, hi, **kw), n, vals, lo, hi,
                                     min_host, dmin, (ty, n))
            else:                                                           # the other intervals: one combiner each, in turn
                cb = COMBINE[q % 3]
                args = dict(mask=dmin, combine=cb) if cb != "new" else {}
                got = got_mask(fl.undelta_compare_range_widths(dw, doff, dcol, dbases, lo, hi, output=prefilled(n), **args))
                assert np.array_equal(got, dd.want_mask(vals, lo, hi, cb, min_host)), (ty, n, cb, lo, hi)
    assert four_routes[T + 1] and four_routes[263], four_routes


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_every_width(fl, oracle, ty):
    """Delta.undelta_compare_range over a uniform-width column of 37 blocks at every (T, W): both sides of the read route's switch, W = 0
    (no packed bytes: BASES or decided) and W = T among them"""
    T = tbits(ty)
    N = 1 << T
    n = 37
    L = lanes(ty)
    for w in range(T + 1):
        pk = values(ty, n * packed_len(ty, w), 11500 + 64 * T + w)
        bases = dd.delta_bases(ty, n, 11600 + 64 * T + w)
        vals = dd.decode_uniform(oracle, ty, w, pk, bases, n)
        dpk, dbases = to_dev(pk), to_dev(bases)
        reach = T * ((1 << w) - 1)
        b5, b9 = int(bases[5 * L]), int(bases[9 * L])
        ivs = [(b5, (b5 + 6 + reach) % N), ((b5 + 7 + reach) % N, (b5 - 1) % N), ((b9 + (reach >> 1)) % N, (b9 + (reach >> 1)) % N),
               (b9, (b5 + (reach >> 1)) % N), ((b9 - 1) % N, (b9 - 2) % N)]
        min_host = dd.incoming_mask(n, 11700 + w, shift=w)
        dmin = to_dev(min_host)
        for q, (lo, hi) in enumerate(ivs):
            if q == w % len(ivs):
                check_every_combiner(fl, lambda **kw: fl.Delta.undelta_compare_range(w, dpk, dbases, lo, hi, n_blocks=n, **kw), n, vals, lo, hi,
                                     min_host, dmin, (ty, w))
            else:
                cb = COMBINE[(q + w) % 3]
                args = dict(mask=dmin, combine=cb) if cb != "new" else {}
                got = got_mask(fl.Delta.undelta_compare_range(w, dpk, dbases, lo, hi, output=prefilled(n), **args))
                assert np.array_equal(got, dd.want_mask(vals, lo, hi, cb, min_host)), (ty, w, cb, lo, hi)


@pytest.fixture(scope="module")
def sorted_columns(oracle):
    """ty -> the sorted column of 67 blocks, built once (the round trip through the oracle is asserted while it is built)"""
    return {ty: dd.sorted_column(oracle, ty, 67, 11800 + tbits(ty)) for ty in TYS}


@pytest.mark.parametrize("ty", TYS)
def test_sorted_columns_where_one_element_decides(fl, oracle, sorted_columns, ty):
    """A sorted column Delta-coded on the CPU (base = the predecessor in original order, width from the largest delta): narrow intervals
    whose ends are the values at a block's first and last row, at the first and last row of a T-bit group and of an R-row piece, and
    long ones that end there -- so ONE row decides a mask bit at every place where the kernel joins pieces.  Mixed-width form, and the
    uniform form of the same blocks repacked at the widest width."""
    T = tbits(ty)
    L = lanes(ty)
    v, widths, blocks, bases = sorted_columns[ty]
    n = len(blocks)
    off, col = dd.column_of(blocks, ty)
    import torch
    dw, doff = torch.from_numpy(widths).cuda(), torch.from_numpy(off).cuda()
    dcol, dbases = to_dev(col), to_dev(bases)
    wmax = int(widths.max())
    upk = np.concatenate([oracle.pack(ty, wmax, oracle.delta(ty, oracle.transpose(ty, v[b * 1024:(b + 1) * 1024]), bases[b * L:(b + 1) * L]))
                          for b in range(n)])
    assert np.array_equal(dd.decode_uniform(oracle, ty, wmax, upk, bases, n), v)
    dupk = to_dev(upk)
    rows = dd.edge_rows(ty)
    ivs = []
    for k, r in enumerate(rows):
        b = (5 + 11 * k) % n
        p = b * 1024 + r
        q = min(p + (T // 8 if k % 2 else 3 * 1024 + 17), n * 1024 - 1)
        ivs += [(int(v[p]), int(v[p])), (int(v[p]), int(v[q])), (int(v[max(p - 1, 0)]), int(v[q]))]
    ivs += [(int(v[9 * 1024]), int(v[12 * 1024 - 1])), (int(v[9 * 1024 - 1]), int(v[12 * 1024])), (int(v[40 * 1024 + 500]), int(v[3 * 1024 + 7]))]
    ivs = list(dict.fromkeys(ivs))
    seen = set()
    for q, (lo, hi) in enumerate(ivs):
        seen |= set(dd.column_verdicts(ty, lo, hi, bases, widths))
        min_host = dd.incoming_mask(n, 11900 + T, shift=q)
        dmin = to_dev(min_host)
        cb = COMBINE[q % 3]
        args = dict(mask=dmin, combine=cb) if cb != "new" else {}
        want = dd.want_mask(v, lo, hi, cb, min_host)
        got = got_mask(fl.undelta_compare_range_widths(dw, doff, dcol, dbases, lo, hi, output=prefilled(n), **args))
        assert np.array_equal(got, want), (ty, "mixed", cb, lo, hi)
        got = got_mask(fl.Delta.undelta_compare_range(wmax, dupk, dbases, lo, hi, output=prefilled(n), **args))
        assert np.array_equal(got, want), (ty, "uniform", cb, lo, hi)
    assert {dd.ALL, dd.NONE, dd.EACH} <= seen, (ty, seen)                    # a sorted column: most blocks lie wholly inside or outside


@pytest.mark.parametrize("ty", TYS)
def test_skipped_blocks_keep_their_words_and_raise_their_bits(fl, oracle, ty):
    """A block with a width > T, one with a misaligned offset, one outside the packed column: the kernel checks them itself, err_flag
    holds the three bits, the skipped blocks' mask words keep their prefill, every other block is right, and check=True raises."""
    import ctypes
    import torch
    T = tbits(ty)
    esz = T // 8
    n = 40
    rng = np.random.default_rng(12000 + T)
    widths = rng.integers(1, T + 1, size=n).astype(np.uint8)
    dw, doff, col, blocks = mixed_column(ty, widths, 12001)
    bases = dd.delta_bases(ty, n, 12002)
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
    lo = int(bases[20 * lanes(ty)])
    hi = (lo + (1 << (T - 2))) % (1 << T)
    min_host = dd.incoming_mask(n, 12003)
    dmin = to_dev(min_host)
    skipped = np.zeros(n, dtype=bool)
    skipped[[5, 7, 11]] = True
    for code, cb in enumerate(COMBINE):
        mask = prefilled(n)
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(lib, f"fl_{ty}_undelta_compare_range_widths")(dbw.data_ptr(), dboff.data_ptr(), dcol.data_ptr(), col.size * esz, dbases.data_ptr(),
                                                                  lo, hi, code, dmin.data_ptr() if code else None, n, mask.data_ptr(), err.data_ptr(), stream)
        assert rc == 0
        assert int(err.item()) == 1 | 4 | 8, (ty, cb, int(err.item()))
        g = got_mask(mask).reshape(n, 32)
        w = dd.want_mask(vals, lo, hi, cb, min_host).reshape(n, 32)
        assert (g[skipped] == PREFILL).all(), (ty, cb, "a skipped block was written")
        assert np.array_equal(g[~skipped], w[~skipped]), (ty, cb)
    for status, w_, o_ in ((1, dbw, doff), (4, dw, torch.from_numpy(np.where(np.arange(n) == 5, off + 8, off)).cuda()),
                           (6, dw, torch.from_numpy(np.where(np.arange(n) == 11, off + (1 << 40), off)).cuda())):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.undelta_compare_range_widths(w_, o_, dcol, dbases, lo, hi, mask=dmin, combine="and")
        assert ei.value.status == status, (ty, status)


@pytest.mark.parametrize("policy", [0, 2 + 256 * 4 + 65536 * 4 + (1 << 24), 2 + 256 * 6 + 65536 * 3, 2 + 256 * 4 + 65536 * 12 + (1 << 24)])
@pytest.mark.parametrize("ty", TYS)
def test_policies_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Forced waves / blocks per wavefront / prefetch (the kernel takes a wavefront's blocks one after the other, whatever the shape), a
    non-default stream, an empty column and columns of width-0 blocks with no packed bytes."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    N = 1 << T
    L = lanes(ty)
    rng = np.random.default_rng(12100 + T)
    n = 131
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 12101)
    bases = dd.delta_bases(ty, n, 12102)
    vals = dd.decode(oracle, ty, blocks, bases)
    b = int(bases[(n // 3) * L])
    lo, hi = (b - (N >> 3)) % N, (b + (N >> 2)) % N
    pk2 = values(ty, n * packed_len(ty, T // 2), 12103)
    vals2 = dd.decode_uniform(oracle, ty, T // 2, pk2, bases, n)
    min_host = dd.incoming_mask(n, 12104)
    s = torch.cuda.Stream()
    dcol, dbases, dpk2, dmin = to_dev(col), to_dev(bases), to_dev(pk2), to_dev(min_host)
    torch.cuda.synchronize()
    for cb in COMBINE:
        args = dict(mask=dmin, combine=cb) if cb != "new" else {}
        inplace = dmin.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            m1 = fl.undelta_compare_range_widths(dw, doff, dcol, dbases, lo, hi, check=False, output=prefilled(n), **args)
            m2 = fl.Delta.undelta_compare_range(T // 2, dpk2, dbases, hi, lo, output=prefilled(n), **args)
            if cb != "new":
                fl.undelta_compare_range_widths(dw, doff, dcol, dbases, lo, hi, mask=inplace, combine=cb, output=inplace, check=False)
        s.synchronize()
        assert np.array_equal(got_mask(m1), dd.want_mask(vals, lo, hi, cb, min_host)), (ty, policy, cb)
        assert np.array_equal(got_mask(m2), dd.want_mask(vals2, hi, lo, cb, min_host)), (ty, policy, cb, "uniform")
        if cb != "new":
            assert np.array_equal(got_mask(inplace), dd.want_mask(vals, lo, hi, cb, min_host)), (ty, policy, cb, "in place")
    # empty columns
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    nomask = torch.empty(0, dtype=torch.int32, device="cuda:0")
    ew, eo = torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0")
    assert fl.undelta_compare_range_widths(ew, eo, empty, empty, 1, 2).numel() == 0
    assert fl.undelta_compare_range_widths(ew, eo, empty, empty, 1, 2, mask=nomask, combine="and").numel() == 0
    assert fl.Delta.undelta_compare_range(3, empty, empty, 1, 2).numel() == 0
    # width-0 blocks, no packed bytes: lane l's T rows repeat base_l
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    vz = np.concatenate([oracle.untranspose(ty, np.tile(bases[k * L:(k + 1) * L], T)) for k in range(5)])
    mz = dd.incoming_mask(5, 12105, shift=1)
    b1 = int(bases[L + 1])
    for lo0, hi0 in ((lo, hi), (b1, (b1 + 2) % N), (int(bases[3]), int(bases[3]))):
        got = got_mask(fl.undelta_compare_range_widths(z, zoff, empty, dbases[:5 * L], lo0, hi0, mask=to_dev(mz), combine="or"))
        assert np.array_equal(got, dd.want_mask(vz, lo0, hi0, "or", mz)), (ty, policy, "width 0")
        got = got_mask(fl.Delta.undelta_compare_range(0, empty, dbases[:5 * L], lo0, hi0, mask=to_dev(mz), combine="and"))
        assert np.array_equal(got, dd.want_mask(vz, lo0, hi0, "and", mz)), (ty, policy, "uniform width 0")
        got = got_mask(fl.Delta.undelta_compare_range(0, empty, dbases[:5 * L], lo0, hi0))
        assert np.array_equal(got, dd.want_mask(vz, lo0, hi0)), (ty, policy, "uniform width 0, new, n_blocks from the bases")


def test_chain_delta_date_then_for_predicate_then_aggregate(fl, oracle, sorted_columns):
    """WHERE shipdate BETWEEN a AND b AND discount BETWEEN 5 AND 7, then COUNT / SUM / MIN / MAX of quantity (TPC-H Q6's shape) with the
    date column DELTA-coded: undelta_compare_range_widths -> unfor_compare_range_widths(mask=.., combine="and") ->
    unfor_aggregate_widths equals the same chain run on the materialised date column (decoded to original order on the device, then
    FoR-packed by the library's own encoder), and numpy."""
    import torch
    ty = "u32"
    v, widths, blocks, bases = sorted_columns[ty]
    n = len(blocks)
    off, col = dd.column_of(blocks, ty)
    dw, doff = torch.from_numpy(widths).cuda(), torch.from_numpy(off).cuda()
    dcol, dbases = to_dev(col), to_dev(bases)
    rng = np.random.default_rng(12200)
    discount = rng.integers(0, 11, size=n * 1024).astype(np.uint8)
    discount[17 * 1024:19 * 1024] = 6                                        # blocks the second predicate decides
    discount[30 * 1024:31 * 1024] = 9
    quantity = rng.integers(1, 51, size=n * 1024).astype(np.uint16)

    def for_column(ty_, dv):
        mins, maxs = fl.BitPacking.block_min_max(dv)
        w = fl.for_widths(mins, maxs)
        o, total = fl.widths_to_offsets(ty_, w)
        pk = torch.zeros(max(int(total.item()) // (tbits(ty_) // 8), 1), dtype=getattr(torch, TDT[ty_]), device="cuda:0")
        fl.for_pack_widths(w, o, dv, mins, pk)
        return w, o, pk, mins

    decoded = fl.undelta_pack_widths(dw, doff, dcol, dbases, untranspose=True)
    assert np.array_equal(decoded.cpu().numpy().view(np.uint32), v)
    date_for, disc, qty = for_column("u32", decoded), for_column("u8", to_dev(discount)), for_column("u16", to_dev(quantity))
    a, b = int(v[15 * 1024 + 300]), int(v[33 * 1024 + 77])
    results = []
    for head in (lambda: fl.undelta_compare_range_widths(dw, doff, dcol, dbases, a, b), lambda: fl.unfor_compare_range_widths(*date_for, a, b)):
        m = head()
        out = fl.unfor_compare_range_widths(*disc, 5, 7, mask=m, combine="and", output=m)
        assert out is m
        result, slots = fl.unfor_aggregate_widths(*qty, mask=m)
        results.append((got_mask(m), result.cpu().numpy().view(np.uint64), slots.cpu().numpy().view(np.uint64)))
    for x, y in zip(*results):
        assert np.array_equal(x, y)
    keep = dd.hit_bits(v, a, b) & (discount >= 5) & (discount <= 7)
    assert np.array_equal(results[0][0], np.packbits(keep, bitorder="little").view(np.int32))
    kept = quantity[keep].astype(np.uint64)
    assert kept.size > 2048
    assert [int(x) for x in results[0][1]] == [kept.size, int(kept.sum()), int(kept.min()), int(kept.max())]
