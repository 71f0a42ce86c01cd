"""GPU: unfor_aggregate / unfor_aggregate_widths / aggregate_reduce -- COUNT / SUM / MIN / MAX of a FoR-packed column under a selection
mask -- against the oracle's unfor_pack per block (ffor.rs:38-50) reduced with numpy under the mask's bits: per block
{count, wrapping uint64 sum, min, max} (nothing kept: {0, 0, 2^64 - 1, 0}), and numpy's combination of the blocks.  Bit-exact."""
import ctypes

import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import (IDENTITY, POLICIES, SENTINEL, SIGNED, TDT, TYS, BackgroundLoad, combine, expected_blocks, mask_set, mask_words,
                         mixed_column, sentinel_slots, to_dev, u64_of)

pytestmark = pytest.mark.gpu


def decodes_something(bits, widths, n):
    """some block has a non-empty mask AND a non-zero width: the decode path cannot be skipped wholesale"""
    kept = np.ones(n, bool) if bits is None else bits.reshape(n, 1024).any(axis=1)
    return bool((kept & (np.asarray(widths) > 0)).any())


def check_slots(buf, n, result, want, what):
    got = u64_of(buf)
    assert np.array_equal(got[:n * 4].reshape(n, 4), want), what
    assert (got[n * 4:] == SENTINEL).all(), (what, "the guard was written")
    assert np.array_equal(u64_of(result), combine(want)), (what, "result")


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_columns_every_mask(fl, oracle, ty):
    """Every width 0..T plus a ragged random tail (263 blocks); random wrapping per-block references and one broadcast reference; the
    whole mask set and no mask; bit-exact, slots pre-filled with a sentinel, the guard behind them untouched."""
    T = tbits(ty)
    rng = np.random.default_rng(16100 + T)
    n = 263
    widths = np.concatenate([np.arange(T + 1), rng.integers(0, T + 1, size=n - (T + 1))])
    dw, doff, col, blocks = mixed_column(ty, widths, 16200 + T)
    dcol = to_dev(col)
    refs = values(ty, n, 16300 + T)
    masks = mask_set(n, rng, with_none=True)
    for rname, r_host, dref in (("per block", refs, to_dev(refs)), ("broadcast", np.full(n, refs[3], dtype=refs.dtype), to_dev(refs[3:4]))):
        vals = np.concatenate([oracle.unfor_pack(ty, w, pk, r_host[b]) for b, (w, pk) in enumerate(blocks)])
        for name, bits in masks.items():
            assert name == "zeros" or decodes_something(bits, widths, n)
            want = expected_blocks(vals, bits)
            if ty == "u64" and name in ("ones", "no mask"):
                assert (want[:, 1] < want[:, 3]).any()                      # a sum smaller than its block's max: it wrapped
            buf, slots = sentinel_slots(n)
            result, got = fl.unfor_aggregate_widths(dw, doff, dcol, dref, None if bits is None else mask_words(bits), block_aggs=slots)
            assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (n, 4) and tuple(result.shape) == (4,)
            check_slots(buf, n, result, want, (ty, rname, name))
        # the convenience path: the slots allocated inside the call
        result, got = fl.unfor_aggregate_widths(dw, doff, dcol, dref, mask_words(masks["random 1 %"]))
        want = expected_blocks(vals, masks["random 1 %"])
        assert np.array_equal(u64_of(got), want) and np.array_equal(u64_of(result), combine(want)), (ty, rname, "block_aggs=None")


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_form(fl, oracle, ty):
    T = tbits(ty)
    rng = np.random.default_rng(16400 + T)
    n = 61
    masks = mask_set(n, rng, with_none=True)
    for w in sorted({0, 1, 3, T // 2, T - 1, T}):
        pk = values(ty, n * packed_len(ty, w), 16500 + 64 * T + w)
        refs = values(ty, n, 16600 + 64 * T + w)
        vals = oracle.batch("unfor_pack", ty, w, pk, aux=refs, n_blocks=n)
        plain = oracle.batch("unpack", ty, w, pk, n_blocks=n)
        dpk, drefs = to_dev(pk), to_dev(refs)
        for name, bits in masks.items():
            assert name == "zeros" or w == 0 or decodes_something(bits, np.full(n, w), n)
            dm = None if bits is None else mask_words(bits)
            buf, slots = sentinel_slots(n)
            result, _ = fl.FoR.unfor_aggregate(w, dpk, drefs, dm, n_blocks=n, block_aggs=slots)
            check_slots(buf, n, result, expected_blocks(vals, bits), (ty, w, name))
            # a plain bit-packed column: one zero reference
            buf, slots = sentinel_slots(n)
            result, got = fl.FoR.unfor_aggregate(w, dpk, 0, dm, n_blocks=n, block_aggs=slots)
            check_slots(buf, n, result, expected_blocks(plain, bits), (ty, w, name, "reference 0"))
            if bits is None:                                                # an older, independently tested kernel
                sums = fl.BitPacking.unpack_block_sums(w, dpk, n_blocks=n)
                assert np.array_equal(u64_of(got)[:, 1], u64_of(sums)), (ty, w, "unpack_block_sums")


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, (1 << 20) + 1])
def test_aggregate_reduce_against_numpy(fl, n):
    import torch
    rng = np.random.default_rng(16700 + n % 1000)
    lib = fl.load()
    for kind in ("identity", "dense", "half"):
        if kind == "identity":
            slots = np.tile(IDENTITY, (n, 1))
        else:
            slots = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)   # the sums wrap
            if kind == "half":
                slots[rng.random(n) < 0.5] = IDENTITY
        want = combine(slots)
        d = to_dev(slots.view(np.int64).reshape(-1)).view(n, 4)
        got = fl.aggregate_reduce(d)
        assert got.dtype == torch.int64 and tuple(got.shape) == (4,)
        assert np.array_equal(u64_of(got), want), (n, kind)
        # twice into the same result, which starts as garbage: the init launch makes each call stand alone
        result = to_dev(np.full(4, SENTINEL, dtype=np.uint64).view(np.int64))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            assert lib.fl_aggregate_reduce(d.data_ptr(), n, result.data_ptr(), stream) == 0
            assert np.array_equal(u64_of(result), want), (n, kind, "same result twice")
    # no blocks: the identity
    assert np.array_equal(u64_of(fl.aggregate_reduce(torch.empty((0, 4), dtype=torch.int64, device="cuda:0"))), IDENTITY)


@pytest.mark.parametrize("ty", TYS)
def test_filter_then_aggregate_end_to_end(fl, oracle, ty):
    """SELECT COUNT(*), SUM(y), MIN(y), MAX(y) WHERE x < k: the mask from unfor_compare_widths on column x, the aggregate of column y"""
    T = tbits(ty)
    rng = np.random.default_rng(16800 + T)
    n = 97
    ywidths = rng.integers(0, T + 1, size=n)
    xw, xoff, xcol, xblocks = mixed_column(ty, rng.integers(0, T + 1, size=n), 16801)
    yw, yoff, ycol, yblocks = mixed_column(ty, ywidths, 16802)
    xr, yr = values(ty, n, 16803), values(ty, n, 16804)
    x = np.concatenate([oracle.unfor_pack(ty, w, pk, xr[b]) for b, (w, pk) in enumerate(xblocks)])
    y = np.concatenate([oracle.unfor_pack(ty, w, pk, yr[b]) for b, (w, pk) in enumerate(yblocks)])
    decoded = 0
    for k in (int(xr[n // 2]), (1 << T) // 3, 0, (1 << T) - 1):
        bits = x < np.array(k, dtype=np.uint64).astype(x.dtype)
        decoded += decodes_something(bits, ywidths, n)
        mask = fl.unfor_compare_widths(xw, xoff, to_dev(xcol), to_dev(xr), "<", k)
        result, slots = fl.unfor_aggregate_widths(yw, yoff, to_dev(ycol), to_dev(yr), mask)
        want = expected_blocks(y, bits)
        assert np.array_equal(u64_of(slots), want), (ty, k)
        assert np.array_equal(u64_of(result), combine(want)), (ty, k)
    assert decoded >= 3                                                     # (k = 0 keeps nothing)


def raw_aggregate_widths(fl, ty, dw, doff, dcol, drefs, dm, slots):
    """The C ABI call with its own err_flag; returns the flag's value."""
    import torch
    esz = tbits(ty) // 8
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(fl.load(), f"fl_{ty}_unfor_aggregate_widths")(dw.data_ptr(), doff.data_ptr(), dcol.data_ptr(), dcol.numel() * esz, drefs.data_ptr(), 1,
                                                              dm.data_ptr(), dw.numel(), slots.data_ptr(), err.data_ptr(), stream)
    assert rc == 0
    return int(err.item())


@pytest.mark.parametrize("ty", TYS)
def test_device_errors_flag_and_give_the_identity(fl, oracle, ty):
    """A block with a width > T, one with a misaligned offset, one outside the packed column: its bit is raised, its slot holds the
    identity (not the sentinel: the slot feeds a reduction), every other slot is right, the result combines the valid blocks;
    check=True raises."""
    import torch
    T = tbits(ty)
    n = 40
    rng = np.random.default_rng(16900 + T)
    widths = rng.integers(1, T + 1, size=n).astype(np.uint8)
    dw, doff, col, blocks = mixed_column(ty, widths, 16901)
    refs = values(ty, n, 16902)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    bits = rng.random(n * 1024) < 0.2
    assert decodes_something(bits, widths, n)
    dm = mask_words(bits)
    off = doff.cpu().numpy()
    bad_w = widths.copy()
    bad_w[7] = T + 1
    boff = off.copy()
    boff[5] += 8
    boff[11] += 1 << 40
    dcol, drefs = to_dev(col), to_dev(refs)
    buf, slots = sentinel_slots(n)
    flag = raw_aggregate_widths(fl, ty, torch.from_numpy(bad_w).cuda(), torch.from_numpy(boff).cuda(), dcol, drefs, dm, slots)
    assert flag == 1 | 4 | 8, (ty, flag)
    want = expected_blocks(vals, bits)
    for b in (5, 7, 11):
        want[b] = IDENTITY
    check_slots(buf, n, fl.aggregate_reduce(slots), want, ty)
    for status, w_, o_ in ((1, torch.from_numpy(bad_w).cuda(), doff), (4, dw, torch.from_numpy(np.where(np.arange(n) == 5, off + 8, off)).cuda()),
                           (6, dw, torch.from_numpy(np.where(np.arange(n) == 11, off + (1 << 40), off)).cuda())):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_aggregate_widths(w_, o_, dcol, drefs, dm)
        assert ei.value.status == status, (ty, status)


@pytest.mark.parametrize("policy", POLICIES + [8 << 25, 12 << 25, 31 << 25, 2 + (8 << 25)])
@pytest.mark.parametrize("ty", TYS)
def test_policies_windows_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Kernel policies 0 / 1 / 2 (and forced waves / blocks per wavefront / prefetch), the tile-map windows 2^8 / 2^12 / whole column,
    a non-default stream, an empty column and a column of width-0 blocks with no packed bytes: identical results."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    rng = np.random.default_rng(17000 + T)
    n = 1031 if policy >> 25 else 131                                       # more than one 2^8-block window
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 17001)
    refs = values(ty, n, 17002)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    pk2 = values(ty, n * packed_len(ty, T // 2), 17003)
    vals2 = oracle.batch("unfor_pack", ty, T // 2, pk2, aux=refs, n_blocks=n)
    dcol, drefs, dpk2 = to_dev(col), to_dev(refs), to_dev(pk2)
    s = torch.cuda.Stream()
    for name, bits in mask_set(n, rng, full=False, with_none=True).items():
        assert name == "zeros" or decodes_something(bits, widths, n)
        dm = None if bits is None else mask_words(bits)
        (buf1, slots1), (buf2, slots2) = sentinel_slots(n), sentinel_slots(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            r1, _ = fl.unfor_aggregate_widths(dw, doff, dcol, drefs, dm, block_aggs=slots1, check=False)
            r2, _ = fl.FoR.unfor_aggregate(T // 2, dpk2, drefs, dm, block_aggs=slots2)
        s.synchronize()
        check_slots(buf1, n, r1, expected_blocks(vals, bits), (ty, policy, name))
        check_slots(buf2, n, r2, expected_blocks(vals2, bits), (ty, policy, name, "uniform"))
    # empty columns: the identity
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    no_mask = torch.empty(0, dtype=torch.int32, device="cuda:0")
    for m in (no_mask, None):
        result, slots = fl.unfor_aggregate_widths(torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0"),
                                                  empty, drefs[:1], m)
        assert tuple(slots.shape) == (0, 4) and np.array_equal(u64_of(result), IDENTITY)
        result, slots = fl.FoR.unfor_aggregate(3, empty, 0, m)
        assert tuple(slots.shape) == (0, 4) and np.array_equal(u64_of(result), IDENTITY)
    # width-0 blocks, no packed bytes at all: every value is its block's reference
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    bits = rng.random(5 * 1024) < 0.4
    for b_ in (bits, None):
        want = expected_blocks(np.repeat(refs[:5], 1024), b_)
        dm = None if b_ is None else mask_words(b_)
        result, slots = fl.unfor_aggregate_widths(z, zoff, empty, drefs[:5], dm)
        assert np.array_equal(u64_of(slots), want) and np.array_equal(u64_of(result), combine(want)), (ty, policy, "width 0")
        result, slots = fl.FoR.unfor_aggregate(0, empty, drefs[:5], dm, n_blocks=5)
        assert np.array_equal(u64_of(slots), want) and np.array_equal(u64_of(result), combine(want)), (ty, policy, "uniform width 0")


@pytest.mark.parametrize("ty", ["u32", "u8"])
def test_at_scale_under_load_equals_the_composition(fl, ty):
    """500 037 blocks, a random mask at 10 %, a second stream keeping the chip busy: equal, on the device, to the composition the feature
    is defined by -- unfor_pack_widths' output viewed [n, 1024] and reduced under the expanded mask with torch (int64 sums wrap as
    uint64 ones do; these two types' min / max fit int64)."""
    import torch
    T = tbits(ty)
    esz = T // 8
    tdt = getattr(torch, TDT[ty])
    n = 500_037
    lib = fl.load()
    load = BackgroundLoad(fl)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(17100 + T)
    widths = torch.randint(0, T + 1, (n,), generator=g, device="cuda:0").to(torch.uint8)
    offsets, total_bytes = fl.widths_to_offsets(ty, widths)
    pbytes = max(int(total_bytes.item()), 16)
    col = torch.empty(pbytes // esz, dtype=tdt, device="cuda:0")
    assert lib.fl_fill_random(col.data_ptr(), pbytes & ~7, 17101, None) == 0
    refs = torch.empty((n + 7) & ~7, dtype=tdt, device="cuda:0")
    assert lib.fl_fill_random(refs.data_ptr(), (refs.numel() * esz) & ~7, 17102, None) == 0
    refs = refs[:n]
    bits = torch.rand(n * 1024, generator=g, device="cuda:0") < 0.1
    w64 = (bits.view(-1, 32).to(torch.int64) << torch.arange(32, device="cuda:0")).sum(dim=1)
    mask = torch.where(w64 >= 1 << 31, w64 - (1 << 32), w64).to(torch.int32)
    del w64
    bits = bits.view(n, 1024)
    assert bool((bits.any(dim=1) & (widths > 0)).any())                     # the decode path cannot be skipped wholesale
    torch.cuda.synchronize()
    load.refill()
    full = fl.unfor_pack_widths(widths, offsets, col, refs)
    load.refill()
    result, slots = fl.unfor_aggregate_widths(widths, offsets, col, refs, mask)
    torch.cuda.current_stream().synchronize()
    load.drain()
    v = full.view(getattr(torch, SIGNED[ty])).view(n, 1024).to(torch.int64) & ((1 << T) - 1)   # zero-extended
    del full
    zero = torch.zeros((), dtype=torch.int64, device="cuda:0")
    count = bits.sum(dim=1)
    want = torch.stack([count, torch.where(bits, v, zero).sum(dim=1),
                        torch.where(count > 0, torch.where(bits, v, torch.full_like(zero, 1 << 62)).amin(dim=1), torch.full_like(zero, -1)),
                        torch.where(bits, v, zero).amax(dim=1)], dim=1)
    assert torch.equal(slots, want), ty
    assert bool((count > 0).any())                                          # (an empty block's min is -1 as int64: kept out of the minimum)
    total = torch.stack([want[:, 0].sum(), want[:, 1].sum(), torch.where(count > 0, want[:, 2], torch.full_like(zero, 1 << 62)).min(),
                         want[:, 3].max()])
    assert torch.equal(result, total), ty
