"""GPU: mask_offsets / unfor_select / unfor_select_widths -- decode only the rows a selection mask keeps -- against the oracle's
unfor_pack per block (ffor.rs:38-50) indexed by the mask's bits with numpy: out = concat over blocks of values[bits], in column order."""
import ctypes

import numpy as np
import pytest

from datagen import values
from oracle_lib import packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import GUARD, POLICIES, SIGNED, TDT, TYS, BackgroundLoad, mask_set, mask_words, mixed_column, sentinel_buffer, sentinel_of, to_dev, to_np

pytestmark = pytest.mark.gpu


def check_select(ty, got_buf, total_dev, vals, bits, what):
    """got_buf: the sentinel-filled output (kept values, then GUARD untouched sentinels)"""
    want = vals[bits]
    assert int(total_dev.item()) == want.size, (what, int(total_dev.item()), want.size)
    got = to_np(got_buf, ty)
    assert np.array_equal(got[:want.size], want), what
    assert (got[want.size:] == sentinel_of(ty)).all(), (what, "the guard was written")


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_columns_every_mask(fl, oracle, ty):
    """Every width 0..T plus a ragged random tail (263 blocks); random wrapping per-block references and one broadcast reference; the
    whole mask set; bit-exact, and the sentinel guard behind `total` untouched."""
    T = tbits(ty)
    rng = np.random.default_rng(14100 + T)
    n = 263
    widths = np.concatenate([np.arange(T + 1), rng.integers(0, T + 1, size=n - (T + 1))])
    dw, doff, col, blocks = mixed_column(ty, widths, 14200 + T)
    dcol = to_dev(col)
    refs = values(ty, n, 14300 + T)
    masks = mask_set(n, rng)
    for rname, r_host, dref in (("per block", refs, to_dev(refs)), ("broadcast", np.full(n, refs[3], dtype=refs.dtype), to_dev(refs[3:4]))):
        vals = np.concatenate([oracle.unfor_pack(ty, w, pk, r_host[b]) for b, (w, pk) in enumerate(blocks)])
        for name, bits in masks.items():
            dm = mask_words(bits)
            oo, total = fl.mask_offsets(dm)
            buf = sentinel_buffer(ty, int(bits.sum()) + GUARD)
            out = fl.unfor_select_widths(dw, doff, dcol, dref, dm, out_offsets=oo, total=total, output=buf)
            assert out.data_ptr() == buf.data_ptr()
            check_select(ty, buf, total, vals, bits, (ty, rname, name))
        # the convenience path: offsets and the output sized inside the call
        bits = masks["random 1 %"]
        got = fl.unfor_select_widths(dw, doff, dcol, dref, mask_words(bits))
        assert np.array_equal(to_np(got, ty), vals[bits]), (ty, rname, "output=None")


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_form(fl, oracle, ty):
    T = tbits(ty)
    rng = np.random.default_rng(14400 + T)
    n = 61
    masks = mask_set(n, rng)
    for w in sorted({0, 1, 3, T // 2, T - 1, T}):
        pk = values(ty, n * packed_len(ty, w), 14500 + 64 * T + w)
        refs = values(ty, n, 14600 + 64 * T + w)
        vals = oracle.batch("unfor_pack", ty, w, pk, aux=refs, n_blocks=n)
        dpk, drefs = to_dev(pk), to_dev(refs)
        for name, bits in masks.items():
            dm = mask_words(bits)
            oo, total = fl.mask_offsets(dm)
            buf = sentinel_buffer(ty, int(bits.sum()) + GUARD)
            fl.FoR.unfor_select(w, dpk, drefs, dm, out_offsets=oo, total=total, n_blocks=n, output=buf)
            check_select(ty, buf, total, vals, bits, (ty, w, name))
        # a plain bit-packed column: one zero reference
        bits = masks["random 50 %"]
        got = fl.FoR.unfor_select(w, dpk, 0, mask_words(bits), n_blocks=n)
        plain = oracle.batch("unpack", ty, w, pk, n_blocks=n)
        assert np.array_equal(to_np(got, ty), plain[bits]), (ty, w, "reference 0")


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, (1 << 20) + 1])
def test_mask_offsets_against_cumsum(fl, n):
    import torch
    rng = np.random.default_rng(14700 + n % 1000)
    for density in (0.0, 0.002, 0.5, 1.0):
        if density in (0.0, 1.0):
            words = np.full(n * 32, 0 if density == 0.0 else -1, dtype=np.int32)
        else:
            # random words thinned by ANDing: dense = one draw (50 %), sparse = mostly empty words
            words = rng.integers(0, 1 << 32, size=n * 32, dtype=np.uint64).astype(np.uint32)
            if density < 0.5:
                words &= np.where(rng.random(n * 32) < 0.004, np.uint32(0xFFFFFFFF), np.uint32(0)).astype(np.uint32)
            words = words.view(np.int32)
        pop = np.unpackbits(words.view(np.uint8)).reshape(n, 1024).sum(axis=1, dtype=np.int64)
        oo, total = fl.mask_offsets(to_dev(words))
        assert oo.dtype == torch.int64 and total.dtype == torch.int64 and total.numel() == 1
        want = np.concatenate([[0], np.cumsum(pop)[:-1]])
        assert np.array_equal(oo.cpu().numpy(), want), (n, density)
        assert int(total.item()) == int(pop.sum()), (n, density)


@pytest.mark.parametrize("ty", TYS)
def test_filter_then_select_end_to_end(fl, oracle, ty):
    """SELECT y WHERE x < k: the mask from unfor_compare_widths on column x, the values from column y"""
    T = tbits(ty)
    rng = np.random.default_rng(14800 + T)
    n = 97
    xw, xoff, xcol, xblocks = mixed_column(ty, rng.integers(0, T + 1, size=n), 14801)
    yw, yoff, ycol, yblocks = mixed_column(ty, rng.integers(0, T + 1, size=n), 14802)
    xr, yr = values(ty, n, 14803), values(ty, n, 14804)
    x = np.concatenate([oracle.unfor_pack(ty, w, pk, xr[b]) for b, (w, pk) in enumerate(xblocks)])
    y = np.concatenate([oracle.unfor_pack(ty, w, pk, yr[b]) for b, (w, pk) in enumerate(yblocks)])
    for k in (int(xr[n // 2]), (1 << T) // 3, 0, (1 << T) - 1):
        mask = fl.unfor_compare_widths(xw, xoff, to_dev(xcol), to_dev(xr), "<", k)
        got = fl.unfor_select_widths(yw, yoff, to_dev(ycol), to_dev(yr), mask)
        assert np.array_equal(to_np(got, ty), y[x < np.array(k, dtype=np.uint64).astype(x.dtype)]), (ty, k)


def raw_select_widths(fl, ty, dw, doff, dcol, drefs, dm, oo, buf, out_len):
    """The C ABI call with its own err_flag; returns the flag's value."""
    import torch
    esz = tbits(ty) // 8
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(fl.load(), f"fl_{ty}_unfor_select_widths")(dw.data_ptr(), doff.data_ptr(), dcol.data_ptr(), dcol.numel() * esz, drefs.data_ptr(), 1,
                                                           dm.data_ptr(), oo.data_ptr(), buf.data_ptr(), out_len, dw.numel(), err.data_ptr(), stream)
    assert rc == 0
    return int(err.item())


@pytest.mark.parametrize("ty", TYS)
def test_device_errors_skip_and_flag(fl, oracle, ty):
    """A block with a width > T, one with a misaligned offset, one outside the packed column: its bit is raised, its output slots keep
    the sentinel, every other block is right; check=True raises."""
    import torch
    T = tbits(ty)
    n = 40
    rng = np.random.default_rng(14900 + T)
    widths = rng.integers(1, T + 1, size=n).astype(np.uint8)
    dw, doff, col, blocks = mixed_column(ty, widths, 14901)
    refs = values(ty, n, 14902)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    bits = rng.random(n * 1024) < 0.2
    dm = mask_words(bits)
    oo, total = fl.mask_offsets(dm)
    off = doff.cpu().numpy()
    bad_w = widths.copy()
    bad_w[7] = T + 1
    boff = off.copy()
    boff[5] += 8
    boff[11] += 1 << 40
    dcol, drefs = to_dev(col), to_dev(refs)
    buf = sentinel_buffer(ty, int(bits.sum()) + GUARD)
    flag = raw_select_widths(fl, ty, torch.from_numpy(bad_w).cuda(), torch.from_numpy(boff).cuda(), dcol, drefs, dm, oo, buf, buf.numel())
    assert flag == 1 | 4 | 8, (ty, flag)
    want = vals.copy()
    for b in (5, 7, 11):
        want[b * 1024:(b + 1) * 1024] = sentinel_of(ty)
    got = to_np(buf, ty)
    assert np.array_equal(got[:int(bits.sum())], want[bits]), ty
    assert (got[int(bits.sum()):] == sentinel_of(ty)).all()
    for status, w_, o_ in ((1, torch.from_numpy(bad_w).cuda(), doff), (4, dw, torch.from_numpy(np.where(np.arange(n) == 5, off + 8, off)).cuda()),
                           (6, dw, torch.from_numpy(np.where(np.arange(n) == 11, off + (1 << 40), off)).cuda())):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_select_widths(w_, o_, dcol, drefs, dm)
        assert ei.value.status == status, (ty, status)


@pytest.mark.parametrize("ty", TYS)
def test_output_bounds_never_write_outside(fl, oracle, ty):
    """out_len one short of total, and one block's out_offsets shifted up with out_len tight: exactly the overflowing block is skipped,
    FL_DEVERR_BOUNDS is raised, the guard behind out_len stays untouched."""
    T = tbits(ty)
    n = 53
    rng = np.random.default_rng(15000 + T)
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 15001)
    refs = values(ty, n, 15002)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    bits = rng.random(n * 1024) < 0.3
    bits[-3 * 1024:] = False                                       # the last three blocks keep nothing: block n - 4 ends the output
    dm = mask_words(bits)
    oo, total_dev = fl.mask_offsets(dm)
    total = int(bits.sum())
    dcol, drefs = to_dev(col), to_dev(refs)
    last = n - 4
    start_last = int(bits[:last * 1024].sum())
    want = vals[bits].copy()
    want[start_last:] = sentinel_of(ty)                            # the overflowing block's slots stay as they were
    shifted = oo.clone()
    shifted[last] += 3
    for what, offs, out_len in (("one short", oo, total - 1), ("shifted", shifted, total)):
        buf = sentinel_buffer(ty, total + GUARD)
        flag = raw_select_widths(fl, ty, dw, doff, dcol, drefs, dm, offs, buf, out_len)
        assert flag == 8, (ty, what, flag)
        got = to_np(buf, ty)
        assert np.array_equal(got[:total], want), (ty, what)
        assert (got[total:] == sentinel_of(ty)).all(), (ty, what, "the guard was written")
    # the Python mirror reports it
    with pytest.raises(fl.FastLanesError) as ei:
        fl.unfor_select_widths(dw, doff, dcol, drefs, dm, out_offsets=oo, total=total_dev, output=sentinel_buffer(ty, total + GUARD)[:total - 1])
    assert ei.value.status == 6


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_form_raises_its_error_flag(fl, oracle, ty):
    """The uniform-width entry point takes an err_flag too, alone among the consumers' uniform forms: 3 blocks with out_len one short of
    the total raise FL_DEVERR_BOUNDS in it and skip exactly the last block; with out_len right the flag stays 0."""
    import torch
    T, n, w = tbits(ty), 3, 5
    pk, refs = values(ty, n * packed_len(ty, w), 15100 + T), values(ty, n, 15101 + T)
    vals = oracle.batch("unfor_pack", ty, w, pk, aux=refs, n_blocks=n)
    bits = np.random.default_rng(15102 + T).random(n * 1024) < 0.3
    dm = mask_words(bits)
    oo, _ = fl.mask_offsets(dm)
    total, start_last = int(bits.sum()), int(bits[:(n - 1) * 1024].sum())
    assert start_last < total
    dpk, drefs = to_dev(pk), to_dev(refs)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for out_len, flag in ((total, 0), (total - 1, 8)):
        want = vals[bits].copy()
        if flag:
            want[start_last:] = sentinel_of(ty)                    # the overflowing block's slots stay as they were
        buf = sentinel_buffer(ty, total + GUARD)
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(fl.load(), f"fl_{ty}_unfor_select")(w, dpk.data_ptr(), drefs.data_ptr(), 1, dm.data_ptr(), oo.data_ptr(), buf.data_ptr(), out_len,
                                                         n, err.data_ptr(), stream)
        assert rc == 0 and int(err.item()) == flag, (ty, out_len, rc, int(err.item()))
        got = to_np(buf, ty)
        assert np.array_equal(got[:total], want), (ty, out_len)
        assert (got[total:] == sentinel_of(ty)).all(), (ty, out_len, "the guard was written")


@pytest.mark.parametrize("policy", POLICIES + [8 << 25, 12 << 25, 31 << 25, 2 + (8 << 25)])
@pytest.mark.parametrize("ty", TYS)
def test_policies_windows_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Kernel policies 0 / 1 / 2 (and forced waves / blocks per wavefront / prefetch), the tile-map windows 2^8 / 2^12 / whole column,
    a non-default stream, an empty column and a column of width-0 blocks with no packed bytes: identical results."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    rng = np.random.default_rng(15100 + T)
    n = 1031 if policy >> 25 else 131                                       # more than one 2^8-block window
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 15101)
    refs = values(ty, n, 15102)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    pk2 = values(ty, n * packed_len(ty, T // 2), 15103)
    vals2 = oracle.batch("unfor_pack", ty, T // 2, pk2, aux=refs, n_blocks=n)
    dcol, drefs, dpk2 = to_dev(col), to_dev(refs), to_dev(pk2)
    s = torch.cuda.Stream()
    for name, bits in mask_set(n, rng, full=False).items():
        dm = mask_words(bits)
        buf1, buf2 = sentinel_buffer(ty, int(bits.sum()) + GUARD), sentinel_buffer(ty, int(bits.sum()) + GUARD)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            oo, total = fl.mask_offsets(dm)
            fl.unfor_select_widths(dw, doff, dcol, drefs, dm, out_offsets=oo, total=total, output=buf1, check=False)
            fl.FoR.unfor_select(T // 2, dpk2, drefs, dm, out_offsets=oo, total=total, output=buf2)
        s.synchronize()
        check_select(ty, buf1, total, vals, bits, (ty, policy, name))
        check_select(ty, buf2, total, vals2, bits, (ty, policy, name, "uniform"))
    # empty columns
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    no_mask = torch.empty(0, dtype=torch.int32, device="cuda:0")
    oo, total = fl.mask_offsets(no_mask)
    assert oo.numel() == 0 and int(total.item()) == 0
    assert fl.unfor_select_widths(torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0"),
                                  empty, drefs[:1], no_mask).numel() == 0
    assert fl.FoR.unfor_select(3, empty, 0, no_mask).numel() == 0
    # width-0 blocks, no packed bytes: every value is its block's reference
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    bits = rng.random(5 * 1024) < 0.4
    got = fl.unfor_select_widths(z, zoff, empty, drefs[:5], mask_words(bits))
    assert np.array_equal(to_np(got, ty), np.repeat(refs[:5], 1024)[bits]), (ty, policy, "width 0")
    got = fl.FoR.unfor_select(0, empty, drefs[:5], mask_words(bits), n_blocks=5)
    assert np.array_equal(to_np(got, ty), np.repeat(refs[:5], 1024)[bits]), (ty, policy, "uniform width 0")


@pytest.mark.parametrize("ty", ["u32", "u8"])
def test_at_scale_under_load_equals_the_composition(fl, ty):
    """500 037 blocks, a random mask at 10 %, a second stream keeping the chip busy: equal, on the device, to the composition the feature
    is defined by -- unfor_pack_widths indexed by the expanded mask."""
    import torch
    T = tbits(ty)
    esz = T // 8
    tdt = getattr(torch, TDT[ty])
    n = 500_037
    lib = fl.load()
    load = BackgroundLoad(fl)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(15200 + T)
    widths = torch.randint(0, T + 1, (n,), generator=g, device="cuda:0").to(torch.uint8)
    offsets, total_bytes = fl.widths_to_offsets(ty, widths)
    pbytes = max(int(total_bytes.item()), 16)
    col = torch.empty(pbytes // esz, dtype=tdt, device="cuda:0")
    assert lib.fl_fill_random(col.data_ptr(), pbytes & ~7, 15201, None) == 0
    refs = torch.empty((n + 7) & ~7, dtype=tdt, device="cuda:0")
    assert lib.fl_fill_random(refs.data_ptr(), (refs.numel() * esz) & ~7, 15202, None) == 0
    refs = refs[:n]
    bits = torch.rand(n * 1024, generator=g, device="cuda:0") < 0.1
    w64 = (bits.view(-1, 32).to(torch.int64) << torch.arange(32, device="cuda:0")).sum(dim=1)
    mask = torch.where(w64 >= 1 << 31, w64 - (1 << 32), w64).to(torch.int32)
    torch.cuda.synchronize()
    load.refill()
    full = fl.unfor_pack_widths(widths, offsets, col, refs)
    load.refill()
    got = fl.unfor_select_widths(widths, offsets, col, refs, mask)
    torch.cuda.current_stream().synchronize()
    load.drain()
    sdt = getattr(torch, SIGNED[ty])
    want = full.view(sdt)[bits]
    assert got.numel() == int(bits.sum().item())
    assert torch.equal(got.view(sdt), want), ty
