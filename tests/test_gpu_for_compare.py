"""GPU: unfor_compare / unfor_compare_widths -- selection masks from FoR-packed columns -- against the mask numpy builds from the
oracle's unfor_pack per block (ffor.rs:38-50): bit i of word i // 32 of block b, LSB first, = (value i of block b <op> constant)."""
import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TDT, TYS, got_mask, mixed_column, to_dev, to_np, want_mask

pytestmark = pytest.mark.gpu

OPS = ["==", "!=", "<", "<=", ">", ">="]


def constants_for(ty, widths, refs, picks):
    """0, M, and r - 1, r, r + 2^W - 1, r + 2^W (mod 2^T) of the picked blocks: every decision branch"""
    T = tbits(ty)
    M = (1 << T) - 1
    ks = {0, M}
    for b in picks:
        r, w = int(refs[b]), int(widths[b])
        ks |= {(r - 1) % (M + 1), r, (r + (1 << w) - 1) % (M + 1), (r + (1 << w)) % (M + 1)}
    return sorted(ks)


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_columns_every_op(fl, oracle, ty):
    """Every width 0..T and a ragged random column of 263 blocks; random per-block references (wrapping) and one broadcast
    reference; all six ops; constants at 0, M and at each side of several blocks' value ranges."""
    T = tbits(ty)
    rng = np.random.default_rng(9100 + T)
    for n, widths in ((T + 1, np.arange(T + 1)), (263, rng.integers(0, T + 1, size=263))):
        dw, doff, col, blocks = mixed_column(ty, widths, 9200 + n)
        dcol = to_dev(col)
        refs = values(ty, n, 9300 + n)
        for rname, r_host, dref in (("per block", refs, to_dev(refs)), ("broadcast", np.full(n, refs[3], dtype=refs.dtype), to_dev(refs[3:4]))):
            vals = np.concatenate([oracle.unfor_pack(ty, w, pk, r_host[b]) for b, (w, pk) in enumerate(blocks)])
            picks = [0, 3, n // 2, n - 1] + list(rng.integers(0, n, size=3))
            for k in constants_for(ty, widths, r_host, picks):
                for op in OPS:
                    got = got_mask(fl.unfor_compare_widths(dw, doff, dcol, dref, op, k))
                    assert np.array_equal(got, want_mask(vals, op, k)), (ty, n, rname, op, k)


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_every_width_and_op(fl, oracle, ty):
    """FoR.unfor_compare over a uniform-width column, every (T, W) x six ops, per-block and scalar references"""
    T = tbits(ty)
    M = (1 << T) - 1
    n = 37
    for w in range(T + 1):
        pk = values(ty, n * packed_len(ty, w), 9400 + 64 * T + w)
        refs = values(ty, n, 9500 + 64 * T + w)
        vals = oracle.batch("unfor_pack", ty, w, pk, aux=refs, n_blocks=n)
        dpk, drefs = to_dev(pk), to_dev(refs)
        ks = [0, M, int(refs[5]), (int(refs[5]) + (1 << w) - 1) % (M + 1), (int(refs[9]) + (1 << max(w - 1, 0))) % (M + 1)]
        for op in OPS:
            for k in ks:
                got = got_mask(fl.FoR.unfor_compare(w, dpk, drefs, op, k, n_blocks=n))
                assert np.array_equal(got, want_mask(vals, op, k)), (ty, w, op, k)
        # one scalar reference for every block (reference_stride 0)
        r0 = int(refs[1])
        vals0 = oracle.batch("unfor_pack", ty, w, pk, aux=np.full(n, r0, dtype=refs.dtype), n_blocks=n)
        got = got_mask(fl.FoR.unfor_compare(w, dpk, r0, "<", ks[4], n_blocks=n))
        assert np.array_equal(got, want_mask(vals0, "<", ks[4])), (ty, w, "scalar reference")


@pytest.mark.parametrize("ty", TYS)
def test_encoder_chain_ascending_column_is_mostly_decided(fl, ty):
    """The library's own encoder (block_min_max -> for_widths -> widths_to_offsets -> for_pack_widths) over an ascending column,
    `x < k` at about the 1 % quantile: equal to `values < k` computed directly, >= 90 % of the blocks decided by their metadata,
    and every decided block's mask fully written (the output starts as 0xAA bytes)."""
    import torch
    T = tbits(ty)
    esz = T // 8
    n = 400
    i = np.arange(n * 1024, dtype=np.uint64)
    # ascending, never wrapping: the whole type's range for u8 .. u32, a slope of 3 for u64
    v = (i * np.uint64((1 << T) - 1) // np.uint64(n * 1024) if T <= 32 else i * np.uint64(3) + np.uint64(11)).astype(TYPES[ty][0])
    dv = to_dev(v)
    mins, maxs = fl.BitPacking.block_min_max(dv)
    dw = fl.for_widths(mins, maxs)
    doff, dtotal = fl.widths_to_offsets(ty, dw)
    dpk = torch.zeros(max(int(dtotal.item()) // esz, 1), dtype=getattr(torch, TDT[ty]), device="cuda:0")
    fl.for_pack_widths(dw, doff, dv, mins, dpk)
    for op, k in (("<", int(v[len(v) // 100])), (">=", int(v[len(v) // 100])), ("<=", int(v[-1]) // 2), ("==", int(v[777]))):
        out = torch.full((n * 32,), -0x55555556, dtype=torch.int32, device="cuda:0")          # 0xAAAAAAAA
        got = got_mask(fl.unfor_compare_widths(dw, doff, dpk, mins, op, k, output=out))
        assert np.array_equal(got, want_mask(v, op, k)), (ty, op, k)
    # the decided share of `x < k1%`, from the blocks' metadata (fl_for_decide.hpp's rule for s = k - 1, c = r)
    k = int(v[len(v) // 100])
    lo = to_np(mins, ty).astype(object)
    wd = dw.cpu().numpy().astype(int)
    decided = sum(1 for r, w in zip(lo, wd) if r + (1 << w) - 1 <= k - 1 or r >= k)
    assert decided >= 0.9 * n, (ty, decided, n)


@pytest.mark.parametrize("ty", TYS)
def test_device_checks_match_unfor_pack_widths(fl, oracle, ty):
    """A block with a width > T, one with a misaligned offset, one outside the packed column: err_flag equals what
    unfor_pack_widths reports on the same column, the skipped blocks' mask words keep their sentinel, every other block is right,
    and check=True raises."""
    import ctypes
    import torch
    T = tbits(ty)
    esz = T // 8
    n = 40
    rng = np.random.default_rng(9600 + T)
    widths = rng.integers(1, T + 1, size=n).astype(np.uint8)
    dw, doff, col, blocks = mixed_column(ty, widths, 9601)
    refs = values(ty, n, 9602)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    off = doff.cpu().numpy()
    bad_w = widths.copy()
    bad_w[7] = T + 1
    boff = off.copy()
    boff[5] += 8
    boff[11] += 1 << 40
    dbw, dboff = torch.from_numpy(bad_w).cuda(), torch.from_numpy(boff).cuda()
    dcol, drefs = to_dev(col), to_dev(refs)
    lib = fl.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    k = int(refs[20])
    for op in OPS:
        mask = torch.full((n * 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(lib, f"fl_{ty}_unfor_compare_widths")(dbw.data_ptr(), dboff.data_ptr(), dcol.data_ptr(), col.size * esz, drefs.data_ptr(), 1,
                                                          fl.BitPacking.CMP[op], k, n, mask.data_ptr(), err.data_ptr(), stream)
        assert rc == 0
        out = torch.empty(n * 1024, dtype=getattr(torch, TDT[ty]), device="cuda:0")
        err2 = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(lib, f"fl_{ty}_unfor_pack_widths")(dbw.data_ptr(), dboff.data_ptr(), dcol.data_ptr(), col.size * esz, drefs.data_ptr(), 1,
                                                       out.data_ptr(), n, err2.data_ptr(), stream)
        assert rc == 0
        assert int(err.item()) == int(err2.item()) == 1 | 4 | 8, (ty, op, int(err.item()), int(err2.item()))
        g = got_mask(mask).reshape(n, 32)
        w = want_mask(vals, op, k).reshape(n, 32)
        skipped = np.zeros(n, dtype=bool)
        skipped[[5, 7, 11]] = True
        assert (g[skipped] == 0x5A5A5A5A).all(), (ty, op, "a skipped block was written")
        assert np.array_equal(g[~skipped], w[~skipped]), (ty, op)
    for status, w_, o_ in ((1, dbw, doff), (4, dw, torch.from_numpy(np.where(np.arange(n) == 5, off + 8, off)).cuda()),
                           (6, dw, torch.from_numpy(np.where(np.arange(n) == 11, off + (1 << 40), off)).cuda())):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_compare_widths(w_, o_, dcol, drefs, "<", k)
        assert ei.value.status == status, (ty, status)


@pytest.mark.parametrize("policy", [0, 1, 2, 2 + 256 * 4 + 65536 * 4 + (1 << 24), 2 + 256 * 6 + 65536 * 3])
@pytest.mark.parametrize("ty", TYS)
def test_policies_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Kernel policies 0 / 1 / 2 (and forced waves / blocks per wavefront / prefetch), a non-default stream, an empty column and a
    column of width-0 blocks with no packed bytes."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    rng = np.random.default_rng(9700 + T)
    n = 131
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 9701)
    refs = values(ty, n, 9702)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    k = int(refs[n // 3])
    pk2 = values(ty, n * packed_len(ty, T // 2), 9703)
    vals2 = oracle.batch("unfor_pack", ty, T // 2, pk2, aux=refs, n_blocks=n)
    s = torch.cuda.Stream()
    dcol, drefs, dpk2 = to_dev(col), to_dev(refs), to_dev(pk2)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        m1 = fl.unfor_compare_widths(dw, doff, dcol, drefs, "<=", k, check=False)
        m2 = fl.FoR.unfor_compare(T // 2, dpk2, drefs, ">", k)
    s.synchronize()
    assert np.array_equal(got_mask(m1), want_mask(vals, "<=", k)), (ty, policy)
    assert np.array_equal(got_mask(m2), want_mask(vals2, ">", k)), (ty, policy, "uniform")
    # empty columns
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    assert fl.unfor_compare_widths(torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0"),
                                   empty, drefs[:1], "<", 1).numel() == 0
    assert fl.FoR.unfor_compare(3, empty, 0, "<", 1).numel() == 0
    # width-0 blocks, no packed bytes: every value is its block's reference
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    got = got_mask(fl.unfor_compare_widths(z, zoff, empty, drefs[:5], ">=", k))
    assert np.array_equal(got, want_mask(np.repeat(refs[:5], 1024), ">=", k)), (ty, policy, "width 0")
    got = got_mask(fl.FoR.unfor_compare(0, empty, drefs[:5], "!=", int(refs[2]), n_blocks=5))
    assert np.array_equal(got, want_mask(np.repeat(refs[:5], 1024), "!=", int(refs[2]))), (ty, policy, "uniform width 0")


def test_column_of_more_than_2_32_values(fl, oracle):
    """u8 at W = 1 over 4 200 000 blocks (4.3 G values): the first, the last and a sample of blocks against the oracle -- index
    arithmetic that wraps at 32 bits would misplace the blocks past 2^32 values."""
    import ctypes
    import torch
    n = 4_200_000
    assert n * 1024 > 1 << 32
    pk = torch.empty(n * 128, dtype=torch.uint8, device="cuda:0")
    lib = fl.load()
    assert lib.fl_fill_random(pk.data_ptr(), pk.numel(), 77, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    refs = torch.from_numpy((np.arange(n) % 200).astype(np.uint8)).cuda()
    k = 100
    mask = fl.FoR.unfor_compare(1, pk, refs, "==", k)            # blocks with reference 99 or 100 are undecided, the rest decided
    torch.cuda.synchronize()
    rng = np.random.default_rng(9800)
    picks = np.unique(np.concatenate([[0, 1, 99, 100, n // 2, (1 << 22) - 1, 1 << 22, n - 2, n - 1],
                                      rng.integers(0, n, size=200), (np.arange(n - 4000, n, 200) // 200) * 200 + 99]))
    picks = picks[picks < n]
    host_pk = pk.view(n, 128)[torch.from_numpy(picks).cuda()].cpu().numpy()
    got = mask.view(n, 32)[torch.from_numpy(picks).cuda()].cpu().numpy().view(np.int32)
    for j, b in enumerate(picks):
        vals = oracle.unfor_pack("u8", 1, host_pk[j], int(b % 200))
        assert np.array_equal(got[j], want_mask(vals, "==", k)), int(b)
    # a wrong decision anywhere in the column shows up as a wrong population count of its block
    bits = mask.view(n, 32).view(torch.uint8).view(n, 128)
    pop = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    for bit in range(8):
        pop += ((bits >> bit) & 1).sum(dim=1)
    r = refs.to(torch.int64)
    ones = pk.view(n, 128)
    nset = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    for bit in range(8):
        nset += ((ones >> bit) & 1).sum(dim=1)
    # W = 1: a value is r + f; r = 100 -> the 1024 - popcount(packed) zero fields match, r = 99 -> the popcount one fields match
    counts = torch.where(r == 100, 1024 - nset, torch.where(r == 99, nset, torch.zeros_like(nset)))
    assert torch.equal(pop, counts)
