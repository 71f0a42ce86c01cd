"""GPU: unfor_compare_range / unfor_compare_range_widths -- interval predicates over FoR-packed columns, chained through a mask --
against the mask numpy builds from the oracle's unfor_pack per block (ffor.rs:38-50):
    hit = ((v - lo) mod 2^T) <= ((hi - lo) mod 2^T);   new: hit,  and: mask_in & hit,  or: mask_in | hit
in unpack_compare's layout (bit i of word i // 32 of block b, LSB first)."""
import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TDT, TYS, got_mask, mixed_column, to_dev

pytestmark = pytest.mark.gpu

OPS = ["==", "!=", "<", "<=", ">", ">="]
COMBINE = ["new", "and", "or"]
EACH, ALL, NONE = 0, 1, 2
PREFILL = 0x5A5A5A5A


def prefilled(n):
    import torch
    return torch.full((n * 32,), PREFILL, dtype=torch.int32, device="cuda:0")


def hit_bits(vals, lo, hi):
    """the definition, in the values' own unsigned type (numpy wraps mod 2^T): one bool per value"""
    dt = vals.dtype.type
    with np.errstate(over="ignore"):
        return (vals - dt(lo)) <= dt((hi - lo) % (1 << (8 * vals.dtype.itemsize)))


def want_mask(vals, lo, hi, combine="new", mask_in=None):
    """32 int32 words per 1024-value block, bit i of word i // 32, LSB first"""
    hit = np.packbits(hit_bits(vals, lo, hi), bitorder="little").view(np.int32)
    return hit if combine == "new" else (mask_in & hit) if combine == "and" else (mask_in | hit)


# single-bit positions: the block's ends, the ends of the 16-byte slices lanes 0..7 load and store, and the first and last index of a
# lane's cell (16 / 8 / 4 / 2 indices for u8 / u16 / u32 / u64) in the first and a later 1-KiB group
ONE_BIT = [0, 1023, 127, 128, 895, 896] + [base + 5 * n + e for n in (16, 8, 4, 2) for base in (0, 512) for e in (0, n - 1)]


def incoming_mask(n, seed, shift=0):
    """[n * 32] int32: random half-density blocks mixed with all-zero blocks, all-ones blocks, blocks with ONE bit set and blocks with
    one bit clear; `shift` rotates which block gets which kind"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << 32, size=(n, 32), dtype=np.uint64).astype(np.uint32)
    for b in range(n):
        kind = (b + shift) % 6
        if kind == 1:
            m[b] = 0
        elif kind == 2:
            m[b] = 0xFFFFFFFF
        elif kind in (4, 5):
            i = ONE_BIT[((b + shift) // 6) % len(ONE_BIT)]
            m[b] = 0
            m[b, i // 32] = np.uint32(1) << np.uint32(i % 32)
            if kind == 5:
                m[b] = ~m[b]
    return m.reshape(-1).view(np.int32)


def verdict_of(T, lo, hi, r, w):
    """fl_for_decide.hpp's rule, from the definition: the fields cover [c, c + 2^W - 1] in exact arithmetic"""
    N = 1 << T
    c, s, span = (r - lo) % N, (hi - lo) % N, (1 << w) - 1
    if s == N - 1 or (c <= s and span <= s - c):
        return ALL
    if c > s and span <= N - 1 - c:
        return NONE
    return EACH


def intervals_for(ty, widths, refs, picks):
    """plain, wrapping, single-value and full intervals; bounds at r - 1, r, r + 2^W - 1, r + 2^W of the picked blocks"""
    T = tbits(ty)
    N = 1 << T
    H = N >> 1
    out = [(0, N - 1), (5, 4), (N - 1, 0), (1, N - 2), (H, H - 1), (H - 3, H + 3), (H + 3, H - 3), (0, 0), (N - 1, N - 1)]
    for b in picks:
        r, top = int(refs[b]), (1 << int(widths[b])) - 1
        e = [(r - 1) % N, r, (r + top) % N, (r + top + 1) % N]
        out += [(e[1], e[2]), (e[0], e[3]), (e[3], e[0]), (e[2], e[1]), (e[1], e[1]), (e[2], e[2]), (e[0], e[2]), (e[1], e[3])]
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_columns_every_combiner(fl, oracle, ty):
    """Every width 0..T, a ragged random column of 263 blocks, and 1 / 2 / 3 / 5 blocks (the tails of the shapes with 2 and 4 blocks
    per wavefront); per-block wrapping references and one broadcast reference; plain, wrapping, single-value and full intervals with
    bounds at each side of several blocks' value ranges; the three combiners over incoming masks that mix random blocks with empty,
    full and one-bit ones.  Out of place into an output prefilled with 0x5A bytes (every block must be overwritten, the ones the
    incoming mask had already decided included), and in place."""
    T = tbits(ty)
    rng = np.random.default_rng(9100 + T)
    three_verdicts = {}
    for n, widths in ((T + 1, np.arange(T + 1)), (263, rng.integers(0, T + 1, size=263)), (1, [T // 2]), (2, [3, T]), (3, [T, 0, 1]),
                      (5, [2, T - 1, 0, T, 5])):
        dw, doff, col, blocks = mixed_column(ty, widths, 9200 + n)
        dcol = to_dev(col)
        refs = values(ty, n, 9300 + n)
        for rname, r_host, dref in (("per block", refs, to_dev(refs)), ("broadcast", np.full(n, refs[n // 2], dtype=refs.dtype), to_dev(refs[n // 2:n // 2 + 1]))):
            vals = np.concatenate([oracle.unfor_pack(ty, w, pk, r_host[b]) for b, (w, pk) in enumerate(blocks)])
            picks = sorted({0, n // 3, n // 2, n - 1} | set(rng.integers(0, n, size=2).tolist()))
            ivs = intervals_for(ty, widths, r_host, picks)
            if n < 10:
                ivs = ivs[::3]
            for q, (lo, hi) in enumerate(ivs):
                seen = {verdict_of(T, lo, hi, int(r_host[b]), int(widths[b])) for b in range(n)}
                three_verdicts[n, rname] = three_verdicts.get((n, rname), False) or seen == {EACH, ALL, NONE}
                min_host = incoming_mask(n, 9400 + n, shift=q)
                dmin = to_dev(min_host)
                for cb in COMBINE:
                    want = want_mask(vals, lo, hi, cb, min_host)
                    args = dict(mask=dmin, combine=cb) if cb != "new" else {}
                    got = got_mask(fl.unfor_compare_range_widths(dw, doff, dcol, dref, lo, hi, output=prefilled(n), **args))
                    assert np.array_equal(got, want), (ty, n, rname, cb, lo, hi)
                    if cb != "new":
                        inplace = dmin.clone()
                        out = fl.unfor_compare_range_widths(dw, doff, dcol, dref, lo, hi, mask=inplace, combine=cb, output=inplace)
                        assert out is inplace and np.array_equal(got_mask(inplace), want), (ty, n, rname, cb, lo, hi, "in place")
                        assert np.array_equal(got_mask(dmin), min_host)                     # out of place left mask_in alone
                # "new" ignores a mask it is given
                got = got_mask(fl.unfor_compare_range_widths(dw, doff, dcol, dref, lo, hi, mask=dmin, combine="new"))
                assert np.array_equal(got, want_mask(vals, lo, hi)), (ty, n, rname, "new with a mask", lo, hi)
    # all three verdicts occur under ONE interval of the larger columns, so one launch takes every path
    assert three_verdicts[T + 1, "per block"] and three_verdicts[263, "per block"], three_verdicts


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_every_width(fl, oracle, ty):
    """FoR.unfor_compare_range over a uniform-width column of 37 blocks at every (T, W): per-block and scalar references, the three
    combiners, in place"""
    T = tbits(ty)
    N = 1 << T
    n = 37
    for w in range(T + 1):
        pk = values(ty, n * packed_len(ty, w), 9400 + 64 * T + w)
        refs = values(ty, n, 9500 + 64 * T + w)
        vals = oracle.batch("unfor_pack", ty, w, pk, aux=refs, n_blocks=n)
        dpk, drefs = to_dev(pk), to_dev(refs)
        top = (1 << w) - 1
        r5, r9 = int(refs[5]), int(refs[9])
        ivs = [(r5, (r5 + top) % N), ((r5 + top + 1) % N, (r5 - 1) % N), ((r9 + (top >> 1)) % N, (r9 + (top >> 1)) % N), (r9, (r5 + (top >> 1)) % N),
               ((r9 - 1) % N, (r9 - 2) % N)]
        min_host = incoming_mask(n, 9600 + w, shift=w)
        dmin = to_dev(min_host)
        for q, (lo, hi) in enumerate(ivs):
            for cb in COMBINE:
                want = want_mask(vals, lo, hi, cb, min_host)
                args = dict(mask=dmin, combine=cb) if cb != "new" else {}
                got = got_mask(fl.FoR.unfor_compare_range(w, dpk, drefs, lo, hi, n_blocks=n, output=prefilled(n), **args))
                assert np.array_equal(got, want), (ty, w, cb, lo, hi)
            if q == w % len(ivs):
                inplace = dmin.clone()
                fl.FoR.unfor_compare_range(w, dpk, drefs, lo, hi, mask=inplace, combine="or", output=inplace)
                assert np.array_equal(got_mask(inplace), want_mask(vals, lo, hi, "or", min_host)), (ty, w, "in place")
        # one scalar reference for every block (reference_stride 0)
        r0 = int(refs[1])
        vals0 = oracle.batch("unfor_pack", ty, w, pk, aux=np.full(n, r0, dtype=refs.dtype), n_blocks=n)
        lo, hi = (r0 + (top >> 2)) % N, (r0 + (top >> 1)) % N
        got = got_mask(fl.FoR.unfor_compare_range(w, dpk, r0, lo, hi, mask=dmin, combine="and", n_blocks=n))
        assert np.array_equal(got, want_mask(vals0, lo, hi, "and", min_host)), (ty, w, "scalar reference")


@pytest.mark.parametrize("ty", TYS)
def test_new_equals_unfor_compare_for_the_six_unsigned_ops(fl, oracle, ty):
    """NEW through predicate_interval is unfor_compare / unfor_compare_widths, bit for bit; an op whose interval is None (x < 0,
    x > M) is left to the caller, and there unfor_compare answers with the zero mask the docstring names."""
    T = tbits(ty)
    M = (1 << T) - 1
    rng = np.random.default_rng(9700 + T)
    n = 70
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 9701)
    refs = values(ty, n, 9702)
    dcol, drefs = to_dev(col), to_dev(refs)
    w = T // 2 + 1
    pk2 = to_dev(values(ty, n * packed_len(ty, w), 9703))
    top = (1 << int(widths[7])) - 1
    for k in (0, 1, M - 1, M, int(refs[7]), (int(refs[7]) + top) % (M + 1), (int(refs[7]) + top + 1) % (M + 1), int(refs[40]) ^ 5):
        for op in OPS:
            iv = fl.predicate_interval(ty, op, k)
            old_mixed = fl.unfor_compare_widths(dw, doff, dcol, drefs, op, k)
            old_uniform = fl.FoR.unfor_compare(w, pk2, drefs, op, k)
            if iv is None:
                assert (op, k) in (("<", 0), (">", M))
                assert not old_mixed.any().item() and not old_uniform.any().item()
                continue
            assert np.array_equal(got_mask(fl.unfor_compare_range_widths(dw, doff, dcol, drefs, *iv)), got_mask(old_mixed)), (ty, op, k)
            assert np.array_equal(got_mask(fl.FoR.unfor_compare_range(w, pk2, drefs, *iv)), got_mask(old_uniform)), (ty, op, k, "uniform")


@pytest.mark.parametrize("ty", TYS)
def test_device_checks_match_unfor_compare_widths(fl, oracle, ty):
    """A block with a width > T, one with a misaligned offset, one outside the packed column: the kernel checks them itself, err_flag
    holds the three bits, the skipped blocks' mask words keep their prefill, every other block is right, and check=True raises."""
    import ctypes
    import torch
    T = tbits(ty)
    esz = T // 8
    n = 40
    rng = np.random.default_rng(9800 + T)
    widths = rng.integers(1, T + 1, size=n).astype(np.uint8)
    dw, doff, col, blocks = mixed_column(ty, widths, 9801)
    refs = values(ty, n, 9802)
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
    lo, hi = int(refs[20]), (int(refs[20]) + (1 << (T - 2))) % (1 << T)
    min_host = incoming_mask(n, 9803)
    dmin = to_dev(min_host)
    skipped = np.zeros(n, dtype=bool)
    skipped[[5, 7, 11]] = True
    for code, cb in enumerate(COMBINE):
        mask = prefilled(n)
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(lib, f"fl_{ty}_unfor_compare_range_widths")(dbw.data_ptr(), dboff.data_ptr(), dcol.data_ptr(), col.size * esz, drefs.data_ptr(), 1,
                                                                lo, hi, code, dmin.data_ptr() if code else None, n, mask.data_ptr(), err.data_ptr(), stream)
        assert rc == 0
        assert int(err.item()) == 1 | 4 | 8, (ty, cb, int(err.item()))
        g = got_mask(mask).reshape(n, 32)
        w = want_mask(vals, lo, hi, cb, min_host).reshape(n, 32)
        assert (g[skipped] == PREFILL).all(), (ty, cb, "a skipped block was written")
        assert np.array_equal(g[~skipped], w[~skipped]), (ty, cb)
    for status, w_, o_ in ((1, dbw, doff), (4, dw, torch.from_numpy(np.where(np.arange(n) == 5, off + 8, off)).cuda()),
                           (6, dw, torch.from_numpy(np.where(np.arange(n) == 11, off + (1 << 40), off)).cuda())):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_compare_range_widths(w_, o_, dcol, drefs, lo, hi, mask=dmin, combine="and")
        assert ei.value.status == status, (ty, status)


@pytest.mark.parametrize("policy", [0, 1, 2, 2 + 256 * 4 + 65536 * 4 + (1 << 24), 2 + 256 * 6 + 65536 * 3, 2 + 256 * 4 + 65536 * 12 + (1 << 24)])
@pytest.mark.parametrize("ty", TYS)
def test_policies_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Kernel policies 0 / 1 / 2 (and forced waves / blocks per wavefront / prefetch, up to 12 blocks per wavefront: the second
    incoming-mask register of the prefetched form), a non-default stream, an empty column and a column of width-0 blocks with no
    packed bytes."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    N = 1 << T
    rng = np.random.default_rng(9900 + T)
    n = 131
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 9901)
    refs = values(ty, n, 9902)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    r = int(refs[n // 3])
    lo, hi = (r - (N >> 3)) % N, (r + (N >> 2)) % N
    pk2 = values(ty, n * packed_len(ty, T // 2), 9903)
    vals2 = oracle.batch("unfor_pack", ty, T // 2, pk2, aux=refs, n_blocks=n)
    min_host = incoming_mask(n, 9904)
    s = torch.cuda.Stream()
    dcol, drefs, dpk2, dmin = to_dev(col), to_dev(refs), to_dev(pk2), to_dev(min_host)
    torch.cuda.synchronize()
    for cb in COMBINE:
        args = dict(mask=dmin, combine=cb) if cb != "new" else {}
        inplace = dmin.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            m1 = fl.unfor_compare_range_widths(dw, doff, dcol, drefs, lo, hi, check=False, output=prefilled(n), **args)
            m2 = fl.FoR.unfor_compare_range(T // 2, dpk2, drefs, hi, lo, output=prefilled(n), **args)
            if cb != "new":
                fl.unfor_compare_range_widths(dw, doff, dcol, drefs, lo, hi, mask=inplace, combine=cb, output=inplace, check=False)
        s.synchronize()
        assert np.array_equal(got_mask(m1), want_mask(vals, lo, hi, cb, min_host)), (ty, policy, cb)
        assert np.array_equal(got_mask(m2), want_mask(vals2, hi, lo, cb, min_host)), (ty, policy, cb, "uniform")
        if cb != "new":
            assert np.array_equal(got_mask(inplace), want_mask(vals, lo, hi, cb, min_host)), (ty, policy, cb, "in place")
    # empty columns
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    nomask = torch.empty(0, dtype=torch.int32, device="cuda:0")
    ew, eo = torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0")
    assert fl.unfor_compare_range_widths(ew, eo, empty, drefs[:1], 1, 2).numel() == 0
    assert fl.unfor_compare_range_widths(ew, eo, empty, drefs[:1], 1, 2, mask=nomask, combine="and").numel() == 0
    assert fl.FoR.unfor_compare_range(3, empty, 0, 1, 2).numel() == 0
    # width-0 blocks, no packed bytes: every value is its block's reference
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    vz = np.repeat(refs[:5], 1024)
    mz = incoming_mask(5, 9905, shift=1)
    got = got_mask(fl.unfor_compare_range_widths(z, zoff, empty, drefs[:5], lo, hi, mask=to_dev(mz), combine="or"))
    assert np.array_equal(got, want_mask(vz, lo, hi, "or", mz)), (ty, policy, "width 0")
    got = got_mask(fl.FoR.unfor_compare_range(0, empty, drefs[:5], int(refs[2]), int(refs[2]), mask=to_dev(mz), combine="and"))
    assert np.array_equal(got, want_mask(vz, int(refs[2]), int(refs[2]), "and", mz)), (ty, policy, "uniform width 0")
    got = got_mask(fl.FoR.unfor_compare_range(0, empty, drefs[:5], int(refs[2]), int(refs[2]), n_blocks=5))
    assert np.array_equal(got, want_mask(vz, int(refs[2]), int(refs[2]))), (ty, policy, "uniform width 0, new")


def test_signed_column_less_than_a_negative_constant(fl, oracle):
    """a u32 column read as int32: x < -5 through predicate_interval(..., signed=True), against numpy on the int32 view"""
    T = 32
    rng = np.random.default_rng(10000)
    n = 45
    widths = rng.integers(0, T + 1, size=n)
    widths[:7] = [0, 3, 3, 31, 32, 2, 0]
    dw, doff, col, blocks = mixed_column("u32", widths, 10001)
    refs = values("u32", n, 10002)
    refs[:7] = [0xFFFFFFF0, 0xFFFFFFF8, 0x7FFFFFFC, 0x80000000, 5, 0xFFFFFFF8, 0x80000000]   # around -5, around the sign change, INT_MIN
    vals = np.concatenate([oracle.unfor_pack("u32", w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    dcol, drefs = to_dev(col), to_dev(refs)
    for op, k in (("<", -5), (">=", -5), ("<=", 0), (">", 2 ** 31 - 2), ("==", -1), ("!=", -(2 ** 31))):
        iv = fl.predicate_interval("u32", op, k, signed=True)
        want = {"<": np.less, ">=": np.greater_equal, "<=": np.less_equal, ">": np.greater, "==": np.equal, "!=": np.not_equal}[op](vals.view(np.int32), np.int32(k))
        assert want.any() and not want.all()
        got = got_mask(fl.unfor_compare_range_widths(dw, doff, dcol, drefs, *iv))
        assert np.array_equal(got, np.packbits(want, bitorder="little").view(np.int32)), (op, k)


def test_chain_between_and_equals_then_aggregate(fl):
    """WHERE ts BETWEEN a AND b AND status = 3, then COUNT / SUM / MIN / MAX of z: three small columns of different types through the
    library's own encoder, the second predicate chained in place through the first one's mask, against numpy."""
    import torch
    n = 96
    rng = np.random.default_rng(10100)
    ts = (np.arange(n * 1024, dtype=np.uint64) * 37 + 1000).astype(np.uint32)                # ascending: most blocks decided
    status = rng.integers(0, 6, size=n * 1024).astype(np.uint8)
    status[17 * 1024:19 * 1024] = 3                                                           # blocks the second predicate decides
    status[30 * 1024:31 * 1024] = 4
    z = rng.integers(0, 50000, size=n * 1024).astype(np.uint16)
    cols = {}
    for name, ty, v in (("ts", "u32", ts), ("status", "u8", status), ("z", "u16", z)):
        dv = to_dev(v)
        mins, maxs = fl.BitPacking.block_min_max(dv)
        dw = fl.for_widths(mins, maxs)
        doff, dtotal = fl.widths_to_offsets(ty, dw)
        dpk = torch.zeros(max(int(dtotal.item()) // (tbits(ty) // 8), 1), dtype=getattr(torch, TDT[ty]), device="cuda:0")
        fl.for_pack_widths(dw, doff, dv, mins, dpk)
        cols[name] = (dw, doff, dpk, mins)
    a, b = int(ts[15 * 1024 + 300]), int(ts[33 * 1024 + 77])
    m = fl.unfor_compare_range_widths(*cols["ts"], a, b)
    out = fl.unfor_compare_range_widths(*cols["status"], 3, 3, mask=m, combine="and", output=m)
    assert out is m
    keep = (ts >= a) & (ts <= b) & (status == 3)
    assert np.array_equal(got_mask(m), np.packbits(keep, bitorder="little").view(np.int32))
    result, _ = fl.unfor_aggregate_widths(*cols["z"], mask=m)
    kept = z[keep].astype(np.uint64)
    assert kept.size > 2048
    assert [int(x) for x in result.cpu().numpy().view(np.uint64)] == [kept.size, int(kept.sum()), int(kept.min()), int(kept.max())]
