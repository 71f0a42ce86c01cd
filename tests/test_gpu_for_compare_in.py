"""GPU: unfor_compare_in / unfor_compare_in_widths -- set membership over FoR-packed columns, chained through a mask -- against numpy
on the oracle's unfor_pack per block (ffor.rs:38-50), then np.isin against the set's member VALUES:
    hit = isin(v, members) != negate;   new: hit,  and: mask_in & hit,  or: mask_in | hit
in unpack_compare's layout (bit i of word i // 32 of block b, LSB first).  A set is given to the kernel as a window (lo, bits) plus a
bitmap; the expected side never looks at the bitmap, only at the values it stands for."""
import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TDT, TYS, got_mask, mixed_column, to_dev
from test_gpu_for_compare_range import COMBINE, PREFILL, prefilled
from test_gpu_for_consumer_shapes import BAD_W, SHAPES, ZERO_W, column_masks, raw_masks

pytestmark = pytest.mark.gpu

PIVOT, WRAP, FAR = 4, 3, 8                    # blocks of the mixed column the sets are placed around (besides ZERO_W, BAD_W, EMPTY, FULL)


class Set:
    """a window (lo, bits), the bitmap bits `js` inside it, and the member values they stand for; garbage: the last word's bits at
    positions >= bits are all set"""

    def __init__(self, ty, name, lo, bits, js, garbage=False):
        N = 1 << tbits(ty)
        js = np.unique(np.asarray(js, dtype=np.uint64))
        assert bits <= min(N, 1 << 32) and (js.size == 0 or int(js.max()) < bits)
        self.name, self.lo, self.bits = name, lo % N, bits
        self.words = np.zeros((bits + 31) // 32, dtype=np.uint32)
        np.bitwise_or.at(self.words, (js >> np.uint64(5)).astype(np.int64), np.uint32(1) << (js & np.uint64(31)).astype(np.uint32))
        if garbage:
            assert bits % 32
            self.words[-1] |= np.uint32((0xFFFFFFFF << (bits % 32)) & 0xFFFFFFFF)
        with np.errstate(over="ignore"):
            self.members = ((js + np.uint64(self.lo)) & np.uint64(N - 1)).astype(TYPES[ty][0])

    def member_set(self, fl, ty):
        """the kernel's argument, as given: fl.member_set would tighten the window and clear the garbage"""
        return fl.MemberSet(ty, self.lo, self.bits, self.words)


def want_in(vals, members, negate, combine="new", mask_in=None):
    """32 int32 words per 1024-value block, bit i of word i // 32, LSB first"""
    hit = np.packbits(np.isin(vals, members) != bool(negate), bitorder="little").view(np.int32)
    return hit if combine == "new" else (mask_in & hit) if combine == "and" else (mask_in | hit)


def half(rng, bits, *always):
    """about half of the bits 0 .. bits - 1, and `always`"""
    js = np.flatnonzero(rng.random(bits) < 0.5)
    return np.concatenate([js, np.array(always, dtype=np.int64)]).astype(np.uint64)


def column_for_sets(ty, n, seed):
    """(widths, refs): values gathered in a few thousand values just below 2^T (so windows find them, and wrap), with a width-1 and a
    width-T block, a width-0 block, a block of 64 values at the pivot, a block that wraps past 2^T - 1, and a block far away"""
    T = tbits(ty)
    N = 1 << T
    rs = np.random.default_rng(seed)
    widths = rs.integers(1, min(T, 11) + 1, size=n)
    widths[[0, 1]] = [1, T]
    widths[ZERO_W] = 0
    widths[PIVOT], widths[WRAP], widths[FAR] = 6, 5, 3
    refs = [(N - min(3000, N // 2) + int(x)) % N for x in rs.integers(0, min(4096, N), size=n)]    # Python integers: they pass 2^63
    refs[WRAP], refs[FAR] = N - 20, N // 2 + 7
    return widths, np.array(refs, dtype=np.uint64).astype(TYPES[ty][0])


def sets_for(ty, widths, refs, rng):
    T = tbits(ty)
    N = 1 << T
    P, Z, F = int(refs[PIVOT]), int(refs[ZERO_W]), int(refs[FAR])
    out = [Set(ty, "one member", P + 5, 1, [0]),
           Set(ty, "bits 0, 31, 32 and the last", P, 61, [0, 31, 32, 60]),
           Set(ty, "33 bits, garbage behind them", P + 2, 33, half(rng, 33, 32), garbage=True),
           Set(ty, "wraps past 2^T - 1", N - 10, 30, half(rng, 30, 0, 29)),
           Set(ty, "empty", 0, 0, []),
           Set(ty, "every value of the width-0 block", Z - 1, 3, [1]),
           Set(ty, "beside the width-0 block's value", Z - 1, 3, [0, 2]),
           Set(ty, "a window no narrow block reaches", N // 4, 40, half(rng, 40, 0, 39), garbage=True)]
    if T > 8:                                                            # the tier boundary: 2048 bits ride in registers, 2049 do not
        out += [Set(ty, "2048 bits", P + 5 - 2047, 2048, half(rng, 2048, 0, 2047)),        # the last bit: a value the pivot block holds
                Set(ty, "2049 bits, a member at bit 2048", P + 5 - 2048, 2049, half(rng, 2048, 2048)),
                Set(ty, "65536 bits", P - 30000, 65536, half(rng, 65536, 0, 65535))]
    if T <= 16:                                                          # the whole domain: no block is outside the window, and
        js = set(half(rng, N).tolist())                                  # the width-0 block and the far block must still miss
        js -= {(Z - 77) % N} | {(F + f - 77) % N for f in range(8)}
        out.append(Set(ty, "2^T bits", 77, N, sorted(js)))
    return out


@pytest.mark.parametrize("policy,bpw", SHAPES)
@pytest.mark.parametrize("ty", TYS)
def test_every_set_over_tails_and_special_blocks(fl, oracle, kernel_policy, ty, policy, bpw):
    """n = 2 * 4 * bpw + r blocks under every launch shape; a width-0 block, a block of width T + 1 (FL_DEVERR_WIDTH: its prefilled
    mask words stay), an incoming mask with an empty and a full block; every set, negate both ways, the three combiners, in place."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    for r in sorted({1, bpw - 1, bpw + 1} - {0}):
        n = 2 * 4 * bpw + r
        widths, refs = column_for_sets(ty, n, 41000 + 64 * T + n)
        dw, doff, col, blocks = mixed_column(ty, widths, 41100 + n)
        vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
        bad_w = widths.astype(np.uint8)
        bad_w[BAD_W] = T + 1
        dbw = torch.from_numpy(bad_w).cuda()
        dcol, drefs = to_dev(col), to_dev(refs)
        bits, words = column_masks(n, 41200 + n)
        dm = to_dev(words)
        ok = np.arange(n) != BAD_W
        for q, s in enumerate(sets_for(ty, widths, refs, np.random.default_rng(41300 + n))):
            what = (ty, policy, n, s.name)
            dset = to_dev(s.words.view(np.int32)) if s.bits else None
            ptr = dset.data_ptr() if s.bits else None
            hits = np.isin(vals, s.members)
            if s.name in ("2^T bits", "beside the width-0 block's value"):
                assert not hits[ZERO_W * 1024:(ZERO_W + 1) * 1024].any(), what
            if s.name == "every value of the width-0 block":
                assert hits[ZERO_W * 1024:(ZERO_W + 1) * 1024].all(), what
            if s.name not in ("empty", "a window no narrow block reaches", "beside the width-0 block's value"):
                assert hits.any() and not hits.all(), what
            for negate in (0, 1):
                for code, cb in enumerate(COMBINE):
                    want = want_in(vals, s.members, negate, cb, words).reshape(n, 32)
                    g, flag = raw_masks(fl, ty, "unfor_compare_in", dbw, doff, dcol, drefs, n,
                                        dict(args=(s.lo, s.bits, ptr, negate, code, dm.data_ptr() if code else None)))
                    assert flag == 1, (what, negate, cb, flag)
                    assert (g[BAD_W] == PREFILL).all(), (what, negate, cb, "the skipped block was written")
                    assert np.array_equal(g[ok], want[ok]), (what, negate, cb, np.flatnonzero((g != want).any(axis=1) & ok))
            # in place, alternating AND / OR and negate over the sets; the skipped block keeps its incoming mask
            code, negate = 1 + q % 2, (q // 2) % 2
            inplace = dm.clone()
            g, flag = raw_masks(fl, ty, "unfor_compare_in", dbw, doff, dcol, drefs, n,
                                dict(args=(s.lo, s.bits, ptr, negate, code, inplace.data_ptr()), output=inplace))
            want = want_in(vals, s.members, negate, COMBINE[code], words).reshape(n, 32)
            assert flag == 1 and np.array_equal(g[ok], want[ok]), (what, "in place")
            assert np.array_equal(g[BAD_W], words.reshape(n, 32)[BAD_W]), (what, "in place: the skipped block keeps its incoming mask")
            # the Python call on the sound column, the window as given
            got = got_mask(fl.unfor_compare_in_widths(dw, doff, dcol, drefs, s.member_set(fl, ty), negate=bool(negate), mask=dm, combine="or"))
            assert np.array_equal(got, want_in(vals, s.members, negate, "or", words)), (what, "python")
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_compare_in_widths(dbw, doff, dcol, drefs, [int(refs[PIVOT])])
        assert ei.value.status == 1, (ty, policy, n)


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_columns_and_member_lists(fl, oracle, ty):
    """FoR.unfor_compare_in at widths 0, 1, T // 2 + 1 and T over 37 blocks; `members` as plain lists and arrays (built by member_set
    inside the call), as a member_set on the device reused over calls, signed values; a window that excludes EVERY block; the three
    combiners, negate, in place; one scalar reference"""
    T = tbits(ty)
    N = 1 << T
    n = 37
    rng = np.random.default_rng(42000 + T)
    bits, words = column_masks(n, 42001)
    dm = to_dev(words)
    for w in (0, 1, T // 2 + 1, T):
        pk = values(ty, n * packed_len(ty, w), 42100 + 64 * T + w)
        span = min(600, N // 4)
        refs = np.array([(N - span // 2 + int(x)) % N for x in rng.integers(0, span, size=n)], dtype=np.uint64).astype(TYPES[ty][0])
        vals = oracle.batch("unfor_pack", ty, w, pk, aux=refs, n_blocks=n)
        dpk, drefs = to_dev(pk), to_dev(refs)
        top = (1 << w) - 1
        if top + span < 1 << 26:
            pick = rng.choice(vals, size=40)                              # values the column holds (some below 2^T, some wrapped)
        else:                                                             # values too far apart for one window: one of them, and near it
            pick = vals[100] + np.arange(40, dtype=vals.dtype) * vals.dtype.type(3)
        signed = pick.view(np.int64) if T == 64 else np.where(pick.astype(np.int64) >= N // 2, pick.astype(np.int64) - N, pick.astype(np.int64))
        lists = {"a list of ints": [int(v) for v in pick], "an array": pick, "one value": [int(pick[0])], "no value": []}
        for name, members in lists.items():
            mv = np.array([int(v) for v in members], dtype=np.uint64).astype(TYPES[ty][0])
            for negate in (False, True):
                for cb in COMBINE:
                    args = dict(mask=dm, combine=cb) if cb != "new" else {}
                    got = got_mask(fl.FoR.unfor_compare_in(w, dpk, drefs, members, negate=negate, n_blocks=n, output=prefilled(n), **args))
                    assert np.array_equal(got, want_in(vals, mv, negate, cb, words)), (ty, w, name, negate, cb)
        ms = fl.member_set(ty, signed, signed=True, device="cuda:0")
        assert ms.words.is_cuda and ms.bits <= top + span + 120
        for negate in (False, True):
            inplace = dm.clone()
            out = fl.FoR.unfor_compare_in(w, dpk, drefs, ms, negate=negate, mask=inplace, combine="and", output=inplace)
            assert out is inplace and np.array_equal(got_mask(inplace), want_in(vals, pick, negate, "and", words)), (ty, w, "signed, in place")
        if w < T:                                                          # every block lies outside this window: no packed byte is read
            s = Set(ty, "outside", N // 2 - 50, 100 if T > 8 else 20, half(rng, 20))
            assert not np.isin(vals, s.members).any()
            for negate in (False, True):
                got = got_mask(fl.FoR.unfor_compare_in(w, dpk, drefs, s.member_set(fl, ty), negate=negate, mask=dm, combine="or", n_blocks=n))
                assert np.array_equal(got, want_in(vals, s.members, negate, "or", words)), (ty, w, "outside", negate)
        r0 = int(refs[1])
        vals0 = oracle.batch("unfor_pack", ty, w, pk, aux=np.full(n, r0, dtype=refs.dtype), n_blocks=n)
        near = min(top, 1000)                                             # (members a window of at most 2^27 bits holds)
        mv = np.array([(r0 + (near >> 1)) % N, r0, (r0 + near) % N], dtype=np.uint64).astype(TYPES[ty][0])
        got = got_mask(fl.FoR.unfor_compare_in(w, dpk, r0, mv, n_blocks=n))
        assert np.array_equal(got, want_in(vals0, mv, False)), (ty, w, "scalar reference")


@pytest.mark.parametrize("ty", TYS)
def test_mixed_column_outside_every_window_and_empty_columns(fl, oracle, ty):
    """a mixed-width column of narrow blocks and a window none of them reaches (every block decided from its metadata), negate both
    ways; a column of width-0 blocks with no packed bytes; an empty column; a member set of another element type"""
    import torch
    T = tbits(ty)
    N = 1 << T
    n = 21
    rng = np.random.default_rng(43000 + T)
    widths = rng.integers(0, 5, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 43001)
    refs = rng.integers(0, min(N // 4, 5000), size=n).astype(np.uint64).astype(TYPES[ty][0])
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    dcol, drefs = to_dev(col), to_dev(refs)
    s = Set(ty, "outside", N // 2, 33, half(rng, 33, 0, 32), garbage=True)
    assert not np.isin(vals, s.members).any()
    for negate in (False, True):
        got = got_mask(fl.unfor_compare_in_widths(dw, doff, dcol, drefs, s.member_set(fl, ty), negate=negate, output=prefilled(n)))
        assert np.array_equal(got, want_in(vals, s.members, negate)), (ty, negate)
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    vz = np.repeat(refs[:5], 1024)
    for members in ([int(refs[0]), int(refs[3])], [(int(refs[0]) + 1) % N], np.concatenate([refs[:5], refs[:5] + refs.dtype.type(1)])):
        mv = np.array([int(v) for v in members], dtype=np.uint64).astype(TYPES[ty][0])
        got = got_mask(fl.unfor_compare_in_widths(z, zoff, empty, drefs[:5], members))
        assert np.array_equal(got, want_in(vz, mv, False)), (ty, "width 0", members)
        got = got_mask(fl.FoR.unfor_compare_in(0, empty, drefs[:5], members, negate=True, n_blocks=5))
        assert np.array_equal(got, want_in(vz, mv, True)), (ty, "uniform width 0", members)
    ew, eo = torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0")
    assert fl.unfor_compare_in_widths(ew, eo, empty, drefs[:1], [1, 2]).numel() == 0
    assert fl.FoR.unfor_compare_in(3, empty, 0, [1, 2]).numel() == 0
    other = "u16" if ty != "u16" else "u32"
    with pytest.raises(TypeError):
        fl.unfor_compare_in_widths(dw, doff, dcol, drefs, fl.member_set(other, [1, 2]))


@pytest.mark.parametrize("ty", TYS)
def test_an_empty_set_never_looks_at_its_words(fl, ty):
    """set_bits == 0 through the C ABI, both forms, 3 blocks: set_words is deliberately NOT NULL and NOT 16-byte aligned (4 bytes into a
    live allocation).  The call must be accepted and answer for the empty set: no row is a member, every row is under negate."""
    import ctypes
    import torch
    T, n, w = tbits(ty), 3, 5
    dpk, drefs = to_dev(values(ty, n * packed_len(ty, w), 43100 + T)), to_dev(values(ty, n, 43101 + T))
    dw = torch.full((n,), w, dtype=torch.uint8, device="cuda:0")
    doff, _ = fl.widths_to_offsets(ty, dw)
    live = torch.full((64,), PREFILL, dtype=torch.int32, device="cuda:0")
    odd = live.data_ptr() + 4
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = fl.load()
    for negate in (0, 1):
        mask, err = prefilled(n), torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(lib, f"fl_{ty}_unfor_compare_in")(w, dpk.data_ptr(), drefs.data_ptr(), 1, 17, 0, odd, negate, 0, None, n, mask.data_ptr(), stream)
        assert rc == 0 and (got_mask(mask) == -negate).all(), (ty, negate, rc, "uniform")
        mask = prefilled(n)
        rc = getattr(lib, f"fl_{ty}_unfor_compare_in_widths")(dw.data_ptr(), doff.data_ptr(), dpk.data_ptr(), dpk.numel() * (T // 8), drefs.data_ptr(), 1,
                                                              17, 0, odd, negate, 0, None, n, mask.data_ptr(), err.data_ptr(), stream)
        assert rc == 0 and int(err.item()) == 0 and (got_mask(mask) == -negate).all(), (ty, negate, rc, "mixed")
    assert (live.cpu().numpy() == PREFILL).all()


def test_chain_in_and_between_then_aggregate(fl):
    """WHERE mode IN (1, 4, 6) AND ts BETWEEN a AND b, then COUNT / SUM / MIN / MAX of z: three small columns of different types
    through the library's own encoder, the second predicate chained in place through the first one's mask, against numpy."""
    import torch
    n = 96
    rng = np.random.default_rng(44000)
    ts = (np.arange(n * 1024, dtype=np.uint64) * 37 + 1000).astype(np.uint32)                # ascending: most blocks decided
    mode = rng.integers(0, 7, size=n * 1024).astype(np.uint8)
    mode[17 * 1024:19 * 1024] = 4                                                             # width-0 blocks: one bitmap bit each
    mode[30 * 1024:31 * 1024] = 5
    mode[40 * 1024:42 * 1024] = rng.integers(2, 4, size=2048)                                 # inside the window, no member
    z = rng.integers(0, 50000, size=n * 1024).astype(np.uint16)
    cols = {}
    for name, ty, v in (("ts", "u32", ts), ("mode", "u8", mode), ("z", "u16", z)):
        dv = to_dev(v)
        mins, maxs = fl.BitPacking.block_min_max(dv)
        dw = fl.for_widths(mins, maxs)
        doff, dtotal = fl.widths_to_offsets(ty, dw)
        dpk = torch.zeros(max(int(dtotal.item()) // (tbits(ty) // 8), 1), dtype=getattr(torch, TDT[ty]), device="cuda:0")
        fl.for_pack_widths(dw, doff, dv, mins, dpk)
        cols[name] = (dw, doff, dpk, mins)
    a, b = int(ts[15 * 1024 + 300]), int(ts[45 * 1024 + 77])
    members = fl.member_set("u8", [1, 4, 6], device="cuda:0")
    assert (members.lo, members.bits) == (1, 6)
    m = fl.unfor_compare_in_widths(*cols["mode"], members)
    assert np.array_equal(got_mask(m), np.packbits(np.isin(mode, [1, 4, 6]), bitorder="little").view(np.int32))
    out = fl.unfor_compare_range_widths(*cols["ts"], a, b, mask=m, combine="and", output=m)
    assert out is m
    keep = np.isin(mode, [1, 4, 6]) & (ts >= a) & (ts <= b)
    assert np.array_equal(got_mask(m), np.packbits(keep, bitorder="little").view(np.int32))
    # the other order: the interval first, the set chained through its mask in place
    m2 = fl.unfor_compare_range_widths(*cols["ts"], a, b)
    fl.unfor_compare_in_widths(*cols["mode"], members, mask=m2, combine="and", output=m2)
    assert np.array_equal(got_mask(m2), got_mask(m))
    result, _ = fl.unfor_aggregate_widths(*cols["z"], mask=m)
    kept = z[keep].astype(np.uint64)
    assert kept.size > 2048
    assert [int(x) for x in result.cpu().numpy().view(np.uint64)] == [kept.size, int(kept.sum()), int(kept.min()), int(kept.max())]
