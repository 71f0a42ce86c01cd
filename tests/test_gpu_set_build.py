"""GPU: unfor_set_build / unfor_set_build_widths -- the member set of the values a mask keeps of a FoR-packed column, ORed into a
window's bitmap on the device -- against numpy over the oracle's unfor_pack per block (ffor.rs:38-50):
    j = (vals[keep] - lo) mod 2^T;   words = PREFILL | bits(j[j < bits]);   stats = prefill + (count inside, count outside)
(tests/set_build_data.py).  The expected side never reads the kernel's bitmap."""
import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TDT, TYS, got_mask, mixed_column, to_dev, u64_of
from set_build_data import STATS_PREFILL, encode, expected_build, prefill_words, raw_build, stats_of, words_of
from test_gpu_for_compare_in import PIVOT, column_for_sets, sets_for
from test_gpu_for_consumer_shapes import BAD_W, SHAPES, ZERO_W, column_masks

pytestmark = pytest.mark.gpu

RUN_OF_16 = 2 + 256 * 3 + 65536 * 16           # kernel policy: a wavefront's run is at least 16 blocks


def windows_for(ty, widths, refs, rng):
    """(name, lo, bits) of sets_for's windows; the tier boundary sits at 65536 / 65537 bits for T > 16 (u8 / u16: 2^T bits is the
    largest window, and sets_for has it)"""
    T = tbits(ty)
    out = [(s.name, s.lo, s.bits) for s in sets_for(ty, widths, refs, rng)]
    if T > 16:
        assert any(b == 65536 for _, _, b in out)
        out.append(("65537 bits", (int(refs[PIVOT]) - 30000) % (1 << T), 65537))
    else:
        assert any(b == 1 << T for _, _, b in out)
    return out


def check_call(fl, ty, col, n, dmask, lo, bits, want_vals, keep, rng, what, flag_want=0, with_stats=True):
    """one raw call into a prefilled bitmap and prefilled counters, bit for bit"""
    dw, doff, dcol, drefs = col
    pre = prefill_words(bits, rng)
    dwords = to_dev(pre.view(np.int32)) if bits else None
    dstats = to_dev(STATS_PREFILL.view(np.int64)) if with_stats else None
    rc, flag = raw_build(fl, ty, dw, doff, dcol, drefs, n, dmask, lo, bits, dwords, dstats)
    assert rc == 0 and flag == flag_want, (what, rc, flag)
    words, stats = expected_build(ty, want_vals, keep, lo, bits, pre, STATS_PREFILL)
    if bits:
        got = words_of(dwords)
        assert np.array_equal(got, words), (what, np.flatnonzero(got != words)[:8])
        if bits % 32:
            assert got[-1] >> np.uint32(bits % 32) == 0xFFFFFFFF >> (bits % 32), (what, "garbage above set_bits was changed")
    if with_stats:
        assert stats_of(dstats).tolist() == stats.tolist(), (what, stats_of(dstats), stats)


@pytest.mark.parametrize("policy,bpw", SHAPES)
@pytest.mark.parametrize("ty", TYS)
def test_every_window_over_tails_and_special_blocks(fl, oracle, kernel_policy, ty, policy, bpw):
    """n = 2 * 4 * bpw + r blocks under every launch shape; width-1 and width-T blocks, a width-0 block, a wrapping block, a far block
    and a block of width T + 1 (flag 1; bitmap and stats are those of the column without it); mask None and a mask with an empty and
    a full block; every window of sets_for and the tier boundary; stats NULL; set_bits == 0."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    for r in sorted({1, bpw - 1, bpw + 1} - {0}):
        n = 2 * 4 * bpw + r
        widths, refs = column_for_sets(ty, n, 61000 + 64 * T + n)
        dw, doff, col, blocks = mixed_column(ty, widths, 61100 + n)
        vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
        bad_w = widths.astype(np.uint8)
        bad_w[BAD_W] = T + 1
        dbw = torch.from_numpy(bad_w).cuda()
        dcol, drefs = to_dev(col), to_dev(refs)
        bits_m, words_m = column_masks(n, 61200 + n)
        dm = to_dev(words_m)
        sound = np.repeat(np.arange(n) != BAD_W, 1024)
        rng = np.random.default_rng(61300 + n)
        seen_zero = False
        for name, lo, bits in windows_for(ty, widths, refs, rng):
            what = (ty, policy, n, name)
            seen_zero |= bits == 0
            for mname, dmask, keep in (("no mask", None, np.ones(n * 1024, bool)), ("mask", dm, bits_m)):
                check_call(fl, ty, (dw, doff, dcol, drefs), n, dmask, lo, bits, vals, keep, rng, (*what, mname))
                check_call(fl, ty, (dbw, doff, dcol, drefs), n, dmask, lo, bits, vals, keep & sound, rng, (*what, mname, "width T + 1"), flag_want=1)
            check_call(fl, ty, (dw, doff, dcol, drefs), n, dm, lo, bits, vals, bits_m, rng, (*what, "stats NULL"), with_stats=False)
        assert seen_zero
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_set_build_widths(dbw, doff, dcol, drefs, int(refs[PIVOT]), 40)
        assert ei.value.status == 1, (ty, policy, n)


def tier_windows(ty, centre):
    """a window of each tier the type has around `centre`: (lo, bits)"""
    T = tbits(ty)
    N = 1 << T
    out = [((centre - 1500) % N, min(4000, N))]
    if T > 16:
        out.append(((centre - 30000) % N, 70001))
    return out


def clustered_column(ty, n, seed):
    """(widths, refs): narrow blocks within a few thousand values around 2^T - 1 (they wrap), one width-0 block"""
    T = tbits(ty)
    N = 1 << T
    rs = np.random.default_rng(seed)
    widths = rs.integers(1, min(T, 9) + 1, size=n)
    widths[ZERO_W % n] = 0
    span = min(3000, N // 2)
    refs = np.array([(N - span // 2 + int(x)) % N for x in rs.integers(0, span, size=n)], dtype=np.uint64).astype(TYPES[ty][0])
    return widths, refs


@pytest.mark.parametrize("ty", TYS)
def test_union_of_two_calls_and_into(fl, oracle, ty):
    """two calls with complementary masks into one bitmap equal one call with mask=None, through the C ABI and through into=; into=
    refuses anything but a device MemberSet of the same ty, lo and bits"""
    import torch
    T = tbits(ty)
    n = 23
    widths, refs = clustered_column(ty, n, 62000 + T)
    dw, doff, col, blocks = mixed_column(ty, widths, 62001)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    dcol, drefs = to_dev(col), to_dev(refs)
    bits_m, words_m = column_masks(n, 62002)
    dm, dnot = to_dev(words_m), to_dev(~words_m)
    for lo, bits in tier_windows(ty, int(refs[1])):
        words, stats = expected_build(ty, vals, None, lo, bits)
        assert 0 < stats[0] and words.any()
        one, st = fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits)
        assert (one.ty, one.lo, one.bits) == (ty, lo, bits) and one.words.is_cuda and one.words.dtype == torch.int32
        assert np.array_equal(words_of(one.words), words) and stats_of(st).tolist() == stats.tolist(), (ty, bits)
        dwords = torch.zeros((bits + 31) // 32, dtype=torch.int32, device="cuda:0")
        dstats = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        for m in (dm, dnot):
            assert raw_build(fl, ty, dw, doff, dcol, drefs, n, m, lo, bits, dwords, dstats) == (0, 0)
        assert np.array_equal(words_of(dwords), words) and stats_of(dstats).tolist() == stats.tolist(), (ty, bits, "two calls")
        a, sa = fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits, mask=dm)
        wa, _ = expected_build(ty, vals, bits_m, lo, bits)
        assert np.array_equal(words_of(a.words), wa)
        b, sb = fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits, mask=dnot, into=a)
        assert b is a and np.array_equal(words_of(a.words), words), (ty, bits, "into")
        assert (stats_of(sa) + stats_of(sb)).tolist() == stats.tolist()
        with pytest.raises(ValueError):
            fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo + 1, bits, into=a)
        with pytest.raises(ValueError):
            fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits - 1, into=a)
        with pytest.raises(TypeError):
            fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits, into=fl.MemberSet(ty, lo, bits, words))      # host words
        with pytest.raises(TypeError):
            fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits, into=a.words)
        other = "u16" if ty != "u16" else "u32"
        with pytest.raises(TypeError):
            fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits, into=fl.MemberSet(other, lo, bits, a.words))
    with pytest.raises(ValueError):
        fl.unfor_set_build_widths(dw, doff, dcol, drefs, 0, min(1 << T, 1 << 32) + 1)


@pytest.mark.parametrize("variant", ["1", "2"])
@pytest.mark.parametrize("ty", ["u32", "u64"])
def test_both_memory_tier_variants_give_the_same_bits(fl, oracle, monkeypatch, ty, variant):
    """one atomic per element (1) and test-before-set (2), chosen as the timing tool chooses them: the same bitmap and counters, into
    a prefilled bitmap, with a mask, a width-0 block inside the window and a block of width T + 1"""
    import torch
    monkeypatch.setenv("FL_INTERNAL_SET_BUILD_VARIANT", variant)
    T = tbits(ty)
    n = 41
    widths, refs = clustered_column(ty, n, 67000 + T)
    dw, doff, col, blocks = mixed_column(ty, widths, 67001)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    bad_w = widths.astype(np.uint8)
    bad_w[BAD_W] = T + 1
    dcol, drefs = to_dev(col), to_dev(refs)
    keep, words_m = column_masks(n, 67002)
    rng = np.random.default_rng(67003)
    lo, bits = tier_windows(ty, int(refs[ZERO_W]))[1]
    assert bits > 65536
    sound = np.repeat(np.arange(n) != BAD_W, 1024)
    for dmask, kept in ((None, np.ones(n * 1024, bool)), (to_dev(words_m), keep)):
        check_call(fl, ty, (dw, doff, dcol, drefs), n, dmask, lo, bits, vals, kept, rng, (ty, variant))
        check_call(fl, ty, (torch.from_numpy(bad_w).cuda(), doff, dcol, drefs), n, dmask, lo, bits, vals, kept & sound, rng, (ty, variant, "bad"), flag_want=1)
        # a second call into the first one's bitmap: every bit is already set (test-before-set issues nothing), the counters still add
        first, st1 = fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits, mask=dmask)
        before = words_of(first.words).copy()
        again, st2 = fl.unfor_set_build_widths(dw, doff, dcol, drefs, lo, bits, mask=dmask, into=first)
        assert np.array_equal(words_of(again.words), before) and stats_of(st1).tolist() == stats_of(st2).tolist(), (ty, variant)


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_columns(fl, oracle, ty):
    """FoR.unfor_set_build at widths 0, 1, T // 2 + 1 and T over 37 blocks, one scalar reference, mask=None, a window of each tier"""
    T = tbits(ty)
    N = 1 << T
    n = 37
    for w in (0, 1, T // 2 + 1, T):
        pk = values(ty, n * packed_len(ty, w), 63000 + 64 * T + w)
        r0 = (N - 700) % N
        vals = oracle.batch("unfor_pack", ty, w, pk, aux=np.full(n, r0, dtype=TYPES[ty][0]), n_blocks=n)
        dpk = to_dev(pk)
        for lo, bits in tier_windows(ty, r0) + [((r0 + 5) % N, 0)]:
            words, stats = expected_build(ty, vals, None, lo, bits)
            ms, st = fl.FoR.unfor_set_build(w, dpk, r0, lo, bits, n_blocks=n)
            assert np.array_equal(words_of(ms.words), words) and stats_of(st).tolist() == stats.tolist(), (ty, w, lo, bits)
            assert int(stats.sum()) == n * 1024
        if w <= 1:
            assert stats_of(fl.FoR.unfor_set_build(w, dpk, r0, (r0 - 3) % N, 8, n_blocks=n)[1]).tolist() == [n * 1024, 0]


@pytest.mark.parametrize("ty", TYS)
def test_contention_and_density_in_both_tiers(fl, oracle, ty):
    """9 decoded blocks whose 9216 values are one value; 1024 consecutive values = 32 full words with no neighbour touched; values
    alternating between bit 31 of one word and bit 0 of the next"""
    import torch
    T = tbits(ty)
    N = 1 << T
    esz = T // 8
    centre = N // 2 + 64
    for lo, bits in tier_windows(ty, centre):
        # one value, width 3, all fields 0: every lane of every instruction hits one bit
        n = 9
        dw = torch.full((n,), 3, dtype=torch.uint8, device="cuda:0")
        doff = torch.arange(n, dtype=torch.int64, device="cuda:0") * 384
        dcol = torch.zeros(n * 384 // esz, dtype=getattr(torch, TDT[ty]), device="cuda:0")
        ref = np.array([(lo + 77) % N], dtype=np.uint64).astype(TYPES[ty][0])
        dwords = torch.zeros((bits + 31) // 32, dtype=torch.int32, device="cuda:0")
        dstats = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        assert raw_build(fl, ty, dw, doff, dcol, to_dev(ref), n, None, lo, bits, dwords, dstats, ref_stride=0) == (0, 0)
        want = np.zeros((bits + 31) // 32, dtype=np.uint32)
        want[77 >> 5] = 1 << (77 & 31)
        assert np.array_equal(words_of(dwords), want) and stats_of(dstats).tolist() == [9216, 0], (ty, bits, "one value")
        if T == 8:
            continue                                                        # (a u8 block of 1024 consecutive values does not exist)
        # 1024 consecutive values from a word boundary: words 2 .. 33 full, their neighbours clear
        run = ((np.arange(1024, dtype=np.uint64) + np.uint64((lo + 64) % N)) & np.uint64(N - 1)).astype(TYPES[ty][0])
        alt = ((np.tile(np.array([31, 32], dtype=np.uint64), 512) + np.uint64((lo + 320) % N)) & np.uint64(N - 1)).astype(TYPES[ty][0])
        for name, vals, full_words in (("consecutive", run, range(2, 34)), ("bit 31 / bit 0", alt, ())):
            col = encode(fl, ty, vals)
            ms, st = fl.unfor_set_build_widths(*col, lo, bits)
            words, stats = expected_build(ty, vals, None, lo, bits)
            got = words_of(ms.words)
            assert np.array_equal(got, words) and stats_of(st).tolist() == stats.tolist() == [1024, 0], (ty, bits, name)
            assert all(got[i] == 0xFFFFFFFF for i in full_words) and int(np.count_nonzero(got)) == (32 if full_words else 2), (ty, bits, name)
        assert got[10] == 1 << 31 and got[11] == 1


@pytest.mark.parametrize("ty", TYS)
def test_persistent_runs_flush_what_they_own(fl, oracle, kernel_policy, ty):
    """the LDS tier under runs of at least 16 blocks: members set only by the first, and only by the last, block of the column; 1, 2
    and 3 blocks (most wavefronts own no block and flush nothing); a window with a partial last word and every bit of it set"""
    kernel_policy(RUN_OF_16)
    T = tbits(ty)
    N = 1 << T
    lo, bits = N // 2 - 100, min(1000, N - 56)
    inside = ((np.arange(1024, dtype=np.uint64) % np.uint64(bits) + np.uint64(lo)) & np.uint64(N - 1)).astype(TYPES[ty][0])   # every bit of the window
    outside = ((np.arange(1024, dtype=np.uint64) % np.uint64(50) + np.uint64(lo + bits + 3)) & np.uint64(N - 1)).astype(TYPES[ty][0])
    rng = np.random.default_rng(64000 + T)
    some = ((rng.integers(0, bits, size=1024).astype(np.uint64) + np.uint64(lo)) & np.uint64(N - 1)).astype(TYPES[ty][0])
    for name, n, first, last in (("first block only", 50, some, outside), ("last block only", 50, outside, some), ("one block", 1, inside, inside),
                                 ("two blocks", 2, some, inside), ("three blocks", 3, outside, some), ("every bit", 35, inside, outside)):
        vals = np.concatenate([first] + [outside] * max(n - 2, 0) + ([last] if n > 1 else []))
        assert vals.size == n * 1024
        words, stats = expected_build(ty, vals, None, lo, bits)
        ms, st = fl.unfor_set_build_widths(*encode(fl, ty, vals), lo, bits)
        assert np.array_equal(words_of(ms.words), words) and stats_of(st).tolist() == stats.tolist(), (ty, name)
        if name in ("one block", "every bit"):
            assert bits % 32 and (words[:-1] == 0xFFFFFFFF).all() and words[-1] == (1 << (bits % 32)) - 1, (ty, name)


@pytest.mark.parametrize("ty", TYS)
def test_round_trip_with_member_set_and_compare_in(fl, oracle, ty):
    """with lo, bits taken from fl.member_set(ty, vals[keep]) the built words equal that member set's words bit for bit, and
    unfor_compare_in_widths of the same column with the built set yields exactly the rows whose value occurs among the kept rows"""
    T = tbits(ty)
    n = 29
    widths, refs = clustered_column(ty, n, 65000 + T)
    dw, doff, col, blocks = mixed_column(ty, widths, 65001)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
    dcol, drefs = to_dev(col), to_dev(refs)
    keep, words_m = column_masks(n, 65002)
    keep &= np.random.default_rng(65003).random(n * 1024) < 0.1
    words_m = np.packbits(keep, bitorder="little").view(np.int32)
    host = fl.member_set(ty, vals[keep])
    assert 1 < host.bits <= 1 << 16
    built, st = fl.unfor_set_build_widths(dw, doff, dcol, drefs, host.lo, host.bits, mask=to_dev(words_m))
    assert np.array_equal(words_of(built.words), host.words), ty
    assert stats_of(st).tolist() == [int(keep.sum()), 0]
    got = got_mask(fl.unfor_compare_in_widths(dw, doff, dcol, drefs, built))
    assert np.array_equal(got, np.packbits(np.isin(vals, vals[keep]), bitorder="little").view(np.int32)), ty


def test_q4_chain(fl):
    """SELECT o_priority, COUNT(*) FROM orders WHERE o_key IN (SELECT l_key FROM lineitem WHERE l_commit < l_receipt) GROUP BY
    o_priority: three small columns through the library's own encoder, 96 blocks on the build side and 24 on the probe side, against
    numpy isin and bincount"""
    rng = np.random.default_rng(66000)
    nl, no = 96, 24
    o_key = (np.arange(no * 1024, dtype=np.uint64) * 4 + 100000).astype(np.uint32)        # ascending, sparse
    o_pri = rng.integers(0, 5, size=no * 1024).astype(np.uint8)
    l_key = np.sort(rng.choice(o_key, size=nl * 1024)).astype(np.uint32)                      # a foreign key in table order
    l_key[5 * 1024:6 * 1024] = 7                                                              # keys no order has: outside the window
    commit = rng.integers(9000, 9400, size=nl * 1024).astype(np.uint16)
    receipt = (commit.astype(np.int64) + rng.integers(-30, 10, size=nl * 1024)).astype(np.uint16)
    lk, ok, cm, rc, pr = (encode(fl, ty, v) for ty, v in (("u32", l_key), ("u32", o_key), ("u16", commit), ("u16", receipt), ("u8", o_pri)))
    m = fl.unfor_compare_columns_widths(*cm, "<", *rc)
    late = commit < receipt
    assert np.array_equal(got_mask(m), np.packbits(late, bitorder="little").view(np.int32))
    lo, bits = fl.column_window("u32", ok[0], ok[3])
    assert lo == int(o_key.min()) and lo + bits - 1 >= int(o_key.max())
    s, stats = fl.unfor_set_build_widths(*lk, lo, bits, mask=m)
    st = stats_of(stats)
    assert int(st[0]) + int(st[1]) == int(late.sum()) and int(st[1]) == int((late & (l_key == 7)).sum()) > 0
    hit = fl.unfor_compare_in_widths(*ok, s)
    want_hit = np.isin(o_key, l_key[late])
    assert np.array_equal(got_mask(hit), np.packbits(want_hit, bitorder="little").view(np.int32))
    by = u64_of(fl.unfor_aggregate_by_widths(*pr, *pr, mask=hit))                             # COUNT(*) per priority
    assert by[:, 0].tolist() == np.bincount(o_pri[want_hit], minlength=256).tolist() and 0 < want_hit.sum() < want_hit.size
