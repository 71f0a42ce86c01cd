"""GPU: unfor_aggregate_by_window / unfor_aggregate_by_window_widths -- COUNT / SUM / MIN / MAX of a FoR-packed value column grouped by a
FoR-packed key column of the same type inside a dense window of the key domain, accumulated into the caller's arrays -- against numpy
over the oracle's unfor_pack per block (ffor.rs:38-50):
    j = (keys[keep] - lo) mod 2^T;   np.add.at / np.minimum.at / np.maximum.at(PREFILL, j[j < n_groups], vals);   stats = prefill +
    (count inside, count outside)
(tests/aggregate_by_window_data.py).  The expected side never reads the kernel's arrays."""
import numpy as np
import pytest

from aggregate_by_window_data import (LDS_GROUPS, STATS_PREFILL, WHAT, expected_table, identities, prefill_arrays, raw_window, table_arrays,
                                      u64)
from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TYS, got_mask, mixed_column, to_dev
from set_build_data import encode
from test_gpu_for_compare_in import FAR, PIVOT, WRAP, column_for_sets
from test_gpu_for_consumer_shapes import BAD_W, SHAPES, ZERO_W, column_masks

pytestmark = pytest.mark.gpu

BAD_V = 0                                        # the block of the VALUE column that gets width T + 1 (the key column's: BAD_W)
RUN_OF_16 = 2 + 256 * 3 + 65536 * 16             # kernel policy: a wavefront's run is at least 16 blocks


def dev64(a):
    return to_dev(a.view(np.int64))


def value_widths(ty, n, seed):
    """widths of the value column: random ones, 0 / 1 / T among them, next to the key column's special blocks"""
    T = tbits(ty)
    w = np.random.default_rng(seed).integers(0, T + 1, size=n)
    w[[1, PIVOT, WRAP, ZERO_W, FAR]] = [T, 1, 0, T // 2 + 1, 0]
    return w


def windows_for(ty, refs):
    """(name, lo, n_groups): 0, 1, 255, 256, 257 and, for T > 16, 70001 groups that END inside the pivot block's 64 keys (the keys
    straddle every one of them), and two windows of both tiers around the width-0 key block's key"""
    T = tbits(ty)
    N = 1 << T
    P, Z = int(refs[PIVOT]), int(refs[ZERO_W])
    sizes = [g for g in (0, 1, 255, 256, 257, 70001 if T > 16 else None) if g is not None and g <= N]
    out = [(f"{g} groups", (P + 30 - max(g, 1) + 1) % N, g) for g in sizes]
    out.append(("the width-0 key block inside", (Z - 3) % N, min(9, N)))
    if T > 8:
        out.append(("the width-0 key block inside, memory tier", (Z - 200) % N, 300))
    return out


def check_call(fl, ty, val, key, n, dmask, lo, ng, vals, keys, keep, rng, what, flag_want=0, which=(1, 1, 1, 1), with_stats=True):
    """one raw call into prefilled arrays and prefilled counters, bit for bit; which[i] == 0: array i is passed as NULL"""
    pre = prefill_arrays(ng, rng)
    darrays = [dev64(a) if on and ng else None for a, on in zip(pre, which)]
    dstats = dev64(STATS_PREFILL) if with_stats else None
    rc, flag = raw_window(fl, ty, val, key, n, dmask, lo, ng, darrays, dstats)
    assert rc == 0 and flag == flag_want, (what, rc, flag)
    want, stats = expected_table(ty, vals, keys, keep, lo, ng, pre, STATS_PREFILL)
    for name, d, w in zip(WHAT, darrays, want):
        if d is not None:
            got = u64(d)
            assert np.array_equal(got, w), (what, name, np.flatnonzero(got != w)[:8], got[got != w][:4], w[got != w][:4])
    if with_stats:
        assert u64(dstats).tolist() == stats.tolist(), (what, u64(dstats), stats)
    return stats - STATS_PREFILL


@pytest.mark.parametrize("policy,bpw", SHAPES)
@pytest.mark.parametrize("ty", TYS)
def test_every_window_over_tails_and_special_blocks(fl, oracle, kernel_policy, ty, policy, bpw):
    """n = 2 * 4 * bpw + r blocks under every launch shape.  Key column: width-1 and width-T blocks, a width-0 block (inside and outside
    the windows), a wrapping block, a far block; value column: widths 0 / 1 / T; a block of width T + 1 in either column (flag 1;
    arrays and stats are those of the column without it); mask None and a mask with an empty and a full block; windows of 0, 1, 255,
    256, 257 and 70001 groups into prefilled arrays; stats NULL."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    for r in sorted({1, bpw - 1, bpw + 1} - {0}):
        n = 2 * 4 * bpw + r
        kw, krefs = column_for_sets(ty, n, 91000 + 64 * T + n)
        dkw, dkoff, kcol, kblocks = mixed_column(ty, kw, 91100 + n)
        keys = np.concatenate([oracle.unfor_pack(ty, w, pk, krefs[b]) for b, (w, pk) in enumerate(kblocks)])
        vw = value_widths(ty, n, 91200 + n)
        vrefs = values(ty, n, 91300 + n)
        dvw, dvoff, vcol, vblocks = mixed_column(ty, vw, 91400 + n)
        vals = np.concatenate([oracle.unfor_pack(ty, w, pk, vrefs[b]) for b, (w, pk) in enumerate(vblocks)])
        bad_k, bad_v = kw.astype(np.uint8), vw.astype(np.uint8)
        bad_k[BAD_W] = T + 1
        bad_v[BAD_V] = T + 1
        dbk, dbv = torch.from_numpy(bad_k).cuda(), torch.from_numpy(bad_v).cuda()
        val, key = (dvw, dvoff, to_dev(vcol), to_dev(vrefs)), (dkw, dkoff, to_dev(kcol), to_dev(krefs))
        bits_m, words_m = column_masks(n, 91500 + n)
        dm = to_dev(words_m)
        every = np.ones(n * 1024, bool)
        rng = np.random.default_rng(91600 + n)
        zero_block, straddled = set(), []
        for name, lo, ng in windows_for(ty, krefs):
            what = (ty, policy, n, name)
            zero_block.add((ng > 0, (int(krefs[ZERO_W]) - lo) % (1 << T) < ng))
            for mname, dmask, keep in (("no mask", None, every), ("mask", dm, bits_m)):
                added = check_call(fl, ty, val, key, n, dmask, lo, ng, vals, keys, keep, rng, (*what, mname))
                assert int(added.sum()) == int(keep.sum()), (what, mname, added)
                if dmask is None and 0 < ng < 1 << T:
                    straddled.append(added[0] > 0 and added[1] > 0)
            for bval, bkey, bad in (((dbv, *val[1:]), key, BAD_V), (val, (dbk, *key[1:]), BAD_W)):
                keep = bits_m & np.repeat(np.arange(n) != bad, 1024)
                check_call(fl, ty, bval, bkey, n, dm, lo, ng, vals, keys, keep, rng, (*what, "width T + 1 in block", bad), flag_want=1)
            check_call(fl, ty, val, key, n, dm, lo, ng, vals, keys, bits_m, rng, (*what, "stats NULL"), with_stats=False)
        assert {(True, True), (True, False)} <= zero_block and all(straddled), (ty, n, zero_block, straddled)
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_aggregate_by_window_widths(dvw, dvoff, val[2], val[3], dbk, dkoff, key[2], key[3], int(krefs[PIVOT]), 40)
        assert ei.value.status == 1, (ty, policy, n)


def tier_windows(ty, centre):
    """a window of each tier the type has around `centre`: (lo, n_groups)"""
    T = tbits(ty)
    N = 1 << T
    out = [((centre - 100) % N, min(LDS_GROUPS, N - 56))]
    if T > 8:
        out.append(((centre - 100) % N, 257))
    if T > 16:
        out.append(((centre - 30000) % N, 70001))
    return out


def clustered_keys(ty, n, seed):
    """(widths, refs) of a key column: narrow blocks within a few hundred keys around 2^T - 1 (they wrap), one width-0 block"""
    T = tbits(ty)
    N = 1 << T
    rs = np.random.default_rng(seed)
    widths = rs.integers(1, min(T, 7) + 1, size=n)
    widths[ZERO_W % n] = 0
    span = min(400, N // 2)
    refs = np.array([(N - span // 2 + int(x)) % N for x in rs.integers(0, span, size=n)], dtype=np.uint64).astype(TYPES[ty][0])
    return widths, refs


def two_columns(oracle, ty, n, seed):
    """a clustered key column and a random value column of n blocks: (val, key, vals, keys, key refs)"""
    T = tbits(ty)
    kw, krefs = clustered_keys(ty, n, seed)
    dkw, dkoff, kcol, kblocks = mixed_column(ty, kw, seed + 1)
    keys = np.concatenate([oracle.unfor_pack(ty, w, pk, krefs[b]) for b, (w, pk) in enumerate(kblocks)])
    vw = np.random.default_rng(seed + 2).integers(0, T + 1, size=n)
    vrefs = values(ty, n, seed + 3)
    dvw, dvoff, vcol, vblocks = mixed_column(ty, vw, seed + 4)
    vals = np.concatenate([oracle.unfor_pack(ty, w, pk, vrefs[b]) for b, (w, pk) in enumerate(vblocks)])
    return (dvw, dvoff, to_dev(vcol), to_dev(vrefs)), (dkw, dkoff, to_dev(kcol), to_dev(krefs)), vals, keys, krefs


@pytest.mark.parametrize("ty", TYS)
def test_every_null_combination(fl, oracle, ty):
    """each of the 16 NULL / non-NULL combinations of counts, sums, mins, maxs, in every tier the type has, with a mask: the arrays
    passed are exact, stats is counted whatever is passed (all four NULL included)"""
    n = 19
    val, key, vals, keys, krefs = two_columns(oracle, ty, n, 92000 + tbits(ty))
    bits_m, words_m = column_masks(n, 92010)
    dm = to_dev(words_m)
    rng = np.random.default_rng(92020)
    for lo, ng in tier_windows(ty, int(krefs[1])):
        for code in range(16):
            which = tuple((code >> i) & 1 for i in range(4))
            added = check_call(fl, ty, val, key, n, dm, lo, ng, vals, keys, bits_m, rng, (ty, ng, which), which=which)
            assert added[0] > 0


@pytest.mark.parametrize("ty", TYS)
def test_count_only_never_reads_the_value_column(fl, oracle, ty):
    """with sums, mins and maxs NULL the value column is not read: through the C ABI its packed pointer is NULL with packed_bytes == 0
    and widths 0 (its per-block checks still run and pass); packed=None in Python"""
    import torch
    n = 19
    val, key, vals, keys, krefs = two_columns(oracle, ty, n, 93000 + tbits(ty))
    zero_w = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    zero_off = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    none_val = (zero_w, zero_off, None, val[3])
    rng = np.random.default_rng(93010)
    for lo, ng in tier_windows(ty, int(krefs[1])):
        check_call(fl, ty, none_val, key, n, None, lo, ng, vals, keys, None, rng, (ty, ng, "NULL value column"), which=(1, 0, 0, 0))
        want, stats = expected_table(ty, keys, keys, None, lo, ng)
        table, st = fl.unfor_aggregate_by_window_widths(None, None, None, None, *key, lo, ng, what=("count",))
        assert table_arrays(table)[1:] == [None, None, None] and np.array_equal(table_arrays(table)[0], want[0]), (ty, ng)
        assert u64(st).tolist() == stats.tolist()
        with pytest.raises(ValueError):
            fl.unfor_aggregate_by_window_widths(None, None, None, None, *key, lo, ng)            # the default what names "sum"


def contended(ty, pattern):
    """three blocks whose keys take two neighbouring values in the given pattern (key width 1): all 64 lanes of an instruction hit two
    slots"""
    T = tbits(ty)
    N = 1 << T
    base = N // 2 + 40
    i = np.arange(3 * 1024, dtype=np.uint64)
    step = (i & np.uint64(1)) if pattern == "alternating" else ((i >> np.uint64(4)) & np.uint64(1))
    return ((step + np.uint64(base)) & np.uint64(N - 1)).astype(TYPES[ty][0]), base


@pytest.mark.parametrize("pattern", ["alternating", "runs of 16"])
@pytest.mark.parametrize("ty", TYS)
def test_no_update_is_lost_under_contention(fl, oracle, ty, pattern):
    """3072 rows on two neighbouring slots in both tiers (the memory tier forced with a 257-group window around them), values at
    2^T - 1 (a width-0 value column) and at 2^T - 1 / 2^T - 2 (decoded); for u64 the sums wrap mod 2^64"""
    T = tbits(ty)
    N = 1 << T
    keys, base = contended(ty, pattern)
    kcol = encode(fl, ty, keys)
    assert kcol[0].cpu().tolist() == [1, 1, 1]
    top = np.full(3 * 1024, N - 1, dtype=np.uint64).astype(TYPES[ty][0])
    mixed = (np.uint64(N - 1) - (np.arange(3 * 1024, dtype=np.uint64) % np.uint64(3) == 0).astype(np.uint64)).astype(TYPES[ty][0])
    for vname, vals in (("2^T - 1", top), ("2^T - 1 and 2^T - 2", mixed)):
        vcol = encode(fl, ty, vals)
        for lo, ng in [((base - 1) % N, 4)] + ([((base - 128) % N, 257)] if T > 8 else []):
            want, stats = expected_table(ty, vals, keys, None, lo, ng)
            table, st = fl.unfor_aggregate_by_window_widths(*vcol, *kcol, lo, ng, what=WHAT)
            got = table_arrays(table)
            for name, g, w in zip(WHAT, got, want):
                assert np.array_equal(g, w), (ty, pattern, vname, ng, name, g[g != w], w[g != w])
            assert u64(st).tolist() == stats.tolist() == [3072, 0]
            j = (base - lo) % N
            assert int(got[0][j]) + int(got[0][j + 1]) == 3072 and int(got[0].sum()) == 3072
            assert int(got[1][j]) == sum(int(v) for v in vals[keys == base]) % (1 << 64)
            if T == 64:
                assert sum(int(v) for v in vals[keys == base]) >= 1 << 64, "the sum must have wrapped"


@pytest.mark.parametrize("ty", TYS)
def test_two_calls_accumulate_into_one_table(fl, oracle, ty):
    """two calls with complementary masks into one table equal one call with mask=None, through the C ABI and through into=; into=
    refuses another ty, window or set of arrays"""
    import torch
    T = tbits(ty)
    n = 23
    val, key, vals, keys, krefs = two_columns(oracle, ty, n, 94000 + T)
    bits_m, words_m = column_masks(n, 94010)
    dm, dnot = to_dev(words_m), to_dev(~words_m)
    for lo, ng in tier_windows(ty, int(krefs[1])):
        want, stats = expected_table(ty, vals, keys, None, lo, ng)
        assert stats[0] > 0 and (ng > 257 or stats[1] > 0)                  # (the 70001-group window holds every clustered key)
        one, st = fl.unfor_aggregate_by_window_widths(*val, *key, lo, ng, what=WHAT)
        assert (one.ty, one.lo, one.n_groups) == (ty, lo, ng) and one.sums.is_cuda and one.sums.dtype == torch.int64
        assert all(np.array_equal(g, w) for g, w in zip(table_arrays(one), want)) and u64(st).tolist() == stats.tolist(), (ty, ng)
        darrays = [dev64(a) for a in identities(ng)]
        dstats = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        for m in (dm, dnot):
            assert raw_window(fl, ty, val, key, n, m, lo, ng, darrays, dstats) == (0, 0)
        assert all(np.array_equal(u64(d), w) for d, w in zip(darrays, want)) and u64(dstats).tolist() == stats.tolist(), (ty, ng, "two calls")
        a, sa = fl.unfor_aggregate_by_window_widths(*val, *key, lo, ng, mask=dm, what=WHAT)
        wa, _ = expected_table(ty, vals, keys, bits_m, lo, ng)
        assert all(np.array_equal(g, w) for g, w in zip(table_arrays(a), wa))
        b, sb = fl.unfor_aggregate_by_window_widths(*val, *key, lo, ng, mask=dnot, what=WHAT, into=a)
        assert b is a and all(np.array_equal(g, w) for g, w in zip(table_arrays(a), want)), (ty, ng, "into")
        assert (u64(sa) + u64(sb)).tolist() == stats.tolist()
        default, _ = fl.unfor_aggregate_by_window_widths(*val, *key, lo, ng)
        assert default.what() == ("count", "sum") and default.mins is None and np.array_equal(u64(default.sums), want[1])
        for kwargs in (dict(lo=lo + 1), dict(ng=ng - 1), dict(what=("count", "sum"))):
            with pytest.raises(ValueError):
                fl.unfor_aggregate_by_window_widths(*val, *key, kwargs.get("lo", lo), kwargs.get("ng", ng), what=kwargs.get("what", WHAT), into=a)
        other = "u16" if ty != "u16" else "u32"
        with pytest.raises(ValueError):
            fl.unfor_aggregate_by_window_widths(*val, *key, lo, ng, what=WHAT, into=fl.GroupTable(other, lo, ng, a.counts, a.sums, a.mins, a.maxs))
        with pytest.raises(TypeError):
            fl.unfor_aggregate_by_window_widths(*val, *key, lo, ng, what=WHAT, into=a.counts)
    with pytest.raises(ValueError):
        fl.unfor_aggregate_by_window_widths(*val, *key, 0, min(1 << T, 1 << 32) + 1)


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_columns(fl, oracle, ty):
    """FoR.unfor_aggregate_by_window at key widths 0, 1 and T // 2 + 1 against value widths 0, 3 and T over 37 blocks, one scalar
    reference each, mask=None, a window of each tier and the empty window; packed=None counts alone"""
    T = tbits(ty)
    N = 1 << T
    n = 37
    r0 = (N - 60) % N
    for kw, w in ((0, 3), (1, T), (T // 2 + 1, 0), (min(T, 7), 3)):
        kpk, pk = values(ty, n * packed_len(ty, kw), 95000 + 64 * T + kw), values(ty, n * packed_len(ty, w), 95500 + 64 * T + w)
        keys = oracle.batch("unfor_pack", ty, kw, kpk, aux=np.full(n, r0, dtype=TYPES[ty][0]), n_blocks=n)
        vals = oracle.batch("unfor_pack", ty, w, pk, aux=np.full(n, 11, dtype=TYPES[ty][0]), n_blocks=n)
        dkpk, dpk = to_dev(kpk), to_dev(pk)
        for lo, ng in tier_windows(ty, r0) + [((r0 + 5) % N, 0)]:
            want, stats = expected_table(ty, vals, keys, None, lo, ng)
            table, st = fl.FoR.unfor_aggregate_by_window(w, dpk, 11, kw, dkpk, r0, lo, ng, what=WHAT, n_blocks=n)
            assert all(np.array_equal(g, x) for g, x in zip(table_arrays(table), want)) and u64(st).tolist() == stats.tolist(), (ty, kw, w, lo, ng)
            assert int(stats.sum()) == n * 1024
            counted, st = fl.FoR.unfor_aggregate_by_window(None, None, None, kw, dkpk, r0, lo, ng, what=("count",), n_blocks=n)
            assert np.array_equal(u64(counted.counts), want[0]) and u64(st).tolist() == stats.tolist(), (ty, kw, lo, ng)


@pytest.mark.parametrize("ty", TYS)
def test_persistent_runs_flush_what_they_own(fl, oracle, kernel_policy, ty):
    """the LDS tier under runs of at least 16 blocks: groups updated only by the first, and only by the last, block of the column; 1, 2
    and 3 blocks (most wavefronts own no block and flush nothing); every slot of the window"""
    kernel_policy(RUN_OF_16)
    T = tbits(ty)
    N = 1 << T
    lo, ng = N // 2 - 100, min(200, N - 56)
    inside = ((np.arange(1024, dtype=np.uint64) % np.uint64(ng) + np.uint64(lo)) & np.uint64(N - 1)).astype(TYPES[ty][0])     # every slot
    outside = ((np.arange(1024, dtype=np.uint64) % np.uint64(50) + np.uint64(lo + ng + 3)) & np.uint64(N - 1)).astype(TYPES[ty][0])
    rng = np.random.default_rng(96000 + T)
    some = ((rng.integers(0, ng, size=1024).astype(np.uint64) + np.uint64(lo)) & np.uint64(N - 1)).astype(TYPES[ty][0])
    for name, n, first, last in (("first block only", 50, some, outside), ("last block only", 50, outside, some), ("one block", 1, inside, inside),
                                 ("two blocks", 2, some, inside), ("three blocks", 3, outside, some), ("every slot", 35, inside, outside)):
        keys = np.concatenate([first] + [outside] * max(n - 2, 0) + ([last] if n > 1 else []))
        vals = values(ty, n * 1024, 96100 + n)
        want, stats = expected_table(ty, vals, keys, None, lo, ng)
        table, st = fl.unfor_aggregate_by_window_widths(*encode(fl, ty, vals), *encode(fl, ty, keys), lo, ng, what=WHAT)
        assert all(np.array_equal(g, x) for g, x in zip(table_arrays(table), want)) and u64(st).tolist() == stats.tolist(), (ty, name)
        if name in ("one block", "every slot"):
            assert (want[0] > 0).all()


def test_q18_chain(fl):
    """SELECT l_orderkey, SUM(l_quantity) FROM lineitem WHERE l_shipdate BETWEEN .. GROUP BY l_orderkey HAVING SUM(l_quantity) > k:
    unfor_compare_range_widths -> unfor_aggregate_by_window_widths -> torch sums > k, three packed u32 columns of 96 blocks through
    the library's own encoder, against numpy on the decoded columns"""
    rng = np.random.default_rng(97000)
    n = 96
    orderkey = (np.sort(rng.integers(0, n * 256, size=n * 1024)) * 4 + 500000).astype(np.uint32)       # ascending, ~4 rows per order
    quantity = rng.integers(1, 51, size=n * 1024).astype(np.uint32)
    shipdate = rng.integers(8000, 10500, size=n * 1024).astype(np.uint32)
    ok, qt, sd = (encode(fl, "u32", v) for v in (orderkey, quantity, shipdate))
    m = fl.unfor_compare_range_widths(*sd, 9000, 9999)
    kept = (shipdate >= 9000) & (shipdate <= 9999)
    assert np.array_equal(got_mask(m), np.packbits(kept, bitorder="little").view(np.int32))
    lo, ng = fl.column_window("u32", ok[0], ok[3])
    assert lo == int(orderkey.min()) and lo + ng - 1 >= int(orderkey.max()) and ng > 70000
    table, stats = fl.unfor_aggregate_by_window_widths(*qt, *ok, lo, ng, mask=m)
    assert u64(stats).tolist() == [int(kept.sum()), 0]
    k = 120
    hit = (table.sums > k).cpu().numpy()
    sums = np.bincount(orderkey[kept].astype(np.int64) - lo, weights=quantity[kept], minlength=ng).astype(np.int64)
    assert np.array_equal(u64(table.sums).astype(np.int64), sums) and np.array_equal(hit, sums > k) and 0 < hit.sum() < ng
    assert np.array_equal(u64(table.counts).astype(np.int64), np.bincount(orderkey[kept].astype(np.int64) - lo, minlength=ng))
