"""GPU: unfor_lookup / unfor_lookup_widths and their uint8-payload twins -- table[(key - key_lo) mod 2^T] of the rows a mask keeps of a
FoR-packed key column, written in full-width packed order with the hits as a mask beside it -- against the numpy model of the
definition over the oracle's unfor_pack and pack(ty, T_BITS, .) (tests/lookup_data.py): `out` byte for byte, the hit mask and stats
exactly.  The expected side never reads the kernel's output."""
import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TYS, got_mask, mask_words, mixed_column, to_dev, to_np, u64_of
from lookup_data import (ABSENT_SLOT, B_FAR, B_ZERO_ABSENT, B_ZERO_IN, B_ZERO_OUT, PAIRS, RUN_OF_3, STATS_PREFILL, boundary_slots,
                         expected_lookup, present_words, raw_lookup, route_column, route_masks, table_of, window_lo, window_sizes)
from set_build_data import encode

pytestmark = pytest.mark.gpu

PAIR_IDS = [f"{t}-{u}" for t, u in PAIRS]
OUT_SENTINEL, HIT_SENTINEL = 0x5A, 0x3C3C3C3C


def decoded(oracle, ty, blocks, refs):
    return np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])


def member_set_of(fl, ty, lo, n_slots, words):
    """the kernel's argument, as given (stray bits included)"""
    return fl.MemberSet(ty, lo % (1 << tbits(ty)), n_slots, words)


def check(got, want, ty_of_out, what):
    out, hit, stats = got
    w_out, w_hit, w_stats = want[:3]
    g = to_np(out, ty_of_out)
    assert g.tobytes() == w_out.tobytes(), (what, "out", np.flatnonzero(g != w_out)[:8], g[g != w_out][:4], w_out[g != w_out][:4])
    gh = got_mask(hit)
    assert np.array_equal(gh, w_hit), (what, "hit mask", np.flatnonzero(gh != w_hit)[:8])
    assert u64_of(stats).tolist() == w_stats.tolist(), (what, "stats", u64_of(stats), w_stats)


@pytest.mark.parametrize("n,policy", [(3, 0), (11, RUN_OF_3)], ids=["3 blocks", "runs of 3"])
@pytest.mark.parametrize("ty,uty", PAIRS, ids=PAIR_IDS)
def test_every_route_window_mask_and_set(fl, oracle, kernel_policy, ty, uty, n, policy):
    """3 blocks (fewer than wavefronts) and 11 blocks in runs of at least 3: every route of fl_lookup_map.hpp, every window size
    (0, 1, 45, the LDS / memory boundary, one slot more, 2^T for u8 / u16) around a key_lo near 2^T - 1; mask None, random, empty and
    `hit is mask`; present None and given (stray bits past n_slots set, the width-0 block's bit clear); missing 0 and all-ones; into
    prefilled outputs and prefilled counters"""
    import torch
    kernel_policy(policy)
    T, U = tbits(ty), tbits(uty)
    N = 1 << T
    lo = window_lo(ty)
    widths, refs = route_column(ty, n)
    dw, doff, col, blocks = mixed_column(ty, widths, 98000 + T + n)
    keys = decoded(oracle, ty, blocks, refs)
    column = (dw, doff, to_dev(col), to_dev(refs))
    masks = route_masks(n, 98100 + n)
    seen_routes, call = set(), 0
    for n_slots in window_sizes(ty, uty):
        table = table_of(uty, n_slots, 98200 + n_slots % 1000)
        dtable = to_dev(table)
        pw = present_words(n_slots, 98300 + n_slots % 1000, clear=(ABSENT_SLOT,))
        if n_slots:
            pw[0] |= 1                                                      # slot 0 (the width-0 block inside) stays present
        for mname, keep in masks.items():
            for with_present in (False, True):
                for in_place in ((False, True) if mname == "random" else (False,)):
                    call += 1
                    missing = 0 if call % 2 else (1 << U) - 1
                    present = pw if with_present else None
                    want = expected_lookup(oracle, ty, uty, keys, keep, lo, table, present, missing, STATS_PREFILL)
                    dmask = mask_words(keep) if keep is not None else None
                    out = torch.full((n * 1024 * (U // 8),), OUT_SENTINEL, dtype=torch.uint8, device="cuda:0").view(dtable.dtype)
                    hit = dmask if in_place else torch.full((n * 32,), HIT_SENTINEL, dtype=torch.int32, device="cuda:0")
                    stats = to_dev(STATS_PREFILL.view(np.int64))
                    got = fl.unfor_lookup_widths(*column, lo, dtable, present=member_set_of(fl, ty, lo, n_slots, pw) if with_present else None,
                                                 missing=missing, mask=dmask, hit=hit, output=out, stats=stats)
                    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == hit.data_ptr() and got[2].data_ptr() == stats.data_ptr()
                    check(got, want, uty, (ty, uty, n, n_slots, mname, with_present, in_place, missing))
                    h = want[4].reshape(n, 1024)
                    if keep is None and n > B_FAR and 0 < n_slots < N:
                        seen_routes |= {("zero in", bool(h[B_ZERO_IN].all())), ("zero out", bool(h[B_ZERO_OUT].any())), ("far", bool(h[B_FAR].any()))}
                        if n_slots > ABSENT_SLOT:
                            seen_routes.add(("absent", with_present, bool(h[B_ZERO_ABSENT].all())))
    if n > B_FAR and N > 256:
        assert {("zero in", True), ("zero out", False), ("far", False), ("absent", True, False), ("absent", False, True)} <= seen_routes, seen_routes


@pytest.mark.parametrize("ty,uty", PAIRS, ids=PAIR_IDS)
def test_uniform_width_form(fl, oracle, ty, uty):
    """FoR.unfor_lookup at key widths 0, 3 and T over 5 blocks, one scalar reference, a table of each tier the pair has; mask None and
    random; present given at width 3"""
    T = tbits(ty)
    N = 1 << T
    n = 5
    lo = window_lo(ty)
    rng = np.random.default_rng(98500 + T)
    keep = rng.random(n * 1024) < 0.6
    for w in (0, 3, T):
        col = values(ty, n * 128 * w // (T // 8), 98600 + T + w)
        ref = (lo + 2) % N
        keys = np.concatenate([oracle.unfor_pack(ty, w, col[b * (col.size // n):(b + 1) * (col.size // n)], ref) for b in range(n)])
        for n_slots in sorted({min(9, N), min(boundary_slots(ty, uty) + 1, N)}):
            table = table_of(uty, n_slots, 98700 + n_slots % 1000)
            pw = present_words(n_slots, 98800 + w, clear=(3,))
            for k, present in ((None, None), (keep, pw if w == 3 else None)):
                want = expected_lookup(oracle, ty, uty, keys, k, lo, table, present, 7)
                got = fl.FoR.unfor_lookup(w, to_dev(col), ref, lo, to_dev(table), present=member_set_of(fl, ty, lo, n_slots, pw) if present is not None else None,
                                          missing=7, mask=mask_words(k) if k is not None else None, n_blocks=n)
                check(got, want, uty, (ty, uty, w, n_slots, k is not None))


@pytest.mark.parametrize("ty,uty", PAIRS, ids=PAIR_IDS)
def test_one_element_decides(fl, oracle, ty, uty):
    """1024 blocks; in block b exactly row b lies inside the window (its value and its hit bit stand alone in the block: the output
    permutation and the hit-bit position are pinned for every index); then exactly row b misses, on a clear `present` bit"""
    T = tbits(ty)
    N = 1 << T
    dt = TYPES[ty][0]
    lo, n_slots = window_lo(ty), 100
    b, i = np.divmod(np.arange(1024 * 1024, dtype=np.uint64), np.uint64(1024))
    table = table_of(uty, n_slots, 98900 + T)
    dtable = to_dev(table)
    alone = np.where(b == i, np.uint64(lo) + b % np.uint64(n_slots), np.uint64((lo + n_slots) % 2 ** 64) + i % np.uint64(50))
    keys = (alone & np.uint64(N - 1)).astype(dt)
    want = expected_lookup(oracle, ty, uty, keys, None, lo, table, None, 0)
    assert (want[4].reshape(1024, 1024).sum(axis=1) == 1).all() and want[4].reshape(1024, 1024).diagonal().all()
    check(fl.unfor_lookup_widths(*encode(fl, ty, keys), lo, dtable), want, uty, (ty, uty, "one row hits"))
    absent = np.where(b == i, np.uint64((lo + 99) % 2 ** 64), np.uint64(lo) + (b + i) % np.uint64(99))
    keys = (absent & np.uint64(N - 1)).astype(dt)
    pw = present_words(n_slots, 0, clear=(99,))
    pw[:] |= np.uint32(0xFFFFFFFF)
    pw[99 // 32] &= ~np.uint32(1 << (99 % 32))                              # every slot but 99; the stray bits past 100 stay set
    want = expected_lookup(oracle, ty, uty, keys, None, lo, table, pw, (1 << tbits(uty)) - 1)
    assert (want[4].reshape(1024, 1024).sum(axis=1) == 1023).all() and not want[4].reshape(1024, 1024).diagonal().any()
    got = fl.unfor_lookup_widths(*encode(fl, ty, keys), lo, dtable, present=member_set_of(fl, ty, lo, n_slots, pw), missing=(1 << tbits(uty)) - 1)
    check(got, want, uty, (ty, uty, "one row misses"))


@pytest.mark.parametrize("ty,uty", PAIRS, ids=PAIR_IDS)
def test_failing_blocks_are_left_untouched(fl, oracle, ty, uty):
    """a column with one width above T and one offset off the 16-byte grid: both FL_DEVERR_* bits are raised, the two blocks' `out`
    bytes keep their sentinel and their mask words are untouched, stats counts the other blocks only; the Python mirror raises"""
    import torch
    T, U = tbits(ty), tbits(uty)
    n, bad_w, bad_off = 11, 4, 3
    lo, n_slots = window_lo(ty), 45
    widths, refs = route_column(ty, n)
    dw, doff, col, blocks = mixed_column(ty, widths, 99000 + T)
    keys = decoded(oracle, ty, blocks, refs)
    table = table_of(uty, n_slots, 99100)
    bw = widths.astype(np.uint8)
    bw[bad_w] = T + 1
    boff = doff.cpu().numpy().copy()
    boff[bad_off] += 8
    ok = np.repeat(~np.isin(np.arange(n), (bad_w, bad_off)), 1024)
    want = expected_lookup(oracle, ty, uty, keys, ok, lo, table, None, 0, STATS_PREFILL)
    out = torch.full((n * 1024 * (U // 8),), OUT_SENTINEL, dtype=torch.uint8, device="cuda:0")
    hit = torch.full((n * 32,), HIT_SENTINEL, dtype=torch.int32, device="cuda:0")
    stats = to_dev(STATS_PREFILL.view(np.int64))
    dbw, dboff = torch.from_numpy(bw).cuda(), torch.from_numpy(boff).cuda()
    rc, flag = raw_lookup(fl, ty, uty, dbw, dboff, to_dev(col), to_dev(refs), n, None, lo, n_slots, to_dev(table), None, 0, out, hit, stats)
    assert (rc, flag) == (0, 1 | 4), (rc, flag)
    g_out, w_out = out.cpu().numpy().reshape(n, -1), want[0].view(np.uint8).reshape(n, -1)
    g_hit, w_hit = got_mask(hit).reshape(n, 32), want[1].reshape(n, 32)
    for blk in range(n):
        if blk in (bad_w, bad_off):
            assert (g_out[blk] == OUT_SENTINEL).all() and (g_hit[blk] == HIT_SENTINEL).all(), (ty, uty, blk)
        else:
            assert np.array_equal(g_out[blk], w_out[blk]) and np.array_equal(g_hit[blk], w_hit[blk]), (ty, uty, blk)
    assert u64_of(stats).tolist() == want[2].tolist()
    with pytest.raises(fl.FastLanesError) as ei:
        fl.unfor_lookup_widths(dbw, doff, to_dev(col), to_dev(refs), lo, to_dev(table))
    assert ei.value.status == 1


def test_python_mirror_refuses_a_window_that_is_not_the_tables(fl):
    import torch
    n = 2
    col = torch.zeros(n * 96, dtype=torch.uint32, device="cuda:0")
    table = torch.zeros(40, dtype=torch.uint8, device="cuda:0")
    for lo, bits in ((5, 41), (6, 40)):
        with pytest.raises(ValueError):
            fl.FoR.unfor_lookup(3, col, 0, 5, table, present=fl.MemberSet("u32", lo, bits, np.zeros(2, np.uint32)))
    with pytest.raises(TypeError):
        fl.FoR.unfor_lookup(3, col, 0, 5, table, present=fl.MemberSet("u16", 5, 40, np.zeros(2, np.uint32)))
    with pytest.raises(TypeError):
        fl.FoR.unfor_lookup(3, col, 0, 5, torch.zeros(40, dtype=torch.uint16, device="cuda:0"))
    w, o, r = fl.full_width_column("u16", 3, "cuda:0")
    assert w.tolist() == [16] * 3 and o.tolist() == [0, 2048, 4096] and r.tolist() == [0] and r.dtype == torch.uint16


def test_chain_lookup_feeds_group_by(fl, oracle):
    """SELECT n_name, SUM(revenue) GROUP BY n_name through l_suppkey: a u8 lookup through a u32 key column is, as it stands, the key
    column of unfor_aggregate_by_widths (fl.full_width_column("u8", ..)), with mask = hit; the result equals a numpy group-by"""
    n, lo, n_slots = 24, 1000, 3000
    rng = np.random.default_rng(99200)
    keys = rng.integers(lo - 200, lo + n_slots + 200, size=n * 1024).astype(np.uint32)
    revenue = rng.integers(0, 1 << 20, size=n * 1024).astype(np.uint32)
    nation = rng.integers(0, 25, size=n_slots).astype(np.uint8)
    codes, hit, stats = fl.unfor_lookup_widths(*encode(fl, "u32", keys), lo, to_dev(nation), missing=255)
    result = fl.unfor_aggregate_by_widths(*encode(fl, "u32", revenue), *fl.full_width_column("u8", n, "cuda:0")[:2], codes,
                                          fl.full_width_column("u8", n, "cuda:0")[2], mask=hit)
    inside = (keys >= lo) & (keys < lo + n_slots)
    g = nation[np.where(inside, keys - lo, 0)]
    got = u64_of(result)
    assert u64_of(stats).tolist() == [int(inside.sum()), int((~inside).sum())]
    for code in range(256):
        rows = inside & (g == code)
        assert int(got[code, 0]) == int(rows.sum()) and int(got[code, 1]) == int(revenue[rows].sum(dtype=np.uint64)), code
    assert int(got[255, 0]) == 0                                            # the misses carry 255 but the mask drops them


@pytest.mark.parametrize("ty", TYS[1:])
def test_chain_second_lookup_and_unpack(fl, oracle, ty):
    """l_orderkey -> o_custkey -> c_nationkey: a U = T lookup's output is the key column of a second (u8) lookup through
    fl.full_width_column(ty, ..), equal to t2[t1[k - lo1] - lo2]; and BitPacking.unpack(T, out) is the plain numpy gather"""
    T = tbits(ty)
    dt = TYPES[ty][0]
    n, lo1, n1, lo2, n2 = 7, 500, 5000, 20000, 300
    rng = np.random.default_rng(99300 + T)
    keys = rng.integers(lo1, lo1 + n1, size=n * 1024).astype(dt)
    t1 = (lo2 + rng.integers(0, n2, size=n1)).astype(dt)
    t2 = rng.integers(0, 200, size=n2).astype(np.uint8)
    first, hit, _ = fl.unfor_lookup_widths(*encode(fl, ty, keys), lo1, to_dev(t1))
    assert np.array_equal(to_np(fl.BitPacking.unpack(T, first), ty), t1[keys.astype(np.int64) - lo1])
    second, hit2, stats = fl.unfor_lookup_widths(*fl.full_width_column(ty, n, "cuda:0")[:2], first, fl.full_width_column(ty, n, "cuda:0")[2], lo2,
                                                 to_dev(t2), mask=hit)
    assert np.array_equal(to_np(second, "u8"), t2[t1[keys.astype(np.int64) - lo1].astype(np.int64) - lo2])
    assert u64_of(stats).tolist() == [n * 1024, 0] and (got_mask(hit2) == -1).all()


def test_u8_twin_is_the_same_lookup(fl, oracle):
    """fl_u8_unfor_lookup_u8_widths (u8's payload under the _u8 name: one surface per element type) against the same model"""
    import torch
    n, lo, n_slots = 11, window_lo("u8"), 45
    widths, refs = route_column("u8", n)
    dw, doff, col, blocks = mixed_column("u8", widths, 99400)
    keys = decoded(oracle, "u8", blocks, refs)
    table = table_of("u8", n_slots, 99500)
    want = expected_lookup(oracle, "u8", "u8", keys, None, lo, table, None, 9)
    out = torch.zeros(n * 1024, dtype=torch.uint8, device="cuda:0")
    hit = torch.zeros(n * 32, dtype=torch.int32, device="cuda:0")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    rc, flag = raw_lookup(fl, "u8", "u8", dw, doff, to_dev(col), to_dev(refs), n, None, lo, n_slots, to_dev(table), None, 9, out, hit, stats, twin=True)
    assert (rc, flag) == (0, 0)
    check((out, hit, stats), want, "u8", "the u8 twin")
