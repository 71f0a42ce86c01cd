"""GPU: unfor_aggregate_by_lookup / unfor_aggregate_by_lookup_widths -- COUNT / SUM / MIN / MAX of a FoR-packed value column grouped by
the u8 code table[(key - key_lo) mod 2^T] of a FoR-packed key column of the same type, with no per-row output -- against the numpy
model of the definition over the oracle's unfor_pack (tests/aggregate_by_lookup_data.py): all 256 result slots and stats exactly, and
bit for bit against the chain the call replaces (unfor_lookup_widths + unfor_aggregate_by_widths under the hits).  The expected side
never reads the kernel's output."""
import numpy as np
import pytest

from aggregate_by_lookup_data import (ABSENT_SLOT, BAD_KEY_BLOCK, BAD_VALUE_BLOCK, RUN_OF_3, STATS_PREFILL, code_table, expected_fused,
                                      present_words, raw_fused, route_masks, route_pair, routes_taken, upload, window_lo, window_sizes)
from datagen import values
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import IDENTITY, TYS, mask_words, sentinel_slots, to_dev, u64_of
from oracle_lib import TYPES, tbits
from set_build_data import encode

pytestmark = pytest.mark.gpu


def member_set_of(fl, ty, lo, n_slots, words):
    """the kernel's argument, as given (stray bits included)"""
    return fl.MemberSet(ty, lo % (1 << tbits(ty)), n_slots, words)


def check(got, want, what):
    result, stats = got
    g = u64_of(result)
    assert g.shape == (256, 4)
    assert np.array_equal(g, want[0]), (what, "result", np.flatnonzero((g != want[0]).any(axis=1))[:8], g[(g != want[0]).any(axis=1)][:3],
                                        want[0][(g != want[0]).any(axis=1)][:3])
    assert u64_of(stats).tolist() == want[1].tolist(), (what, "stats", u64_of(stats), want[1])


@pytest.mark.parametrize("n,policy", [(3, 0), (11, RUN_OF_3)], ids=["3 blocks", "runs of 3"])
@pytest.mark.parametrize("ty", TYS)
def test_every_route_window_mask_and_set(fl, oracle, kernel_policy, ty, n, policy):
    """3 blocks (fewer than wavefronts) and 11 blocks in runs of at least 3: every route of fl_aggregate_by_lookup_map.hpp, every
    window size (0, 1, 45, 8192, 8193, 2^T for u8 / u16) around a key_lo near 2^T - 1; mask None, random and empty; present None and
    given (stray bits past n_slots set, the width-0 block's slot clear); into a sentinel-filled result and prefilled counters.  The
    routes the chosen columns take are computed from the CPU model BEFORE the first launch."""
    kernel_policy(policy)
    T = tbits(ty)
    lo = window_lo(ty)
    pair = route_pair(oracle, ty, n, 41000 + T + n)
    vals, keys = pair["val"]["decoded"], pair["key"]["decoded"]
    masks = route_masks(n, 41100 + n)
    cases, seen = [], set()
    for n_slots in window_sizes(ty):
        table = code_table(n_slots, 41200 + n_slots % 1000)
        pw = present_words(n_slots, 41300 + n_slots % 1000, clear=(ABSENT_SLOT,))
        if n_slots:
            pw[0] |= 1                                                      # slot 0 (the width-0 block inside) stays present
        for mname, keep in masks.items():
            for present in (None, pw):
                cases.append((n_slots, table, pw, mname, keep, present))
                seen |= routes_taken(ty, pair, keep, lo, n_slots, present)
    if n == 11:                                                             # SKIP-free: no block of these columns fails a check
        assert seen == {"NOTHING", "MISSING", "ONE_GROUP present", "ONE_GROUP absent", "EACH"}, seen
    lead = upload(pair)
    for n_slots, table, pw, mname, keep, present in cases:
        want = expected_fused(ty, vals, keys, keep, lo, table, present, STATS_PREFILL)
        buf, result = sentinel_slots(256)
        stats = to_dev(STATS_PREFILL.view(np.int64))
        got = fl.unfor_aggregate_by_lookup_widths(*lead, lo, to_dev(table), present=member_set_of(fl, ty, lo, n_slots, pw) if present is not None else None,
                                                  mask=mask_words(keep) if keep is not None else None, result=result, stats=stats)
        assert got[0].data_ptr() == result.data_ptr() and got[1].data_ptr() == stats.data_ptr()
        check(got, want, (ty, n, n_slots, mname, present is not None))
        assert (u64_of(buf)[256 * 4:] == 0xA5A5A5A5A5A5A5A5).all(), "slots behind the result were written"


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_form(fl, oracle, ty):
    """FoR.unfor_aggregate_by_lookup at key widths 0, 3 and T and value widths 0, 5 and T over 5 blocks, one scalar reference each, a
    small and a large table; mask None and random; present given at key width 3"""
    T = tbits(ty)
    N = 1 << T
    n = 5
    lo = window_lo(ty)
    rng = np.random.default_rng(42000 + T)
    keep = rng.random(n * 1024) < 0.6
    for kw in (0, 3, T):
        kcol = values(ty, n * 128 * kw // (T // 8), 42100 + T + kw)
        kref = (lo + 2) % N
        keys = np.concatenate([oracle.unfor_pack(ty, kw, kcol[b * (kcol.size // n):(b + 1) * (kcol.size // n)], kref) for b in range(n)])
        for vw in (0, 5, T):
            vcol = values(ty, n * 128 * vw // (T // 8), 42200 + T + vw)
            vref = 77 + vw
            vals = np.concatenate([oracle.unfor_pack(ty, vw, vcol[b * (vcol.size // n):(b + 1) * (vcol.size // n)], vref) for b in range(n)])
            for n_slots in sorted({min(9, N), min(8193, N)}):
                table = code_table(n_slots, 42300 + n_slots % 1000)
                pw = present_words(n_slots, 42400 + kw, clear=(3,))
                for k, present in ((None, None), (keep, pw if kw == 3 else None)):
                    want = expected_fused(ty, vals, keys, k, lo, table, present)
                    got = fl.FoR.unfor_aggregate_by_lookup(vw, to_dev(vcol), vref, kw, to_dev(kcol), kref, lo, to_dev(table),
                                                           present=member_set_of(fl, ty, lo, n_slots, pw) if present is not None else None,
                                                           mask=mask_words(k) if k is not None else None, n_blocks=n)
                    check(got, want, (ty, kw, vw, n_slots, k is not None))


@pytest.mark.parametrize("ty", TYS)
def test_one_element_decides(fl, oracle, ty):
    """1024 blocks; in block b exactly row b hits.  In one pass it carries a value BELOW every other value of the column (the global
    MIN of its group), in another one ABOVE them (the global MAX): a lane map that differs between the two columns at any index
    takes a neighbour's value and moves a group's min, max and sum.  Then exactly row b MISSES, on a clear `present` bit, while it
    carries the column's greatest value."""
    T = tbits(ty)
    N = 1 << T
    dt = TYPES[ty][0]
    lo, n_slots = window_lo(ty), 100
    b, i = np.divmod(np.arange(1024 * 1024, dtype=np.uint64), np.uint64(1024))
    table = code_table(n_slots, 42500 + T)
    dtable = to_dev(table)
    alone = np.where(b == i, np.uint64(lo) + b % np.uint64(n_slots), np.uint64((lo + n_slots) % 2 ** 64) + i % np.uint64(50))
    keys = (alone & np.uint64(N - 1)).astype(dt)
    dkeys = encode(fl, ty, keys)
    others = np.uint64(100) + (b * np.uint64(7) + i * np.uint64(3)) % np.uint64(50)          # 100 .. 149 everywhere else
    for name, mine in (("min", b % np.uint64(90)), ("max", np.uint64(160) + b % np.uint64(90))):
        vals = np.where(b == i, mine, others).astype(dt)
        want = expected_fused(ty, vals, keys, None, lo, table, None)
        assert (want[2].reshape(1024, 1024).sum(axis=1) == 1).all() and want[2].reshape(1024, 1024).diagonal().all()
        assert int(want[1][0]) == 1024
        check(fl.unfor_aggregate_by_lookup_widths(*encode(fl, ty, vals), *dkeys, lo, dtable), want, (ty, "one row hits", name))
    absent = np.where(b == i, np.uint64((lo + 99) % 2 ** 64), np.uint64(lo) + (b + i) % np.uint64(99))
    keys = (absent & np.uint64(N - 1)).astype(dt)
    vals = np.where(b == i, np.uint64(250), others).astype(dt)
    pw = present_words(n_slots, 0, clear=(99,))
    pw[:] |= np.uint32(0xFFFFFFFF)
    pw[99 // 32] &= ~np.uint32(1 << (99 % 32))                              # every slot but 99; the stray bits past 100 stay set
    want = expected_fused(ty, vals, keys, None, lo, table, pw)
    assert (want[2].reshape(1024, 1024).sum(axis=1) == 1023).all() and not want[2].reshape(1024, 1024).diagonal().any()
    assert int(want[0][:, 3].max()) < 250
    got = fl.unfor_aggregate_by_lookup_widths(*encode(fl, ty, vals), *encode(fl, ty, keys), lo, dtable, present=member_set_of(fl, ty, lo, n_slots, pw))
    check(got, want, (ty, "one row misses"))


@pytest.mark.parametrize("ty", TYS)
def test_collisions(fl, oracle, kernel_policy, ty):
    """11 blocks in runs of 3 (four wavefronts flush into the same slots): every row of every block reaches ONE group through as many
    different slots as the key type has (1024, u8: 256) -- 64 lanes update one LDS slot in one instruction -- with values whose SUM
    wraps mod 2^64 for u64; then the table's codes are 0 and 255 alternately"""
    kernel_policy(RUN_OF_3)
    T = tbits(ty)
    N = 1 << T
    dt = TYPES[ty][0]
    n, lo = 11, window_lo(ty)
    n_slots = min(N, 1024)
    rng = np.random.default_rng(42600 + T)
    keys = ((np.concatenate([rng.permutation(1024) % n_slots for _ in range(n)]).astype(np.uint64) + np.uint64(lo)) & np.uint64(N - 1)).astype(dt)
    top = (1 << T) - 1
    vals = (np.uint64(top) - rng.integers(0, 200, size=n * 1024).astype(np.uint64)).astype(dt)    # near 2^T - 1: 11264 of them wrap a u64 sum
    dvals, dkeys = encode(fl, ty, vals), encode(fl, ty, keys)
    for name, table in (("one group", np.full(n_slots, 7, np.uint8)), ("codes 0 and 255", np.where(np.arange(n_slots) % 2 == 0, 0, 255).astype(np.uint8))):
        want = expected_fused(ty, vals, keys, None, lo, table, None)
        if name == "one group":
            assert int(want[0][7, 0]) == n * 1024 and (want[0][np.arange(256) != 7] == IDENTITY).all()
            if T == 64:
                assert int(want[0][7, 1]) != int(vals.astype(object).sum()) and int(want[0][7, 1]) == int(vals.astype(object).sum()) % 2 ** 64
        else:
            assert int(want[0][0, 0]) + int(want[0][255, 0]) == n * 1024 and int(want[0][0, 0]) > 0 and int(want[0][255, 0]) > 0
        check(fl.unfor_aggregate_by_lookup_widths(*dvals, *dkeys, lo, to_dev(table)), want, (ty, name))


@pytest.mark.parametrize("ty", TYS)
def test_failing_blocks_contribute_nothing(fl, oracle, ty):
    """one block with an offset off the 16-byte grid in the KEY column only, another in the VALUE column only: the FL_DEVERR_* bit is
    raised, the two blocks add nothing to result or stats, every other block counts; the Python mirror raises"""
    import torch
    T = tbits(ty)
    n, lo, n_slots = 11, window_lo(ty), 45
    pair = route_pair(oracle, ty, n, 42700 + T)
    assert pair["key"]["widths"][BAD_KEY_BLOCK] > 0 and pair["val"]["widths"][BAD_VALUE_BLOCK] > 0
    table = code_table(n_slots, 42800)
    lead = upload(pair)
    koff, voff = pair["key"]["off"].copy(), pair["val"]["off"].copy()
    koff[BAD_KEY_BLOCK] += 8
    voff[BAD_VALUE_BLOCK] += 8
    bad = list(lead)
    bad[1], bad[5] = torch.from_numpy(voff).cuda(), torch.from_numpy(koff).cuda()
    want = expected_fused(ty, pair["val"]["decoded"], pair["key"]["decoded"], None, lo, table, None, STATS_PREFILL, without=(BAD_KEY_BLOCK, BAD_VALUE_BLOCK))
    whole = expected_fused(ty, pair["val"]["decoded"], pair["key"]["decoded"], None, lo, table, None, STATS_PREFILL)
    assert not np.array_equal(want[0], whole[0]) and want[1].tolist() != whole[1].tolist()        # the two blocks would have counted
    buf, result = sentinel_slots(256)
    stats = to_dev(STATS_PREFILL.view(np.int64))
    rc, flag = raw_fused(fl, ty, bad, n, None, lo, n_slots, to_dev(table), None, result, stats)
    assert (rc, flag) == (0, 4), (rc, flag)
    check((result, stats), want, (ty, "two failing blocks"))
    with pytest.raises(fl.FastLanesError) as ei:
        fl.unfor_aggregate_by_lookup_widths(*bad, lo, to_dev(table))
    assert ei.value.status == 4


@pytest.mark.parametrize("ty", TYS)
def test_equals_the_chain_it_replaces(fl, oracle, kernel_policy, ty):
    """result and stats equal, bit for bit, unfor_lookup_widths (u8 table, its hit mask) followed by unfor_aggregate_by_widths with the
    codes as the full-width u8 key column and mask = the hits, on the same inputs: 11 blocks in runs of 3, a small window and one above
    8192 slots, mask None and random, present None and given"""
    kernel_policy(RUN_OF_3)
    T = tbits(ty)
    N = 1 << T
    n, lo = 11, window_lo(ty)
    pair = route_pair(oracle, ty, n, 41000 + T + n)
    lead = upload(pair)
    kw8, ko8, kr8 = fl.full_width_column("u8", n, "cuda:0")
    for n_slots in sorted({45, min(8193, N)}):
        table = code_table(n_slots, 41200 + n_slots % 1000)
        dtable = to_dev(table)
        pw = present_words(n_slots, 41300 + n_slots % 1000, clear=(ABSENT_SLOT,))
        for mname, keep in route_masks(n, 41100 + n).items():
            for with_present in (False, True):
                present = member_set_of(fl, ty, lo, n_slots, pw) if with_present else None
                dmask = mask_words(keep) if keep is not None else None
                codes, hit, cstats = fl.unfor_lookup_widths(*lead[4:], lo, dtable, present=present, missing=9, mask=dmask)
                chain = fl.unfor_aggregate_by_widths(*lead[:4], kw8, ko8, codes, kr8, mask=hit)
                result, stats = fl.unfor_aggregate_by_lookup_widths(*lead, lo, dtable, present=present, mask=dmask)
                assert np.array_equal(u64_of(result), u64_of(chain)), (ty, n_slots, mname, with_present)
                assert u64_of(stats).tolist() == u64_of(cstats).tolist(), (ty, n_slots, mname, with_present)


def test_empty_column_writes_the_identities(fl):
    """n_blocks == 0 through the C ABI, whatever the other pointers: FL_OK, result receives the 256 identities as unfor_aggregate_by's
    does, stats is untouched"""
    import ctypes
    import torch
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ty in TYS:
        buf, result = sentinel_slots(256)
        stats = to_dev(STATS_PREFILL.view(np.int64))
        lib = fl.load()
        assert getattr(lib, f"fl_{ty}_unfor_aggregate_by_lookup")(3, None, None, 0, 2, None, None, 0, None, 0, 5, 40, None, None, result.data_ptr(),
                                                                   stats.data_ptr(), None, stream) == 0
        assert (u64_of(result) == IDENTITY).all() and u64_of(stats).tolist() == STATS_PREFILL.tolist()
        buf, result = sentinel_slots(256)
        assert getattr(lib, f"fl_{ty}_unfor_aggregate_by_lookup_widths")(None, None, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, 5, 40, None,
                                                                          None, result.data_ptr(), None, None, stream) == 0
        assert (u64_of(result) == IDENTITY).all() and (u64_of(buf)[256 * 4:] == 0xA5A5A5A5A5A5A5A5).all()


def test_python_mirror_refuses_a_window_that_is_not_the_tables(fl):
    import torch
    n = 2
    col = torch.zeros(n * 96, dtype=torch.uint32, device="cuda:0")
    table = torch.zeros(40, dtype=torch.uint8, device="cuda:0")
    for lo, bits in ((5, 41), (6, 40)):
        with pytest.raises(ValueError):
            fl.FoR.unfor_aggregate_by_lookup(3, col, 0, 3, col, 0, 5, table, present=fl.MemberSet("u32", lo, bits, np.zeros(2, np.uint32)))
    with pytest.raises(TypeError):
        fl.FoR.unfor_aggregate_by_lookup(3, col, 0, 3, col, 0, 5, table, present=fl.MemberSet("u16", 5, 40, np.zeros(2, np.uint32)))
    with pytest.raises(TypeError):                                          # the table holds u8 codes
        fl.FoR.unfor_aggregate_by_lookup(3, col, 0, 3, col, 0, 5, torch.zeros(40, dtype=torch.uint32, device="cuda:0"))
