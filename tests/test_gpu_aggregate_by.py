"""GPU: unfor_aggregate_by / unfor_aggregate_by_widths -- COUNT / SUM / MIN / MAX of a FoR-packed column grouped by a FoR-packed u8 key
column under a selection mask -- against the oracle's unfor_pack of BOTH columns (ffor.rs:38-50) reduced with numpy (np.add.at /
np.minimum.at / np.maximum.at on uint64, tests/group_data.py): uint64[256, 4], bit-exact."""
import ctypes

import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import (GUARD, IDENTITY, SENTINEL, TYS, UNIFORM_BLOCKS, combine, mask_set, mask_words, mixed_column_host, placed,
                         sentinel_slots, to_dev, u64_of, uniform_widths)
from group_data import GROUPS, KEY_KINDS, KEY_WIDTH, expected_groups, key_blocks, key_column

pytestmark = pytest.mark.gpu

RUN_OF_4 = 2 + 65536 * 4                        # kernel policy: wave-per-block mode, at least 4 blocks per wavefront's run
SHAPES = [0, RUN_OF_4, 2 + 256 * 3 + 65536 * 16]


def check_result(buf, got, want, what):
    """all 256 slots are the expected ones (so every sentinel was overwritten), the guard behind them is untouched"""
    assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (GROUPS, 4), what
    now = u64_of(buf)
    assert np.array_equal(now[:GROUPS * 4].reshape(GROUPS, 4), want), what
    assert now.size == (GROUPS + GUARD) * 4 and (now[GROUPS * 4:] == SENTINEL).all(), (what, "the guard was written")


def value_column(oracle, ty, widths, seed, refs):
    """a mixed-width value column and the oracle's decode of it"""
    w, off, col, blocks = mixed_column_host(ty, widths, seed)
    vals = np.concatenate([oracle.unfor_pack(ty, bw, pk, refs[b]) for b, (bw, pk) in enumerate(blocks)]) if len(blocks) else np.zeros(0, TYPES[ty][0])
    return w, off, col, vals


def dev_column(widths, offsets, col, refs):
    import torch
    return torch.from_numpy(widths).cuda(), torch.from_numpy(offsets).cuda(), to_dev(col), to_dev(refs)


def masks_of(n, rng):
    return mask_set(n, rng, full=False, with_none=True)


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_form(fl, oracle, ty):
    """Value widths 0, 1, T/2 - 1, T/2, T crossed with every key distribution (key widths 0, 1, 2, 3, 8), the mask set and no mask,
    35 blocks and 1 block; per-block references on both sides, and one broadcast pair."""
    T = tbits(ty)
    rng = np.random.default_rng(18000 + T)
    for n in (UNIFORM_BLOCKS, 1):
        masks = masks_of(n, rng)
        keycols = {kind: key_column(oracle, key_blocks(oracle, kind, n, rng)) for kind in KEY_KINDS}
        assert {KEY_WIDTH[k] for k in KEY_KINDS} >= {0, 1, 3, 8}
        for w in uniform_widths(ty):
            pk = values(ty, n * packed_len(ty, w), 18100 + 64 * T + w)
            refs = values(ty, n, 18200 + 64 * T + w)
            vals = oracle.batch("unfor_pack", ty, w, pk, aux=refs, n_blocks=n)
            dpk, drefs = to_dev(pk), to_dev(refs)
            for kind, (kw, _, kcol, krefs, keys) in keycols.items():
                assert (kw == KEY_WIDTH[kind]).all()
                dk, dkr = to_dev(kcol), to_dev(krefs)
                for name, bits in (masks.items() if n > 1 or kind in ("uniform", "clustered") else [("no mask", None)]):
                    buf, slots = sentinel_slots(GROUPS)
                    got = fl.FoR.unfor_aggregate_by(w, dpk, drefs, KEY_WIDTH[kind], dk, dkr, None if bits is None else mask_words(bits),
                                                    n_blocks=n, result=slots)
                    check_result(buf, got, expected_groups(vals, keys, bits), (ty, n, w, kind, name))
        # scalar references: broadcast with stride 0
        w, kind = T // 2, "wrapping"
        pk = values(ty, n * packed_len(ty, w), 18300 + T)
        kw, _, kcol, krefs, keys = keycols[kind]
        vals = oracle.batch("unfor_pack", ty, w, pk, aux=np.full(n, 5, dtype=TYPES[ty][0]), n_blocks=n)
        got = fl.FoR.unfor_aggregate_by(w, to_dev(pk), 5, KEY_WIDTH[kind], to_dev(kcol), 250)
        assert np.array_equal(u64_of(got), expected_groups(vals, keys, None)), (ty, n, "scalar references")


def mixed_case(oracle, ty, n, rng, seed):
    """value widths cycling through 0, 1, T/2 - 1, T/2, T and random ones; key blocks cycling through every distribution"""
    T = tbits(ty)
    cyc = uniform_widths(ty)
    widths = np.array([cyc[b % 5] if b % 3 else int(rng.integers(0, T + 1)) for b in range(n)], dtype=np.int64)
    refs = values(ty, n, seed + 1)
    vw, voff, vcol, vals = value_column(oracle, ty, widths, seed, refs)
    kblocks = [key_blocks(oracle, KEY_KINDS[(b + b // 7) % len(KEY_KINDS)], 1, rng)[0] for b in range(n)]
    kw, koff, kcol, krefs, keys = key_column(oracle, kblocks)
    return (vw, voff, vcol, refs, vals), (kw, koff, kcol, krefs, keys)


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_form(fl, oracle, ty):
    T = tbits(ty)
    rng = np.random.default_rng(18400 + T)
    for n in (UNIFORM_BLOCKS, 1):
        (vw, voff, vcol, refs, vals), (kw, koff, kcol, krefs, keys) = mixed_case(oracle, ty, n, rng, 18500 + 64 * T + n)
        if n > 1:
            assert {0, 1, T // 2 - 1, T // 2, T} <= set(int(w) for w in vw) and {0, 1, 3, 8} <= set(int(w) for w in kw)
        dv, dk = dev_column(vw, voff, vcol, refs), dev_column(kw, koff, kcol, krefs)
        for name, bits in masks_of(n, rng).items():
            buf, slots = sentinel_slots(GROUPS)
            got = fl.unfor_aggregate_by_widths(*dv, *dk, None if bits is None else mask_words(bits), result=slots)
            check_result(buf, got, expected_groups(vals, keys, bits), (ty, n, name))
        # the convenience path: the result allocated inside the call
        got = fl.unfor_aggregate_by_widths(*dv, *dk)
        assert tuple(got.shape) == (GROUPS, 4) and np.array_equal(u64_of(got), expected_groups(vals, keys, None)), (ty, n, "result=None")


@pytest.mark.parametrize("ty", TYS)
def test_empty_column_gives_256_identities(fl, ty):
    import torch
    from gpu_support import TDT
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    e8 = torch.empty(0, dtype=torch.uint8, device="cuda:0")
    e64 = torch.empty(0, dtype=torch.int64, device="cuda:0")
    want = np.tile(IDENTITY, (GROUPS, 1))
    for m in (None, torch.empty(0, dtype=torch.int32, device="cuda:0")):
        buf, slots = sentinel_slots(GROUPS)
        check_result(buf, fl.FoR.unfor_aggregate_by(3, empty, 0, 3, e8, 0, m, result=slots), want, (ty, "uniform"))
        buf, slots = sentinel_slots(GROUPS)
        check_result(buf, fl.unfor_aggregate_by_widths(e8, e64, empty, to_dev(np.zeros(1, TYPES[ty][0])), e8, e64, e8, to_dev(np.zeros(1, np.uint8)), m,
                                                       result=slots), want, (ty, "mixed"))


@pytest.mark.parametrize("policy", SHAPES[1:])
@pytest.mark.parametrize("ty", TYS)
def test_runs_of_mixed_routes_uneven_tail_and_idle_wavefronts(fl, oracle, kernel_policy, ty, policy):
    """A cap on the grid through the kernel policy's blocks-per-wavefront field: 35 blocks in runs of 4 are eight full runs, a tail of 3
    and 26 wavefronts of the 35-workgroup grid without a block (runs of 16: 16, 16, 3 and 32 idle).  Run 0 holds a block of every
    route: an empty mask, key width 0, both columns decoded.  Equal to the reference, and to the call without the cap."""
    T = tbits(ty)
    n = UNIFORM_BLOCKS
    run = (policy >> 16) & 0xFF
    assert n % run == 3 and -(-n // run) < n                               # an uneven tail; wavefronts without a block
    rng = np.random.default_rng(18600 + T)
    cyc = uniform_widths(ty)
    widths = np.array([cyc[(b + b // 5) % 5] for b in range(n)], dtype=np.int64)
    refs = values(ty, n, 18601 + T)
    vw, voff, vcol, vals = value_column(oracle, ty, widths, 18602 + T, refs)
    kinds = ["clustered", "clustered", "wrapping", "uniform", "two", "clustered", "permutation"]
    kw, koff, kcol, krefs, keys = key_column(oracle, [key_blocks(oracle, kinds[b % len(kinds)], 1, rng)[0] for b in range(n)])
    bits = rng.random(n * 1024) < 0.3
    bits.reshape(n, 1024)[::5] = False                                      # blocks 0, 5, ..: nothing kept
    kept = bits.reshape(n, 1024).any(axis=1)
    routes = [0 if not kept[b] else 1 if kw[b] == 0 else 2 for b in range(n)]
    assert set(routes[:run]) == {0, 1, 2} and len(routes[:run]) >= 3
    assert {(routes[b], bool(vw[b])) for b in range(n)} == {(r, v) for r in (0, 1, 2) for v in (False, True)}
    dv, dk, dm = dev_column(vw, voff, vcol, refs), dev_column(kw, koff, kcol, krefs), mask_words(bits)
    want = expected_groups(vals, keys, bits)
    plain = fl.unfor_aggregate_by_widths(*dv, *dk, dm)                      # policy 0
    kernel_policy(policy)
    buf, slots = sentinel_slots(GROUPS)
    check_result(buf, fl.unfor_aggregate_by_widths(*dv, *dk, dm, result=slots), want, (ty, policy))
    assert np.array_equal(u64_of(plain), want), (ty, "policy 0")
    # no mask under the cap: the tail run (blocks 32..34) and a full one are both non-trivial
    buf, slots = sentinel_slots(GROUPS)
    check_result(buf, fl.unfor_aggregate_by_widths(*dv, *dk, None, result=slots), expected_groups(vals, keys, None), (ty, policy, "no mask"))


@pytest.mark.parametrize("ty", TYS)
def test_special_keys_and_values(fl, oracle, ty):
    """Key 255 in exactly one kept row; every key exactly 4 times per block; u64 references near 2^64 (the per-group sums wrap); for
    u8 / u16 a block of all-maximum values at full mask under a single key, through each route."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    rng = np.random.default_rng(18700 + T)
    n = 6
    widths = np.array([T, T // 2, 1, T, 0, T // 2 - 1], dtype=np.int64)
    refs = values(ty, n, 18701 + T)
    if ty == "u64":
        refs = (np.uint64(2 ** 64 - 1) - values(ty, n, 18702, bits=20)).astype(dt)
    vw, voff, vcol, vals = value_column(oracle, ty, widths, 18703 + T, refs)
    dv = dev_column(vw, voff, vcol, refs)
    # key 255 once
    keys = rng.integers(0, 255, size=n * 1024).astype(np.uint8)
    at = 3 * 1024 + 517
    keys[at] = 255
    bits = rng.random(n * 1024) < 0.5
    bits[at] = True
    kblocks = [(8, 0, oracle.for_pack("u8", 8, keys[b * 1024:(b + 1) * 1024], 0)) for b in range(n)]
    kw, koff, kcol, krefs, decoded = key_column(oracle, kblocks)
    assert np.array_equal(decoded, keys) and (keys == 255).sum() == 1
    got = u64_of(fl.unfor_aggregate_by_widths(*dv, *dev_column(kw, koff, kcol, krefs), mask_words(bits)))
    want = expected_groups(vals, keys, bits)
    assert np.array_equal(got, want), (ty, "rare key")
    assert tuple(int(x) for x in got[255]) == (1, int(vals[at]), int(vals[at]), int(vals[at]))
    if ty == "u64":
        occupied = want[:, 0] > 1
        assert (want[occupied, 1] < want[occupied, 3]).any()                # a sum smaller than its group's max: it wrapped
    # a permutation: every block holds every key exactly 4 times
    kw, koff, kcol, krefs, keys = key_column(oracle, key_blocks(oracle, "permutation", n, rng))
    assert (np.bincount(keys.reshape(n, 1024)[2], minlength=256) == 4).all()
    got = u64_of(fl.unfor_aggregate_by_widths(*dv, *dev_column(kw, koff, kcol, krefs)))
    assert np.array_equal(got, expected_groups(vals, keys, None)) and (got[:, 0] == 4 * n).all(), (ty, "permutation")
    # the largest per-group sum one block can give: 1024 maximal values under one key (u8 / u16: the narrow accumulators)
    if T <= 16:
        top = (1 << T) - 1
        ones = np.full(2 * 1024 * T // 8, 0xFF, dtype=np.uint8).view(dt)   # two blocks of width T, every bit set
        zero_ref = to_dev(np.zeros(1, dt))
        for what, kwidth, kpacked, kref in (("key width 0", 0, np.zeros(0, np.uint8), 77),
                                            ("key width 8", 8, np.tile(oracle.for_pack("u8", 8, np.full(1024, 77, np.uint8), 0), 2), 0)):
            got = u64_of(fl.FoR.unfor_aggregate_by(T, to_dev(ones), zero_ref, kwidth, to_dev(kpacked), kref, n_blocks=2))
            want = np.tile(IDENTITY, (GROUPS, 1))
            want[77] = (2048, 2048 * top, top, top)
            assert np.array_equal(got, want), (ty, what)
        # ... and as a width-0 value column whose reference is the maximum (nothing is read at all)
        got = u64_of(fl.FoR.unfor_aggregate_by(0, to_dev(np.zeros(0, dt)), top, 0, to_dev(np.zeros(0, np.uint8)), 77, n_blocks=2))
        assert np.array_equal(got, want), (ty, "both widths 0")


def raw_by_widths(fl, ty, dv, dk, dm, n, result):
    """The C ABI call with its own err_flag; returns the flag's value."""
    import torch
    esz = tbits(ty) // 8
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    (w, o, col, refs), (kw, ko, kcol, krefs) = dv, dk
    rc = getattr(fl.load(), f"fl_{ty}_unfor_aggregate_by_widths")(
        w.data_ptr(), o.data_ptr(), col.data_ptr(), col.numel() * esz, refs.data_ptr(), 1, kw.data_ptr(), ko.data_ptr(), kcol.data_ptr(),
        kcol.numel(), krefs.data_ptr(), 1, None if dm is None else dm.data_ptr(), n, result.data_ptr(), err.data_ptr(), stream)
    assert rc == 0
    return int(err.item())


@pytest.mark.parametrize("ty", TYS)
def test_device_errors_flag_and_skip_the_block(fl, oracle, ty):
    """A value block of width T + 1, a key block of width 9, a misaligned key offset, a value block outside its column: exactly that
    block's FL_DEVERR_* bits, the result is the reference without that block -- whichever column failed -- and check=True raises."""
    import torch
    T = tbits(ty)
    n = 20
    rng = np.random.default_rng(18800 + T)
    widths = rng.integers(1, T + 1, size=n)
    refs = values(ty, n, 18801 + T)
    vw, voff, vcol, vals = value_column(oracle, ty, widths, 18802 + T, refs)
    kw, koff, kcol, krefs, keys = key_column(oracle, [key_blocks(oracle, ("uniform", "wrapping", "two")[b % 3], 1, rng)[0] for b in range(n)])
    bits = rng.random(n * 1024) < 0.4
    dm = mask_words(bits)

    def changed(a, b, v):
        a = a.copy()
        a[b] = v
        return a
    cases = [("value width T + 1", 7, 1, 1, changed(vw, 7, T + 1), voff, kw, koff),
             ("key width 9", 3, 1, 1, vw, voff, changed(kw, 3, 9), koff),
             ("key offset + 8", 5, 4, 4, vw, voff, kw, changed(koff, 5, koff[5] + 8)),
             ("value block out of bounds", 11, 8, 6, vw, changed(voff, 11, voff[11] + (1 << 40)), kw, koff)]
    for what, b, flag, status, vw_, voff_, kw_, koff_ in cases:
        dv, dk = dev_column(vw_, voff_, vcol, refs), dev_column(kw_, koff_, kcol, krefs)
        for m, mbits in ((dm, bits), (None, None)):
            buf, slots = sentinel_slots(GROUPS)
            assert raw_by_widths(fl, ty, dv, dk, m, n, slots) == flag, (ty, what)
            check_result(buf, slots, expected_groups(vals, keys, mbits, without=(b,)), (ty, what))
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_aggregate_by_widths(*dv, *dk, dm)
        assert ei.value.status == status, (ty, what)
    # all four at once: every bit, every one of the blocks skipped
    dv = dev_column(changed(vw, 7, T + 1), changed(voff, 11, voff[11] + (1 << 40)), vcol, refs)
    dk = dev_column(changed(kw, 3, 9), changed(koff, 5, koff[5] + 8), kcol, krefs)
    buf, slots = sentinel_slots(GROUPS)
    assert raw_by_widths(fl, ty, dv, dk, dm, n, slots) == 1 | 4 | 8
    check_result(buf, slots, expected_groups(vals, keys, bits, without=(3, 5, 7, 11)), (ty, "all four"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("residue", [16, 80])
@pytest.mark.parametrize("ty", TYS)
def test_buffers_at_16_byte_residues(fl, oracle, ty, residue):
    """keys, mask and result placed at a 16-byte residue off the 128-byte boundary: the result is right and no byte around them changes"""
    T = tbits(ty)
    n = 9
    rng = np.random.default_rng(18900 + T + residue)
    w = T // 2
    pk = values(ty, n * packed_len(ty, w), 18901 + T)
    refs = values(ty, n, 18902 + T)
    vals = oracle.batch("unfor_pack", ty, w, pk, aux=refs, n_blocks=n)
    _, _, kcol, krefs, keys = key_column(oracle, key_blocks(oracle, "wrapping", n, rng))
    bits = rng.random(n * 1024) < 0.5
    seed = 18910 + 8 * T + residue
    pkeys = placed(kcol, "u8", residue, seed)
    pmask = placed(np.packbits(bits, bitorder="little").view(np.int32), "int32", residue, seed + 1)
    pres = placed(np.full(GROUPS * 4, SENTINEL, dtype=np.uint64).view(np.int64), "int64", residue, seed + 2)
    got = fl.FoR.unfor_aggregate_by(w, to_dev(pk), to_dev(refs), 3, pkeys.t, to_dev(krefs), pmask.t, result=pres.t)
    assert got.data_ptr() == pres.t.data_ptr() and got.data_ptr() % 128 == residue
    assert np.array_equal(pres.np().view(np.uint64).reshape(GROUPS, 4), expected_groups(vals, keys, bits)), (ty, residue)
    for p, what in ((pkeys, "keys"), (pmask, "mask"), (pres, "result")):
        p.check_guards((ty, residue, what))
    assert np.array_equal(pkeys.np().view(np.uint8), pkeys.before()) and np.array_equal(pmask.np().view(np.uint8), pmask.before())


@pytest.mark.parametrize("ty", TYS)
def test_deterministic_and_consistent_with_unfor_aggregate(fl, oracle, ty):
    """Two runs of the same call are bit-identical, and the 256 slots combined are what aggregate_reduce(unfor_aggregate_widths(..))
    gives for the value column under the same mask."""
    T = tbits(ty)
    n = 67
    rng = np.random.default_rng(19000 + T)
    (vw, voff, vcol, refs, vals), (kw, koff, kcol, krefs, keys) = mixed_case(oracle, ty, n, rng, 19001 + T)
    dv, dk = dev_column(vw, voff, vcol, refs), dev_column(kw, koff, kcol, krefs)
    for name, bits in masks_of(n, rng).items():
        dm = None if bits is None else mask_words(bits)
        first = u64_of(fl.unfor_aggregate_by_widths(*dv, *dk, dm))
        again = u64_of(fl.unfor_aggregate_by_widths(*dv, *dk, dm))
        assert np.array_equal(first, again), (ty, name, "two runs differ")
        assert np.array_equal(first, expected_groups(vals, keys, bits)), (ty, name)
        whole, _ = fl.unfor_aggregate_widths(*dv, dm)
        assert np.array_equal(combine(first), u64_of(whole)), (ty, name, "the groups do not add up to the column")
