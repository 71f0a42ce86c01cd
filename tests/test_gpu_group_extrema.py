"""GPU: the grouped aggregates -- unfor_aggregate_by, unfor_aggregate_by_columns, unfor_aggregate_by_window, in their `_widths` forms --
where ONE row decides a group's minimum, maximum and sum:
 * one row per block: 1024 blocks, in block b only row b carries a key of the reserved range (u8 keys 200..249; for the window kernel
   the window itself, every other row falls outside and is counted in stats[1]).  Once it carries a value below every other value of
   the column, once one above; the diagonal rows of one group differ by 1 from block to block, so ONE row of ONE block decides each
   group's minimum (maximum), with the runner-up in another block: a lane map that pairs a value with a neighbour's key moves it;
 * the folded routes: a key column of width 0 (ONE_KEY / ONE_GROUP) over the sweep blocks of tests/extrema_data.py (by_columns:
   tests/expr_extrema_data.py's sweep against a constant) under the named masks.  The key reference is chosen per block so that every
   block of a call lands in a slot of its own: the slot must hold that block's aggregate, whose minimum and maximum sit at one
   position each.  Run under a launch shape whose wavefronts walk 16 blocks each, too: the fold of one block into the table while the
   wavefront goes on; and value blocks of width 0 under it, where the slot is count x reference from the mask's bits alone;
 * by_columns: the largest sums a u8 / u16 block can hold under one key (tests/test_gpu_aggregate_by.py has unfor_aggregate_by's).
Expected values: group_data.expected_groups / aggregate_by_window_data.expected_table -- numpy's add.at / minimum.at / maximum.at --
over the CONSTRUCTED values and keys; python integers for the largest sums.  Columns are packed by the oracle's for_pack or the
library's own encoder (set_build_data.encode); nothing is unpacked on the host.  Bit-exact."""
import numpy as np
import pytest

import expr_extrema_data as xd
import extrema_data as ed
from aggregate_by_window_data import WHAT, expected_table, table_arrays, u64
from group_columns_data import expr
from group_data import GROUPS, expected_groups
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import IDENTITY, SLOTS, TYS, mask_words, place, to_dev, u64_of
from oracle_lib import TYPES, packed_len, tbits
from set_build_data import encode

pytestmark = pytest.mark.gpu

U = np.uint64
RUN_OF_16 = 2 + 256 * 3 + 65536 * 16             # kernel policy: a wavefront's run is at least 16 blocks (test_gpu_aggregate_by_window.py)
RESERVED = (200, 50)                             # the reserved u8 keys: 200 .. 249
N_DIAG = 1024


# ---------------------------------------------------------------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------------------------------------------------------------
def uniform_blocks(ty, W, packed, refs, first=0, count=None):
    """blocks [first, first + count) of a uniform-width packed column as the (widths, offsets, packed, references) of the `_widths` forms"""
    import torch
    pl = packed_len(ty, W)
    n = refs.size
    count = n - first if count is None else count
    widths = torch.full((count,), W, dtype=torch.uint8, device="cuda:0")
    offsets = torch.arange(count, dtype=torch.int64, device="cuda:0") * (128 * W)
    return widths, offsets, to_dev(packed[first * pl:(first + count) * pl]), to_dev(refs[first:first + count])


def constant_blocks(oracle, ty, n, w, r, value):
    """n blocks that decode to `value` in every row: width w with the reference r, packed by the oracle's for_pack"""
    dt = TYPES[ty][0]
    pk = np.tile(oracle.for_pack(ty, w, np.full(1024, value, dtype=dt), r), n)
    return uniform_blocks(ty, w, pk, np.full(n, r, dtype=dt))


def key_width_0(ty, refs):
    """a key column of width 0: no packed byte, block b's keys are all refs[b]"""
    import torch
    n = refs.size
    z = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    return z, torch.zeros(n, dtype=torch.int64, device="cuda:0"), to_dev(np.zeros(0, TYPES[ty][0])), to_dev(refs.astype(TYPES[ty][0]))


def own_slots(count, n_slots, salt):
    """slot of each of `count` blocks, all different: a stride-37 walk through the n_slots slots"""
    assert count <= n_slots and np.gcd(37, n_slots) == 1
    return (np.arange(count, dtype=np.int64) * 37 + salt) % n_slots


# ---------------------------------------------------------------------------------------------------------------------------------
# one row per block decides
# ---------------------------------------------------------------------------------------------------------------------------------
def diagonal(n_groups):
    """(b, i, is row i of block b the diagonal row, the group's index of block b, the rank of block b inside its group)"""
    b, i = np.divmod(np.arange(N_DIAG * 1024, dtype=U), U(1024))
    return b, i, b == i, b % U(n_groups), b // U(n_groups)


def diagonal_values(n_groups):
    """[(pass, values uint64)]: everywhere else 100 .. 149; the diagonal row of block b holds its rank inside its group (`min`: 0, 1, 2,
    ... all below 100) or 160 + its rank (`max`: above 149, at most 160 + 1023 // n_groups <= 181 for the group counts used)"""
    b, i, diag, _, rank = diagonal(n_groups)
    others = U(100) + (b * U(7) + i * U(3)) % U(50)
    assert 160 + 1023 // n_groups <= 255
    return [("min", np.where(diag, rank, others)), ("max", np.where(diag, U(160) + rank, others))]


def deciding(n_groups, which, g):
    """the block (and row) whose diagonal row decides group g's minimum (rank 0) or maximum (the highest rank)"""
    blocks = np.arange(g, N_DIAG, n_groups)
    return int(blocks[0] if which == "min" else blocks[-1])


def check_diagonal_groups(T, got, want, groups, n_groups, which, what):
    """got / want: uint64[n, 4] rows count, sum, min, max of the reserved groups (in group order)"""
    if not np.array_equal(got, want):
        wrong = np.argwhere(got != want)
        g, s = (int(x) for x in wrong[0])
        blk = deciding(n_groups, which, g)
        raise AssertionError(f"{what}: {len(wrong)} entries differ, the first in group {groups[g]}: {SLOTS[s]} is {int(got[g, s])}, not {int(want[g, s])}; "
                             f"its {which}imum is decided by block {blk} alone, at {place(T, blk)}")


@pytest.mark.parametrize("ty", TYS)
def test_by_one_row_per_block_decides(fl, oracle, ty):
    """unfor_aggregate_by_widths and unfor_aggregate_by_columns_widths (x = a o b, b a packed constant): the reserved keys 200 .. 249"""
    T = tbits(ty)
    dt = TYPES[ty][0]
    first, ng = RESERVED
    b, i, diag, group, rank = diagonal(ng)
    keys = np.where(diag, U(first) + group, (b * U(7) + i * U(3)) % U(first)).astype(np.uint8)
    dkeys = encode(fl, "u8", keys)
    groups = list(range(first, first + ng))
    for which, vals in diagonal_values(ng):
        want = expected_groups(vals, keys, None)
        size = np.bincount((np.arange(N_DIAG) % ng), minlength=ng)
        assert (want[first:first + ng, 0] == size).all() and want[:first, 0].sum() == N_DIAG * 1023 and (want[first + ng:, 0] == 0).all()
        edge = want[first:first + ng, 2] if which == "min" else want[first:first + ng, 3]
        assert (edge == (0 if which == "min" else 160 + (size - 1))).all()                   # rank 0 / the last rank: one row of one block
        got = u64_of(fl.unfor_aggregate_by_widths(*encode(fl, ty, vals.astype(dt)), *dkeys))
        check_diagonal_groups(T, got[first:first + ng], want[first:first + ng], groups, ng, which, f"{ty} unfor_aggregate_by_widths, pass {which}")
        assert np.array_equal(got, want), (ty, which, "the other groups")
        for op, c, shift in (("*", 3, 0), ("+", 3, 0), ("-", 7, 7)):                         # '-': a = value + 7 against 7, x = value
            a = vals + U(shift)
            x = expr(op, a, U(c))
            want = expected_groups(x, keys, None)
            edge = want[first:first + ng, 2] if which == "min" else want[first:first + ng, 3]
            runner = x[~diag].min() if which == "min" else x[~diag].max()
            assert (edge < runner).all() if which == "min" else (edge > runner).all()        # the diagonal rows alone decide
            cw, cr, _ = xd.constant_side(T, c, "packed")
            got = u64_of(fl.unfor_aggregate_by_columns_widths(*encode(fl, ty, a.astype(dt)), op, *constant_blocks(oracle, ty, N_DIAG, cw, cr, c), *dkeys))
            check_diagonal_groups(T, got[first:first + ng], want[first:first + ng], groups, ng, which,
                                  f"{ty} unfor_aggregate_by_columns_widths a {op} {c}, pass {which}")
            assert np.array_equal(got, want), (ty, which, op, "the other groups")


@pytest.mark.parametrize("ty,ng", [(ty, ng) for ty in TYS for ng in (100, 300) if ng < 1 << tbits(ty)])
def test_by_window_one_row_per_block_decides(fl, ty, ng):
    """unfor_aggregate_by_window_widths in both tiers (100 groups: the wavefront's LDS table; 300 groups, T > 8: device memory): the
    window starts 40 keys below 2^T, only the diagonal rows fall inside; all four arrays together, then each one alone."""
    T = tbits(ty)
    N = 1 << T
    dt = TYPES[ty][0]
    lo = N - 40
    b, i, diag, group, rank = diagonal(ng)
    keys = ((np.where(diag, U(lo) + group, U((lo + ng) % 2 ** 64) + i % U(50))) & U(N - 1)).astype(dt)
    dkeys = encode(fl, ty, keys)
    groups = list(range(ng))
    for which, vals in diagonal_values(ng):
        vals = vals.astype(dt)
        want, stats = expected_table(ty, vals, keys, None, lo, ng)
        assert stats.tolist() == [N_DIAG, N_DIAG * 1023]
        size = np.bincount(np.arange(N_DIAG) % ng, minlength=ng)
        assert (want[0] == size).all() and ((want[2] == 0).all() if which == "min" else (want[3] == 160 + (size - 1)).all())
        dvals = encode(fl, ty, vals)
        for names in (WHAT, *((w,) for w in WHAT)):
            table, dstats = fl.unfor_aggregate_by_window_widths(*dvals, *dkeys, lo, ng, what=names)
            got = table_arrays(table)
            assert [g is not None for g in got] == [w in names for w in WHAT]
            have = [k for k in range(4) if got[k] is not None]
            check_diagonal_groups(T, np.stack([got[k] for k in have], axis=1), np.stack([want[k] for k in have], axis=1), groups, ng, which,
                                  f"{ty} unfor_aggregate_by_window_widths, {ng} groups, arrays {names} (columns {[WHAT[k] for k in have]}), pass {which}")
            assert u64(dstats).tolist() == stats.tolist(), (ty, ng, names, u64(dstats))


# ---------------------------------------------------------------------------------------------------------------------------------
# the folded routes: key width 0
# ---------------------------------------------------------------------------------------------------------------------------------
def check_folded(T, got, want, slot, first, min_pos, max_pos, what):
    """got / want: uint64[n_slots, 4]; slot[j]: the slot of block first + j"""
    if not np.array_equal(got, want):
        wrong = np.argwhere(got != want)
        g, s = (int(x) for x in wrong[0])
        at = np.flatnonzero(slot == g)
        where = "no block's slot" if not at.size else (f"the slot of block {first + int(at[0])} alone, whose minimum sits at {place(T, min_pos[first + at[0]])}, "
                                                       f"its maximum at {place(T, max_pos[first + at[0]])}")
        raise AssertionError(f"{what}: {len(wrong)} entries differ, the first in slot {g}: {SLOTS[s]} is {int(got[g, s])}, not {int(want[g, s])}; {where}")


def chunks(n, size):
    return [(s, min(size, n - s)) for s in range(0, n, size)]


def folded_columns(T):
    """(W, reference kind) of the sweep columns the folded routes run over: the three widths, one kind each"""
    return list(zip((2, T // 2 + 1, T), ed.REFERENCES))


@pytest.mark.parametrize("ty", TYS)
def test_by_key_width_0_folds_each_block_into_its_own_slot(fl, oracle, kernel_policy, ty):
    """unfor_aggregate_by_widths, ONE_KEY: 256 blocks of a sweep column per call, block j under the key 37 j + salt mod 256"""
    T = tbits(ty)
    dt = TYPES[ty][0]
    for W, kind in folded_columns(T):
        col = ed.column(T, W, kind)
        ed.check_column(col, kind)
        pk = oracle.batch("for_pack", ty, W, col.values.astype(dt), aux=np.full(col.n, col.r, dtype=dt))
        refs = np.full(col.n, col.r, dtype=dt)
        masks = col.masks()
        for q, (first, count) in enumerate(chunks(col.n, GROUPS)):
            slot = own_slots(count, GROUPS, q)
            dv, dk = uniform_blocks(ty, W, pk, refs, first, count), key_width_0("u8", slot.astype(np.uint8))
            rows = slice(first * 1024, (first + count) * 1024)
            for name, bits in masks.items():
                keep = None if bits is None else bits[rows]
                want = expected_groups(col.values[rows], np.repeat(slot, 1024), keep)
                dm = None if keep is None else mask_words(keep)
                for policy in (0, RUN_OF_16):
                    kernel_policy(policy)
                    got = u64_of(fl.unfor_aggregate_by_widths(*dv, *dk, dm))
                    check_folded(T, got, want, slot, first, col.min_pos, col.max_pos,
                                 f"{ty} unfor_aggregate_by_widths, key width 0, W={W} reference {kind} ({col.r}), blocks {first}.., mask '{name}' policy={policy}")


@pytest.mark.parametrize("op", ["*", "+"])
@pytest.mark.parametrize("ty", TYS)
def test_by_columns_key_width_0_folds_each_block_into_its_own_slot(fl, oracle, kernel_policy, ty, op):
    """unfor_aggregate_by_columns_widths, ONE_KEY: the sweep against a constant of expr_extrema_data.sweep_plan at W in {2, T / 2 + 1, T},
    column a sweeping against the constant packed one way, column b against the other"""
    T = tbits(ty)
    dt = TYPES[ty][0]
    for W, kind, c, pack_a, pack_b in xd.sweep_plan(T, op):
        if W not in (2, T // 2 + 1, T) or c == 1 << (T - 1):
            continue
        col = ed.column(T, W, kind)
        x = expr(op, col.values, U(c))
        min_pos, max_pos = xd.check_sweep(T, W, op, c, col, x)
        pk = oracle.batch("for_pack", ty, W, col.values.astype(dt), aux=np.full(col.n, col.r, dtype=dt))
        refs = np.full(col.n, col.r, dtype=dt)
        masks = ed.named_masks(col.n, min_pos, max_pos, ed.seed_of(T, W, "zero") + 13)
        for q, (first, count) in enumerate(chunks(col.n, GROUPS)):
            slot = own_slots(count, GROUPS, q)
            sweep, dk = uniform_blocks(ty, W, pk, refs, first, count), key_width_0("u8", slot.astype(np.uint8))
            role, packing = ("a", pack_a) if q % 2 == 0 else ("b", pack_b)
            cw, cr, _ = xd.constant_side(T, c, packing)
            const = constant_blocks(oracle, ty, count, cw, cr, c)
            left, right = (sweep, const) if role == "a" else (const, sweep)
            rows = slice(first * 1024, (first + count) * 1024)
            for name, bits in masks.items():
                keep = None if bits is None else bits[rows]
                want = expected_groups(x[rows], np.repeat(slot, 1024), keep)
                dm = None if keep is None else mask_words(keep)
                for policy in (0, RUN_OF_16):
                    kernel_policy(policy)
                    got = u64_of(fl.unfor_aggregate_by_columns_widths(*left, op, *right, *dk, dm))
                    check_folded(T, got, want, slot, first, min_pos, max_pos,
                                 f"{ty} unfor_aggregate_by_columns_widths, key width 0, column {role} sweeps at W={W} (reference {kind}) {op} {c} "
                                 f"({packing}), blocks {first}.., mask '{name}' policy={policy}")


@pytest.mark.parametrize("ty", TYS)
def test_by_window_key_width_0_folds_each_block_into_its_own_slot(fl, oracle, kernel_policy, ty):
    """unfor_aggregate_by_window_widths, ONE_GROUP: the key reference of every block inside the window.  The LDS tier: 199 blocks per call
    into 199 groups; the memory tier (T > 8): the whole column into 1049 groups.  The window starts 40 keys below 2^T."""
    T = tbits(ty)
    N = 1 << T
    dt = TYPES[ty][0]
    lo = N - 40
    for W, kind in folded_columns(T):
        col = ed.column(T, W, kind)
        pk = oracle.batch("for_pack", ty, W, col.values.astype(dt), aux=np.full(col.n, col.r, dtype=dt))
        refs = np.full(col.n, col.r, dtype=dt)
        masks = col.masks()
        calls = [(first, count, 199) for first, count in chunks(col.n, 199)] + ([(0, col.n, 1049)] if T > 8 else [])
        for q, (first, count, ng) in enumerate(calls):
            slot = own_slots(count, ng, q)
            key_refs = np.array([(int(s) + lo) % N for s in slot], dtype=U).astype(dt)
            dv, dk = uniform_blocks(ty, W, pk, refs, first, count), key_width_0(ty, key_refs)
            rows = slice(first * 1024, (first + count) * 1024)
            for name, bits in masks.items():
                keep = None if bits is None else bits[rows]
                want, stats = expected_table(ty, col.values[rows].astype(dt), np.repeat(key_refs, 1024), keep, lo, ng)
                assert int(stats[1]) == 0
                dm = None if keep is None else mask_words(keep)
                for policy in (0, RUN_OF_16):
                    kernel_policy(policy)
                    table, dstats = fl.unfor_aggregate_by_window_widths(*dv, *dk, lo, ng, mask=dm, what=WHAT)
                    check_folded(T, np.stack(table_arrays(table), axis=1), np.stack(want, axis=1), slot, first, col.min_pos, col.max_pos,
                                 f"{ty} unfor_aggregate_by_window_widths, key width 0, {ng} groups, W={W} reference {kind} ({col.r}), blocks {first}.., "
                                 f"mask '{name}' policy={policy}")
                    assert u64(dstats).tolist() == stats.tolist(), (ty, W, ng, name, policy)


@pytest.mark.parametrize("kernel,n", [("by", GROUPS), ("by_window", 199)])
@pytest.mark.parametrize("ty", TYS)
def test_constant_value_blocks_fold_into_their_own_slots(fl, kernel_policy, ty, kernel, n):
    """Value width 0 under key width 0 -- no packed byte of either column: block j holds its own reference in every row, its slot
    receives count x reference from the mask's bits alone.  256 blocks under all 256 keys (unfor_aggregate_by_widths) or 199 blocks in
    199 groups (unfor_aggregate_by_window_widths); under `only min` / `only max` ONE kept row per block carries the whole slot."""
    T = tbits(ty)
    N = 1 << T
    dt = TYPES[ty][0]
    lo = N - 40
    rng = np.random.default_rng(95000 + T + n)
    refs = np.frombuffer(rng.bytes(8 * n), dtype=U) & U(N - 1)
    refs[0], refs[1] = U(0), U(N - 1)
    min_pos = (np.arange(n) * 37) % 1024
    max_pos = 1023 - min_pos
    vals = np.repeat(refs, 1024).astype(dt)
    slot = own_slots(n, n, 5)
    dv = key_width_0(ty, refs)                                          # (the value column has the key column's shape: width 0)
    key_refs = np.array([(int(s) + lo) % N for s in slot], dtype=U).astype(dt)
    dk = key_width_0("u8", slot.astype(np.uint8)) if kernel == "by" else key_width_0(ty, key_refs)
    for name, bits in ed.named_masks(n, min_pos, max_pos, 95100 + T).items():
        dm = None if bits is None else mask_words(bits)
        for policy in (0, RUN_OF_16):
            kernel_policy(policy)
            what = f"{ty} unfor_aggregate_{kernel}_widths, value and key width 0, mask '{name}' policy={policy}"
            if kernel == "by":
                want = expected_groups(vals, np.repeat(slot, 1024), bits)
                got = u64_of(fl.unfor_aggregate_by_widths(*dv, *dk, dm))
            else:
                arrays, stats = expected_table(ty, vals, np.repeat(key_refs, 1024), bits, lo, n)
                want = np.stack(arrays, axis=1)
                table, dstats = fl.unfor_aggregate_by_window_widths(*dv, *dk, lo, n, mask=dm, what=WHAT)
                got = np.stack(table_arrays(table), axis=1)
                assert u64(dstats).tolist() == stats.tolist(), what
            check_folded(T, got, want, slot, 0, min_pos, max_pos, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# by_columns: the largest sums
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", ["u8", "u16"])
def test_by_columns_largest_sums_under_one_key(fl, oracle, ty):
    """Two blocks whose 2048 rows all hold a = b = 2^T - 1 ('*', '+'; '-': 0 and 2^T - 1, and the reverse) under the key 77, at full mask:
    the largest per-group sum the narrow accumulators can meet, through key width 0 and key width 8 and the four value routes."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    for op, a, b, (count, total, lo, hi) in xd.largest_sums(T):
        want = np.tile(IDENTITY, (GROUPS, 1))
        want[77] = (2 * count, (2 * total) % 2 ** 64, lo, hi)
        for pa, pb in xd.ROUTES:
            (wa, ra), (wb, rb) = xd.side(T, a, pa), xd.side(T, b, pb)
            dpa = to_dev(np.tile(oracle.for_pack(ty, wa, np.full(1024, a, dtype=dt), ra), 2))
            dpb = to_dev(np.tile(oracle.for_pack(ty, wb, np.full(1024, b, dtype=dt), rb), 2))
            for what, kwidth, kpacked, kref in (("key width 0", 0, np.zeros(0, np.uint8), 77),
                                                ("key width 8", 8, np.tile(oracle.for_pack("u8", 8, np.full(1024, 77, np.uint8), 0), 2), 0)):
                got = u64_of(fl.FoR.unfor_aggregate_by_columns(wa, dpa, ra, op, wb, dpb, rb, kwidth, to_dev(kpacked), kref, n_blocks=2))
                assert np.array_equal(got, want), (ty, f"2048 rows of {a} {op} {b}, W={wa} and W={wb}", what, [int(v) for v in got[77]], [int(v) for v in want[77]])
