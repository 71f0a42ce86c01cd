"""GPU: unfor_aggregate_columns / unfor_aggregate_columns_widths -- COUNT / SUM / MIN / MAX of a * b, a + b, a - b between two packed
columns -- on column pairs in which ONE row decides (tests/expr_extrema_data.py):
 * '*' and '+': a sweeping column of tests/extrema_data.py against a constant one, in both roles and with the constant side packed
   as width 0 (the DECODE_A / DECODE_B routes) and with equal fields under a nonzero reference (DECODE_BOTH): every position of a
   block is the only minimum of x in one block and the only maximum in another, the runner-up one step (c, or 1) away and next to it;
   c = 2^(T-1) sets the pair blocks' leading values apart in one bit round the 16- and 32-bit edges of the narrow accumulators;
 * '-': blocks that cross zero -- d = 0 once (the unsigned minimum), d = -1 once (the unsigned maximum 2^64 - 1), their runner-ups
   +1 and -2 next to them -- at narrow, middle and full width, and d = -(2^T - 1) / +(2^T - 1);
 * the named masks of extrema_data, taken from x: under `without min` a zero-crossing block's minimum is 1, under `without max` its
   maximum 2^64 - 2 -- a masked-off row that still took part would win;
 * u8 / u16 blocks whose 1024 rows hold the extreme operands: the largest sums the narrow accumulators are argued to hold.
Uniform random data (tests/test_gpu_aggregate_columns.py) sees none of this: tests/checker/make_badextrema_sources.py holds four
defects of fl_aggregate_columns.hpp that only these columns meet (profiles/expr_extrema_known_bad.txt).

Every expected value is a numpy reduction of x = group_columns_data.expr(op, a, b) over the CONSTRUCTED values (or python integers);
the columns are packed by the oracle's for_pack and nothing is unpacked on the host.  Bit-exact.  The conditions are asserted on the
CPU before any launch."""
import numpy as np
import pytest

import expr_extrema_data as xd
import extrema_data as ed
from group_columns_data import expr
from oracle_lib import TYPES, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import POLICIES, TYS, check_slots, expected_blocks, mask_words, sentinel_slots, to_dev

pytestmark = pytest.mark.gpu

U = np.uint64
_SWEEPS = {}                                                                # (ty, W, kind) -> (Column, packed), one type's at a time


def sweep_column(oracle, ty, W, kind):
    """(extrema_data.Column, the column packed by the oracle's for_pack): '*' and '+' of a type share the columns"""
    if _SWEEPS and next(iter(_SWEEPS))[0] != ty:
        _SWEEPS.clear()
    if (ty, W, kind) not in _SWEEPS:
        dt = TYPES[ty][0]
        c = ed.column(tbits(ty), W, kind)
        _SWEEPS[ty, W, kind] = (c, oracle.batch("for_pack", ty, W, c.values.astype(dt), aux=np.full(c.n, c.r, dtype=dt)))
    return _SWEEPS[ty, W, kind]


def constant_column(oracle, ty, n, w, r, value):
    """n blocks that hold `value` in every row at width w under the reference r, packed by the oracle (width 0: no bytes)"""
    dt = TYPES[ty][0]
    return np.tile(oracle.for_pack(ty, w, np.full(1024, value, dtype=dt), r), n)


def masks_and_expectations(n, x, min_pos, max_pos, seed):
    """[(name, device mask or None, expected slots)] for the named masks"""
    return [(name, None if bits is None else mask_words(bits), expected_blocks(x, bits))
            for name, bits in ed.named_masks(n, min_pos, max_pos, seed).items()]


# ---------------------------------------------------------------------------------------------------------------------------------
# '*' and '+': sweep o constant, uniform width
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["*", "+"])
@pytest.mark.parametrize("ty", TYS)
def test_sweep_against_a_constant(fl, oracle, kernel_policy, ty, op):
    """expr_extrema_data.sweep_plan(T, op): W in {2, T / 2 + 1, T} (and 1, and 3 for u32, under '*'), each under its reference kind and
    constant; column a sweeps against the constant packed one way, then column b sweeps against it packed the other way; every named
    mask; the kernel policies of test_gpu_aggregate.py.  The deciding row of every block: min_pos / max_pos, taken from x."""
    T = tbits(ty)
    for W, kind, c, pack_a, pack_b in xd.sweep_plan(T, op):
        col, pk = sweep_column(oracle, ty, W, kind)
        x = expr(op, col.values, U(c))
        min_pos, max_pos = xd.check_sweep(T, W, op, c, col, x)
        calls = masks_and_expectations(col.n, x, min_pos, max_pos, ed.seed_of(T, W, "zero") + 11)
        dpk = to_dev(pk)
        for role, packing in (("a", pack_a), ("b", pack_b)):
            cw, cr, _ = xd.constant_side(T, c, packing)
            dcpk = to_dev(constant_column(oracle, ty, col.n, cw, cr, c))
            sweep, const = (W, dpk, col.r), (cw, dcpk, cr)
            left, right = (sweep, const) if role == "a" else (const, sweep)
            for policy in POLICIES:
                kernel_policy(policy)
                for name, dm, want in calls:
                    buf, slots = sentinel_slots(col.n)
                    result, _ = fl.FoR.unfor_aggregate_columns(*left, op, *right, mask=dm, n_blocks=col.n, block_aggs=slots)
                    check_slots(buf, col.n, result, want, T, min_pos, max_pos,
                                f"{ty} unfor_aggregate_columns: column {role} sweeps at W={W} (reference {kind}, {col.r}) {op} {c} ({packing}: "
                                f"W={cw}, reference {cr}) mask '{name}' policy={policy}")
    if op == "+":
        _SWEEPS.clear()


# ---------------------------------------------------------------------------------------------------------------------------------
# '*' and '+': the mixed-width pair
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_blocks(oracle, ty, widths, refs, values):
    """(device widths, device byte offsets, device packed column, device references) of per-block widths and references"""
    import torch
    dt = TYPES[ty][0]
    v = values.astype(dt).reshape(-1, 1024)
    r = refs.astype(dt)
    blocks = [oracle.for_pack(ty, int(w), v[b], r[b]) for b, w in enumerate(widths)]
    col = np.concatenate(blocks) if blocks else np.zeros(0, dt)
    off = np.concatenate([[0], np.cumsum(widths.astype(np.int64) * 128)])
    assert off[-1] == col.size * (tbits(ty) // 8)
    return torch.from_numpy(widths.astype(np.uint8)).cuda(), torch.from_numpy(off[:-1].copy()).cuda(), to_dev(col), to_dev(r)


@pytest.mark.parametrize("op", ["*", "+"])
@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_pair(fl, oracle, kernel_policy, ty, op):
    """expr_extrema_data.mixed_pair: 1024 blocks, block b with the sweep pattern of position b at a width of its own (five widths and
    the reference kinds in turn), the constant side cycling through the constants, width 0 in the even blocks and packed in the odd
    ones, then a tail in which width-0 blocks of both sides meet; both roles."""
    T = tbits(ty)
    m = xd.mixed_pair(T, op)
    xd.check_mixed_pair(m)
    sweep = pack_blocks(oracle, ty, m.widths, m.refs, m.values)
    const = pack_blocks(oracle, ty, m.cw, m.cr, m.cvalues)
    calls = masks_and_expectations(m.n, m.x, m.min_pos, m.max_pos, 97100 + T)
    for role, left, right in (("a", sweep, const), ("b", const, sweep)):
        for policy in POLICIES:
            kernel_policy(policy)
            for name, dm, want in calls:
                buf, slots = sentinel_slots(m.n)
                result, _ = fl.unfor_aggregate_columns_widths(*left, op, *right, mask=dm, block_aggs=slots)
                check_slots(buf, m.n, result, want, T, m.min_pos, m.max_pos,
                            f"{ty} unfor_aggregate_columns_widths: column {role} sweeps, {op}, mask '{name}' policy={policy}",
                            lambda b: f" (W={int(m.widths[b])}, reference {int(m.refs[b])}, against {int(m.c[b])} at W={int(m.cw[b])})")


# ---------------------------------------------------------------------------------------------------------------------------------
# '-' across zero
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYS)
def test_differences_across_zero(fl, oracle, kernel_policy, ty):
    """expr_extrema_data.zero_crossing at the three spans: every block packed at its own width under its own minimum
    (unfor_aggregate_columns_widths), and the whole column at the widest block's width with the per-block references (the uniform
    form).  Block p: the minimum 0 sits at position p alone, the maximum 2^64 - 1 (d = -1) at 1023 - p alone."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    for which in xd.SPANS:
        z = xd.zero_crossing(T, which)
        xd.check_crossing(z)
        calls = masks_and_expectations(z.n, z.x, z.min_pos, z.max_pos, 96100 + T)
        by_name = {name: want for name, _, want in calls}
        assert (by_name["without min"][:1024, 2] == U(1)).all() and (by_name["without max"][:1024, 3] == U(2 ** 64 - 2)).all()
        assert (by_name["all"][:1024, 2] == U(0)).all() and (by_name["all"][:1024, 3] == U(2 ** 64 - 1)).all()
        a, b = pack_blocks(oracle, ty, z.wa, z.ra, z.a), pack_blocks(oracle, ty, z.wb, z.rb, z.b)
        ua, ub = int(z.wa.max()), int(z.wb.max())
        dua = to_dev(oracle.batch("for_pack", ty, ua, z.a.astype(dt), aux=z.ra.astype(dt)))
        dub = to_dev(oracle.batch("for_pack", ty, ub, z.b.astype(dt), aux=z.rb.astype(dt)))
        for policy in POLICIES:
            kernel_policy(policy)
            for name, dm, want in calls:
                what = f"{ty} a - b across zero, span {which} ({z.S}), mask '{name}' policy={policy}"
                buf, slots = sentinel_slots(z.n)
                result, _ = fl.unfor_aggregate_columns_widths(*a, "-", *b, mask=dm, block_aggs=slots)
                check_slots(buf, z.n, result, want, T, z.min_pos, z.max_pos, "unfor_aggregate_columns_widths " + what,
                            lambda blk: f" (W={int(z.wa[blk])} - W={int(z.wb[blk])})")
                buf, slots = sentinel_slots(z.n)
                result, _ = fl.FoR.unfor_aggregate_columns(ua, dua, a[3], "-", ub, dub, b[3], mask=dm, n_blocks=z.n, block_aggs=slots)
                check_slots(buf, z.n, result, want, T, z.min_pos, z.max_pos, f"unfor_aggregate_columns W={ua} - W={ub} " + what)


# ---------------------------------------------------------------------------------------------------------------------------------
# the largest sums
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", ["u8", "u16"])
def test_largest_sums_a_block_can_hold(fl, oracle, kernel_policy, ty):
    """One block, every row kept, all 1024 rows a = b = 2^T - 1 ('*', '+') or a = 0, b = 2^T - 1 and the reverse ('-'): 1024 times the
    largest magnitude of x, through both sides packed at W = T, either side width 0 and both width 0.  Every row decides the sum."""
    T = tbits(ty)
    for op, a, b, want in xd.largest_sums(T):
        want = np.array([want], dtype=U)
        for pa, pb in xd.ROUTES:
            (wa, ra), (wb, rb) = xd.side(T, a, pa), xd.side(T, b, pb)
            dpa, dpb = to_dev(constant_column(oracle, ty, 1, wa, ra, a)), to_dev(constant_column(oracle, ty, 1, wb, rb, b))
            for policy in POLICIES:
                kernel_policy(policy)
                buf, slots = sentinel_slots(1)
                result, _ = fl.FoR.unfor_aggregate_columns(wa, dpa, ra, op, wb, dpb, rb, mask=None, n_blocks=1, block_aggs=slots)
                check_slots(buf, 1, result, want, T, [0], [1023], f"{ty} unfor_aggregate_columns: 1024 rows of {a} {op} {b}, W={wa} and W={wb}, policy={policy}")
