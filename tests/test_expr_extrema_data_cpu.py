"""CPU: the column pairs of tests/expr_extrema_data.py meet their conditions for every combination that tests/test_gpu_expr_extrema.py
and tests/test_gpu_group_extrema.py run, the combinations left out are exactly the listed u64 ones, the largest-sum blocks reach the
magnitudes the comments of fl_aggregate_columns.hpp rest on, and the checks themselves bite."""
import numpy as np
import pytest

import expr_extrema_data as xd
import extrema_data as ed
from group_columns_data import expr
from gpu_support import TYS
from oracle_lib import tbits

U = np.uint64

# (T, op, W, reference kind, c): a sum that wraps past 2^64 inside a block moves the block's extremes.  u64 only, by construction of
# this list: nothing of a narrower type may ever be left out.
LEFT_OUT = [(64, "+", 64, "wrap", 1)]


def test_only_the_listed_u64_combinations_are_left_out():
    assert all(T == 64 for T, *_ in LEFT_OUT)
    got = [(T, op, *k) for T in (8, 16, 32, 64) for op in ("*", "+") for k in xd.left_out(T, op)]
    assert got == LEFT_OUT
    for T in (8, 16, 32, 64):
        for op in ("*", "+"):
            plan = xd.sweep_plan(T, op)
            assert len(plan) + len(xd.left_out(T, op)) == len(xd.candidates(T, op))
            assert {W for W, *_ in plan} >= ({2, T // 2 + 1, T} if (T, op) != (64, "+") else {2, T // 2 + 1})
            assert {k for _, k, *_ in plan} >= ({"zero", "mid", "wrap"} if (T, op) != (64, "+") else {"zero", "mid"})
            assert {c for _, _, c, *_ in plan} >= set(xd.constants(T, op))
            assert {p for *_, p, _ in plan} == {p for *_, p in plan} == set(xd.PACKINGS)     # both packings in both roles
        assert (1, "mid", 3) in [k[:3] for k in xd.sweep_plan(T, "*")]        # W = 1 once per type


@pytest.mark.parametrize("op", ["*", "+"])
@pytest.mark.parametrize("ty", TYS)
def test_sweep_conditions_hold_for_every_combination_handed_out(ty, op):
    T = tbits(ty)
    for W, kind, c, pack_a, pack_b in xd.sweep_plan(T, op):
        col = ed.column(T, W, kind)
        ed.check_column(col, kind)
        x = expr(op, col.values, U(c))
        assert np.array_equal(x, expr(op, U(c), col.values))                 # either role: the same x
        pmin, pmax = xd.check_sweep(T, W, op, c, col, x)
        xb = x.reshape(col.n, 1024)
        rows = np.arange(col.n)
        assert (xb[rows, pmin] == xb.min(axis=1)).all() and (xb[rows, pmax] == xb.max(axis=1)).all() and (pmin != pmax).all()
        if T <= 32:                                                         # nothing wraps: x is the python integer, the extremes stay put
            assert (col.values <= U((1 << T) - 1)).all() and (pmin == col.min_pos).all() and (pmax == col.max_pos).all()
            big = [int(v) * c if op == "*" else int(v) + c for v in col.values[:2048]]
            assert [int(v) for v in x[:2048]] == big
        if W >= 2:                                                          # a masked-off minimum leaves min + step
            masks = ed.named_masks(col.n, pmin, pmax, 1)
            left = np.where(masks["without min"].reshape(col.n, 1024), xb, U(2 ** 64 - 1)).min(axis=1)
            assert (left[:1024] - xb[:1024].min(axis=1) == U(c if op == "*" else 1)).all()
        for packing in (pack_a, pack_b):
            w, r, f = xd.constant_side(T, c, packing)
            assert (f + r) % (1 << T) == c and (w == 0 or (r != 0 and f < 1 << w)) and (w > 0) == (packing == "packed")


@pytest.mark.parametrize("T", [8, 16, 32])
def test_the_half_range_constant_reaches_the_bits_round_the_accumulator_edges(T):
    assert set(xd.HIGH_BITS[T]) <= xd.high_bits_reached(T)
    assert xd.HIGH_BITS[16] == (15, 16, 30) and xd.HIGH_BITS[32] == (31, 32, 33, 62)


@pytest.mark.parametrize("op", ["*", "+"])
@pytest.mark.parametrize("ty", TYS)
def test_mixed_pair(ty, op):
    T = tbits(ty)
    m = xd.mixed_pair(T, op)
    xd.check_mixed_pair(m)
    assert m.n == 1024 + len(xd.MIXED_TAIL) and m.values.dtype == U and int(m.values.max()) < 1 << T
    v = m.values.reshape(m.n, 1024)
    M = U((1 << T) - 1)
    for b in range(m.n):                                                    # the fields fit the widths, the constant side decodes to c
        w = int(m.widths[b])
        assert w == T or int(((v[b] - m.refs[b]) & M).max()) < 1 << w
        assert int(m.cw[b]) in (0, 3, T) and (5 * int(m.cw[b] > 0) + int(m.cr[b])) % (1 << T) == int(m.c[b])
    # width-0 blocks of either side stand next to decoded ones
    assert any(m.cw[b] == 0 and m.cw[b + 1] > 0 for b in range(m.n - 1)) and any(m.widths[b] == 0 and m.widths[b + 1] > 0 for b in range(m.n - 1))


@pytest.mark.parametrize("which", xd.SPANS)
@pytest.mark.parametrize("ty", TYS)
def test_zero_crossing_blocks(ty, which):
    T = tbits(ty)
    z = xd.zero_crossing(T, which)
    xd.check_crossing(z)
    assert z.n == 1024 + 3 * (which == "full")
    masks = ed.named_masks(z.n, z.min_pos, z.max_pos, 2)
    xb = z.x.reshape(z.n, 1024)
    left = np.where(masks["without min"].reshape(z.n, 1024), xb, U(2 ** 64 - 1)).min(axis=1)
    assert (left[:1024] == U(1)).all()                                      # a masked-off d = 0 that took part would win
    left = np.where(masks["without max"].reshape(z.n, 1024), xb, U(0)).max(axis=1)
    assert (left[:1024] == U(2 ** 64 - 2)).all()                            # ... and a masked-off d = -1
    if T < 64:                                                              # the definition, in python integers
        assert [int(v) for v in z.x[:4096]] == [(int(a) - int(b)) % 2 ** 64 for a, b in zip(z.a[:4096], z.b[:4096])]
    if which == "full":
        M = (1 << T) - 1
        e = xb[1024:]
        assert U((-M) % 2 ** 64) in e[0] and U(M) in e[1] and U((-M) % 2 ** 64) in e[2] and U(M) in e[2]
        if T < 64:                                                          # the only negative d is the unsigned maximum, the only positive the minimum
            assert int(e[0].max()) == (-M) % 2 ** 64 and (e[0] == e[0].max()).sum() == 1
            assert int(e[1].min()) == M and (e[1] == e[1].min()).sum() == 1


def test_zero_crossing_check_refuses_a_second_zero_and_a_missing_neighbour():
    z = xd.zero_crossing(16, "middle")
    xd.check_crossing(z)
    keep = z.x.copy()
    far = [p for p in range(1024) if keep[300 * 1024 + p] not in (0, 1, 2 ** 64 - 1, 2 ** 64 - 2)][0]
    z.x = keep.copy()
    z.x[300 * 1024 + far] = U(0)
    with pytest.raises(AssertionError, match="d = 0 is not alone"):
        xd.check_crossing(z)
    z.x = keep.copy()
    z.x[300 * 1024 + ed.neighbours(16, 1)[300][2]] = U(5)
    with pytest.raises(AssertionError, match=r"d = \+1 is missing"):
        xd.check_crossing(z)
    z.x = keep.copy()
    z.x[300 * 1024 + far] = U(2)
    with pytest.raises(AssertionError, match="outside 3 .. span"):
        xd.check_crossing(z)


def test_sweep_check_refuses_a_duplicated_extreme_and_a_loose_runner_up():
    T, W, kind, op, c = 16, 9, "mid", "*", 3
    col = ed.column(T, W, kind)
    x = expr(op, col.values, U(c))
    xd.check_sweep(T, W, op, c, col, x)
    y = x.copy()
    y[300 * 1024 + 777] = y[300 * 1024 + 300]
    with pytest.raises(AssertionError, match="condition 1"):
        xd.check_sweep(T, W, op, c, col, y)
    with pytest.raises(AssertionError, match="condition 3"):
        xd.check_sweep(T, W, op, c, col, expr(op, col.values, U(5)))
    y = x.copy()                                                            # two blocks with their minimum at one position: a position is missed
    y[301 * 1024:302 * 1024] = y[300 * 1024:301 * 1024]
    with pytest.raises(AssertionError, match="condition 2"):
        xd.check_sweep(T, W, op, c, col, y)


@pytest.mark.parametrize("T", [8, 16])
def test_largest_sums_are_the_largest_the_accumulators_are_argued_to_hold(T):
    """fl_aggregate_columns.hpp: a u8 block sums to a magnitude < 2^26, u16 '+' and '-' to < 2^27, u16 '*' needs 64 bits"""
    M = (1 << T) - 1
    cases = xd.largest_sums(T)
    assert [op for op, *_ in cases] == ["*", "+", "-", "-"]
    for op, a, b, want in cases:
        x = a * b if op == "*" else a + b if op == "+" else a - b           # python integers
        assert want == [1024, 1024 * x % 2 ** 64, x % 2 ** 64, x % 2 ** 64]
        # no pair of operands of the type gives a larger magnitude
        assert abs(x) == max(abs(p * q if op == "*" else p + q if op == "+" else p - q) for p in (0, M) for q in (0, M))
        total = 1024 * abs(x)
        if T == 8:
            assert total < 2 ** 26 and (op != "*" or total >= 2 ** 25)
        elif op == "*":
            assert total >= 2 ** 32 and 16 * x >= 2 ** 32
        else:
            assert total < 2 ** 27 and (op != "+" or total >= 2 ** 26)
        xs = expr(op, np.full(1024, a, dtype=U), np.full(1024, b, dtype=U))
        assert int(xs.sum(dtype=U)) == want[1] and int(xs.min()) == want[2]
    assert xd.ROUTES == ((1, 1), (0, 1), (1, 0), (0, 0)) and xd.side(T, M, 1) == (T, 0) and xd.side(T, M, 0) == (0, M)
