"""CPU: the columns of tests/extrema_data.py meet their coverage conditions for every (T, W, reference) that tests/test_gpu_extrema.py
runs, the oracle's for_pack + unfor_pack gives the constructed values back (so the fields really fit their width and the GPU tests'
expectations -- numpy reductions of the constructed values -- owe nothing to anybody's unpack), and check_coverage itself bites."""
import numpy as np
import pytest

import bitmodel
import extrema_data as ed
from gpu_support import TYS
from oracle_lib import TYPES, tbits

U = np.uint64


@pytest.mark.parametrize("ty", TYS)
def test_coverage_conditions_hold_for_every_width_and_reference(ty):
    T = tbits(ty)
    assert {1, 2, T // 2 + 1, T} <= set(ed.widths_of(T))                    # block_min_max's widths are among the aggregate's
    for W in ed.widths_of(T):
        for kind in ed.REFERENCES:
            c = ed.column(T, W, kind)
            assert c.n == (2048 if W == 1 else 1024) + 2 * len(ed.pair_bits(W)) and c.values.dtype == U and c.fields.dtype == U
            ed.check_column(c, kind)
            v = c.values.reshape(c.n, 1024)
            rows = np.arange(c.n)
            assert (v[rows, c.min_pos] == v.min(axis=1)).all() and (v[rows, c.max_pos] == v.max(axis=1)).all()
            assert (c.min_pos != c.max_pos).all()
            masks = c.masks()
            assert list(masks) == ["all", "without min", "without max", "without both", "only min", "only max", "min and max only", "random 50 %"]
            assert masks["all"] is None
            for name, per_block in (("without min", 1023), ("without max", 1023), ("without both", 1022), ("only min", 1), ("only max", 1),
                                    ("min and max only", 2)):
                assert masks[name].dtype == bool and (masks[name].reshape(c.n, 1024).sum(axis=1) == per_block).all(), name
            # from W = 2 up, leaving the minimum out leaves min + 1: a masked-off row that still took part would show
            if W >= 2:
                left = np.where(masks["without min"].reshape(c.n, 1024), v, U(2 ** 64 - 1)).min(axis=1)
                assert (left[:1024] == v[:1024].min(axis=1) + U(1)).all()


def test_the_references_are_zero_one_inside_the_type_and_one_that_wraps():
    for T in (8, 16, 32, 64):
        for W in range(1, T + 1):
            zero, mid, wrap = (ed.reference(T, W, k) for k in ed.REFERENCES)
            assert zero == 0 and 0 < mid < 1 << T and 0 < wrap < 1 << T
            assert W == T or mid + (1 << W) - 1 < 1 << T
            assert wrap + (1 << W) - 1 >= 1 << T and wrap < 1 << T              # the largest field wraps, field 0 does not


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_column_covers_every_width_and_position(ty):
    T = tbits(ty)
    widths, refs, values, pmin, pmax, pos = ed.mixed_column(T)
    n = widths.size
    assert n == 1024 + T + len(ed.mixed_tail(T)) and (widths[:1024 + T] == 1 + np.arange(1024 + T) % T).all()
    assert (widths[1024 + T:] == 0).sum() >= 3 and (1024 + T) % 4 == 0         # the tail is one group of four: width 0 next to a decoded block
    ed.check_mixed_coverage(T, widths, refs, values, pos)
    v = values.reshape(n, 1024)
    assert (v[np.arange(n), pmin] == v.min(axis=1)).all() and (v[np.arange(n), pmax] == v.max(axis=1)).all() and (pmin != pmax).all()
    # the three kinds of reference all occur at every width
    for W in range(1, T + 1):
        assert {int(r) for r in refs[widths == W]} == {ed.reference(T, W, k) for k in ed.REFERENCES}, (ty, W)


@pytest.mark.parametrize("ty", TYS)
def test_oracle_for_pack_and_unfor_pack_round_trip_the_constructed_values(oracle, ty):
    """One width per type, all three references; the packed words of a sweep block agree with the independent bit model too."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    W = T // 2 + 1
    for kind in ed.REFERENCES:
        c = ed.column(T, W, kind)
        v = c.values.astype(dt)
        refs = np.full(c.n, c.r, dtype=dt)
        pk = oracle.batch("for_pack", ty, W, v, aux=refs)
        assert np.array_equal(oracle.batch("unfor_pack", ty, W, pk, aux=refs, n_blocks=c.n), v), (ty, W, kind)
        b = 517
        want = bitmodel.pack_bits([int(x) for x in c.fields[b * 1024:(b + 1) * 1024]], T, W)
        assert [int(x) for x in pk[b * len(want):(b + 1) * len(want)]] == want, (ty, W, kind)


def test_coverage_check_refuses_a_duplicated_minimum_and_a_loose_runner_up():
    T, W, kind = 16, 9, "mid"
    c = ed.column(T, W, kind)
    ed.check_column(c, kind)
    F = c.fields.reshape(c.n, 1024)
    # a second copy of block 300's minimum
    G = F.copy()
    G[300, 777] = G[300, 300]
    with pytest.raises(AssertionError, match="condition 1"):
        ed.check_coverage(G, T, W, c.r, c.n_sweep, c.pairs, False)
    # block 300's min + 1 becomes min + 2 everywhere
    G = F.copy()
    G[300] = np.where(F[300] == F[300, 300] + U(1), F[300, 300] + U(2), F[300])
    with pytest.raises(AssertionError, match="condition 2.*min \\+ 1"):
        ed.check_coverage(G, T, W, c.r, c.n_sweep, c.pairs, False)
    # max - 1 missing in the row below the maximum only
    G = F.copy()
    G[300, ed.neighbours(T, 1)[1023 - 300][0]] -= U(1)
    with pytest.raises(AssertionError, match="condition 2.*next to a maximum"):
        ed.check_coverage(G, T, W, c.r, c.n_sweep, c.pairs, False)
    # a pair block whose runner-up differs in two bits
    b, j, which = c.pairs[0]
    assert which == "min"
    G = F.copy()
    runner = np.sort(F[b])[1]
    G[b] = np.where(F[b] == runner, runner ^ U(1 << 3), F[b])
    with pytest.raises(AssertionError, match="condition 3"):
        ed.check_coverage(G, T, W, c.r, c.n_sweep, c.pairs, False)
    # a column that never wraps is refused as a wrapping one
    with pytest.raises(AssertionError, match="condition 4"):
        ed.check_coverage(F, T, W, c.r, c.n_sweep, c.pairs, True)
    # a field beyond the width
    G = F.copy()
    G[5, 5] = U(1 << W)
    with pytest.raises(AssertionError, match="wider than W"):
        ed.check_coverage(G, T, W, c.r, c.n_sweep, c.pairs, False)


def test_positions_and_neighbours_follow_the_bit_model():
    for T in (8, 16, 32, 64):
        L = 1024 // T
        near = ed.neighbours(T, 1)
        for r, l in ((0, 0), (T - 1, L - 1), (T // 2, 3), (9 % T, L - 2)):
            p = bitmodel.index(r, l)
            assert ed.row_lane(T, p) == (r, l)
            assert list(near[p]) == [bitmodel.index((r + 1) % T, l), bitmodel.index((r - 1) % T, l), bitmodel.index(r, (l + 1) % L),
                                     bitmodel.index(r, (l - 1) % L)]
