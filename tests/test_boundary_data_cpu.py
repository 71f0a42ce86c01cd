"""CPU: the boundary-dense columns of tests/boundary_data.py meet their coverage conditions for every (T, W, kf) that
tests/test_gpu_compare_boundaries.py runs, and the oracle's pack of them agrees with the independent bit model -- so the expected
masks of the GPU test (numpy comparisons of the constructed values themselves) owe nothing to anybody's unpack."""
import numpy as np
import pytest

import bitmodel
import boundary_data as bd
from gpu_support import TYS
from oracle_lib import TYPES, packed_len, tbits


@pytest.mark.parametrize("ty", TYS)
def test_coverage_conditions_hold_for_every_width_and_constant(ty):
    T = tbits(ty)
    n = 0
    for W in range(T + 1):
        for kf in bd.constants(W, bd.seed_of(T, W)):
            F = bd.fields(T, W, kf, bd.seed_of(T, W))
            assert F.shape == (bd.N_SWEEP + 18 + bd.N_RANDOM, T, 1024 // T) and F.dtype == np.uint64
            bd.check_coverage(F, W, kf)
            n += 1
    assert n >= 5 * (T - 2)        # five distinct constants from W = 3 up


def test_constants_are_the_field_edges_and_one_mid_value():
    for W in range(65):
        ks = bd.constants(W, 5)
        m = (1 << W) - 1
        assert {0, 1 & m, (m - 1) & m, m} <= set(ks) and all(0 <= k <= m for k in ks)
        if W >= 3:
            assert len(ks) == 5 and 2 <= ks[2] <= m - 3


def test_coverage_check_notices_a_missing_boundary():
    """The check itself bites: a column without kf in one position, or without one neighbour pair, is refused."""
    T, W, kf = 16, 7, 41
    F = bd.fields(T, W, kf, 1)
    G = F.copy()
    G[:, 5, 9] = np.where(G[:, 5, 9] == kf, kf + 1, G[:, 5, 9])
    with pytest.raises(AssertionError, match="condition 1"):
        bd.check_coverage(G, W, kf)
    G = F.copy()
    G[:, 4, :] = np.where((F[:, 3, :] == kf) & (F[:, 4, :] == 0), 1, F[:, 4, :])
    with pytest.raises(AssertionError, match="condition 2"):
        bd.check_coverage(G, W, kf)
    with pytest.raises(AssertionError, match="condition 3"):
        bd.check_coverage(F[:bd.N_SWEEP], W, kf)


def test_index_order_matches_the_bit_model():
    F = np.arange(3 * 1024, dtype=np.uint64).reshape(3, 32, 32)
    v = bd.in_index_order(F).reshape(3, 1024)
    for b, r, l in ((0, 0, 0), (1, 7, 31), (2, 19, 4), (2, 31, 31)):
        assert v[b, bitmodel.index(r, l)] == F[b, r, l]
    F8 = np.arange(1024, dtype=np.uint64).reshape(1, 8, 128)
    assert bd.in_index_order(F8)[bitmodel.index(5, 77)] == F8[0, 5, 77]


@pytest.mark.parametrize("ty", TYS)
def test_oracle_pack_of_a_boundary_block_agrees_with_the_bit_model(oracle, ty):
    """Two blocks per (T, W) -- a sweep block and a checkerboard block -- packed by the oracle and by bitmodel.pack_bits."""
    T = tbits(ty)
    for W in range(T + 1):
        kf = bd.constants(W, bd.seed_of(T, W))[-2 if W else 0]
        F = bd.fields(T, W, kf, bd.seed_of(T, W))
        v = bd.in_index_order(F).reshape(-1, 1024)
        for b in (W % bd.N_SWEEP, bd.N_SWEEP + W % 18):
            got = oracle.pack(ty, W, v[b].astype(TYPES[ty][0]))
            assert got.size == packed_len(ty, W)
            assert [int(x) for x in got] == bitmodel.pack_bits([int(x) for x in v[b]], T, W), (ty, W, b)
