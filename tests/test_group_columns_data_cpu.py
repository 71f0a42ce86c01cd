"""CPU: the three-column cases of tests/group_columns_data.py exercise what they claim -- asserted on the reference alone (the
oracle's unfor_pack and numpy), so the GPU test that compares against them cannot pass on a case that lost its point."""
import numpy as np
import pytest

from group_columns_data import (MIXED_BLOCKS, OPS, PAIR_CLASSES, blocks_of_group, expected, expr, kept_rows, mixed_case, pair_classes,
                                routed_case, wrapped_products)
from group_data import KEY_KINDS, KEY_WIDTH, expected_groups
from gpu_support import IDENTITY, UNIFORM_BLOCKS, mask_set
from oracle_lib import tbits

TYS = ["u8", "u16", "u32", "u64"]
SEED = 21000


@pytest.fixture(scope="module")
def cases(oracle):
    return {ty: mixed_case(oracle, ty, SEED + tbits(ty)) for ty in TYS}


def test_expr_is_the_definition():
    a, b = np.array([3, 0, 255], np.uint8), np.array([5, 1, 255], np.uint8)
    assert expr("*", a, b).tolist() == [15, 0, 65025] and expr("+", a, b).tolist() == [8, 1, 510]
    assert expr("-", a, b).tolist() == [2 ** 64 - 2, 2 ** 64 - 1, 0]        # widened first: the two's-complement 64-bit pattern
    big = np.array([2 ** 63 + 1], np.uint64)
    assert expr("*", big, np.array([2], np.uint64)).tolist() == [2] and expr("+", big, big).tolist() == [2]


@pytest.mark.parametrize("ty", TYS)
def test_mixed_case_widths_and_keys(cases, ty):
    T = tbits(ty)
    a, b, key, kinds = cases[ty]
    n = MIXED_BLOCKS[ty]
    assert n % 4 and a[0].size == b[0].size == key[0].size == n and a[4].size == b[4].size == key[4].size == n * 1024
    assert pair_classes(a[0], b[0], T) == PAIR_CLASSES                      # every (wa, wb) class of {0, 0 < w < T, T}^2
    assert ((a[0] > 0) & (b[0] > 0) & (a[0] != b[0])).any()
    assert {0, 1, 3, 8} <= set(int(w) for w in key[0]) and set(kinds) == set(KEY_KINDS)
    assert all(int(key[0][blk]) == KEY_WIDTH[kinds[blk]] for blk in range(n))
    # FoR's own add wraps mod 2^T somewhere in both value columns
    assert (a[4] < np.repeat(a[3], 1024)).any() and (b[4] < np.repeat(b[3], 1024)).any()
    keys = key[4].reshape(n, 1024)
    constant = [blk for blk in range(n) if kinds[blk] == "constant"]
    assert constant and all(key[0][blk] == 8 and len(set(keys[blk].tolist())) == 1 for blk in constant)   # one key at key width 8
    permutation = [blk for blk in range(n) if kinds[blk] == "permutation"]
    assert permutation and all((np.bincount(keys[blk], minlength=256) == 4).all() for blk in permutation)


@pytest.mark.parametrize("ty", TYS)
def test_mixed_case_values(cases, ty):
    a, b, key, _ = cases[ty]
    n = MIXED_BLOCKS[ty]
    va, vb = a[4], b[4]
    masks = mask_set(n, np.random.default_rng(SEED + 1), with_none=True)
    for name, bits in masks.items():
        kept = kept_rows(bits, va.size)
        if kept.reshape(n, 1024).any(axis=1).sum() > 1:
            assert (kept & (va < vb)).any(), (ty, name)                     # `-`: a kept row below zero
    if ty == "u64":
        assert wrapped_products(va, vb).any()
        assert (expr("+", va, vb) < va.astype(np.uint64)).any()
    if ty == "u32":
        assert (expr("*", va, vb) >= np.uint64(1 << 32)).any()
    if ty == "u16":
        assert (expected("*", a, b, key, None)[:, 1] >= np.uint64(1 << 32)).any()   # a group's sum past 32 bits
    # a group fed from more than one block, and -- at 4 and at 16 blocks per run -- from more than one wavefront's run
    g = int(np.argmax(expected("*", a, b, key, None)[:, 0]))
    blocks = blocks_of_group(key[4], None, g)
    assert blocks.size > 1 and len(set((blocks // 4).tolist())) > 1 and len(set((blocks // 16).tolist())) > 1


@pytest.mark.parametrize("ty", TYS)
def test_expected_is_the_per_row_definition(cases, ty):
    """expected() against a plain Python loop over the kept rows of a few groups"""
    a, b, key, _ = cases[ty]
    bits = np.random.default_rng(SEED + 2).random(a[4].size) < 0.01
    for op in OPS:
        got = expected(op, a, b, key, bits)
        assert got.shape == (256, 4) and got.dtype == np.uint64
        assert int(got[:, 0].sum()) == int(bits.sum())
        for g in (0, 77, 255):
            rows = np.flatnonzero(bits & (key[4] == g))
            xs = [{"*": int(x) * int(y), "+": int(x) + int(y), "-": int(x) - int(y)}[op] % 2 ** 64 for x, y in zip(a[4][rows], b[4][rows])]
            want = (len(xs), sum(xs) % 2 ** 64, min(xs), max(xs)) if xs else tuple(int(x) for x in IDENTITY)
            assert tuple(int(x) for x in got[g]) == want, (ty, op, g)
        without = expected(op, a, b, key, bits, without=(1, 2))
        bits2 = bits.copy()
        bits2[1024:3 * 1024] = False
        assert np.array_equal(without, expected_groups(expr(op, a[4], b[4]), key[4], bits2))


@pytest.mark.parametrize("ty", TYS)
def test_broadcast_case_has_one_reference_per_column(oracle, ty):
    a, b, key, _ = mixed_case(oracle, ty, SEED + 100 + tbits(ty), broadcast=True)
    assert len(set(a[3].tolist())) == 1 and len(set(b[3].tolist())) == 1 and len(set(key[3].tolist())) == 1


@pytest.mark.parametrize("ty", TYS)
def test_routed_case_holds_every_route_in_its_first_run(oracle, ty):
    n = UNIFORM_BLOCKS
    a, b, key, bits, routes = routed_case(oracle, ty, n, SEED + 200 + tbits(ty))
    assert set(routes[:4]) == {0, 1, 2} and n % 4 == 3 and n % 16 == 3      # runs of 4 and of 16: an uneven tail
    seen = {(routes[blk], bool(a[0][blk]), bool(b[0][blk])) for blk in range(n)}
    assert {(r, x, y) for r in (1, 2) for x in (False, True) for y in (False, True)} <= seen   # every expr route under ONE_KEY and DECODE
    want = expected("*", a, b, key, bits)
    g = int(np.argmax(want[:, 0]))
    blocks = blocks_of_group(key[4], bits, g)
    assert len(set((blocks // 16).tolist())) > 1                            # a group fed from several runs
