"""GPU: the edges of the run walk the six run-walking kernels have in common (fl_block_run.hpp describes it) -- unfor_aggregate_by,
unfor_aggregate_by_columns, unfor_aggregate_by_window, unfor_aggregate_by_lookup, unfor_set_build and unfor_lookup through their
_widths entry points, each against the numpy reference its own data module gives.  The sibling of test_gpu_for_consumer_shapes.py.

Runs of 3 blocks are forced through the kernel policy's blocks-per-wavefront field.  n = 1: a wavefront with one block, whose
look-ahead asks for that block again; n = 3: exactly one run; n = 4: one run and a one-block tail run; n = 7: two runs and a tail.
The mask keeps every row, is None, or is a random one whose last block is empty (n = 1: the only block, so nothing is flushed).
Group 0 (key, slot or bit 0 of the window) occurs in the column's first block only and group 1 in its last block only: a flush that
is dropped, or a run that ends one block early, loses one of them.  (A flush that forgot its count > 0 guard would not show in any
result: combining an identity slot changes nothing.)  The window and lookup kernels run in each tier they have for the type, at the
window on either side of the tier boundary the kernels' *_map.hpp headers name."""
import functools
import os
import re

import numpy as np
import pytest

from aggregate_by_lookup_data import code_table, expected_fused
from aggregate_by_window_data import WHAT, expected_table, table_arrays, u64
from datagen import values
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import got_mask, mask_words, to_dev, to_np, u64_of
from group_columns_data import expr
from group_data import expected_groups
from lookup_data import RUN_OF_3, expected_lookup, table_of, window_lo
from oracle_lib import TYPES, tbits
from set_build_data import encode, expected_build, stats_of, words_of

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fastlanes_amd", "csrc")
FIRST_ONLY, LAST_ONLY = 0, 1                     # the groups only the column's first / last block holds
COMMON = (2, 200)                                # the groups every block holds
FAR = 100000                                     # ... and, where the type has room, rows beyond every window
KERNELS = ("aggregate_by", "aggregate_by_columns", "aggregate_by_window", "aggregate_by_lookup", "set_build", "lookup")
MASKS = ("every row", "no mask", "last block empty")


def header_constant(header, name):
    """the value of `constexpr <integer type> <name> = <number>;` in a csrc header"""
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, header)).read())
    assert m, (header, name)
    return int(m.group(1))


def tiers(ty, boundary):
    """the windows on either side of a tier boundary that the type's domain has room for"""
    N = 1 << tbits(ty)
    return [min(boundary, N)] + ([boundary + 1] if boundary + 1 <= N else [])


def group_ids(ty, n, rng):
    """int64[n * 1024]: a group id per row"""
    ids = rng.integers(*COMMON, size=(n, 1024))
    if tbits(ty) > 16:
        far = rng.random((n, 1024)) < 0.2
        ids[far] = FAR + rng.integers(0, 50, size=int(far.sum()))
    ids[0, [5, 700]] = FIRST_ONLY
    ids[n - 1, [3, 1000]] = LAST_ONLY
    return ids.reshape(-1)


def masks_of(n, rng):
    """name -> bool[n * 1024] or None"""
    sparse = rng.random((n, 1024)) < 0.5
    sparse[0, [5, 700]] = True                   # the first block's own group stays
    sparse[n - 1] = False
    return dict(zip(MASKS, (np.ones(n * 1024, bool), None, sparse.reshape(-1))))


@functools.lru_cache(maxsize=None)
def host_case(ty, n):
    """the (ty, n) column set on the host, built once: (lo, ids, keys, u8 keys, values a, values b, masks)"""
    T = tbits(ty)
    rng = np.random.default_rng(99000 + 64 * T + n)
    lo = window_lo(ty)                           # near 2^T - 1: the windows are cyclic
    ids = group_ids(ty, n, rng)
    keys = ((ids.astype(np.uint64) + np.uint64(lo)) & np.uint64((1 << T) - 1)).astype(TYPES[ty][0])
    keys8 = np.where(ids >= FAR, 250, ids).astype(np.uint8)
    va, vb = values(ty, n * 1024, 99100 + T + n), values(ty, n * 1024, 99200 + T + n)
    masks = masks_of(n, rng)
    for mname in MASKS[:2]:                      # the flush's groups: one block each, and both are kept
        kept = np.ones(n * 1024, bool) if masks[mname] is None else masks[mname]
        for g, blk in ((FIRST_ONLY, 0), (LAST_ONLY, n - 1)):
            assert set(np.flatnonzero((ids == g) & kept) // 1024) == {blk}, (ty, n, mname, g)
    return lo, ids, keys, keys8, va, vb, masks


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [1, 3, 4, 7])
@pytest.mark.parametrize("ty", ["u8", "u64"])
def test_run_edges(fl, oracle, kernel_policy, ty, n, kernel):
    kernel_policy(RUN_OF_3)
    lo, ids, keys, keys8, va, vb, masks = host_case(ty, n)
    a, key = encode(fl, ty, va), encode(fl, ty, keys)
    for mname, keep in masks.items():
        dm = None if keep is None else mask_words(keep)
        what = (ty, n, kernel, mname)
        if kernel == "aggregate_by":
            got = u64_of(fl.unfor_aggregate_by_widths(*a, *encode(fl, "u8", keys8), dm))
            assert np.array_equal(got, expected_groups(va, keys8, keep)), what
        elif kernel == "aggregate_by_columns":
            got = u64_of(fl.unfor_aggregate_by_columns_widths(*a, "*", *encode(fl, ty, vb), *encode(fl, "u8", keys8), dm))
            assert np.array_equal(got, expected_groups(expr("*", va, vb), keys8, keep)), what
        elif kernel == "aggregate_by_window":
            for ng in tiers(ty, header_constant("fl_aggregate_by_window_map.hpp", "AGGREGATE_BY_WINDOW_LDS_GROUPS")):
                want, stats = expected_table(ty, va, keys, keep, lo, ng)
                table, st = fl.unfor_aggregate_by_window_widths(*a, *key, lo, ng, mask=dm, what=WHAT)
                assert all(np.array_equal(g, w) for g, w in zip(table_arrays(table), want)), (what, ng)
                assert u64(st).tolist() == stats.tolist(), (what, "stats", ng)
        elif kernel == "aggregate_by_lookup":    # ONE tier; the windows around unfor_lookup's boundary for a u8 payload
            for n_slots in tiers(ty, header_constant("fl_lookup_map.hpp", "LOOKUP_LDS_BYTES")):
                codes = code_table(n_slots, 99300 + n_slots % 1000)
                want = expected_fused(ty, va, keys, keep, lo, codes, None)
                result, st = fl.unfor_aggregate_by_lookup_widths(*a, *key, lo, to_dev(codes), mask=dm)
                assert np.array_equal(u64_of(result), want[0]), (what, n_slots)
                assert u64_of(st).tolist() == want[1].tolist(), (what, "stats", n_slots)
        elif kernel == "set_build":
            for bits in tiers(ty, header_constant("fl_set_build_map.hpp", "SET_BUILD_LDS_BITS")):
                words, stats = expected_build(ty, keys, keep, lo, bits)
                ms, st = fl.unfor_set_build_widths(*key, lo, bits, mask=dm)
                assert np.array_equal(words_of(ms.words), words) and stats_of(st).tolist() == stats.tolist(), (what, bits)
        else:
            for uty in sorted({ty, "u8"}):
                for n_slots in tiers(ty, header_constant("fl_lookup_map.hpp", "LOOKUP_LDS_BYTES") // (tbits(uty) // 8)):
                    table = table_of(uty, n_slots, 99400 + n_slots % 1000)
                    w_out, w_hit, w_stats = expected_lookup(oracle, ty, uty, keys, keep, lo, table, None, 7)[:3]
                    out, hit, stats = fl.unfor_lookup_widths(*key, lo, to_dev(table), missing=7, mask=dm)
                    assert to_np(out, uty).tobytes() == w_out.tobytes(), (what, uty, n_slots, "out")
                    assert np.array_equal(got_mask(hit), w_hit), (what, uty, n_slots, "hit mask")
                    assert u64_of(stats).tolist() == w_stats.tolist(), (what, uty, n_slots, "stats")
