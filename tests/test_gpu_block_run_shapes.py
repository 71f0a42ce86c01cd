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
from gpu_support import TYS, got_mask, mask_words, to_dev, to_np, u64_of
from group_columns_data import expr
from group_data import expected_groups
from lookup_data import RUN_OF_3, expected_lookup, table_of, window_lo
from oracle_lib import TYPES, packed_len, tbits
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


UNLIKE = ("aggregate_by", "aggregate_by_columns", "aggregate_by_window", "aggregate_by_lookup")
UNLIKE_BLOCKS = 3


def unlike_column(fl, oracle, ty, w, refs, broadcast, seed):
    """UNLIKE_BLOCKS blocks of random packed bytes of one width under per-block `refs` -- or, broadcast, under refs[0] alone: (its
    decoded values, the uniform form's arguments, the mixed form's).  The one broadcast reference is the head of a longer tensor whose
    other elements differ from it: a reference stride of 1 where 0 is meant reads those, not past an allocation."""
    import torch
    refs = np.asarray(refs, dtype=TYPES[ty][0])
    pk = values(ty, UNLIKE_BLOCKS * packed_len(ty, w), seed)
    vals = oracle.batch("unfor_pack", ty, w, pk, aux=np.full(UNLIKE_BLOCKS, refs[0]) if broadcast else refs, n_blocks=UNLIKE_BLOCKS)
    dpk, dref = to_dev(pk), to_dev(refs)[:1] if broadcast else to_dev(refs)
    dw = torch.full((UNLIKE_BLOCKS,), w, dtype=torch.uint8, device="cuda:0")
    doff, _ = fl.widths_to_offsets(ty, dw)
    return vals, (w, dpk, dref), (dw, doff, dpk, dref)


@pytest.mark.parametrize("kernel", UNLIKE)
@pytest.mark.parametrize("ty", TYS)
def test_unlike_columns_in_both_forms(fl, oracle, kernel_policy, ty, kernel):
    """The two- and three-column kernels over 3 blocks in one run of 3 (every other wavefront of the persistent grid has none), through
    the uniform-width entry point and the mixed-width one: the columns of a call differ in width (5, 3, and 2 or 4 for the key) and in
    reference stride -- one reference per block against one broadcast reference, then the other way round -- and a - b tells a from b.
    A column, a width or a stride that reached the kernel in another column's place changes the result."""
    kernel_policy(RUN_OF_3)
    T, n = tbits(ty), UNLIKE_BLOCKS
    N = 1 << T
    rng = np.random.default_rng(99500 + T)
    lo = window_lo(ty)
    keep = rng.random(n * 1024) < 0.6
    dm = mask_words(keep)
    for flip in (False, True):
        what = (ty, kernel, "value broadcast" if flip else "key broadcast")
        va, ua, ma = unlike_column(fl, oracle, ty, 5, values(ty, n, 99600 + T), flip, 99601 + T)
        vb, ub, mb = unlike_column(fl, oracle, ty, 3, values(ty, n, 99602 + T), not flip, 99603 + T)
        k8, uk8, mk8 = unlike_column(fl, oracle, "u8", 2, [10, 50, 90], not flip if kernel == "aggregate_by" else flip, 99604 + T)
        kt, ukt, mkt = unlike_column(fl, oracle, ty, 4, [(lo + d) % N for d in (3, 0, 9)], not flip, 99605 + T)
        if kernel == "aggregate_by":
            want = expected_groups(va, k8, keep)
            assert np.array_equal(u64_of(fl.FoR.unfor_aggregate_by(*ua, *uk8, mask=dm, n_blocks=n)), want), (what, "uniform")
            assert np.array_equal(u64_of(fl.unfor_aggregate_by_widths(*ma, *mk8, dm)), want), (what, "mixed")
        elif kernel == "aggregate_by_columns":
            want = expected_groups(expr("-", va, vb), k8, keep)
            assert np.array_equal(u64_of(fl.FoR.unfor_aggregate_by_columns(*ua, "-", *ub, *uk8, mask=dm, n_blocks=n)), want), (what, "uniform")
            assert np.array_equal(u64_of(fl.unfor_aggregate_by_columns_widths(*ma, "-", *mb, *mk8, dm)), want), (what, "mixed")
        elif kernel == "aggregate_by_window":
            want, stats = expected_table(ty, va, kt, keep, lo, 12)
            for form, (table, st) in (("uniform", fl.FoR.unfor_aggregate_by_window(*ua, *ukt, lo, 12, mask=dm, what=WHAT, n_blocks=n)),
                                      ("mixed", fl.unfor_aggregate_by_window_widths(*ma, *mkt, lo, 12, mask=dm, what=WHAT))):
                assert all(np.array_equal(g, w) for g, w in zip(table_arrays(table), want)), (what, form)
                assert u64(st).tolist() == stats.tolist(), (what, form, "stats")
        else:
            codes = code_table(16, 99606)
            want = expected_fused(ty, va, kt, keep, lo, codes, None)
            for form, (result, st) in (("uniform", fl.FoR.unfor_aggregate_by_lookup(*ua, *ukt, lo, to_dev(codes), mask=dm, n_blocks=n)),
                                       ("mixed", fl.unfor_aggregate_by_lookup_widths(*ma, *mkt, lo, to_dev(codes), mask=dm))):
                assert np.array_equal(u64_of(result), want[0]), (what, form)
                assert u64_of(st).tolist() == want[1].tolist(), (what, form, "stats")


EMPTY = ("set_build", "aggregate_by_window", "lookup", "lookup_u8", "aggregate_by_lookup")


@pytest.mark.parametrize("kernel", EMPTY)
@pytest.mark.parametrize("ty", TYS)
def test_an_empty_window_never_looks_at_its_table(fl, oracle, kernel_policy, ty, kernel):
    """Zero bits, groups or slots through the C ABI, both forms, 3 blocks in one run of 3: the set's words, the window's four arrays, the
    table and its `present` bitmap are deliberately NOT NULL and NOT 16-byte aligned (4 bytes into a live allocation).  The call must
    be accepted, touch none of them, count every row as outside and give the empty window's result."""
    import ctypes
    import torch
    kernel_policy(RUN_OF_3)
    T, n = tbits(ty), UNLIKE_BLOCKS
    lo, rows = window_lo(ty), UNLIKE_BLOCKS * 1024
    vals, uv, mv = unlike_column(fl, oracle, ty, 5, values(ty, n, 99700 + T), False, 99701 + T)
    keys, uk, mk = unlike_column(fl, oracle, ty, 4, [lo, lo + 1, lo + 2], True, 99702 + T)
    live = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    odd = live.data_ptr() + 4
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib, esz = fl.load(), T // 8
    uty = ty if kernel == "lookup" else "u8"
    for form in ("uniform", "mixed"):
        def column(u, m, stride):
            (w, dpk, dref), (dw, doff, _, _) = u, m
            head = [w, dpk.data_ptr()] if form == "uniform" else [dw.data_ptr(), doff.data_ptr(), dpk.data_ptr(), dpk.numel() * esz]
            return head + [dref.data_ptr(), stride]
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        ef = [err.data_ptr()] if form == "mixed" else []
        stats = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        suffix = "_widths" if form == "mixed" else ""
        what = (ty, kernel, form)
        if kernel == "set_build":
            rc = getattr(lib, f"fl_{ty}_unfor_set_build{suffix}")(*column(uk, mk, 0), None, n, lo, 0, odd, stats.data_ptr(), *ef, stream)
        elif kernel == "aggregate_by_window":
            rc = getattr(lib, f"fl_{ty}_unfor_aggregate_by_window{suffix}")(*column(uv, mv, 1), *column(uk, mk, 0), None, n, lo, 0, odd, odd, odd, odd,
                                                                            stats.data_ptr(), *ef, stream)
        elif kernel == "aggregate_by_lookup":
            result = torch.zeros(256 * 4, dtype=torch.int64, device="cuda:0")
            rc = getattr(lib, f"fl_{ty}_unfor_aggregate_by_lookup{suffix}")(*column(uv, mv, 1), *column(uk, mk, 0), None, n, lo, 0, odd, odd,
                                                                            result.data_ptr(), stats.data_ptr(), err.data_ptr(), stream)
            want = expected_fused(ty, vals, keys, None, lo, np.zeros(0, dtype=np.uint8), None)
            assert np.array_equal(u64_of(result).reshape(256, 4), want[0]), what
        else:
            out = torch.zeros(rows * (tbits(uty) // 8), dtype=torch.uint8, device="cuda:0")
            hit = torch.full((n * 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            rc = getattr(lib, f"fl_{ty}_unfor_{kernel}{suffix}")(*column(uk, mk, 0), None, n, lo, 0, odd, odd, 7, out.data_ptr(), hit.data_ptr(),
                                                                 stats.data_ptr(), *ef, stream)
            assert (out.cpu().numpy().view(TYPES[uty][0]) == 7).all() and not got_mask(hit).any(), what
        assert rc == 0 and int(err.item()) == 0, (what, rc, int(err.item()))
        assert u64_of(stats).tolist() == [0, rows], (what, "stats")
        assert (live.cpu().numpy() == 0x5A5A5A5A).all(), (what, "the table was written")
