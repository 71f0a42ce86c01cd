"""GPU: the tail and shape handling the four consumers of a FoR-packed column share (fl_for_block.hpp) -- unfor_compare,
unfor_compare_range, unfor_select and unfor_aggregate on ONE small column per launch shape, each against numpy on the oracle's
unfor_pack per block, through tests/gpu_support.py and the helpers that belong to one kernel's own test file.

The column has n = 2 * 4 * bpw + r blocks (a workgroup takes 4 * bpw): two full workgroups and a tail of r in {1, bpw - 1, bpw + 1}
blocks -- shorter than bpw (the block-by-block route of select and aggregate, the short prefetched route of compare and range) or
starting a second wavefront.  The mixed-width column holds a width-0 block, a block whose width exceeds T (FL_DEVERR_WIDTH: skipped,
its mask words and output slots untouched, its aggregate the identity), a block with an empty incoming mask and one with an all-ones
mask."""
import ctypes

import numpy as np
import pytest

import test_gpu_aggregate as agg
import test_gpu_for_compare_range as rng_
import test_gpu_select as sel
from datagen import values
from oracle_lib import packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import GUARD, IDENTITY, TYS, expected_blocks, got_mask, mixed_column, sentinel_buffer, sentinel_of, sentinel_slots, to_dev, want_mask
from test_gpu_for_compare_range import PREFILL, prefilled

pytestmark = pytest.mark.gpu

# (kernel policy, blocks per wavefront the tails are cut for): the policies of test_gpu_for_compare_range.py; the default shapes take
# at most 4 blocks per wavefront, policy 1 takes one
SHAPES = [(0, 4), (1, 1), (2, 4), (2 + 256 * 4 + 65536 * 4 + (1 << 24), 4), (2 + 256 * 6 + 65536 * 3, 3), (2 + 256 * 4 + 65536 * 12 + (1 << 24), 12)]
ZERO_W, BAD_W, EMPTY, FULL = 2, 5, 6, 7          # the special blocks of the mixed column (all inside the first wavefronts' blocks)


def column_masks(n, seed):
    """bool[n * 1024] at half density with one empty and one full block; the same as int32 words"""
    bits = np.random.default_rng(seed).random(n * 1024) < 0.5
    bits[EMPTY * 1024:(EMPTY + 1) * 1024] = False
    bits[FULL * 1024:(FULL + 1) * 1024] = True
    return bits, np.packbits(bits, bitorder="little").view(np.int32)


def raw_masks(fl, ty, name, dw, doff, dcol, drefs, n, extra):
    """The C ABI call fl_<ty>_<name>_widths with its own err_flag; extra["args"]: its arguments between ref_stride and n_blocks;
    extra["output"]: the mask to write (default: a prefilled one).  Returns (mask words [n, 32], the flag's value)."""
    import torch
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    mask = extra["output"] if "output" in extra else prefilled(n)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (dw.data_ptr(), doff.data_ptr(), dcol.data_ptr(), dcol.numel() * (tbits(ty) // 8), drefs.data_ptr(), 1)
    rc = getattr(fl.load(), f"fl_{ty}_{name}_widths")(*head, *extra["args"], n, mask.data_ptr(), err.data_ptr(), stream)
    assert rc == 0
    return got_mask(mask).reshape(n, 32), int(err.item())


@pytest.mark.parametrize("policy,bpw", SHAPES)
@pytest.mark.parametrize("ty", TYS)
def test_tails_and_special_blocks_through_every_consumer(fl, oracle, kernel_policy, ty, policy, bpw):
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    N = 1 << T
    for r in sorted({1, bpw - 1, bpw + 1} - {0}):
        n = 2 * 4 * bpw + r
        what = (ty, policy, n)
        rs = np.random.default_rng(20000 + 64 * T + n)
        widths = rs.integers(1, T + 1, size=n)
        widths[ZERO_W] = 0
        dw, doff, col, blocks = mixed_column(ty, widths, 20100 + n)
        refs = values(ty, n, 20200 + n)
        vals = np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])
        bad_w = widths.astype(np.uint8)
        bad_w[BAD_W] = T + 1
        dbw = torch.from_numpy(bad_w).cuda()
        dcol, drefs = to_dev(col), to_dev(refs)
        bits, words = column_masks(n, 20300 + n)
        dm = to_dev(words)
        ok = np.arange(n) != BAD_W
        # a uniform-width column of the same shape (no block can fail: the Python surface)
        wu = T // 2 + 1
        pku = values(ty, n * packed_len(ty, wu), 20400 + n)
        valsu = oracle.batch("unfor_pack", ty, wu, pku, aux=refs, n_blocks=n)
        dpku = to_dev(pku)
        # an interval that leaves most blocks undecided, and the constant at its lower end
        lo, hi = int(refs[n // 2]), (int(refs[n // 2]) + (N >> 2)) % N

        # unfor_compare
        g, flag = raw_masks(fl, ty, "unfor_compare", dbw, doff, dcol, drefs, n, dict(args=(fl.BitPacking.CMP["<="], lo)))
        assert flag == 1, (what, "compare", flag)
        assert (g[BAD_W] == PREFILL).all() and np.array_equal(g[ok], want_mask(vals, "<=", lo).reshape(n, 32)[ok]), (what, "compare")
        assert np.array_equal(got_mask(fl.FoR.unfor_compare(wu, dpku, drefs, "<=", lo)), want_mask(valsu, "<=", lo)), (what, "compare, uniform")

        # unfor_compare_range: NEW, AND, OR out of place, AND in place
        for code, cb in enumerate(rng_.COMBINE):
            want = rng_.want_mask(vals, lo, hi, cb, words).reshape(n, 32)
            g, flag = raw_masks(fl, ty, "unfor_compare_range", dbw, doff, dcol, drefs, n, dict(args=(lo, hi, code, dm.data_ptr() if code else None)))
            assert flag == 1, (what, cb, flag)
            assert (g[BAD_W] == PREFILL).all() and np.array_equal(g[ok], want[ok]), (what, cb)
            args = dict(mask=dm, combine=cb) if cb != "new" else {}
            got = got_mask(fl.FoR.unfor_compare_range(wu, dpku, drefs, lo, hi, n_blocks=n, output=prefilled(n), **args))
            assert np.array_equal(got, rng_.want_mask(valsu, lo, hi, cb, words)), (what, cb, "uniform")
        inplace = dm.clone()
        g, flag = raw_masks(fl, ty, "unfor_compare_range", dbw, doff, dcol, drefs, n, dict(args=(lo, hi, 1, inplace.data_ptr()), output=inplace))
        want = rng_.want_mask(vals, lo, hi, "and", words).reshape(n, 32)
        assert flag == 1 and np.array_equal(g[ok], want[ok]), (what, "and in place")
        assert np.array_equal(g[BAD_W], words.reshape(n, 32)[BAD_W]), (what, "and in place: the skipped block keeps its incoming mask")
        inplace = dm.clone()
        fl.FoR.unfor_compare_range(wu, dpku, drefs, lo, hi, mask=inplace, combine="and", output=inplace)
        assert np.array_equal(got_mask(inplace), rng_.want_mask(valsu, lo, hi, "and", words)), (what, "and in place, uniform")

        # unfor_select: the skipped block's run keeps the sentinel
        oo, total = fl.mask_offsets(dm)
        kept = int(bits.sum())
        buf = sentinel_buffer(ty, kept + GUARD)
        assert sel.raw_select_widths(fl, ty, dbw, doff, dcol, drefs, dm, oo, buf, buf.numel()) == 1, (what, "select")
        want = vals.copy()
        want[BAD_W * 1024:(BAD_W + 1) * 1024] = sentinel_of(ty)
        sel.check_select(ty, buf, total, want, bits, (what, "select"))
        buf = sentinel_buffer(ty, kept + GUARD)
        fl.FoR.unfor_select(wu, dpku, drefs, dm, out_offsets=oo, total=total, n_blocks=n, output=buf)
        sel.check_select(ty, buf, total, valsu, bits, (what, "select, uniform"))

        # unfor_aggregate: the skipped block's slot holds the identity
        sbuf, slots = sentinel_slots(n)
        assert agg.raw_aggregate_widths(fl, ty, dbw, doff, dcol, drefs, dm, slots) == 1, (what, "aggregate")
        want = expected_blocks(vals, bits)
        want[BAD_W] = IDENTITY
        agg.check_slots(sbuf, n, fl.aggregate_reduce(slots), want, (what, "aggregate"))
        sbuf, slots = sentinel_slots(n)
        result, _ = fl.FoR.unfor_aggregate(wu, dpku, drefs, dm, n_blocks=n, block_aggs=slots)
        agg.check_slots(sbuf, n, result, expected_blocks(valsu, bits), (what, "aggregate, uniform"))
