#!/usr/bin/env python3
"""unfor_compare_in_widths (WHERE x IN (set) over a mixed-width FoR-packed column: a window of the value domain plus a bitmap) on one
MI355X, next to two baselines timed in the SAME run on the SAME buffers:

  (a) unfor_compare_range_widths with the window's own interval [lo, lo + bits - 1]: the same packed bytes read, the same blocks
      decided from their metadata, no bitmap -- the floor;
  (b) what a caller did before: unfor_pack_widths of the column, then torch.isin against the member values.

The column is the generator's of `sweep.py --cases mixed` (seeded-random widths 1 .. T - 1, random packed bytes, --packed-gb of them).
Rows: windows of 8, 2048, 2049 and 2^20 bits (as far as the element type has them; 2^20 for u32 and u64 only) at about half the bits
set, every block's value range straddling the window's middle (no block is decided from its metadata); and one row at 2048 bits (u8:
8) where 99 % of the blocks lie outside the window, which both kernels answer from the metadata.  2048 bits ride in registers, 2049
are probed in memory.  Every figure is the median of --reps launches, one launch of each variant per round (round-robin), min .. max
beside it.  The kernels are launched through the C ABI (no allocation, no flag read-back inside the timed region).  Before it is timed,
every row's mask is checked bit for bit against (b)'s.

Per row the tool prints whether two expectations are met: the time is below (b)'s; and, in the 99 %-outside row, the time is within
(a)'s own run-to-run spread (max - min over its repeats, printed) of (a)'s.  How far the two tiers sit above (a) in the other rows is
a finding, not a gate.

    python tools/compare_in_timing.py [--packed-gb 1.0] [--reps 7] [--types u32,u64] > profiles/compare_in_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from sweep import SIGNED, dev, fl, median, show  # noqa: E402

UNDER_TEST = "compare_in"


def window_rows(T):
    """(row name, window bits, share of the blocks that straddle the window)"""
    sizes = [b for b in (8, 2048, 2049, 1 << 20) if b <= 1 << T and (b < 1 << 20 or T >= 32)]
    return [(f"{b} bits", b, 1.0) for b in sizes] + [("99 % outside", min(2048, 1 << (T - 5)), 0.01)]


def member_bitmap(bits, seed):
    """(int32 words of a bitmap with about half of the bits 0 .. bits - 1 set, the set positions as int64)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    padded = torch.zeros(-(-bits // 32) * 32, dtype=torch.bool, device=dev)
    padded[:bits] = torch.rand(bits, device=dev, generator=g) < 0.5
    padded[0] = padded[bits - 1] = True
    return sweep.mask_words(padded), torch.nonzero(padded).reshape(-1)


def time_column(ty, c, reps):
    lib = fl.load()
    T, n = c.T, c.n
    in_fn = getattr(lib, f"fl_{ty}_unfor_compare_in_widths")
    range_fn = getattr(lib, f"fl_{ty}_unfor_compare_range_widths")
    mask, mask_a = (torch.empty(n * 32, dtype=torch.int32, device=dev) for _ in range(2))
    x64 = sweep.rnd(n * 8, 5).view(torch.int64)
    lo = 1 << (T - 2)
    print(f"# {ty}: n = {n} blocks, packed {c.pbytes / 1e9:.3f} GB, {reps} launches each, round-robin", flush=True)
    for name, bits, straddling in window_rows(T):
        words, js = member_bitmap(bits, 100 + bits)
        members = sweep.as_type(js + lo, ty).view(SIGNED[ty])                # the values (b) looks for, as torch compares them
        r64 = sweep.undecided_refs(lo + bits // 2, x64, c.widths)            # every block's range holds the window's middle
        if straddling < 1.0:
            every = round(1 / straddling)
            outside = torch.full_like(r64, lo + bits + 16)                   # [r, r + 2^W - 1] ends below lo + 2^T: outside the window
            r64 = torch.where(torch.arange(n, device=dev) % every == 0, r64, outside)
        refs = sweep.as_type(r64, ty)
        head = (c.widths.data_ptr(), c.offsets.data_ptr(), c.col.data_ptr(), c.pbytes, refs.data_ptr(), 1)

        def compare_in():
            return in_fn(*head, lo, bits, words.data_ptr(), 0, 0, None, n, mask.data_ptr(), None, None)

        def compare_range():
            return range_fn(*head, lo, lo + bits - 1, 0, None, n, mask_a.data_ptr(), None, None)

        def unpack_isin():
            fl.unfor_pack_widths(c.widths, c.offsets, c.col, refs, output=c.un, check=False)
            return torch.isin(c.un.view(SIGNED[ty]), members)

        # faster and different is not faster: the row's mask against (b)'s, before anything is timed
        assert compare_in() == 0 and compare_range() == 0
        want = sweep.mask_words(unpack_isin())
        assert torch.equal(mask, want), (ty, name)
        hits = int((want != 0).sum().item())
        del want
        variants = {UNDER_TEST: compare_in, "(a) unfor_compare_range_widths, the window's interval": compare_range,
                    "(b) unfor_pack_widths + torch.isin": unpack_isin}
        ms = sweep.round_robin(variants, reps)
        med = median(ms[UNDER_TEST])
        ka, kb = list(variants)[1:]
        tier = "registers" if bits <= 2048 else "memory"
        print(f"unfor_compare_in_widths {name:13s} {ty:4s} bits {bits:8d} ({tier:9s}) members {js.numel():7d} blocks straddling {straddling:4.2f} "
              f"mask words != 0 {hits / (n * 32):6.4f}  {show(ms[UNDER_TEST])}  {n / med / 1e6:8.3f} Gblocks/s", flush=True)
        for k in (ka, kb):
            print(sweep.format_yardstick_row(k, ty, n, ms[k], med, of_name=UNDER_TEST, pad=54), flush=True)
        med_a, med_b = median(ms[ka]), median(ms[kb])
        spread = max(ms[ka]) - min(ms[ka])
        line = f"    expectations: below (b): {'met' if med < med_b else 'NOT met'}"
        if straddling < 1.0:
            line += f"; within (a)'s spread of (a) ({med - med_a:+.4f} ms against {spread:.4f} ms): {'met' if med <= med_a + spread else 'NOT met'}"
        print(line + f"   [(a)'s spread {spread:.4f} ms = {spread / med_a:.3f} of its median]", flush=True)
        del words, js, members, refs, r64, variants
    del mask, mask_a, x64


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packed-gb", type=float, default=1.0, help="packed bytes of the column (beyond the 256-MiB Infinity Cache)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--types", default="", help="keep only these element types")
    args = ap.parse_args(argv)
    print(sweep.device_header(), flush=True)
    for ty in sweep.chosen_types(args):
        c = sweep.mixed_column(ty, 3.0 * args.packed_gb, refs=None, output=True)     # (its --gb budget counts 1.5 x the unpacked bytes)
        time_column(ty, c, args.reps)
        sweep.release_column(c)


if __name__ == "__main__":
    main()
