#!/usr/bin/env python3
"""unfor_aggregate_by_lookup_widths (COUNT / SUM / MIN / MAX of a mixed-width FoR-packed value column grouped by a uint8 attribute
fetched through a mixed-width key column of the same type inside a dense window: unfor_lookup_u8 and unfor_aggregate_by in one pass,
no per-row output) on one MI355X, next to two baselines timed in the SAME run on the SAME buffers:

  (a) the chain it replaces: unfor_lookup_u8_widths into a temporary code column with its hit mask, then unfor_aggregate_by_widths
      with that temporary as the full-width u8 key column and mask = the hits (two launches and the init);
  (b) unfor_aggregate_columns_widths (a + b) over the same two columns under the same mask: the same packed bytes read with no
      gather, no table and no group table -- the floor.

Rows, on the generator's column of `sweep.py --cases mixed` as the key column (seeded-random widths 1 .. T - 1, random packed bytes,
--packed-gb of them), every block's key range straddling the window's middle, and a second column of the same generator (other seeds,
the same block count) as the value column:
  * tables of 25, 2556, 8193, 2^20 and 2^24 slots;
  * a table of 2^20 slots with `present` half set;
  * a table of 2556 slots with 99 % of the blocks outside the window, and the same table under a random 1 % mask.
Every figure is the median of --reps launches, one launch of each variant per round (round-robin), min .. max beside it.  The kernels
are launched through the C ABI (no allocation, no flag read-back inside the timed region).  Before it is timed, every row's result and
counters are checked bit for bit against (a)'s.

The expectation, stated before the run: the fused call is at or below (a) in every row; what it can save is bounded by the code
column's write and re-read (2 bytes per row), the hit mask's (1/4 byte per row) and the second pass over the mask.  Per row the tool
prints its ratios to (a) and to (b) and whether the expectation is met.  These are reports, not gates: nothing is tuned toward them.

    python tools/aggregate_by_lookup_timing.py [--packed-gb 1.0] [--reps 7] [--types u32] > profiles/aggregate_by_lookup_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from sweep import dev, fl, median, show  # noqa: E402

UNDER_TEST = "fused"
LABEL_A = "(a) unfor_lookup_u8_widths + unfor_aggregate_by_widths(mask=hit)"
LABEL_B = "(b) unfor_aggregate_columns_widths, the same columns and mask"


def time_row(ty, name, k, v, n, lo, n_slots, half_present, mask_bits, straddling, reps):
    """one row: k / v = the key / value column (widths, offsets, col, pbytes, refs), the window, the mask's bits (None: every row)"""
    lib = fl.load()
    fused_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_by_lookup_widths")
    look_fn = getattr(lib, f"fl_{ty}_unfor_lookup_u8_widths")
    by_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_by_widths")
    cols_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_columns_widths")
    khead = (k.widths.data_ptr(), k.offsets.data_ptr(), k.col.data_ptr(), k.pbytes, k.refs.data_ptr(), 1)
    vhead = (v.widths.data_ptr(), v.offsets.data_ptr(), v.col.data_ptr(), v.pbytes, v.refs.data_ptr(), 1)
    g = torch.Generator(device=dev)
    g.manual_seed(77 + n_slots % 1000)
    table = torch.randint(0, 256, (n_slots,), dtype=torch.int64, device=dev, generator=g).to(torch.uint8)
    pp, words = None, None
    if half_present:
        padded = torch.ones((n_slots + 31) // 32 * 32, dtype=torch.bool, device=dev)
        padded[:n_slots] = torch.rand(n_slots, device=dev, generator=g) < 0.5
        words = sweep.mask_words(padded)
        pp = words.data_ptr()
    mask = None if mask_bits is None else sweep.mask_words(mask_bits)
    mp = None if mask is None else mask.data_ptr()
    result, chain = (torch.empty((256, 4), dtype=torch.int64, device=dev) for _ in range(2))
    stats, cstats = (torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(2))
    codes = torch.empty(n * 1024, dtype=torch.uint8, device=dev)           # (a)'s temporaries, allocated once outside the timed region
    hit = torch.empty(n * 32, dtype=torch.int32, device=dev)
    w8, o8, r8 = fl.full_width_column("u8", n, dev)
    block_aggs = torch.empty((n, 4), dtype=torch.int64, device=dev)

    def fused():
        return fused_fn(*vhead, *khead, mp, n, lo, n_slots, table.data_ptr(), pp, result.data_ptr(), stats.data_ptr(), None, None)

    def the_chain():
        rc = look_fn(*khead, mp, n, lo, n_slots, table.data_ptr(), pp, 0, codes.data_ptr(), hit.data_ptr(), cstats.data_ptr(), None, None)
        return rc or by_fn(*vhead, w8.data_ptr(), o8.data_ptr(), codes.data_ptr(), n * 1024, r8.data_ptr(), 0, hit.data_ptr(), n, chain.data_ptr(), None, None)

    def floor():
        return cols_fn(1, *vhead, *khead, mp, n, block_aggs.data_ptr(), None, None)

    # faster and different is not faster: result and counters against (a)'s, before anything is timed
    assert fused() == 0 and the_chain() == 0 and floor() == 0
    torch.cuda.synchronize()
    assert torch.equal(result, chain), (ty, name, "result")
    assert stats.tolist() == cstats.tolist(), (ty, name, stats.tolist(), cstats.tolist())
    hits, misses = stats.tolist()
    groups = int((result[:, 0] != 0).sum().item())
    ms = sweep.round_robin({UNDER_TEST: fused, LABEL_A: the_chain, LABEL_B: floor}, reps)
    med = median(ms[UNDER_TEST])
    print(f"unfor_aggregate_by_lookup_widths {name:18s} {ty:4s} slots {n_slots:9d} present {'half' if half_present else 'none':4s} "
          f"mask {'none' if mask is None else 'random 1 %':10s} blocks straddling {straddling:4.2f} hits {hits:11d} misses {misses:11d} groups {groups:3d} "
          f"bit-for-bit ok  {show(ms[UNDER_TEST])}  {n / med / 1e6:8.3f} Gblocks/s", flush=True)
    for label in (LABEL_A, LABEL_B):
        print(sweep.format_yardstick_row(label, ty, n, ms[label], med, of_name=UNDER_TEST, pad=66), flush=True)
    med_a, med_b = median(ms[LABEL_A]), median(ms[LABEL_B])
    print(f"    ratios: x{med / med_a:.3f} of (a), x{med / med_b:.3f} of (b); at or below (a): {'met' if med <= med_a else 'NOT met'}", flush=True)


def rows_of(ty):
    """(name, n_slots, present half set, share of the blocks that straddle the window, 1 % mask)"""
    top = min(1 << (8 * sweep.ESZ[ty]), 1 << 32)
    rows = [(f"table {s}", s, False, 1.0, False) for s in (25, 2556, 8193, 1 << 20, 1 << 24)]
    rows += [("present half set", 1 << 20, True, 1.0, False), ("99 % outside", 2556, False, 0.01, False), ("1 % mask", 2556, False, 1.0, True)]
    return [r for r in rows if r[1] <= top]


def time_columns(ty, c, v, reps):
    T, n = c.T, c.n
    assert v.n == n
    x64 = sweep.rnd(n * 8, 5).view(torch.int64)
    lo = 1 << (T - 2)
    print(f"# {ty}: n = {n} blocks, packed keys {c.pbytes / 1e9:.3f} GB, packed values {v.pbytes / 1e9:.3f} GB, {reps} launches each, round-robin",
          flush=True)

    def straddling_column(slots, share):
        r64 = sweep.undecided_refs(lo + slots // 2, x64, c.widths)          # every block's range holds the window's middle
        if share < 1.0:
            outside = torch.full_like(r64, lo + slots + 16)                 # [r, r + 2^W - 1] ends below lo + 2^T: outside the window
            r64 = torch.where(torch.arange(n, device=dev) % round(1 / share) == 0, r64, outside)
        return sweep.SimpleNamespace(widths=c.widths, offsets=c.offsets, col=c.col, pbytes=c.pbytes, refs=sweep.as_type(r64, ty))

    g = torch.Generator(device=dev)
    g.manual_seed(91 + T)
    for name, slots, half, share, masked in rows_of(ty):
        sparse = (torch.rand(n * 1024, device=dev, generator=g) < 0.01) if masked else None
        time_row(ty, name, straddling_column(slots, share), v, n, lo, slots, half, sparse, share, reps)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packed-gb", type=float, default=1.0, help="packed bytes of the key column (beyond the 256-MiB Infinity Cache)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--types", default="u32", help="keep only these element types")
    args = ap.parse_args(argv)
    print(sweep.device_header(), flush=True)
    for ty in sweep.chosen_types(args):
        c = sweep.mixed_column(ty, 3.0 * args.packed_gb, refs=None, output=False)    # (its --gb budget counts 1.5 x the unpacked bytes)
        v = sweep.mixed_column(ty, 3.0 * args.packed_gb, width_seed=1, data_seed=1, refs="full", output=False)
        time_columns(ty, c, v, args.reps)
        sweep.release_column(c)
        sweep.release_column(v)


if __name__ == "__main__":
    main()
