#!/usr/bin/env python3
"""unfor_lookup_widths (a dimension attribute fetched through a mixed-width FoR-packed key column inside a dense window, written in
full-width packed order: the probe side of a payload join) on one MI355X, next to two baselines timed in the SAME run on the SAME
buffers:

  (a) unfor_compare_in_widths on the same column, window and bitmap: the same key bytes read, the same blocks decided from their
      metadata, one bit looked up per element and NO payload written -- the floor;
  (b) what a caller does without it: unfor_pack_widths, then torch index arithmetic, a gather from the table and torch.where.

Rows, on the generator's column of `sweep.py --cases mixed` (seeded-random widths 1 .. T - 1, random packed bytes, --packed-gb of them),
every block's key range straddling the window's middle:
  * uint8 tables of 25, 2556 and 8192 slots (the LDS tier) and of 8193, 2^20 and 2^24 slots (the memory tier);
  * tables of the key's own type of 8192 / sizeof(T) slots (LDS) and 2^20 slots (memory);
  * a uint8 table of 2^20 slots with `present` half set;
  * a uint8 table of 2556 slots with 99 % of the blocks outside the window, and the same table under a random 1 % mask.
Every figure is the median of --reps launches, one launch of each variant per round (round-robin), min .. max beside it.  The kernels
are launched through the C ABI (no allocation, no flag read-back inside the timed region).  Before it is timed, every row's column,
hit mask and counters are checked bit for bit against (b)'s (a column of the key's own type through BitPacking.unpack at width T).

Per row the tool prints its ratios to (a) and to (b) and whether it is below (b).  These are reports, not gates: nothing is promised.

    python tools/lookup_timing.py [--packed-gb 1.0] [--reps 7] [--types u32] > profiles/lookup_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from sweep import SIGNED, TDT, dev, fl, median, show  # noqa: E402

UNDER_TEST = "lookup"
LDS_BYTES = 8192                        # fastlanes_amd/csrc/fl_lookup_map.hpp: LOOKUP_LDS_BYTES
CHUNK = 1 << 26                         # rows per torch step: bounds the composition's temporaries at a few GB
LABEL_A = "(a) unfor_compare_in_widths, the same window and bitmap"
LABEL_B = "(b) unfor_pack_widths + torch indexing + torch.where"


def torch_lookup(keys, ty, lo, table, present_bits, kept_bits, missing, out, hit):
    """(b): the looked-up values of the decoded `keys` in row order into `out`, the hits into `hit` (bool); returns (hits, misses).
    table, missing and out are the payload's same-width dtype torch indexes and selects (sweep.SIGNED)"""
    T = 8 * sweep.ESZ[ty]
    n_slots = table.numel()
    lo_s = lo - (1 << 64) if lo >= 1 << 63 else lo
    hits = kept = 0
    for i in range(0, keys.numel(), CHUNK):
        j = keys[i:i + CHUNK].view(SIGNED[ty]).to(torch.int64) - lo_s       # (wraps mod 2^64 for u64)
        if T < 64:
            j &= (1 << T) - 1
        inside = (j >= 0) & (j < n_slots)
        j = torch.where(inside, j, torch.zeros_like(j))
        if present_bits is not None:
            inside &= present_bits[j]
        if kept_bits is not None:
            kept += int(kept_bits[i:i + CHUNK].sum().item())
            inside &= kept_bits[i:i + CHUNK]
        else:
            kept += j.numel()
        out[i:i + CHUNK] = torch.where(inside, table[j], missing)
        hit[i:i + CHUNK] = inside
        hits += int(inside.sum().item())
    return hits, kept - hits


def time_row(ty, uty, name, k, n, lo, n_slots, half_present, mask_bits, straddling, reps, un):
    """one row: k = the column (widths, offsets, col, pbytes, refs), the window, the payload type, the mask's bits (None: every row)"""
    lib = fl.load()
    T = 8 * sweep.ESZ[ty]
    look_fn = getattr(lib, f"fl_{ty}_unfor_lookup{'' if uty == ty else '_u8'}_widths")
    in_fn = getattr(lib, f"fl_{ty}_unfor_compare_in_widths")
    head = (k.widths.data_ptr(), k.offsets.data_ptr(), k.col.data_ptr(), k.pbytes, k.refs.data_ptr(), 1)
    g = torch.Generator(device=dev)
    g.manual_seed(77 + n_slots % 1000)
    table = torch.randint(1, 255, (n_slots,), dtype=torch.int64, device=dev, generator=g).to(TDT[uty] if uty == "u8" else torch.int64)
    if uty != "u8":
        table = sweep.as_type(table * 2654435761, uty)
    table_s = table.view(SIGNED[uty])
    missing = torch.zeros((), dtype=table_s.dtype, device=dev)
    present_bits = (torch.rand(n_slots, device=dev, generator=g) < 0.5) if half_present else None
    nw = (n_slots + 31) // 32
    padded = torch.ones(nw * 32, dtype=torch.bool, device=dev)
    if present_bits is not None:
        padded[:n_slots] = present_bits
    words = sweep.mask_words(padded)                                        # (a) always takes a bitmap: all ones without `present`
    pp = words.data_ptr() if present_bits is not None else None
    out = torch.empty(n * 1024, dtype=table.dtype, device=dev)
    hit = torch.empty(n * 32, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    out_mask = torch.empty(n * 32, dtype=torch.int32, device=dev)
    want_out = torch.empty(n * 1024, dtype=table.dtype, device=dev)
    want_hit = torch.empty(n * 1024, dtype=torch.bool, device=dev)
    mask = None if mask_bits is None else sweep.mask_words(mask_bits)
    mp = None if mask is None else mask.data_ptr()

    def lookup():
        return look_fn(*head, mp, n, lo, n_slots, table.data_ptr(), pp, 0, out.data_ptr(), hit.data_ptr(), stats.data_ptr(), None, None)

    def compare_in():                                                       # NEW without a mask, AND through the same mask with one
        return in_fn(*head, lo, n_slots, words.data_ptr(), 0, 0 if mask is None else 1, mp, n, out_mask.data_ptr(), None, None)

    def composition():
        fl.unfor_pack_widths(k.widths, k.offsets, k.col, k.refs, output=un, check=False)
        return torch_lookup(un, ty, lo, table_s, present_bits, mask_bits, missing, want_out.view(SIGNED[uty]), want_hit)

    tier = "LDS" if n_slots * sweep.ESZ[uty] <= LDS_BYTES else "memory"
    # faster and different is not faster: column, hit mask and counters against (b)'s, before anything is timed
    want_hits, want_misses = composition()
    assert lookup() == 0 and compare_in() == 0
    rows = out if uty == "u8" else fl.BitPacking.unpack(T, out)
    assert torch.equal(rows.view(torch.uint8), want_out.view(torch.uint8)), (ty, uty, name, "column")
    assert torch.equal(hit, sweep.mask_words(want_hit)) and torch.equal(hit, out_mask), (ty, uty, name, "hit mask")
    assert stats.tolist() == [want_hits, want_misses], (ty, uty, name, stats.tolist(), want_hits, want_misses)
    del rows
    timed = {UNDER_TEST: lookup, LABEL_A: compare_in, LABEL_B: composition}
    ms = sweep.round_robin(timed, reps)
    med = median(ms[UNDER_TEST])
    print(f"unfor_lookup_widths {name:22s} {ty:4s} payload {uty:4s} slots {n_slots:9d} ({tier:6s}) present {'half' if half_present else 'none':4s} "
          f"mask {'none' if mask is None else 'random 1 %':10s} blocks straddling {straddling:4.2f} hits {want_hits:11d} misses {want_misses:11d} "
          f"bit-for-bit ok  {show(ms[UNDER_TEST])}  {n / med / 1e6:8.3f} Gblocks/s", flush=True)
    for label in (LABEL_A, LABEL_B):
        print(sweep.format_yardstick_row(label, ty, n, ms[label], med, of_name=UNDER_TEST, pad=56), flush=True)
    med_a, med_b = median(ms[LABEL_A]), median(ms[LABEL_B])
    print(f"    ratios: x{med / med_a:.3f} of (a), x{med / med_b:.3f} of (b); below (b): {'met' if med < med_b else 'NOT met'}", flush=True)


def rows_of(ty):
    """(name, payload type, n_slots, present half set, share of the blocks that straddle the window, 1 % mask)"""
    top = min(1 << (8 * sweep.ESZ[ty]), 1 << 32)
    own = LDS_BYTES // sweep.ESZ[ty]
    rows = [(f"u8 table {s}", "u8", s, False, 1.0, False) for s in (25, 2556, 8192, 8193, 1 << 20, 1 << 24)]
    rows += [(f"{ty} table {own}", ty, own, False, 1.0, False), (f"{ty} table {1 << 20}", ty, 1 << 20, False, 1.0, False),
             ("present half set", "u8", 1 << 20, True, 1.0, False), ("99 % outside", "u8", 2556, False, 0.01, False),
             ("1 % mask", "u8", 2556, False, 1.0, True)]
    return [r for r in rows if r[2] <= top and (r[1] != "u8" or ty != "u8" or r[2] <= 256)]


def time_column(ty, c, reps):
    T, n = c.T, c.n
    x64 = sweep.rnd(n * 8, 5).view(torch.int64)
    lo = 1 << (T - 2)
    print(f"# {ty}: n = {n} blocks, packed {c.pbytes / 1e9:.3f} GB, {reps} launches each, round-robin", flush=True)

    def straddling_column(slots, share):
        r64 = sweep.undecided_refs(lo + slots // 2, x64, c.widths)          # every block's range holds the window's middle
        if share < 1.0:
            outside = torch.full_like(r64, lo + slots + 16)                 # [r, r + 2^W - 1] ends below lo + 2^T: outside the window
            r64 = torch.where(torch.arange(n, device=dev) % round(1 / share) == 0, r64, outside)
        return sweep.SimpleNamespace(widths=c.widths, offsets=c.offsets, col=c.col, pbytes=c.pbytes, refs=sweep.as_type(r64, ty))

    g = torch.Generator(device=dev)
    g.manual_seed(91 + T)
    for name, uty, slots, half, share, masked in rows_of(ty):
        sparse = (torch.rand(n * 1024, device=dev, generator=g) < 0.01) if masked else None
        time_row(ty, uty, name, straddling_column(slots, share), n, lo, slots, half, sparse, share, reps, c.un)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packed-gb", type=float, default=1.0, help="packed bytes of the column (beyond the 256-MiB Infinity Cache)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--types", default="u32", help="keep only these element types")
    args = ap.parse_args(argv)
    print(sweep.device_header(), flush=True)
    for ty in sweep.chosen_types(args):
        c = sweep.mixed_column(ty, 3.0 * args.packed_gb, refs=None, output=True)     # (its --gb budget counts 1.5 x the unpacked bytes)
        time_column(ty, c, args.reps)
        sweep.release_column(c)


if __name__ == "__main__":
    main()
