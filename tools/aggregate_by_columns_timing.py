#!/usr/bin/env python3
"""unfor_aggregate_by_columns_widths (COUNT / SUM / MIN / MAX per u8 key of a * b between two mixed-width FoR-packed columns under a
selection mask) on one MI355X, next to the things a caller could do instead, timed in the SAME run on the SAME buffers:

  (a) two unfor_aggregate_by_widths launches, one per value column, with the same key column and mask: the same value bytes read, the
      key column and the mask read twice, twice the LDS atomics;
  (b) the composition the call replaces: unfor_pack_widths of the three columns, the torch product of the kept rows, bincount and
      scatter_add_ per key -- timed at the 1 % mask and the empty mask only (at a full mask the torch scatter takes seconds per
      launch: DESIGN.md);
  (c) in the clustered-key rows, unfor_aggregate_columns_widths of the same two value columns: what the kernel does there, ungrouped.

Two value columns from the generator of `sweep.py --cases aggregate` (seeded-random widths 1 .. T - 1, random packed bytes, random
references), --packed-gb of packed bytes each, and a u8 key column beside them: clustered (every key block width 0, a random reference
per block), 4 uniform groups (key width 2), 256 uniform groups (key width 8).  Every key kind at mask=None and at a random 1 % mask, and
one empty-mask row.  Every figure is the median of --reps launches, one launch of each variant per round (round-robin), with min ..
max beside it; every row is timed in TWO passes, and the distance between a row's two passes is the run-to-run spread its ratios are
read against.  The kernels are launched through the C ABI (no allocation, no flag read-back inside the timed region).  Before it is
timed, every row's COUNT and SUM per group are checked against the composition's.

    python tools/aggregate_by_columns_timing.py [--packed-gb 0.5] [--reps 7] [--types u32,u64] > profiles/aggregate_by_columns_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from sweep import SIGNED, TDT, dev, fl, median, show  # noqa: E402

CHUNK = 1 << 25                         # rows per torch step: bounds the composition's temporaries at a few GB
KEY_KINDS = (("clustered", 0), ("4 groups", 2), ("256 groups", 8))


def zero_extended(t, ty):
    v = t.view(SIGNED[ty]).to(torch.int64)
    return v if ty == "u64" else v & ((1 << (8 * sweep.ESZ[ty])) - 1)


def key_column(n, kwidth):
    """n key blocks of one width: random packed bytes under reference 0, or -- width 0 -- a random reference per block"""
    k = sweep.SimpleNamespace(widths=torch.full((n,), kwidth, dtype=torch.uint8, device=dev))
    k.offsets, total = fl.widths_to_offsets("u8", k.widths)
    k.pbytes = int(total.item())
    k.col = sweep.rnd(max(k.pbytes, 16), 4).view(torch.uint8)[:k.pbytes]
    k.refs = sweep.rnd((n + 7) // 8 * 8, 3).view(torch.uint8)[:n].contiguous() if kwidth == 0 else torch.zeros(1, dtype=torch.uint8, device=dev)
    return k


def lead(c):
    """a column's six leading C arguments"""
    return (c.widths.data_ptr(), c.offsets.data_ptr(), c.col.data_ptr(), c.pbytes, c.refs.data_ptr(), 0 if c.refs.numel() == 1 else 1)


def time_type(ty, a, b, reps):
    lib = fl.load()
    n = a.n
    T = 8 * sweep.ESZ[ty]
    new_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_by_columns_widths")
    by_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_by_widths")
    col_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_columns_widths")
    result, result2 = (torch.empty((256, 4), dtype=torch.int64, device=dev) for _ in range(2))
    slots = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ua, ub = (torch.empty(n * 1024, dtype=TDT[ty], device=dev) for _ in range(2))
    uk = torch.empty(n * 1024, dtype=torch.uint8, device=dev)
    print(f"# {ty}: n = {n} blocks per column, packed {a.pbytes / 1e9:.3f} + {b.pbytes / 1e9:.3f} GB, {reps} launches each, round-robin, two passes", flush=True)
    g = torch.Generator(device=dev)
    g.manual_seed(77 + T)
    sparse = torch.rand(n * 1024, device=dev, generator=g) < 0.01
    rows = [(kname, kwidth, mname, bits) for kname, kwidth in KEY_KINDS for mname, bits in (("mask=None", None), ("random 1 %", sparse))]
    rows.append(("256 groups", 8, "empty mask", torch.zeros(n * 1024, dtype=torch.bool, device=dev)))
    for kname, kwidth, mname, bits in rows:
        k = key_column(n, kwidth)
        mask = None if bits is None else sweep.mask_words(bits)
        mp = None if mask is None else mask.data_ptr()

        def fused():
            return new_fn(0, *lead(a), *lead(b), *lead(k), mp, n, result.data_ptr(), None, None)

        def two_launches():
            by_fn(*lead(a), *lead(k), mp, n, result.data_ptr(), None, None)
            return by_fn(*lead(b), *lead(k), mp, n, result2.data_ptr(), None, None)

        def ungrouped():
            return col_fn(0, *lead(a), *lead(b), mp, n, slots.data_ptr(), None, None)

        def composition():
            fl.unfor_pack_widths(a.widths, a.offsets, a.col, a.refs, output=ua, check=False)
            fl.unfor_pack_widths(b.widths, b.offsets, b.col, b.refs, output=ub, check=False)
            fl.unfor_pack_widths(k.widths, k.offsets, k.col, k.refs, output=uk, check=False)
            count = torch.zeros(256, dtype=torch.int64, device=dev)
            total = torch.zeros(256, dtype=torch.int64, device=dev)
            for i in range(0, n * 1024, CHUNK):
                j = min(i + CHUNK, n * 1024)
                x, key = zero_extended(ua[i:j], ty) * zero_extended(ub[i:j], ty), uk[i:j].to(torch.int64)
                if bits is not None:
                    x, key = x[bits[i:j]], key[bits[i:j]]
                count += torch.bincount(key, minlength=256)
                total.scatter_add_(0, key, x)
            return count, total

        # faster and different is not faster: the row's COUNT and SUM per group against the composition's, before anything is timed
        assert fused() == 0
        count, total = composition()
        assert torch.equal(result[:, 0], count) and torch.equal(result[:, 1], total), (ty, kname, mname)
        variants = {"aggregate_by_columns": fused, "(a) 2 x unfor_aggregate_by_widths": two_launches}
        if kwidth == 0:
            variants["(c) unfor_aggregate_columns_widths (ungrouped)"] = ungrouped
        if bits is not None:
            variants["(b) 3 x unfor_pack_widths + torch product, bincount, scatter_add_"] = composition
        for p in (1, 2):
            ms = sweep.round_robin(variants, reps)
            med = median(ms["aggregate_by_columns"])
            print(f"unfor_aggregate_by_columns_widths '*' keys {kname:10s} {mname:10s} {ty:4s} pass {p}  {show(ms['aggregate_by_columns'])}  "
                  f"{n / med / 1e6:8.3f} Gblock triples/s", flush=True)
            for v in list(variants)[1:]:
                print(sweep.format_yardstick_row(v, ty, n, ms[v], med, of_name="aggregate_by_columns", pad=66), flush=True)
        del k, mask, variants
    del result, result2, slots, ua, ub, uk, sparse, rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packed-gb", type=float, default=0.5, help="packed bytes per value column")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--types", default="", help="keep only these element types")
    args = ap.parse_args(argv)
    print(sweep.device_header(), flush=True)
    for ty in sweep.chosen_types(args):
        a, b = (sweep.mixed_column(ty, 3.0 * args.packed_gb, width_seed=1000 * i, data_seed=10 * i, refs="full", output=False) for i in (0, 1))
        b.refs = sweep.as_type(sweep.rnd(b.n * 8, 12).view(torch.int64), ty)        # its own references
        time_type(ty, a, b, args.reps)
        sweep.release_column(a)
        sweep.release_column(b)


if __name__ == "__main__":
    main()
