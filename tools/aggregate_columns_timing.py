#!/usr/bin/env python3
"""unfor_aggregate_columns_widths (COUNT / SUM / MIN / MAX per block of a * b between two mixed-width FoR-packed columns under a
selection mask) on one MI355X, next to the two things a caller could do instead, timed in the SAME run on the SAME buffers:

  (a) two unfor_aggregate_widths launches, one per column: the same packed bytes and the same mask read, twice the slots written;
  (b) the composition the call replaces: unfor_select_widths of both columns (mask_offsets given) plus the torch product and sum of
      the kept values; with no mask, unfor_pack_widths of both columns.

Two columns from the generator of `sweep.py --cases aggregate` (seeded-random widths 1 .. T - 1, random packed bytes, random
references), --packed-gb of packed bytes each.  Rows: mask=None, a 100 % mask, a random 1 % mask, an empty mask, and a pair of columns
whose widths are all 0 (answered from the references, no packed byte read).  Every figure is the median of --reps launches, one launch
of each variant per round (round-robin), with min .. max beside it; every row is timed in TWO passes, and the distance between a row's
two passes is the run-to-run spread its ratios are read against.  The kernels are launched through the C ABI (no allocation, no
reduction, no flag read-back inside the timed region).  Before it is timed, every row's SUM is checked against yardstick (b)'s.

    python tools/aggregate_columns_timing.py [--packed-gb 0.5] [--reps 7] [--types u32,u64] > profiles/aggregate_columns_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from sweep import SIGNED, TDT, dev, fl, median, show  # noqa: E402

CHUNK = 1 << 26                         # elements per torch product: bounds the composition's temporaries at a few GB


def zero_extended(t, ty):
    v = t.view(SIGNED[ty]).to(torch.int64)
    return v if ty == "u64" else v & ((1 << (8 * sweep.ESZ[ty])) - 1)


def product_sum(ua, ub, ty, kept):
    """the torch half of yardstick (b): sum of zext(a) * zext(b) over the first `kept` elements, wrapping int64"""
    total = torch.zeros((), dtype=torch.int64, device=dev)
    for i in range(0, kept, CHUNK):
        total += (zero_extended(ua[i:min(i + CHUNK, kept)], ty) * zero_extended(ub[i:min(i + CHUNK, kept)], ty)).sum()
    return total


def column_pair(ty, packed_gb, zero_width):
    """two columns of the aggregate case's generator (its --gb budget counts 1.5 x the unpacked bytes: packed bytes are a third of it);
    zero_width: the same block count with every width 0 and no packed bytes"""
    a, b = (sweep.mixed_column(ty, 3.0 * packed_gb, width_seed=1000 * i, data_seed=10 * i, refs="full", output=False) for i in (0, 1))
    b.refs = sweep.as_type(sweep.rnd(b.n * 8, 12).view(torch.int64), ty)        # its own references
    if zero_width:
        for c in (a, b):
            c.widths = torch.zeros_like(c.widths)
            c.offsets, _ = fl.widths_to_offsets(ty, c.widths)
            c.col, c.pbytes = torch.empty(0, dtype=TDT[ty], device=dev), 0
    return a, b


def time_pair(ty, a, b, rows, reps):
    lib = fl.load()
    n = a.n
    col_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_columns_widths")
    agg_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_widths")
    slots, slots2 = (torch.empty((n, 4), dtype=torch.int64, device=dev) for _ in range(2))
    ua, ub = (torch.empty(n * 1024, dtype=TDT[ty], device=dev) for _ in range(2))
    print(f"# {ty}: n = {n} blocks per column, packed {a.pbytes / 1e9:.3f} + {b.pbytes / 1e9:.3f} GB, {reps} launches each, round-robin, two passes", flush=True)
    for name, mask in rows(n):
        mp = mask.data_ptr() if mask is not None else None
        if mask is not None:
            oo, tot = fl.mask_offsets(mask)
            kept = int(tot.item())
        else:
            oo = tot = None
            kept = n * 1024

        def columns():
            return col_fn(0, a.widths.data_ptr(), a.offsets.data_ptr(), a.col.data_ptr(), a.pbytes, a.refs.data_ptr(), 1,
                          b.widths.data_ptr(), b.offsets.data_ptr(), b.col.data_ptr(), b.pbytes, b.refs.data_ptr(), 1, mp, n, slots.data_ptr(), None, None)

        def two_aggregates():
            agg_fn(a.widths.data_ptr(), a.offsets.data_ptr(), a.col.data_ptr(), a.pbytes, a.refs.data_ptr(), 1, mp, n, slots.data_ptr(), None, None)
            return agg_fn(b.widths.data_ptr(), b.offsets.data_ptr(), b.col.data_ptr(), b.pbytes, b.refs.data_ptr(), 1, mp, n, slots2.data_ptr(), None, None)

        def composition():
            if mask is None:
                fl.unfor_pack_widths(a.widths, a.offsets, a.col, a.refs, output=ua, check=False)
                fl.unfor_pack_widths(b.widths, b.offsets, b.col, b.refs, output=ub, check=False)
            else:
                fl.unfor_select_widths(a.widths, a.offsets, a.col, a.refs, mask, out_offsets=oo, total=tot, output=ua, check=False)
                fl.unfor_select_widths(b.widths, b.offsets, b.col, b.refs, mask, out_offsets=oo, total=tot, output=ub, check=False)
            return product_sum(ua, ub, ty, kept)

        # faster and different is not faster: the row's SUM against the composition's, before anything is timed
        assert columns() == 0
        got = fl.aggregate_reduce(slots)
        want = composition()
        assert int(got[0].item()) == kept and int(got[1].item()) == int(want.item()), (ty, name, got.tolist(), int(want.item()))
        variants = {"aggregate_columns": columns, "(a) 2 x unfor_aggregate_widths": two_aggregates,
                    "(b) " + ("2 x unfor_pack_widths" if mask is None else "2 x unfor_select_widths") + " + torch product, sum": composition}
        for p in (1, 2):
            ms = sweep.round_robin(variants, reps)
            med = median(ms["aggregate_columns"])
            print(f"unfor_aggregate_columns_widths '*' {name:13s} {ty:4s} pass {p} kept {kept / (n * 1024):7.4f}  {show(ms['aggregate_columns'])}  "
                  f"{n / med / 1e6:8.3f} Gblock pairs/s", flush=True)
            for k in list(variants)[1:]:
                print(sweep.format_yardstick_row(k, ty, n, ms[k], med, of_name="aggregate_columns", pad=54), flush=True)
        del mask, oo, tot, variants
    del slots, slots2, ua, ub


def masked_rows(T):
    def rows(n):
        yield "mask=None", None
        yield "mask 100 %", sweep.random_mask(n, 1.0, 77 + T)
        yield "random 1 %", sweep.random_mask(n, 0.01, 77 + T)
        yield "empty mask", sweep.random_mask(n, 0.0, 77 + T)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packed-gb", type=float, default=0.5, help="packed bytes per column")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--types", default="", help="keep only these element types")
    args = ap.parse_args(argv)
    print(sweep.device_header(), flush=True)
    for ty in sweep.chosen_types(args):
        T = 8 * sweep.ESZ[ty]
        a, b = column_pair(ty, args.packed_gb, zero_width=False)
        time_pair(ty, a, b, masked_rows(T), args.reps)
        sweep.release_column(a)
        sweep.release_column(b)
        a, b = column_pair(ty, args.packed_gb, zero_width=True)
        time_pair(ty, a, b, lambda n: [("both widths 0", None)], args.reps)
        sweep.release_column(a)
        sweep.release_column(b)


if __name__ == "__main__":
    main()
