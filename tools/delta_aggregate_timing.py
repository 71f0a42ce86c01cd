#!/usr/bin/env python3
"""undelta_aggregate_widths (COUNT / SUM / MIN / MAX per block straight from a mixed-width DELTA-packed column under a mask: the chains are
aggregated where they are decoded, no value is untransposed, an empty-mask or width-0 block reads no packed byte) on one MI355X, next
to three yardsticks timed in the SAME run on the SAME buffers:

  (b) today's only path: undelta_pack_untranspose_widths into a full-width buffer (4 KiB per u32 block written), then
      unfor_aggregate_widths over that buffer as a full-width column (the 4 KiB read back);
  (c) unfor_aggregate_widths on a FoR column of the same bytes and widths (random references): the same routes with no chain scan and
      no bases;
  (d) a bare stream of the bytes the row must read, one wavefront per block, 32 bytes written per block: the mean packed bytes + the
      128 bytes of bases where the blocks are decoded (the mask's 128 bytes are not streamed), the 128 bytes of mask + the 128 of bases
      where nearly every block's mask is empty, the 128 bytes of bases for the width-0 column.

Rows:
  * no mask       the generator's column of `sweep.py --cases mixed` (seeded-random widths 1 .. T - 1, random packed bytes, --packed-gb
                  of them) under random bases, mask=None: every block EACH;
  * mask 50 %     the same column under a random mask of half density: every block EACH;
  * chained 1 %   the same column, 1 % of the blocks left open by a chained mask: IDENTITY everywhere else;
  * sorted 1 %    an ascending column of the same block count (steps 0 .. 7, Delta-coded by the library's encoder) under the mask
                  undelta_compare_range_widths gives for an interval that holds 1 % of the rows;
  * width 0       a column of width-0 blocks under the same bases, mask=None: every block BASES.
Every figure is the median of --reps launches, one launch of each variant per round (round-robin), min .. max beside it.  The kernels are
launched through the C ABI (no allocation, no flag read-back inside the timed region).  Before it is timed, every row's slots are
checked bit for bit against (b)'s ((b)'s mask is given in its full-width column's row order).

The expectation, stated before the run: (a) is at or below (b) in every row ((b) moves at least 8 KiB per u32 block more).  The ratios
to (c) and (d) are reported, not gated.  Per row the tool prints the ratios and whether "at or below (b)" is met.  These are reports, not
gates: nothing is tuned toward them.

    python tools/delta_aggregate_timing.py [--packed-gb 1.0] [--reps 7] [--types u32] > profiles/delta_aggregate_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from delta_compare_range_timing import in_full_width_order, sorted_column  # noqa: E402
from sweep import dev, fl, median, show  # noqa: E402

UNDER_TEST = "(a)"
LABEL_B = "(b) undelta_pack_untranspose_widths + unfor_aggregate_widths on the materialised column"
LABEL_C = "(c) unfor_aggregate_widths, a FoR column of the same bytes and widths"


def routes_of(widths, mask):
    """how many blocks take each route, from the definition (no block of these columns fails a device check)"""
    n = widths.numel()
    empty = torch.zeros(n, dtype=torch.bool, device=dev) if mask is None else (mask.view(-1, 32) == 0).all(dim=1)
    bases = ~empty & (widths == 0)
    return f"routes skip {0:8d} identity {int(empty.sum().item()):8d} bases {int(bases.sum().item()):8d} each {int((~empty & ~bases).sum().item()):8d}"


def time_row(ty, name, d, refs, mask, stream_of, reps):
    """one row: d = the Delta column (widths, offsets, col, pbytes, bases, un, n), refs = the references of yardstick (c), stream_of =
    what yardstick (d) streams beside the bases ("packed", "mask" or nothing)"""
    lib = fl.load()
    T = sweep.ESZ[ty] * 8
    n = d.n
    agg_fn = getattr(lib, f"fl_{ty}_undelta_aggregate_widths")
    decode_fn = getattr(lib, f"fl_{ty}_undelta_pack_untranspose_widths")
    for_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_widths")
    mp = None if mask is None else mask.data_ptr()
    moved = None if mask is None else in_full_width_order(mask, T)          # (b) reads the buffer as a full-width column: its row order
    mp_b = None if moved is None else moved.data_ptr()
    fw, fo, fr = fl.full_width_column(ty, n, dev)
    slots_a, slots_b, slots_c, slots_d = (torch.empty((n, 4), dtype=torch.int64, device=dev) for _ in range(4))
    head = (d.widths.data_ptr(), d.offsets.data_ptr(), d.col.data_ptr(), d.pbytes, d.bases.data_ptr())
    if stream_of == "packed":
        in_ptr, iu = d.col.data_ptr(), min(8192, d.pbytes // n // 16 * 16)
    elif stream_of == "mask":
        in_ptr, iu = mask.data_ptr(), 128
    else:
        in_ptr, iu = None, 0
    label_d = f"(d) bare stream of {iu} + 128 bytes read and 32 written per block"

    def under_test():
        return agg_fn(*head, mp, n, slots_a.data_ptr(), None, None)

    def two_steps():
        rc = decode_fn(*head, d.un.data_ptr(), n, None, None)
        return rc or for_fn(fw.data_ptr(), fo.data_ptr(), d.un.data_ptr(), n * 128 * T, fr.data_ptr(), 0, mp_b, n, slots_b.data_ptr(), None, None)

    def for_column():
        return for_fn(d.widths.data_ptr(), d.offsets.data_ptr(), d.col.data_ptr(), d.pbytes, refs.data_ptr(), 1, mp, n, slots_c.data_ptr(), None, None)

    def bare():
        return lib.fl_internal_bare_stream(in_ptr, iu, d.bases.data_ptr(), 128, slots_d.data_ptr(), 32, n, 1, 8 if T <= 16 else 6, 31, None)

    # faster and different is not faster: the slots against the two-step path's, bit for bit, before anything is timed
    assert under_test() == 0 and two_steps() == 0 and for_column() == 0 and bare() == 0
    torch.cuda.synchronize()
    assert torch.equal(slots_a, slots_b), (ty, name, "the slots differ from the two-step path's")
    kept = int(slots_a[:, 0].sum().item())
    ms = sweep.round_robin({UNDER_TEST: under_test, LABEL_B: two_steps, LABEL_C: for_column, label_d: bare}, reps)
    med = median(ms[UNDER_TEST])
    print(f"undelta_aggregate_widths {name:12s} {ty:4s} packed {d.pbytes / 1e9:6.3f} GB  kept {kept / (n * 1024):8.5f}  "
          f"{routes_of(d.widths, mask)}  same as (b) ok  {show(ms[UNDER_TEST])}  {n / med / 1e6:8.3f} Gblocks/s", flush=True)
    for label in (LABEL_B, LABEL_C, label_d):
        print(sweep.format_yardstick_row(label, ty, n, ms[label], med, of_name=UNDER_TEST, pad=100), flush=True)
    mb, mc, md = (median(ms[k]) for k in (LABEL_B, LABEL_C, label_d))
    print(f"    ratios: x{med / mb:.3f} of (b), x{med / mc:.3f} of (c), x{med / md:.3f} of (d); at or below (b): {'met' if med <= mb else 'NOT met'}",
          flush=True)


def time_type(ty, packed_gb, reps):
    T = sweep.ESZ[ty] * 8
    N = 1 << T
    c = sweep.mixed_column(ty, 3.0 * packed_gb, refs=None, output=True, bases=True)    # (its --gb budget counts 1.5 x the unpacked bytes)
    n = c.n
    print(f"# {ty}: n = {n} blocks, random column {c.pbytes / 1e9:.3f} GB packed + {n * 128 / 1e9:.3f} GB of bases, {reps} launches each, round-robin",
          flush=True)
    refs = sweep.as_type(sweep.rnd(n * 8, 5).view(torch.int64), ty)
    time_row(ty, "no mask", c, refs, None, "packed", reps)
    time_row(ty, "mask 50 %", c, refs, sweep.random_mask(n, 0.5, 61 + T), "packed", reps)
    time_row(ty, "chained 1 %", c, refs, sweep.random_mask(n, 0.5, 59 + T, every=100), "mask", reps)
    d, _, v64 = sorted_column(ty, n, c.un)
    rows = n * 1024
    lo, hi = int(v64[int(0.30 * rows)].item()) % N, int(v64[int(0.31 * rows)].item()) % N
    interval = fl.undelta_compare_range_widths(d.widths, d.offsets, d.col, d.bases, lo, hi)
    time_row(ty, "sorted 1 %", d, refs, interval, "mask", reps)
    zero = sweep.SimpleNamespace(n=n, widths=torch.zeros_like(c.widths), offsets=torch.zeros_like(c.offsets), col=c.col, pbytes=c.pbytes,
                                 bases=c.bases, un=c.un)
    time_row(ty, "width 0", zero, refs, None, "bases", reps)
    del d, zero, refs, interval
    sweep.release_column(c)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packed-gb", type=float, default=1.0, help="packed bytes of the random column (beyond the 256-MiB Infinity Cache)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--types", default="u32", help="keep only these element types")
    args = ap.parse_args(argv)
    print(sweep.device_header(), flush=True)
    for ty in sweep.chosen_types(args):
        time_type(ty, args.packed_gb, args.reps)


if __name__ == "__main__":
    main()
