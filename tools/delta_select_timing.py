#!/usr/bin/env python3
"""undelta_select_widths (the rows a mask keeps of a mixed-width DELTA-packed column, compacted in original row order: the chains are
compacted where they are decoded, a kept row lands at the popcount of the mask below it, no value is untransposed, an empty-mask or
width-0 block reads no packed byte) on one MI355X, next to three yardsticks timed in the SAME run on the SAME buffers:

  (b) the cost of today's two steps: undelta_pack_untranspose_widths into a full-width buffer (4 KiB per u32 block written), then
      unfor_select_widths over that buffer as a full-width column (the 4 KiB read back), the mask moved into that column's order outside
      the timed region.  The same offsets and the same bytes; its runs are per-block permutations of (a)'s (a full-width column's index
      order is not the row order), so they are checked as sorted-equal (over the leading blocks that hold up to 2^26 kept values);
  (c) unfor_select_widths on a FoR column of the same bytes, widths and mask (random references; the sorted row: the same values
      FoR-coded): the same routes with no chain scan and no bases;
  (d) a bare stream of the bytes the row must move, one wavefront per block: the mean packed bytes + the 128 bytes of bases read where
      the blocks are decoded (the mask's 128 bytes are not streamed), the 128 bytes of mask + the 128 of bases where nearly every block's
      mask is empty or the width is 0, and the mean kept bytes per block written (rounded up to 16).

Rows:
  * mask 50 %     the generator's column of `sweep.py --cases mixed` (seeded-random widths 1 .. T - 1, random packed bytes, --packed-gb
                  of them) under random bases and a random mask of half density: every block EACH;
  * rows 1 %      the same column under a random mask of 1 % density: every block EACH, few rows kept;
  * chained 1 %   the same column, 1 % of the blocks left open by a chained mask: EMPTY everywhere else;
  * sorted 1 %    an ascending column of the same block count (steps 0 .. 7, Delta-coded by the library's encoder) under the mask
                  undelta_compare_range_widths gives for an interval that holds 1 % of the rows;
  * width 0       a column of width-0 blocks under the same bases and the half-density mask: every block BASES.
Every figure is the median of --reps launches, one launch of each variant per round (round-robin), min .. max beside it.  The kernels are
launched through the C ABI with the offsets given (no allocation, no flag read-back inside the timed region).  Before anything is timed,
(a)'s output is compared bit for bit with the decoded buffer indexed by the mask's bits in torch.

The expectation, stated before the run: (a) is at or below (b) in every row ((b) writes and reads back 4 KiB per u32 block more).  The
ratios to (c) and (d) are reported, not gated.  Per row the tool prints the ratios and whether "at or below (b)" is met.  These are
reports, not gates: nothing is tuned toward them.

    python tools/delta_select_timing.py [--packed-gb 1.0] [--reps 7] [--types u32] > profiles/delta_select_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from delta_compare_range_timing import in_full_width_order, sorted_column  # noqa: E402
from sweep import dev, fl, median, show  # noqa: E402

UNDER_TEST = "(a)"
LABEL_B = "(b) undelta_pack_untranspose_widths + unfor_select_widths on the materialised column"
LABEL_C = "(c) unfor_select_widths, a FoR column of the same bytes, widths and mask"
SORT_CHECK_ELEMS = 1 << 26


def routes_of(widths, mask):
    """how many blocks take each route, from the definition (no block of these columns fails a device check or lies outside `out`)"""
    empty = (mask.view(-1, 32) == 0).all(dim=1)
    bases = ~empty & (widths == 0)
    return (f"routes skip {0:8d} empty {int(empty.sum().item()):8d} bounds {0:8d} bases {int(bases.sum().item()):8d} "
            f"each {int((~empty & ~bases).sum().item()):8d}")


def mask_bits(mask, b0, b1):
    """bool[(b1 - b0) * 1024] of blocks b0 .. b1 - 1"""
    sh = torch.arange(32, device=dev, dtype=torch.int32)
    return ((mask[b0 * 32:b1 * 32].view(-1, 1) >> sh) & 1).view(-1).to(torch.bool)


def check_against_decoded(ty, name, out, oo, total, decoded, mask, n, chunk=1 << 15):
    """(a)'s output == the decoded buffer (original row order) indexed by the mask's bits, bit for bit, a chunk of blocks at a time"""
    dec = decoded.view(sweep.SIGNED[ty])
    got = out.view(sweep.SIGNED[ty])
    for b0 in range(0, n, chunk):
        b1 = min(n, b0 + chunk)
        lo = int(oo[b0].item())
        hi = int(oo[b1].item()) if b1 < n else total
        want = dec[b0 * 1024:b1 * 1024][mask_bits(mask, b0, b1)]
        assert want.numel() == hi - lo and torch.equal(got[lo:hi], want), (ty, name, "differs from the decoded buffer indexed by the mask", b0)


def sorted_per_block(ty, out, oo, counts, n_blocks, n_elems):
    """the first n_elems outputs, each block's run sorted"""
    v, i = torch.sort(out[:n_elems].view(sweep.SIGNED[ty]))
    seg = torch.repeat_interleave(torch.arange(n_blocks, device=dev), counts[:n_blocks])[i]
    return v[torch.sort(seg, stable=True).indices]


def time_row(ty, name, d, f, mask, stream_of, reps):
    """one row: d = the Delta column (widths, offsets, col, pbytes, bases, un, n), f = the FoR column of yardstick (c) (widths, offsets,
    col, pbytes, refs), stream_of = what yardstick (d) streams beside the bases ("packed" or "mask")"""
    lib = fl.load()
    T = sweep.ESZ[ty] * 8
    esz = sweep.ESZ[ty]
    n = d.n
    sel_fn = getattr(lib, f"fl_{ty}_undelta_select_widths")
    decode_fn = getattr(lib, f"fl_{ty}_undelta_pack_untranspose_widths")
    for_fn = getattr(lib, f"fl_{ty}_unfor_select_widths")
    moved = in_full_width_order(mask, T)                                    # (b) reads the buffer as a full-width column: its row order
    fw, fo, fr = fl.full_width_column(ty, n, dev)
    oo, total_dev = fl.mask_offsets(mask)
    total = int(total_dev.item())
    out_a, out_b, out_c = (torch.empty(max(total, 16), dtype=sweep.TDT[ty], device=dev) for _ in range(3))
    head = (d.widths.data_ptr(), d.offsets.data_ptr(), d.col.data_ptr(), d.pbytes, d.bases.data_ptr())
    in_ptr, iu = (d.col.data_ptr(), min(8192, d.pbytes // n // 16 * 16)) if stream_of == "packed" else (mask.data_ptr(), 128)
    ou = min(8192, (total * esz // n + 15) // 16 * 16)
    out_d = torch.empty(max(n * ou, 16), dtype=torch.uint8, device=dev)
    label_d = f"(d) bare stream of {iu} + 128 bytes read and {ou} written per block"

    def under_test():
        return sel_fn(*head, mask.data_ptr(), oo.data_ptr(), out_a.data_ptr(), total, n, None, None)

    def two_steps():
        rc = decode_fn(*head, d.un.data_ptr(), n, None, None)
        return rc or for_fn(fw.data_ptr(), fo.data_ptr(), d.un.data_ptr(), n * 128 * T, fr.data_ptr(), 0, moved.data_ptr(), oo.data_ptr(),
                            out_b.data_ptr(), total, n, None, None)

    def for_column():
        return for_fn(f.widths.data_ptr(), f.offsets.data_ptr(), f.col.data_ptr(), f.pbytes, f.refs.data_ptr(), 1, mask.data_ptr(), oo.data_ptr(),
                      out_c.data_ptr(), total, n, None, None)

    def bare():
        return lib.fl_internal_bare_stream(in_ptr, iu, d.bases.data_ptr(), 128, out_d.data_ptr() if ou else None, ou, n, 1, 8 if T <= 16 else 6, 31, None)

    # faster and different is not faster: (a) against the decoded buffer indexed by the mask's bits, bit for bit, before anything is timed
    assert under_test() == 0 and two_steps() == 0 and for_column() == 0 and bare() == 0
    torch.cuda.synchronize()
    check_against_decoded(ty, name, out_a, oo, total, d.un, mask, n)
    # (b)'s runs are per-block permutations of (a)'s
    counts = torch.diff(torch.cat([oo, total_dev.view(1)]))
    nb = int(torch.searchsorted(torch.cumsum(counts, 0), SORT_CHECK_ELEMS, right=True).item())
    ne = int(oo[nb].item()) if nb < n else total
    assert torch.equal(sorted_per_block(ty, out_a, oo, counts, nb, ne), sorted_per_block(ty, out_b, oo, counts, nb, ne)), (ty, name, "(b)'s runs")
    ms = sweep.round_robin({UNDER_TEST: under_test, LABEL_B: two_steps, LABEL_C: for_column, label_d: bare}, reps)
    med = median(ms[UNDER_TEST])
    print(f"undelta_select_widths {name:12s} {ty:4s} packed {d.pbytes / 1e9:6.3f} GB  kept {total / (n * 1024):8.5f}  "
          f"{routes_of(d.widths, mask)}  same as decoded[mask] ok  {show(ms[UNDER_TEST])}  {n / med / 1e6:8.3f} Gblocks/s", flush=True)
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
    f = sweep.SimpleNamespace(widths=c.widths, offsets=c.offsets, col=c.col, pbytes=c.pbytes,
                              refs=sweep.as_type(sweep.rnd(n * 8, 5).view(torch.int64), ty))
    half = sweep.random_mask(n, 0.5, 61 + T)
    time_row(ty, "mask 50 %", c, f, half, "packed", reps)
    time_row(ty, "rows 1 %", c, f, sweep.random_mask(n, 0.01, 67 + T), "packed", reps)
    time_row(ty, "chained 1 %", c, f, sweep.random_mask(n, 0.5, 59 + T, every=100), "mask", reps)
    zero = sweep.SimpleNamespace(n=n, widths=torch.zeros_like(c.widths), offsets=torch.zeros_like(c.offsets), col=c.col, pbytes=c.pbytes,
                                 bases=c.bases, un=c.un)
    fzero = sweep.SimpleNamespace(widths=zero.widths, offsets=zero.offsets, col=c.col, pbytes=c.pbytes, refs=f.refs)
    d, fs, v64 = sorted_column(ty, n, c.un)
    rows = n * 1024
    lo, hi = int(v64[int(0.30 * rows)].item()) % N, int(v64[int(0.31 * rows)].item()) % N
    interval = fl.undelta_compare_range_widths(d.widths, d.offsets, d.col, d.bases, lo, hi)
    time_row(ty, "sorted 1 %", d, fs, interval, "mask", reps)
    time_row(ty, "width 0", zero, fzero, half, "mask", reps)
    del d, fs, zero, fzero, f, interval, half
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
