#!/usr/bin/env python3
"""undelta_compare_range_widths (an interval predicate straight from a mixed-width DELTA-packed column: the chains are decoded in place
of the rows, no value is untransposed, a block its bases decide reads no packed byte) on one MI355X, next to three yardsticks timed in
the SAME run on the SAME buffers:

  (b) today's only path: undelta_pack_untranspose_widths into a full-width buffer (4 KiB per u32 block written), then
      unfor_compare_range_widths over that buffer as a full-width column (the 4 KiB read back);
  (c) unfor_compare_range_widths on a FoR column: in the random rows the same packed bytes and widths with references that leave every
      block undecided -- the floor of the EACH route (no chain scan, no bases) -- in the sorted rows the SAME values FoR-coded by the
      library's encoder (its blocks are decided from the references);
  (d) a bare stream of 256 bytes per block (128 read, 128 written: a device copy of the bases), what a decided block moves.

Rows:
  * random      the generator's column of `sweep.py --cases mixed` (seeded-random widths 1 .. T - 1, random packed bytes, --packed-gb of
                them) under random bases, the interval [2^T / 4, 3 * 2^T / 4]: every block EACH;
  * sorted 1 %, sorted 50 %   an ascending column of the same block count (steps 0 .. 7, Delta-coded by the library's encoder with base =
                the predecessor in original order and the width of the largest delta), an interval that holds 1 % / 50 % of the rows:
                nearly every block ALL or NONE;
  * AND 1 %     the random column again, chained with AND behind an incoming mask that keeps rows in 1 % of the blocks: nearly every
                block KEEP.
Every figure is the median of --reps launches, one launch of each variant per round (round-robin), min .. max beside it.  The kernels are
launched through the C ABI (no allocation, no flag read-back inside the timed region).  Before it is timed, every row's mask is checked
against (b)'s -- bit p of (a) is the original row p, which (b)'s full-width column holds at unpacked index index(r, l), p = LANES r + l
((b)'s incoming mask is given in that order).

The expectations, stated before the run: (a) is at or below (b) in every row ((b) moves at least 8 KiB per u32 block more); on the
sorted rows (a) approaches (d); the EACH row's ratio to (c) is reported, not gated.  Per row the tool prints the ratios and whether
"at or below (b)" is met.  These are reports, not gates: nothing is tuned toward them.

    python tools/delta_compare_range_timing.py [--packed-gb 1.0] [--reps 7] [--types u32] > profiles/delta_compare_range_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from sweep import dev, fl, median, show  # noqa: E402

UNDER_TEST = "(a)"
LABEL_B = "(b) undelta_pack_untranspose_widths + unfor_compare_range_widths on the materialised column"
LABEL_C = {"for": "(c) unfor_compare_range_widths, a FoR column of the same bytes and widths, every block undecided",
           "recoded": "(c) unfor_compare_range_widths, the same values FoR-coded by the library's encoder"}
LABEL_D = "(d) bare stream of 256 bytes per block (a device copy of the bases)"
FL_ORDER = (0, 4, 2, 6, 1, 5, 3, 7)
COMBINE = {"new": 0, "and": 1}


def lane_base(l):
    return (l % 16) * 64 + FL_ORDER[l // 16] * 8


def original_row_to_full_width_index(T):
    """q[p] = the unpacked index at which a full-width (W = T) column holds word p of a block: p = LANES r + l -> index(r, l)"""
    lanes = 1024 // T
    return torch.tensor([FL_ORDER[(p // lanes) // 8] * 16 + ((p // lanes) % 8) * 128 + p % lanes for p in range(1024)], device=dev)


def same_rows(mask_a, mask_b, T, chunk=1 << 15):
    """mask_a (bit p = original row p) against mask_b over the materialised buffer read as a full-width column"""
    q = original_row_to_full_width_index(T)
    sh = torch.arange(32, device=dev, dtype=torch.int32)
    n = mask_a.numel() // 32
    for b0 in range(0, n, chunk):
        a, b = (((m[b0 * 32:(b0 + chunk) * 32].view(-1, 32, 1) >> sh) & 1).view(-1, 1024) for m in (mask_a, mask_b))
        if not torch.equal(a, b[:, q]):
            return False
    return True


def in_full_width_order(mask, T, chunk=1 << 15):
    """the mask whose bit index(r, l) is bit p = LANES r + l of `mask`: the incoming mask as (b)'s full-width column has to see it"""
    q = original_row_to_full_width_index(T)
    sh = torch.arange(32, device=dev, dtype=torch.int32)
    out = torch.empty_like(mask)
    n = mask.numel() // 32
    for b0 in range(0, n, chunk):
        bits = ((mask[b0 * 32:(b0 + chunk) * 32].view(-1, 32, 1) >> sh) & 1).view(-1, 1024).to(torch.bool)
        moved = torch.zeros_like(bits)
        moved[:, q] = bits
        out[b0 * 32:b0 * 32 + moved.numel() // 32] = sweep.mask_words(moved.view(-1))
    return out


def routes_of(ty, widths, bases, lo, hi, mask_in, cb):
    """how many blocks take each route, from the definition (u8 .. u32; int64 arithmetic)"""
    T = sweep.ESZ[ty] * 8
    if T > 32:
        return "routes n/a"
    N = 1 << T
    c = ((bases.view(sweep.SIGNED[ty]).to(torch.int64) & (N - 1)) - lo) % N
    c = c.view(-1, 1024 // T)
    cmin, cmax = c.min(dim=1).values, c.max(dim=1).values
    s = (hi - lo) % N
    reach = T * ((torch.ones_like(cmin) << widths.to(torch.int64)) - 1)
    all_ = (cmax + reach <= s) | (s == N - 1)
    none = ~all_ & (cmin > s) & (cmax + reach <= N - 1)
    bases_ = ~all_ & ~none & (widths == 0)
    keep = torch.zeros_like(all_)
    if cb == COMBINE["and"]:
        keep = (mask_in.view(-1, 32) == 0).all(dim=1)
    live = ~keep
    count = lambda m: int((m & live).sum().item())
    return (f"routes keep {int(keep.sum().item()):8d} all {count(all_):8d} none {count(none):8d} bases {count(bases_):8d} "
            f"each {count(~all_ & ~none & ~bases_):8d}")


def time_row(ty, name, d, f, f_kind, lo, hi, f_lo, f_hi, mask_in, reps):
    """one row: d = the Delta column (widths, offsets, col, pbytes, bases, n), f = the FoR column of yardstick (c) with its own interval"""
    lib = fl.load()
    T = sweep.ESZ[ty] * 8
    n = d.n
    delta_fn = getattr(lib, f"fl_{ty}_undelta_compare_range_widths")
    decode_fn = getattr(lib, f"fl_{ty}_undelta_pack_untranspose_widths")
    range_fn = getattr(lib, f"fl_{ty}_unfor_compare_range_widths")
    cb = COMBINE["new" if mask_in is None else "and"]
    mp = None if mask_in is None else mask_in.data_ptr()
    moved = None if mask_in is None else in_full_width_order(mask_in, T)    # (b) reads the buffer as a full-width column: its row order
    mp_b = None if moved is None else moved.data_ptr()
    fw, fo, fr = fl.full_width_column(ty, n, dev)
    mask_a, mask_b, mask_c = (torch.empty(n * 32, dtype=torch.int32, device=dev) for _ in range(3))
    copy_to = torch.empty_like(d.bases)
    head = (d.widths.data_ptr(), d.offsets.data_ptr(), d.col.data_ptr(), d.pbytes, d.bases.data_ptr())

    def under_test():
        return delta_fn(*head, lo, hi, cb, mp, n, mask_a.data_ptr(), None, None)

    def two_steps():
        rc = decode_fn(*head, d.un.data_ptr(), n, None, None)
        return rc or range_fn(fw.data_ptr(), fo.data_ptr(), d.un.data_ptr(), n * 128 * T, fr.data_ptr(), 0, lo, hi, cb, mp_b, n, mask_b.data_ptr(), None, None)

    def for_column():
        return range_fn(f.widths.data_ptr(), f.offsets.data_ptr(), f.col.data_ptr(), f.pbytes, f.refs.data_ptr(), 1, f_lo, f_hi, cb, mp, n,
                        mask_c.data_ptr(), None, None)

    def bare():
        copy_to.copy_(d.bases)
        return 0

    # faster and different is not faster: the mask against the two-step path's, before anything is timed
    assert under_test() == 0 and two_steps() == 0 and for_column() == 0
    torch.cuda.synchronize()
    assert same_rows(mask_a, mask_b, T), (ty, name, "the mask differs from the two-step path's")
    hits = int(sum(int(torch.bitwise_and(mask_a >> k, 1).sum().item()) for k in range(32)))
    ms = sweep.round_robin({UNDER_TEST: under_test, LABEL_B: two_steps, LABEL_C[f_kind]: for_column, LABEL_D: bare}, reps)
    med = median(ms[UNDER_TEST])
    print(f"undelta_compare_range_widths {name:12s} {ty:4s} packed {d.pbytes / 1e9:6.3f} GB  hits {hits / (n * 1024):8.5f}  "
          f"{routes_of(ty, d.widths, d.bases, lo, hi, mask_in, cb)}  same as (b) ok  {show(ms[UNDER_TEST])}  {n / med / 1e6:8.3f} Gblocks/s", flush=True)
    for label in (LABEL_B, LABEL_C[f_kind], LABEL_D):
        print(sweep.format_yardstick_row(label, ty, n, ms[label], med, of_name=UNDER_TEST, pad=100), flush=True)
    mb, mc, md = (median(ms[k]) for k in (LABEL_B, LABEL_C[f_kind], LABEL_D))
    print(f"    ratios: x{med / mb:.3f} of (b), x{med / mc:.3f} of (c), x{med / md:.3f} of (d); at or below (b): {'met' if med <= mb else 'NOT met'}",
          flush=True)


def sorted_column(ty, n, un):
    """an ascending column of n blocks (steps 0 .. 7 from a start that leaves room: it never wraps for u32 / u64 at these sizes; the
    narrow types wrap round), Delta-coded by the library's own encoder; `un`: an n-block buffer of the type, reused for (b)"""
    T = sweep.ESZ[ty] * 8
    lanes = 1024 // T
    g = torch.Generator(device=dev)
    g.manual_seed(53 + T)
    v64 = torch.cumsum(torch.randint(0, 8, (n * 1024,), dtype=torch.int64, device=dev, generator=g), dim=0) + 1000
    prev = torch.cat([v64[:1], v64[:-1]])
    biggest = (v64 - prev).view(n, 1024).max(dim=1).values
    widths = torch.where(biggest > 0, torch.floor(torch.log2(biggest.clamp(min=1).double())).to(torch.int64) + 1, torch.zeros_like(biggest)).to(torch.uint8)
    first = torch.tensor([lane_base(l) for l in range(lanes)], device=dev)
    bases = sweep.as_type(prev.view(n, 1024)[:, first].reshape(-1).contiguous(), ty)
    vals = sweep.as_type(v64, ty)
    offsets, total = fl.widths_to_offsets(ty, widths)
    pbytes = int(total.item())
    col = torch.zeros(max(pbytes // sweep.ESZ[ty], 16), dtype=sweep.TDT[ty], device=dev)
    fl.transpose_delta_pack_widths(widths, offsets, vals, bases, col)
    back = fl.undelta_pack_widths(widths, offsets, col, bases, output=un, untranspose=True)
    assert torch.equal(back.view(torch.uint8), vals.view(torch.uint8)), (ty, "the sorted column does not decode to its values")
    d = sweep.SimpleNamespace(n=n, widths=widths, offsets=offsets, col=col, pbytes=pbytes, bases=bases, un=un)
    # the same values FoR-coded, for yardstick (c)
    mins, maxs = fl.BitPacking.block_min_max(vals)
    fwid = fl.for_widths(mins, maxs)
    foff, ftotal = fl.widths_to_offsets(ty, fwid)
    fcol = torch.zeros(max(int(ftotal.item()) // sweep.ESZ[ty], 16), dtype=sweep.TDT[ty], device=dev)
    fl.for_pack_widths(fwid, foff, vals, mins, fcol)
    f = sweep.SimpleNamespace(widths=fwid, offsets=foff, col=fcol, pbytes=int(ftotal.item()), refs=mins)
    return d, f, v64


def time_type(ty, packed_gb, reps):
    T = sweep.ESZ[ty] * 8
    N = 1 << T
    c = sweep.mixed_column(ty, 3.0 * packed_gb, refs=None, output=True, bases=True)    # (its --gb budget counts 1.5 x the unpacked bytes)
    n = c.n
    print(f"# {ty}: n = {n} blocks, random column {c.pbytes / 1e9:.3f} GB packed + {n * 128 / 1e9:.3f} GB of bases, {reps} launches each, round-robin",
          flush=True)
    # yardstick (c) of the random rows: the same bytes and widths as a FoR column, every block's range holding N / 2 - 1 and N / 2
    x64 = sweep.rnd(n * 8, 5).view(torch.int64)
    f = sweep.SimpleNamespace(widths=c.widths, offsets=c.offsets, col=c.col, pbytes=c.pbytes,
                              refs=sweep.as_type(sweep.undecided_refs(N >> 1, x64, c.widths), ty))
    time_row(ty, "random", c, f, "for", N >> 2, 3 * (N >> 2), 0, (N >> 1) - 1, None, reps)
    sparse = sweep.random_mask(n, 0.5, 59 + T, every=100)
    time_row(ty, "AND 1 %", c, f, "for", N >> 2, 3 * (N >> 2), 0, (N >> 1) - 1, sparse, reps)
    d, fs, v64 = sorted_column(ty, n, c.un)
    rows = n * 1024
    for name, first, last in (("sorted 1 %", int(0.30 * rows), int(0.31 * rows)), ("sorted 50 %", int(0.25 * rows), int(0.75 * rows))):
        lo, hi = int(v64[first].item()) % N, int(v64[last].item()) % N
        time_row(ty, name, d, fs, "recoded", lo, hi, lo, hi, None, reps)
    del d, fs, f
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
