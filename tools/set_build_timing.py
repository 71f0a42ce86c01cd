#!/usr/bin/env python3
"""unfor_set_build_widths (the member set of a mixed-width FoR-packed key column, ORed into a window's bitmap on the device: the build
side of the semi-join unfor_compare_in probes) on one MI355X, next to two baselines timed in the SAME run on the SAME buffers:

  (a) unfor_compare_in_widths on the same column and window: the same packed bytes read, the same blocks decided from their
      metadata, one bit LOOKED UP per element where this sets one -- the floor;
  (b) the composition this replaces: unfor_select_widths (unfor_pack_widths at mask=None), then torch building the same bitmap
      (index arithmetic, a scatter of True into a bool vector, the words and the two counts).

Rows, per element type as far as it has them:
  * windows of 8, 2048, 65536 and 65537 bits over the generator's column of `sweep.py --cases mixed` (seeded-random widths 1 .. T - 1,
    random packed bytes, --packed-gb of them), every block's value range straddling the window's middle -- up to 65536 bits a
    wavefront builds a private bitmap in LDS, above that every element is one atomic in device memory;
  * a window of 2^24 bits (u8 / u16: the whole domain) over three key columns of as many rows, encoded by the library's own encoder:
    random keys (scattered), ascending keys with 4 duplicates each (a foreign key in table order; the column has more rows than
    the window has keys, so the keys start over every 4 * 2^24 rows), and -- on the generator's widths with all-zero packed
    bytes -- one key for the whole column (full contention);
  * 2048 bits (u8: 8) with 99 % of the blocks outside the window, and the same window under a random 1 % mask.
Memory-tier rows time BOTH variants of the memory tier beside the shipped one: one atomic per kept in-window element, and test before
set (load the word, issue the atomic only when the bit is still clear).  Every figure is the median of --reps launches, one launch of
each variant per round (round-robin), min .. max beside it.  The kernels are launched through the C ABI (no allocation, no flag
read-back inside the timed region); the bitmap and the counters are zeroed in front of EVERY launch, outside its timed region, so
every launch is a first build.  Before it is timed, every row's bitmap and counters -- of every variant -- are checked bit for bit
against (b)'s.

Per row the tool prints whether its expectations are met: (1) the time is below (b)'s; (2) on the LDS-tier rows and the 99 %-outside
row, the time is within WITHIN_A times (a)'s; (3) on the memory-tier rows there is nothing to meet: the atomics give what they give,
both variants' figures stand beside the shipped one's.  These are reports, not gates.

    python tools/set_build_timing.py [--packed-gb 1.0] [--reps 7] [--types u32,u64] > profiles/set_build_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from sweep import SIGNED, TDT, dev, fl, median, show  # noqa: E402

UNDER_TEST = "set_build"
WITHIN_A = 1.5                          # expectation 2: an LDS atomic per element where (a) has a cross-lane read or a cached gather
LDS_BITS = 65536                        # fastlanes_amd/csrc/fl_set_build_map.hpp: SET_BUILD_LDS_BITS
CHUNK = 1 << 26                         # rows per torch step: bounds the composition's temporaries at a few GB
VARIANT_ENV = "FL_INTERNAL_SET_BUILD_VARIANT"
VARIANTS = (("1", "variant: one atomic per element"), ("2", "variant: test before set"))


def torch_bitmap(vals, ty, lo, bits):
    """(int32 words, inserted, outside) of the values `vals` (a tensor of the element type): what (b) builds"""
    T = 8 * sweep.ESZ[ty]
    present = torch.zeros(-(-max(bits, 1) // 32) * 32, dtype=torch.bool, device=dev)
    inside_n = 0
    lo_s = lo - (1 << 64) if lo >= 1 << 63 else lo
    for i in range(0, vals.numel(), CHUNK):
        j = vals[i:i + CHUNK].view(SIGNED[ty]).to(torch.int64) - lo_s       # (wraps mod 2^64 for u64)
        if T < 64:
            j &= (1 << T) - 1
        inside = (j >= 0) & (j < bits)
        present[j[inside]] = True
        inside_n += int(inside.sum().item())
    return sweep.mask_words(present)[:(bits + 31) // 32], inside_n, vals.numel() - inside_n


def round_robin_fresh(variants, reps, reset, warmup=2):
    """sweep.round_robin with `reset` enqueued in front of every launch, outside its event pair: every timed launch builds into a
    zeroed bitmap, as a first call does (into a bitmap that already holds its bits, test-before-set would issue no atomic at all)"""
    for _ in range(warmup):
        for f in variants.values():
            reset()
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            reset()
            ms[k].append(sweep.event_ms(f))
    return ms


def encoded(ty, vals):
    """a key column given as values -> the library's own encoder -> a namespace like sweep.mixed_column's"""
    k = sweep.SimpleNamespace(ty=ty)
    k.refs, maxs = fl.BitPacking.block_min_max(vals)
    k.widths = fl.for_widths(k.refs, maxs)
    k.offsets, total = fl.widths_to_offsets(ty, k.widths)
    k.pbytes = int(total.item())
    k.col = torch.zeros(max(k.pbytes // sweep.ESZ[ty], 16), dtype=TDT[ty], device=dev)
    fl.for_pack_widths(k.widths, k.offsets, vals, k.refs, k.col)
    k.stride = 1
    return k


def key_rows(ty, c, x64, lo, bits):
    """(row name, column) of the three key-column rows; the columns hold c.n * 1024 rows and are built in c.un one after another"""
    rows = c.n * 1024
    yield "random keys", lambda: encoded(ty, sweep.as_type(lo + sweep.rnd(rows * 8, 9).view(torch.int64) % bits, ty))
    yield "ascending x4", lambda: encoded(ty, sweep.as_type(lo + (torch.arange(rows, dtype=torch.int64, device=dev) // 4) % bits, ty))

    def one_key():
        k = sweep.SimpleNamespace(ty=ty, widths=c.widths, offsets=c.offsets, pbytes=c.pbytes, col=torch.zeros_like(c.col))
        k.refs, k.stride = sweep.as_type(torch.full((1,), lo + bits // 2, dtype=torch.int64, device=dev), ty), 0
        return k
    yield "one key", one_key


def time_row(ty, name, k, n, lo, bits, mask_bits, straddling, reps, un):
    """one row: k = the column (widths, offsets, col, pbytes, refs, stride), the window, the mask's bits (None: every row)"""
    lib = fl.load()
    build_fn = getattr(lib, f"fl_{ty}_unfor_set_build_widths")
    in_fn = getattr(lib, f"fl_{ty}_unfor_compare_in_widths")
    head = (k.widths.data_ptr(), k.offsets.data_ptr(), k.col.data_ptr(), k.pbytes, k.refs.data_ptr(), k.stride)
    refs = k.refs if k.stride else k.refs.expand(n).contiguous()
    nw = (bits + 31) // 32
    words, words_a = (torch.zeros(max(nw, 4), dtype=torch.int32, device=dev) for _ in range(2))
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    out_mask = torch.empty(n * 32, dtype=torch.int32, device=dev)
    mask = None if mask_bits is None else sweep.mask_words(mask_bits)
    mp = None if mask is None else mask.data_ptr()
    if mask is not None:
        out_offsets, total = fl.mask_offsets(mask)
        kept = torch.empty(int(total.item()), dtype=TDT[ty], device=dev)

    def set_build():
        return build_fn(*head, mp, n, lo, bits, words.data_ptr(), stats.data_ptr(), None, None)

    def variant(code):
        def run():
            os.environ[VARIANT_ENV] = code
            rc = build_fn(*head, mp, n, lo, bits, words.data_ptr(), stats.data_ptr(), None, None)
            del os.environ[VARIANT_ENV]
            return rc
        return run

    def compare_in():                                                       # NEW without a mask, AND through the same mask with one
        return in_fn(*head, lo, bits, words_a.data_ptr(), 0, 0 if mask is None else 1, mp, n, out_mask.data_ptr(), None, None)

    def composition():
        if mask is None:
            fl.unfor_pack_widths(k.widths, k.offsets, k.col, refs, output=un, check=False)
            return torch_bitmap(un, ty, lo, bits)
        fl.unfor_select_widths(k.widths, k.offsets, k.col, refs, mask, out_offsets=out_offsets, output=kept, check=False)
        return torch_bitmap(kept, ty, lo, bits)

    lds = bits <= LDS_BITS
    tier = "LDS" if lds else "memory"
    timed = {UNDER_TEST: set_build}
    if not lds:
        timed.update({label: variant(code) for code, label in VARIANTS})
    # faster and different is not faster: every variant's bitmap and counters against (b)'s, before anything is timed
    want_words, want_in, want_out = composition()
    for label, f in timed.items():
        words.zero_(); stats.zero_()
        assert f() == 0 and compare_in() == 0
        assert torch.equal(words[:nw], want_words) and stats.tolist() == [want_in, want_out], (ty, name, label, stats.tolist(), want_in, want_out)
    del want_words
    timed["(a) unfor_compare_in_widths, the same window"] = compare_in
    timed["(b) unfor_select_widths / unfor_pack_widths + torch bitmap"] = composition
    ms = round_robin_fresh(timed, reps, lambda: (words.zero_(), stats.zero_()))
    med = median(ms[UNDER_TEST])
    ka, kb = list(timed)[-2:]
    print(f"unfor_set_build_widths {name:13s} {ty:4s} bits {bits:8d} ({tier:6s}) mask {'none' if mask is None else 'random 1 %':10s} blocks straddling {straddling:4.2f} "
          f"inserted {want_in:11d} outside {want_out:11d} bitmap bit-for-bit ok  {show(ms[UNDER_TEST])}  {n / med / 1e6:8.3f} Gblocks/s", flush=True)
    for label in list(timed)[1:]:
        print(sweep.format_yardstick_row(label, ty, n, ms[label], med, of_name=UNDER_TEST, pad=62), flush=True)
    med_a, med_b = median(ms[ka]), median(ms[kb])
    line = f"    expectations: below (b): {'met' if med < med_b else 'NOT met'}"
    if lds or straddling < 1.0:
        line += f"; within x{WITHIN_A:.2f} of (a) (x{med / med_a:.3f}): {'met' if med <= WITHIN_A * med_a else 'NOT met'}"
    else:
        line += f"; memory tier, nothing to meet: x{med / med_a:.3f} of (a), " + ", ".join(f"{label} x{median(ms[label]) / med_a:.3f}" for _, label in VARIANTS)
    print(line, flush=True)


def time_column(ty, c, reps):
    T, n = c.T, c.n
    top = min(1 << T, 1 << 32)
    x64 = sweep.rnd(n * 8, 5).view(torch.int64)
    lo = 1 << (T - 2)
    print(f"# {ty}: n = {n} blocks, packed {c.pbytes / 1e9:.3f} GB, {reps} launches each, round-robin", flush=True)

    def straddling_column(bits, share):
        r64 = sweep.undecided_refs(lo + bits // 2, x64, c.widths)           # every block's range holds the window's middle
        if share < 1.0:
            outside = torch.full_like(r64, lo + bits + 16)                  # [r, r + 2^W - 1] ends below lo + 2^T: outside the window
            r64 = torch.where(torch.arange(n, device=dev) % round(1 / share) == 0, r64, outside)
        return sweep.SimpleNamespace(widths=c.widths, offsets=c.offsets, col=c.col, pbytes=c.pbytes, refs=sweep.as_type(r64, ty), stride=1)

    for bits in (b for b in (8, 2048, 65536, 65537) if b <= top):
        time_row(ty, f"{bits} bits", straddling_column(bits, 1.0), n, lo, bits, None, 1.0, reps, c.un)
    wide = min(1 << 24, top)
    for name, make in key_rows(ty, c, x64, lo, wide):
        k = make()
        time_row(ty, name, k, n, lo, wide, None, 1.0, reps, c.un)
        del k
    small = min(2048, 1 << (T - 5))
    time_row(ty, "99 % outside", straddling_column(small, 0.01), n, lo, small, None, 0.01, reps, c.un)
    g = torch.Generator(device=dev)
    g.manual_seed(91 + T)
    sparse = torch.rand(n * 1024, device=dev, generator=g) < 0.01
    time_row(ty, "1 % mask", straddling_column(small, 1.0), n, lo, small, sparse, 1.0, reps, c.un)


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
