#!/usr/bin/env python3
"""unfor_aggregate_by_window_widths (COUNT / SUM / MIN / MAX of a mixed-width FoR-packed value column grouped by a mixed-width key column
of the same type inside a dense window of the key domain) on one MI355X, next to two baselines timed in the SAME run on the SAME buffers:

  (a) unfor_aggregate_columns_widths (a + b) on the same two columns: the same packed bytes read, the same two columns decoded, no
      scatter -- the floor;
  (b) the composition this replaces: unfor_pack_widths (unfor_select_widths under a mask) of BOTH columns, then torch index_add_ /
      scatter_reduce on int64.

The key column is the generator's column of `sweep.py --cases mixed` (seeded-random widths 1 .. T - 1, random packed bytes, --packed-gb
of them); the value column beside it is narrow (seeded-random widths 1 .. 8, references 1) and of the same element type.  Rows, per
element type as far as it has them, each with what = sum alone and with all four arrays:
  * windows of 8 and 256 groups (a private table per wavefront in LDS) and of 257, 4096, 65536 and 2^20 groups (one device-memory atomic
    per kept in-window element and array), every key block's range straddling the window's middle.  The heavily contended memory-tier
    rows (257 and 4096 groups) run on at most 2^24 rows: DESIGN.md 5b has 2.7 - 11.3 ns per atomic on few addresses, a full-size
    column would take seconds per launch;
  * a window of 2^24 groups (u8 / u16: the whole domain) over key columns of as many rows, encoded by the library's own encoder: random
    keys (scattered) and ascending keys with 4 duplicates each (l_orderkey in table order);
  * one key per block (every key block of width 0: a column clustered by key);
  * 256 groups (u8: 8) with 99 % of the key blocks outside the window, and the same window under a random 1 % mask.
Every figure is the median of --reps launches, one launch of each variant per round (round-robin), min .. max beside it.  The kernels
are launched through the C ABI (no allocation, no flag read-back inside the timed region); the table is re-initialised to the
identities in front of EVERY launch, outside its timed region.  Before it is timed, every row's arrays and counters are checked bit for
bit against (b)'s.

Per row the tool prints the ratio to (a) and to (b) and whether the time is below (b)'s.  These are reports, not gates: no figure is
expected of (a), and the 256 -> 257 rows are what the next decision about the tier boundary is taken from.

    python tools/aggregate_by_window_timing.py [--packed-gb 1.0] [--reps 7] [--types u32,u64] > profiles/aggregate_by_window_timing.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep  # noqa: E402  (the timing helpers, the column generator and the formatters)
from set_build_timing import encoded  # noqa: E402  (a key column given as values -> the library's own encoder)
from sweep import SIGNED, TDT, dev, fl, median, show  # noqa: E402

UNDER_TEST = "aggregate_by_window"
LDS_GROUPS = 256                        # fastlanes_amd/csrc/fl_aggregate_by_window_map.hpp: AGGREGATE_BY_WINDOW_LDS_GROUPS
CONTENDED_ROWS = 1 << 24                # the most rows of a heavily contended memory-tier row
CHUNK = 1 << 25                         # rows per torch step: bounds the composition's temporaries at a few GB
WHATS = (("sum", (0, 1, 0, 0)), ("count sum min max", (1, 1, 1, 1)))
I64_MAX = (1 << 63) - 1


def value_column(ty, n):
    """the narrow value column beside the key column: widths 1 .. 8 (below T), random packed bytes, references 1"""
    T = 8 * sweep.ESZ[ty]
    v = sweep.SimpleNamespace(ty=ty)
    g = torch.Generator(device=dev)
    g.manual_seed(77 + T)
    v.widths = torch.randint(1, min(8, T - 1) + 1, (n,), dtype=torch.int64, device=dev, generator=g).to(torch.uint8)
    v.offsets, total = fl.widths_to_offsets(ty, v.widths)
    v.pbytes = int(total.item())
    v.col = sweep.rnd(max(v.pbytes, 16), 78 + T).view(TDT[ty])
    v.refs, v.stride = sweep.as_type(torch.ones(1, dtype=torch.int64, device=dev), ty), 0
    return v


def first_blocks(k, n):
    """the first n blocks of a column"""
    return sweep.SimpleNamespace(widths=k.widths[:n], offsets=k.offsets[:n], col=k.col, pbytes=k.pbytes, refs=k.refs[:n] if k.stride else k.refs,
                                 stride=k.stride)


def torch_table(vals, keys, ty, lo, ng, which):
    """([counts, sums, mins, maxs] int64[ng] holding uint64 bits, or None where which[i] == 0; inside; outside) of the decoded rows:
    what (b) builds.  The value column is narrow: its values lie far below 2^63, so int64 min / max are the unsigned ones."""
    T = 8 * sweep.ESZ[ty]
    new = lambda fill: torch.full((max(ng, 1),), fill, dtype=torch.int64, device=dev)   # noqa: E731
    counts, sums, mins, maxs = new(0), new(0), new(I64_MAX), new(0)
    inside_n = 0
    lo_s = lo - (1 << 64) if lo >= 1 << 63 else lo
    for i in range(0, keys.numel(), CHUNK):
        j = keys[i:i + CHUNK].view(SIGNED[ty]).to(torch.int64) - lo_s       # (wraps mod 2^64 for u64)
        if T < 64:
            j &= (1 << T) - 1
        inside = (j >= 0) & (j < ng)
        j = j[inside]
        v = vals[i:i + CHUNK].view(SIGNED[ty]).to(torch.int64)
        if T < 64:
            v &= (1 << T) - 1
        v = v[inside]
        inside_n += j.numel()
        if which[0] or which[2]:
            counts.index_add_(0, j, torch.ones_like(j))
        if which[1]:
            sums.index_add_(0, j, v)
        if which[2]:
            mins.scatter_reduce_(0, j, v, "amin")
        if which[3]:
            maxs.scatter_reduce_(0, j, v, "amax")
    mins = torch.where(counts == 0, torch.full_like(mins, -1), mins)        # a slot no row reached keeps the identity 2^64 - 1
    out = [t[:ng] if on else None for t, on in zip((counts, sums, mins, maxs), which)]
    return out, inside_n, keys.numel() - inside_n


def round_robin_fresh(variants, reps, reset, warmup=2):
    """sweep.round_robin with `reset` enqueued in front of every launch, outside its event pair: every timed launch accumulates into a
    table of identities, as a first call does"""
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


def time_row(ty, name, v, k, n, lo, ng, mask_bits, straddling, reps, un_v, un_k):
    """one row: v / k = the value and the key column (widths, offsets, col, pbytes, refs, stride), the window, the mask's bits (None:
    every row); timed once per entry of WHATS"""
    lib = fl.load()
    fn = getattr(lib, f"fl_{ty}_unfor_aggregate_by_window_widths")
    cols_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_columns_widths")
    head = lambda c: (c.widths.data_ptr(), c.offsets.data_ptr(), c.col.data_ptr(), c.pbytes, c.refs.data_ptr(), c.stride)   # noqa: E731
    full = lambda c: c.refs if c.stride else c.refs.expand(n).contiguous()   # noqa: E731
    vrefs, krefs = full(v), full(k)
    arrays = [torch.empty(max(ng, 2), dtype=torch.int64, device=dev) for _ in range(4)]
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    slots = torch.empty((n, 4), dtype=torch.int64, device=dev)
    mask = None if mask_bits is None else sweep.mask_words(mask_bits)
    mp = None if mask is None else mask.data_ptr()
    if mask is not None:
        out_offsets, total = fl.mask_offsets(mask)
        kept_v, kept_k = (torch.empty(int(total.item()), dtype=TDT[ty], device=dev) for _ in range(2))

    def reset():
        for t, fill in zip(arrays, (0, 0, -1, 0)):
            t.fill_(fill)
        stats.zero_()

    def window(which):
        ptrs = [t.data_ptr() if on and ng else None for t, on in zip(arrays, which)]
        return lambda: fn(*head(v), *head(k), mp, n, lo, ng, *ptrs, stats.data_ptr(), None, None)

    def columns():
        return cols_fn(1, *head(v), *head(k), mp, n, slots.data_ptr(), None, None)

    def composition(which):
        def run():
            if mask is None:
                fl.unfor_pack_widths(v.widths, v.offsets, v.col, vrefs, output=un_v[:n * 1024], check=False)
                fl.unfor_pack_widths(k.widths, k.offsets, k.col, krefs, output=un_k[:n * 1024], check=False)
                return torch_table(un_v[:n * 1024], un_k[:n * 1024], ty, lo, ng, which)
            fl.unfor_select_widths(v.widths, v.offsets, v.col, vrefs, mask, out_offsets=out_offsets, output=kept_v, check=False)
            fl.unfor_select_widths(k.widths, k.offsets, k.col, krefs, mask, out_offsets=out_offsets, output=kept_k, check=False)
            return torch_table(kept_v, kept_k, ty, lo, ng, which)
        return run

    tier = "LDS" if ng <= LDS_GROUPS else "memory"
    for wname, which in WHATS:
        under, comp = window(which), composition(which)
        # faster and different is not faster: the arrays and the counters against (b)'s, before anything is timed
        want, want_in, want_out = comp()
        reset()
        assert under() == 0 and columns() == 0
        for t, w, on in zip(arrays, want, which):
            assert not on or torch.equal(t[:ng], w), (ty, name, wname)
        assert stats.tolist() == [want_in, want_out], (ty, name, wname, stats.tolist(), want_in, want_out)
        del want
        timed = {UNDER_TEST: under, "(a) unfor_aggregate_columns_widths, the same two columns": columns,
                 "(b) unfor_pack_widths / unfor_select_widths of both columns + torch index_add_ / scatter_reduce": comp}
        ms = round_robin_fresh(timed, reps, reset)
        med = median(ms[UNDER_TEST])
        ka, kb = list(timed)[1:]
        print(f"unfor_aggregate_by_window_widths {name:13s} {ty:4s} groups {ng:8d} ({tier:6s}) what {wname:17s} mask {'none' if mask is None else 'random 1 %':10s} "
              f"blocks straddling {straddling:4.2f} rows {n * 1024:11d} inside {want_in:11d} outside {want_out:11d} arrays bit-for-bit ok  "
              f"{show(ms[UNDER_TEST])}  {n / med / 1e6:8.3f} Gblocks/s", flush=True)
        for label in (ka, kb):
            print(sweep.format_yardstick_row(label, ty, n, ms[label], med, of_name=UNDER_TEST, pad=96), flush=True)
        print(f"    ratios: x{med / median(ms[ka]):.3f} of (a), x{med / median(ms[kb]):.3f} of (b); below (b): {'met' if med < median(ms[kb]) else 'NOT met'}", flush=True)


def time_column(ty, c, reps):
    T, n = c.T, c.n
    top = min(1 << T, 1 << 32)
    x64 = sweep.rnd(n * 8, 5).view(torch.int64)
    lo = 1 << (T - 2)
    v = value_column(ty, n)
    un_v = torch.empty_like(c.un)
    print(f"# {ty}: n = {n} blocks, key column packed {c.pbytes / 1e9:.3f} GB, value column packed {v.pbytes / 1e9:.3f} GB, {reps} launches each, round-robin", flush=True)

    def straddling_column(ng, share):
        r64 = sweep.undecided_refs(lo + ng // 2, x64, c.widths)             # every key block's range holds the window's middle
        if share < 1.0:
            outside = torch.full_like(r64, lo + ng + 16)                    # [r, r + 2^W - 1] ends below lo + 2^T: outside the window
            r64 = torch.where(torch.arange(n, device=dev) % round(1 / share) == 0, r64, outside)
        return sweep.SimpleNamespace(widths=c.widths, offsets=c.offsets, col=c.col, pbytes=c.pbytes, refs=sweep.as_type(r64, ty), stride=1)

    for ng in (g for g in (8, 256, 257, 4096, 65536, 1 << 20) if g <= top):
        m = min(n, CONTENDED_ROWS // 1024) if ng in (257, 4096) else n
        time_row(ty, f"{ng} groups", first_blocks(v, m), first_blocks(straddling_column(ng, 1.0), m), m, lo, ng, None, 1.0, reps, un_v, c.un)
    wide = min(1 << 24, top)
    rows = n * 1024
    for name, make in (("random keys", lambda: encoded(ty, sweep.as_type(lo + sweep.rnd(rows * 8, 9).view(torch.int64) % wide, ty))),
                       ("ascending x4", lambda: encoded(ty, sweep.as_type(lo + (torch.arange(rows, dtype=torch.int64, device=dev) // 4) % wide, ty)))):
        k = make()
        time_row(ty, name, v, k, n, lo, wide, None, 1.0, reps, un_v, c.un)
        del k
    per_block = sweep.SimpleNamespace(widths=torch.zeros_like(c.widths), offsets=torch.zeros_like(c.offsets), col=c.col, pbytes=0, stride=1,
                                      refs=sweep.as_type(lo + torch.arange(n, dtype=torch.int64, device=dev) % wide, ty))
    time_row(ty, "key per block", v, per_block, n, lo, wide, None, 1.0, reps, un_v, c.un)
    small = min(LDS_GROUPS, 1 << (T - 5))
    time_row(ty, "99 % outside", v, straddling_column(small, 0.01), n, lo, small, None, 0.01, reps, un_v, c.un)
    g = torch.Generator(device=dev)
    g.manual_seed(91 + T)
    sparse = torch.rand(n * 1024, device=dev, generator=g) < 0.01
    time_row(ty, "1 % mask", v, straddling_column(small, 1.0), n, lo, small, sparse, 1.0, reps, un_v, c.un)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packed-gb", type=float, default=1.0, help="packed bytes of the key column (beyond the 256-MiB Infinity Cache)")
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
