#!/usr/bin/env python3
"""Throughput sweep over the kernel families (HIP-event timing, random data, HBM-resident).
    python tools/sweep.py [--gb 24] [--reps 7] [--cases quick|orig|consume|fused|allwidths|widths|host|small|batch|refbench|
                                                         mixed|select|aggregate|aggregate_by|compare_range|compare_columns|single]
quick .. widths print one line per (op, type, width): ms, GB/s (algorithmic bytes), fraction of the 8 TB/s HBM peak,
G ints/s.  Every other case is one function below (case_<name>) whose docstring says what its lines mean."""
import argparse
import ctypes
import json
import os
import re
import sys
import time
from types import SimpleNamespace

import numpy as np

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastlanes_amd as fl  # noqa: E402
from fastlanes_amd import placement as pl  # noqa: E402

ALLWIDTH_OPS = ("unpack", "pack", "unfor_pack", "for_pack", "undelta_pack", "undelta_pack_untranspose", "transpose_delta_pack")
TYPES = ("u32", "u64", "u16", "u8")               # the order the mixed-width cases iterate in
PEAK_GBPS = 8000                                  # the HBM peak every "fraction of the peak" is taken of
ESZ = {"u8": 1, "u16": 2, "u32": 4, "u64": 8}
TDT = {"u8": torch.uint8, "u16": torch.uint16, "u32": torch.uint32, "u64": torch.uint64}
SIGNED = {"u8": torch.uint8, "u16": torch.int16, "u32": torch.int32, "u64": torch.int64}     # int64 -> T by truncation; what torch compares
NPDT = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}
dev = torch.device("cuda:0")


def rnd(nbytes, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randint(-2**63, 2**63 - 1, ((nbytes + 7) // 8,), dtype=torch.int64, device=dev, generator=g).view(torch.uint8)[:nbytes]


def of_peak(nbytes, ms):
    return nbytes / ms / (PEAK_GBPS * 1e6)


def device_header(placement=None):
    props = torch.cuda.get_device_properties(dev)
    return f"# device {props.name} unique id {getattr(props, 'uuid', 'unknown')}" + (f"  placement {placement}" if placement else "")


def chosen_types(args):
    return [ty for ty in TYPES if not args.types or ty in args.types.split(",")]


# ---- timing: every figure of every case comes from these -------------------------------------------------------------------------

def event_ms(f, calls=1):
    """ms between two events around `calls` back-to-back calls of f on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        f()
    b.record(); b.synchronize()
    return a.elapsed_time(b)


def timed(f, reps, warmup=2, calls=1, check=False):
    """[ms, ...]: `reps` event-timed launches of f (each `calls` calls between one event pair) after `warmup` untimed calls and a
    synchronize; check: the untimed calls must return 0"""
    for _ in range(warmup):
        rc = f()
        assert not check or rc == 0
    torch.cuda.synchronize()
    return [event_ms(f, calls) for _ in range(reps)]


def round_robin(variants, reps, warmup=2):
    """{name: [ms, ...]}: `reps` timed launches of every variant, interleaved (one launch of each per round), after `warmup` untimed
    rounds: a variant timed alone right after an idle stretch runs at lower clocks than the ones after it -- round 3's
    batch-vs-contiguous gap was partly that"""
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            ms[k].append(event_ms(f))
    return ms


def per_call_us(f, calls, warmup=20):
    """us per call of `calls` back-to-back calls between one event pair (launch-bound shapes)"""
    return timed(f, 1, warmup=warmup, calls=calls)[0] * 1e3 / calls


def median(ms):
    return sorted(ms)[len(ms) // 2]


def medians(ms):
    return {k: median(v) for k, v in ms.items()}


def show(ms):
    v = sorted(ms)
    return f"{v[len(v) // 2]:9.4f} ms ({v[0]:.4f} .. {v[-1]:.4f})"


# ---- selection masks --------------------------------------------------------------------------------------------------------------

def mask_words(bits, chunk_blocks=32768):
    """int32 words of a bool mask (bit i of word j = bits[32 * j + i]), built `chunk_blocks` blocks at a time"""
    out = torch.empty(bits.numel() // 32, dtype=torch.int32, device=bits.device)
    sh = torch.arange(32, device=bits.device)
    step = chunk_blocks * 1024
    for i in range(0, bits.numel(), step):
        w64 = (bits[i:i + step].view(-1, 32).to(torch.int64) << sh).sum(dim=1)
        out[i // 32:i // 32 + w64.numel()] = torch.where(w64 >= 1 << 31, w64 - (1 << 32), w64).to(torch.int32)
    return out


def random_mask(n, density, seed, every=1, chunk_blocks=32768, device=dev):
    """int32 words of a random mask over n blocks, drawn `chunk_blocks` blocks at a time (densities 0 and 1 draw nothing);
    every > 1: only blocks b % every == 0 keep anything"""
    g = torch.Generator(device=device); g.manual_seed(seed)
    out = torch.empty(n * 32, dtype=torch.int32, device=device)
    for b0 in range(0, n, chunk_blocks):
        nb = min(chunk_blocks, n - b0)
        if density <= 0.0 or density >= 1.0:
            bits = torch.full((nb * 1024,), density >= 1.0, dtype=torch.bool, device=device)
        else:
            bits = torch.rand(nb * 1024, device=device, generator=g) < density
        if every > 1:
            bits &= ((torch.arange(b0, b0 + nb, device=device) % every) == 0).repeat_interleave(1024)
        out[b0 * 32:(b0 + nb) * 32] = mask_words(bits, chunk_blocks)
    return out


def clustered_and_masks(n, T):
    """the four incoming masks of the compare_range / compare_columns cases: density 0, one contiguous run of full blocks (1 %), a
    random 10 % (every block keeps something), 100 %"""
    clustered = torch.zeros(n * 32, dtype=torch.int32, device=dev)
    run = max(1, n // 100)
    clustered[(n // 3) * 32:(n // 3 + run) * 32] = -1
    return {"AND density 0": torch.zeros(n * 32, dtype=torch.int32, device=dev), "AND clustered 1 %": clustered,
            "AND random 10 %": random_mask(n, 0.10, 77 + T), "AND density 100 %": torch.full((n * 32,), -1, dtype=torch.int32, device=dev)}


# ---- the mixed-width column of --cases mixed ----------------------------------------------------------------------------------

def as_type(v64, ty):
    """int64 -> T, mod 2^T (the low sizeof(T) bytes of every element)"""
    return v64.view(torch.uint8).view(-1, 8)[:, :ESZ[ty]].contiguous().view(TDT[ty]).reshape(-1)


def mixed_column(ty, gb, placement="separate", width_seed=0, data_seed=0, share=1, refs=None, output=True, bases=False, encode_pair=False):
    """The mixed-width column every FoR case measures on: n blocks of seeded-random widths 1..T-1 (the --gb budget over the unpacked
    1.5 x 128 T bytes per block, split between `share` columns), random packed bytes.  What the case needs beside them:
      refs         "full": random references; "top_clear": their top bit clear (reference + field never wraps, so an encoder finds
                   widths <= the decoder's); None: the case builds its own
      output       `un`, n unpacked blocks
      bases        `bases`, Delta's n * 128 bytes
      encode_pair  the encoders' direction: they read `un_enc` and `bases_enc`, they write `back`
    placement "interleaved": `col` (+ `bases`) and `un` from one constructed pair (fl_column_pair_alloc(FL_LAYOUT_INTERLEAVED): the
    decoders read one class of memory and write the other two), the encoders' buffers from a second one (one pair per DIRECTION);
    anything else: separate tensors, the encoders reading what the decoders wrote.  release_column() is the matching release."""
    T, esz = ESZ[ty] * 8, ESZ[ty]
    c = SimpleNamespace(ty=ty, T=T, esz=esz, pair=None, pair_enc=None)
    c.n = n = max(64, int(gb * 1e9 / (128 * T * 1.5)) // share)
    g = torch.Generator(device=dev); g.manual_seed(31 + T + width_seed)
    c.widths = torch.randint(1, T, (n,), dtype=torch.int64, device=dev, generator=g).to(torch.uint8)
    c.offsets, total = fl.widths_to_offsets(ty, c.widths)
    c.pbytes = pbytes = int(total.item())
    if placement == "interleaved":
        c.pair = pl.ColumnPair(pbytes, n * 128 * T, dev, aux_bytes=n * 128, layout="interleaved")
        if encode_pair:
            c.pair_enc = pl.ColumnPair(n * 128 * T, pbytes, dev, aux_bytes=n * 128, layout="interleaved")
            c.un_enc, c.back = c.pair_enc.input.view(TDT[ty]), c.pair_enc.output.view(TDT[ty])
        c.col, c.un = c.pair.input.view(TDT[ty]), c.pair.output.view(TDT[ty])
        c.col.view(torch.uint8).copy_(rnd(pbytes, 1 + data_seed))
        if bases:
            c.bases = c.pair.aux.view(TDT[ty])
            c.bases.view(torch.uint8).copy_(rnd(n * 128, 3))
        if encode_pair:
            c.bases_enc = c.pair_enc.aux.view(TDT[ty])
            c.bases_enc.copy_(c.bases)
    else:
        c.col = rnd(pbytes, 1 + data_seed).view(TDT[ty])
        if bases:
            c.bases = rnd(n * 128, 3).view(TDT[ty])
        if output:
            c.un = torch.empty(n * 1024, dtype=TDT[ty], device=dev)
        if encode_pair:
            c.back = torch.empty_like(c.col)
            c.un_enc, c.bases_enc = c.un, c.bases
    if refs is not None:
        r64 = rnd(n * 8, 2).view(torch.int64)
        c.refs = as_type(r64 & ((1 << (T - 1)) - 1) if refs == "top_clear" else r64, ty)
    return c


def release_column(c):
    """drops every tensor of a mixed_column, frees its constructed pairs, hands the memory back to the device"""
    pairs = [p for p in (c.pair, c.pair_enc) if p is not None]
    c.__dict__.clear()
    for p in pairs:
        p.free()
    torch.cuda.empty_cache()


def mixed_columns(args, **needs):
    """one mixed_column per chosen type, its constructed pairs' classes on a line of their own, released when the caller asks for the
    next one (after the `del` of its own tensors)"""
    for ty in chosen_types(args):
        c = mixed_column(ty, args.gb, **needs)
        if c.pair_enc is not None:
            print(f"# {ty}: constructed pairs, measured classes (input + bases first): decode {c.pair.classes} | encode {c.pair_enc.classes}", flush=True)
        elif c.pair is not None:
            print(f"# {ty}: constructed pair, measured classes (input first): {c.pair.classes}", flush=True)
        yield c
        release_column(c)


def undecided_refs(k, x64, widths):
    """int64 references k - 1 - (x mod (2^W - 1)): every block's range [r, r + 2^W - 1] holds k - 1 and k, so `x < k` decides none"""
    return (k - 1) - x64 % ((torch.ones_like(x64) << widths.to(torch.int64)) - 1)


def bare_stream_shape(lib, code, T, w):
    """fl_internal_bare_stream_shape as plain ints (in / aux / out bytes per unit, threads, waves, window, blocks per unit), or None"""
    Z, I = ctypes.c_size_t, ctypes.c_int
    v = (Z(), Z(), Z(), I(), I(), I(), ctypes.c_uint())
    if lib.fl_internal_bare_stream_shape(code, T, w, *[ctypes.byref(x) for x in v]) != 0:
        return None
    return SimpleNamespace(**{k: x.value for k, x in zip(("iu", "au", "ou", "nt", "wv", "wn", "bpu"), v)})


# ---- the uniform-width rows: quick / orig / consume / fused / allwidths / widths ---------------------------------------------

def bytes_per_block(op, ty, w):
    T = ESZ[ty] * 8
    if op in ("pack", "unpack", "for_pack", "unfor_pack"):
        return 128 * w + 128 * T
    if op in ("undelta_pack", "undelta_pack_untranspose", "transpose_delta_pack"):
        return 128 * w + 128 + 128 * T
    if op == "unpack_block_sums":
        return 128 * w + 8
    if op == "unpack_compare":
        return 128 * w + 128
    if op == "block_min_max":
        return 128 * T + 2 * ESZ[ty]
    if op in ("delta", "undelta"):
        return 2 * 128 * T + 128
    return 2 * 128 * T  # transpose / untranspose


SLAB = {"t": None, "classes": None, "map": ""}


def the_slab(nbytes):
    """ONE allocation for the whole sweep, made before anything else and never freed: freeing and re-allocating per case hands the
    cases alternately a fresh and a fragmented piece of the device memory (the class maps of profiles/r03_sweep_consume.txt
    alternated between AAAABBBBBBBBACCC and ABBCAABCAACCCBCC), which showed up as every second row of a sweep being 5-8 % low --
    undelta against delta, untranspose against transpose.  The memory classes of its 8-GiB granules are measured once."""
    if SLAB["t"] is None or SLAB["t"].numel() < nbytes:
        SLAB["t"] = None
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(dev)
        want = max(nbytes, 160 << 30)
        size = min(want, free - (24 << 30)) // pl.GRANULE_BYTES * pl.GRANULE_BYTES
        if size < nbytes:
            return None
        SLAB["t"] = torch.empty(size, dtype=torch.uint8, device=dev)
        SLAB["classes"] = pl.granule_classes(SLAB["t"])
        SLAB["map"] = "".join("." if c is None else "ABC"[c] for c in SLAB["classes"][0])
        print(f"# one {size >> 30}-GiB allocation for every row; memory class of its 8-GiB granules: {SLAB['map']}", flush=True)
    return SLAB["t"]


def run(op, ty, w, args):
    """One op on one column.  The column's input and output are carved from the sweep's ONE allocation (the_slab): for the
    materialising kernels the input at offset 0 and the output centred on the first 64-GiB multiple behind it (where a fresh
    allocation's first boundary between memory classes lies: fastlanes_amd/placement.py); for the fused consumers the input in a
    run of 8-GiB granules of one class and the thin output in a granule of another, by the measured class map.  Separately
    allocated tensors share a class or not at the driver's whim, which moved every row of rounds 1-2 by up to 8 %;
    --placement separate restores that."""
    reps = args.reps
    T = ESZ[ty] * 8
    esz = ESZ[ty]
    bpb = bytes_per_block(op, ty, w)
    n = max(32, int(args.gb * 1e9 / bpb))
    packed_in = op in ("unpack", "unfor_pack", "undelta_pack", "unpack_block_sums", "unpack_compare", "undelta_pack_untranspose")
    in_bytes = n * 128 * w if packed_in else n * 128 * T
    out_bytes = {"pack": n * 128 * w, "for_pack": n * 128 * w, "transpose_delta_pack": n * 128 * w, "unpack_block_sums": n * 8,
                 "unpack_compare": n * 128, "block_min_max": 2 * n * esz}.get(op, n * 128 * T)
    aux_bytes = n * 128 + n * esz          # Delta bases, then FoR references
    lib = fl.load()
    placed = ""
    consumer = op in ("unpack_block_sums", "unpack_compare", "block_min_max")
    total = None
    if args.placement == "zoned":
        try:
            i_off, a_off, o_off, total = pl._layout(in_bytes, out_bytes, aux_bytes)
        except ValueError:
            total = None
    slab = the_slab(max(total, (in_bytes // pl.GRANULE_BYTES + 3) * pl.GRANULE_BYTES)) if total is not None else None
    pair = None
    if args.placement == "interleaved" and not consumer:
        # a CONSTRUCTED pair per row (fl_column_pair_alloc(FL_LAYOUT_INTERLEAVED): the input + aux inside one class of memory, the output
        # rotating through the others by position); the library keeps the 1-GiB chunks between rows (fl_internal_pair_chunk_cache)
        lib.fl_internal_pair_chunk_cache(96)
        pair = pl.ColumnPair(in_bytes, out_bytes, dev, aux_bytes=aux_bytes, layout="interleaved")
        src8, aux8, dst8 = pair.input, pair.aux, pair.output
        placed = f"constructed pair {pair.classes}"
    elif slab is not None and consumer and out_bytes <= pl.GRANULE_BYTES - (1 << 30):
        # a thin write stream: input in a run of granules of one memory class, output in a granule of another (classes measured once
        # on the sweep's slab: fastlanes_amd/placement.py)
        cls, rates = SLAB["classes"]
        k = max(1, (in_bytes + pl.GRANULE_BYTES - 1) // pl.GRANULE_BYTES)
        start, best, one_class = pl.choose_granules(cls, rates, k)
        src8 = slab[start * pl.GRANULE_BYTES:][:in_bytes]
        dst8 = slab[best * pl.GRANULE_BYTES:][:out_bytes]
        aux8 = slab[:0]
        placed = f"input from granule {start}{'' if one_class else ' (SPANS classes)'}, output in {best} of {SLAB['map']}"
    elif slab is not None:
        src8, aux8, dst8 = slab[i_off:i_off + in_bytes], slab[a_off:a_off + aux_bytes], slab[o_off:o_off + out_bytes]
    else:
        src8 = torch.empty(in_bytes, dtype=torch.uint8, device=dev)
        aux8 = torch.empty(aux_bytes, dtype=torch.uint8, device=dev)
        dst8 = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    for t, seed in ((src8, 1), (aux8, 3)):
        if t.numel() & ~7:
            assert lib.fl_fill_random(t.data_ptr(), t.numel() & ~7, seed, None) == 0
    src = src8.view(TDT[ty])
    dst = dst8[:(out_bytes // esz) * esz].view(TDT[ty]) if op not in ("unpack_block_sums", "unpack_compare", "block_min_max") else None
    bases = aux8[:n * 128].view(TDT[ty]) if aux8.numel() else None
    refs = aux8[n * 128:n * 128 + n * esz].view(TDT[ty]) if aux8.numel() else None
    if op == "pack":
        f = lambda: fl.BitPacking.pack(w, src, output=dst)
    elif op == "unpack":
        f = lambda: fl.BitPacking.unpack(w, src, output=dst)
    elif op == "for_pack":
        f = lambda: fl.FoR.for_pack(w, src, refs, output=dst)
    elif op == "unfor_pack":
        f = lambda: fl.FoR.unfor_pack(w, src, refs, output=dst)
    elif op == "undelta_pack":
        f = lambda: fl.Delta.undelta_pack(w, src, bases, output=dst)
    elif op == "unpack_block_sums":
        sums = dst8[:n * 8].view(torch.int64)
        f = lambda: fl.BitPacking.unpack_block_sums(w, src, output=sums)
    elif op == "unpack_compare":
        # the mask is a thin WRITE stream inside a read stream: sharing a region of the device memory with the packed input costs
        # it 10-15 % (profiles/exp_thin_stream_r03.txt); placed like every other output (fastlanes_amd/placement.py)
        mask = dst8[:n * 128].view(torch.int32)
        f = lambda: fl.BitPacking.unpack_compare(w, src, "<", (1 << w) // 2, output=mask)
    elif op == "block_min_max":
        mm = (dst8[:n * esz].view(TDT[ty]), dst8[n * esz:2 * n * esz].view(TDT[ty]))
        f = lambda: fl.BitPacking.block_min_max(src, output=mm)
    elif op == "undelta_pack_untranspose":
        f = lambda: fl.Delta.undelta_pack_untranspose(w, src, bases, output=dst)
    elif op == "transpose_delta_pack":
        f = lambda: fl.Delta.transpose_delta_pack(w, src, bases, output=dst)
    elif op in ("delta", "undelta"):
        g = getattr(fl.Delta, op)
        f = lambda: g(src, bases, output=dst)
    else:
        g = getattr(fl.Transpose, op)
        f = lambda: g(src, output=dst)
    med = median(timed(f, reps))
    gbps = n * bpb / med / 1e6
    if args.window_ab:
        # the same buffers under the whole-column tile map of rounds 1-3 (window 31) and under 2^16-block windows, whatever the
        # library's own choice for this kernel is (fl_tile_map.hpp: xcd_tile), round-robin
        big = {"u64": 20, "u32": 21, "u16": 22, "u8": 23}[ty]            # 8 GiB of unpacked blocks per window
        alt = {31: [], 16: [], big: []}
        for _ in range(reps):
            for wnd in alt:
                lib.fl_internal_set_kernel_policy(wnd << 25)
                alt[wnd].append(event_ms(f))
        lib.fl_internal_set_kernel_policy(0)
        placed = (placed + " " if placed else "") + "whole-column map %.3f, 2^16-block windows %.3f, 8-GiB windows %.3f" % tuple(
            of_peak(n * bpb, median(alt[k])) for k in (31, 16, big))
    bare = None
    if args.bare and op in ALLWIDTH_OPS:
        # a bare stream of the same bytes per wavefront, same cache policy / occupancy / tile map as the kernel the dispatch runs, on the
        # SAME buffers (fl_internal_bare_stream; it overwrites the output, which nothing reads afterwards)
        code = 1 if op in ("pack", "for_pack", "transpose_delta_pack") else 2 if op.startswith("undelta_pack") else 0
        s = bare_stream_shape(lib, code, T, w)
        if s is not None:
            if op == "transpose_delta_pack":              # pack's shape plus the bases on the read side
                s.au = 128 * s.bpu
            nu = n // s.bpu
            if pair is not None and pair.classes:
                s.wn = 31                                  # inside a constructed pair the library launches under the whole-column tile map
            g = lambda: lib.fl_internal_bare_stream(src8.data_ptr(), s.iu, aux8.data_ptr() if s.au else None, s.au, dst8.data_ptr(), s.ou, nu,
                                                    s.nt, s.wv, s.wn, None)
            bare = nu * (s.iu + s.au + s.ou) / median(timed(g, reps)) / 1e6
    if pair is not None:
        src = dst = bases = refs = src8 = aux8 = dst8 = None
        del f
        pair.free()
    return {"op": op, "ty": ty, "w": w, "n_blocks": n, "ms": round(med, 4), "GBps": round(gbps, 1),
            "frac": round(gbps / PEAK_GBPS, 4), "Gints": round(n * 1024 / med / 1e6, 1), "placed": placed,
            "bare_GBps": round(bare, 1) if bare else None, "of_bare": round(gbps / bare, 4) if bare else None}


def rows_quick():
    rows = [("unpack", "u32", 7), ("pack", "u32", 7), ("unfor_pack", "u32", 7), ("for_pack", "u32", 7),
            ("undelta_pack", "u32", 12), ("unpack", "u64", 17), ("pack", "u64", 17),
            ("unpack", "u16", 3), ("pack", "u16", 3), ("unpack", "u8", 3), ("pack", "u8", 3),
            ("undelta_pack", "u16", 9), ("undelta_pack", "u64", 20), ("undelta_pack", "u8", 4)]
    for ty in ESZ:
        rows += [(op, ty, 0) for op in ("delta", "undelta", "transpose", "untranspose")]
    return rows


def rows_orig():
    return [(op, ty, 0) for ty in ESZ for op in ("transpose", "untranspose")] + [
        ("undelta_pack_untranspose", "u32", 12), ("undelta_pack_untranspose", "u64", 20),
        ("undelta_pack_untranspose", "u16", 9), ("undelta_pack_untranspose", "u8", 4),
        ("transpose_delta_pack", "u32", 12), ("transpose_delta_pack", "u64", 20),
        ("transpose_delta_pack", "u16", 9), ("transpose_delta_pack", "u8", 4)]


def rows_consume():
    return [("unpack_compare", "u32", 7), ("unpack_compare", "u32", 20), ("unpack_compare", "u64", 17),
            ("unpack_compare", "u16", 3), ("unpack_compare", "u8", 3),
            ("unpack_block_sums", "u32", 7), ("unpack_block_sums", "u32", 20), ("unpack_block_sums", "u64", 17),
            ("unpack_block_sums", "u16", 3), ("unpack_block_sums", "u8", 3),
            ("block_min_max", "u32", 0), ("block_min_max", "u64", 0), ("block_min_max", "u16", 0), ("block_min_max", "u8", 0)]


def rows_fused():
    return [("undelta_pack", "u32", 12), ("undelta_pack_untranspose", "u32", 12), ("transpose_delta_pack", "u32", 12),
            ("undelta_pack_untranspose", "u64", 20), ("transpose_delta_pack", "u64", 20),
            ("undelta_pack_untranspose", "u16", 9), ("transpose_delta_pack", "u16", 9),
            ("undelta_pack_untranspose", "u8", 4), ("transpose_delta_pack", "u8", 4)]


def rows_allwidths():
    """EVERY (T, W) x {unpack, pack, FoR's two bodies, undelta_pack, the two fused transpose extensions} through the automatic dispatch
    (the `match width` of bitpacking.rs:82-95 that every W must serve), one slab, class map printed; summarised per (op, T) at the end"""
    return [(op, ty, w) for ty in ESZ for w in range(1, ESZ[ty] * 8 + 1) for op in ALLWIDTH_OPS]


def rows_widths():
    rows = []
    for ty in ESZ:
        T = ESZ[ty] * 8
        for w in sorted({1, 2, 3, T // 4, T // 2, T - 1, T}):
            rows += [("unpack", ty, w), ("pack", ty, w)]
    return rows


def format_run_row(r, wide=False):
    """one (op, type, width) line; wide: the allwidths column for the op's name"""
    return (f"{r['op']:{24 if wide else 13}s} {r['ty']:4s} W={r['w']:<3d} n={r['n_blocks']:>9d} {r['ms']:9.4f} ms {r['GBps']:8.1f} GB/s {r['frac']:.3f} "
            f"{r['Gints']:8.1f} Gint/s" + (f"   bare stream {r['bare_GBps']:7.1f} GB/s -> {r['of_bare']:.3f} of it" if r.get("of_bare") else "") +
            (f"   [{r['placed']}]" if r.get("placed") else ""))


def allwidths_summary(out):
    """the lines behind an allwidths run's rows: min / median / max per (op, type), the slowest rows, the rows furthest below their bare stream"""
    lines = ["# ---- summary: fraction of the 8 TB/s peak per (op, type) over all widths 1..T: min (at W) / median / max (at W)"]
    for op in ALLWIDTH_OPS:
        for ty in ESZ:
            rows = sorted((r["frac"], r["w"]) for r in out if r["op"] == op and r["ty"] == ty)
            if not rows:
                continue
            ob = sorted((r["of_bare"], r["w"]) for r in out if r["op"] == op and r["ty"] == ty and r.get("of_bare"))
            lines.append(f"# {op:24s} {ty:4s} min {rows[0][0]:.3f} (W={rows[0][1]:<2d})  median {rows[len(rows) // 2][0]:.3f}  max {rows[-1][0]:.3f} (W={rows[-1][1]:<2d})" +
                         (f"   | of the bare stream of the same bytes on the same buffers: min {ob[0][0]:.3f} (W={ob[0][1]:<2d})  median {ob[len(ob) // 2][0]:.3f}" if ob else ""))
    worst = sorted(out, key=lambda r: r["frac"])[:8]
    lines.append("# ---- the eight slowest (op, T, W): " + "; ".join(f"{r['op']} {r['ty']} W={r['w']} {r['frac']:.3f}" + (f" ({r['of_bare']:.2f} of its bare stream)" if r.get("of_bare") else "") for r in worst))
    wb = sorted((r for r in out if r.get("of_bare")), key=lambda r: r["of_bare"])[:8]
    lines.append("# ---- the eight furthest below their own bare stream: " + "; ".join(f"{r['op']} {r['ty']} W={r['w']} {r['of_bare']:.3f} (frac {r['frac']:.3f})" for r in wb))
    return lines


def run_rows(rows, args):
    """the shared tail of the row cases: --types / --wmin / --wmax, one run() and one line per row, the allwidths summary, --json"""
    if args.types:
        rows = [c for c in rows if c[1] in args.types.split(",")]
    rows = [c for c in rows if args.wmin <= c[2] <= args.wmax]
    out = []
    for op, ty, w in rows:
        out.append(run(op, ty, w, args))
        print(format_run_row(out[-1], wide=args.cases == "allwidths"), flush=True)
        torch.cuda.empty_cache()
    if args.cases == "allwidths":
        print("\n".join(allwidths_summary(out)))
    if args.json:
        json.dump(out, open(args.json, "w"), indent=1)


# ---- one function per remaining case --------------------------------------------------------------------------------------------

def case_host(args, reps=3):
    """PCIe-inclusive rate of the host-pointer tier (numpy in -> numpy out, staged through HBM)."""
    n = 65536
    pk = np.random.default_rng(1).integers(0, 2**32, size=n * 224, dtype=np.uint32)
    fl.BitPacking.unpack(7, pk)
    best = min((lambda t0: (fl.BitPacking.unpack(7, pk), time.perf_counter() - t0)[1])(time.perf_counter()) for _ in range(reps))
    print(f"host tier unpack u32 W=7 n={n}: {best * 1e3:.2f} ms  {n * 1024 / best / 1e9:.2f} Gint/s "
          f"({n * 4992 / best / 1e9:.2f} GB/s over PCIe incl. hipMalloc/hipFree and pageable copies)", flush=True)


def case_small(args):
    """launch-bound regime: one call per small array (e.g. a 64 Ki-value chunk = 64 blocks); then the same loop as a HIP GRAPH (1000
    chunks of 64 blocks, one captured launch each, replayed) next to the batch entry that decodes the same 1000 chunks in ONE launch:
    what capturing a launch-bound caller loop buys, and what the batch entry buys"""
    for nb in (1, 8, 64, 512, 4096, 32768, 262144):
        pk = rnd(nb * 896, 1).view(torch.uint32)
        out = torch.empty(nb * 1024, dtype=torch.uint32, device=dev)
        us = per_call_us(lambda: fl.BitPacking.unpack(7, pk, output=out), 200)
        print(f"unpack u32 W=7 n_blocks={nb:>7d}: {us:9.2f} us per call (back-to-back on one stream)  "
              f"{nb * 1024 / us / 1e3:9.2f} Gint/s  {nb * 4992 / us / 1e3:8.1f} GB/s", flush=True)
    n_arr, nb = 1000, 64
    pk_all = rnd(n_arr * nb * 896, 1).view(torch.uint32)
    un_all = torch.empty(n_arr * nb * 1024, dtype=torch.uint32, device=dev)
    chunks = [pk_all[a * nb * 224:(a + 1) * nb * 224] for a in range(n_arr)]
    outs = [un_all[a * nb * 1024:(a + 1) * nb * 1024] for a in range(n_arr)]
    lib = fl.load()
    side = torch.cuda.Stream()

    def loop(stream_handle):
        for c, o in zip(chunks, outs):
            assert lib.fl_u32_unpack(7, c.data_ptr(), o.data_ptr(), nb, stream_handle) == 0

    with torch.cuda.stream(side):
        direct = median(timed(lambda: loop(ctypes.c_void_p(side.cuda_stream)), 20, warmup=1))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            loop(ctypes.c_void_p(side.cuda_stream))
        graph = median(timed(g.replay, 20, warmup=1))
        batch = fl.Batch(chunks, outs, [7] * n_arr)
        one = median(timed(lambda: batch.unpack(), 20, warmup=1))
    for name, ms in (("one C-ABI call per chunk", direct), ("the same 1000 calls captured in a HIP graph, replayed", graph), ("fl_u32_unpack_batch: ONE launch", one)):
        print(f"1000 chunks x 64 blocks, unpack u32 W=7, {name:56s}: {ms * 1e3:9.1f} us  {ms * 1e3 / n_arr:7.3f} us per chunk  "
              f"{n_arr * nb * 1024 / ms / 1e6:8.1f} Gint/s", flush=True)


def case_batch(args):
    """many small arrays per launch (fl_<ty>_unpack_batch / _pack_batch) next to one device-tier call per array: 10 000 chunks of
    64 blocks (64 Ki values, the chunk size of the callers SURVEY.md 8(b) names).  Batch, the contiguous yardstick and every
    --batch-policies shape are timed round-robin after three untimed rounds.  --batch-all: every type, the pack direction, and at the
    end Delta's fused decode over the same shape (fl_<ty>_undelta_pack_batch) against the same blocks as one contiguous call."""
    lib = fl.load()
    pols = [int(x, 0) for x in args.batch_policies.split(",")] if args.batch_policies else []
    cases = [("u32", 7, "unpack"), ("u32", 12, "unpack"), ("u32", 20, "unpack")]
    if args.batch_all:
        cases += [("u32", 7, "pack"), ("u32", 20, "pack"), ("u64", 17, "unpack"), ("u64", 17, "pack"), ("u16", 9, "unpack"),
                  ("u16", 9, "pack"), ("u8", 3, "unpack"), ("u8", 3, "pack"), ("u32", 12, "undelta_pack"), ("u16", 9, "undelta_pack"),
                  ("u64", 20, "undelta_pack")]
    for ty, w, op in cases:
        delta = op == "undelta_pack"
        n_arr, nb = 10000, 64
        esz, T = ESZ[ty], ESZ[ty] * 8
        L = 1024 // T
        ppb, opb = nb * 1024 * w // T, nb * 1024
        pk_all = rnd(n_arr * ppb * esz, 1).view(TDT[ty])
        bs_all = rnd(n_arr * nb * 128, 3).view(TDT[ty]) if delta else None
        un_all = (rnd(n_arr * opb * esz, 2) if op == "pack" else torch.empty(n_arr * opb * esz, dtype=torch.uint8, device=dev)).view(TDT[ty])
        if op == "pack":
            pk_all = torch.empty_like(pk_all)
        written = pk_all if op == "pack" else un_all
        packed = [pk_all[a * ppb:(a + 1) * ppb] for a in range(n_arr)]
        bases = [bs_all[a * nb * L:(a + 1) * nb * L] for a in range(n_arr)] if delta else None
        outs = [un_all[a * opb:(a + 1) * opb] for a in range(n_arr)]
        batch = fl.Batch(packed, outs, [w] * n_arr, bases=bases)
        run_batch = getattr(batch, op)

        def with_policy(pol):
            def f():
                lib.fl_internal_set_kernel_policy(pol)
                run_batch()
                lib.fl_internal_set_kernel_policy(0)
            return f
        # the yardstick: the same 640 000 blocks as ONE contiguous column through fl_<ty>_unpack / _pack / _undelta_pack, same buffers
        one = {"unpack": lambda: fl.BitPacking.unpack(w, pk_all, output=un_all), "pack": lambda: fl.BitPacking.pack(w, un_all, output=pk_all),
               "undelta_pack": lambda: fl.Delta.undelta_pack(w, pk_all, bs_all, output=un_all)}[op]
        shapes = [] if delta else pols
        variants = {"batch": run_batch, "contiguous": one}
        variants.update({pol: with_policy(pol) for pol in shapes})
        med = medians(round_robin(variants, max(args.reps, 15), warmup=3))
        t, tc = med["batch"], med["contiguous"]
        nbytes = n_arr * nb * (128 * w + 128 * T + (128 if delta else 0))
        for pol in shapes:
            # A/B of the batch kernel's launch shape on the same buffers (fastlanes_amd_internal.h: policy = 2 + 256 * waves/SIMD
            # + 65536 * blocks per wavefront + 2^24 * prefetch)
            print(f"    policy waves={(pol >> 8) & 255} blocks/wave={(pol >> 16) & 255} prefetch={pol >> 24}: {med[pol]:8.4f} ms  "
                  f"{of_peak(nbytes, med[pol]):.3f} of peak", flush=True)
        one()
        want = written.clone()
        written.zero_()
        run_batch()
        same = torch.equal(want.view(torch.uint8), written.view(torch.uint8))
        row = (f"{op}_batch {ty} W={w}: {n_arr} arrays x {nb} blocks in one launch {t:8.4f} ms  {n_arr * nb * 1024 / t / 1e6:7.1f} Gint/s  "
               f"{nbytes / t / 1e6:7.1f} GB/s ({of_peak(nbytes, t):.3f} of peak)  {'== one big ' + op if same else 'MISMATCH'} | "
               f"the same blocks as one contiguous column, one call: {tc:8.4f} ms ({(t / tc - 1) * 100:+.1f} %)")
        if not delta:
            # the same arrays as one call each (what a chunk-at-a-time caller does today), through the raw C ABI: one event pair, no warm-up
            f = getattr(lib, f"fl_{ty}_{op}")
            ptrs = [((p.data_ptr(), o.data_ptr()) if op == "unpack" else (o.data_ptr(), p.data_ptr())) for p, o in zip(packed, outs)]

            def one_call_each():
                for src, dst in ptrs:
                    f(w, src, dst, nb, None)
            t1 = timed(one_call_each, 1, warmup=0)[0]
            row += f" | one call per array: {t1:8.3f} ms  {n_arr * nb * 1024 / t1 / 1e6:7.1f} Gint/s  (x{t1 / t:.1f})"
        print(row, flush=True)
        del batch, pk_all, bs_all, un_all, written, want, packed, bases, outs


def case_refbench(args):
    """What the reference's own criterion benches time (besides benches/bitpacking.rs, which bench.py's headline and cpu_baseline
    cover):
      benches/delta.rs:10-44      fused undelta_pack::<W> vs unpack::<W> followed by undelta (u16 W=9), one block
      benches/transpose.rs:8-19   transpose of one u16 block
    here batched over a column (HBM-resident, GB/s of algorithmic bytes; three untimed calls first) and as ONE-BLOCK device-tier
    calls (us per back-to-back call of 300: launch-bound, the shape of the reference's bench)."""
    for ty, w in (("u16", 9), ("u32", 12)):
        T = ESZ[ty] * 8
        n = int(args.gb * 1e9 / (128 * w + 128 + 2 * 128 * T))
        pk = rnd(n * 128 * w, 1).view(TDT[ty])
        bases = rnd(n * 128, 3).view(TDT[ty])
        out = torch.empty(n * 1024, dtype=TDT[ty], device=dev)
        tmp = torch.empty(n * 1024, dtype=TDT[ty], device=dev)
        fused = median(timed(lambda: fl.Delta.undelta_pack(w, pk, bases, output=out), args.reps, warmup=3))
        want = out.clone()

        def unfused():
            fl.BitPacking.unpack(w, pk, output=tmp)
            fl.Delta.undelta(tmp, bases, output=out)
        unf = median(timed(unfused, args.reps, warmup=3))
        same = torch.equal(want.view(torch.uint8), out.view(torch.uint8))
        alg = n * (128 * w + 128 + 128 * T)
        print(f"benches/delta.rs shape, {ty} W={w}, {n} blocks: fused undelta_pack {fused:8.4f} ms ({alg / fused / 1e6:7.1f} GB/s, "
              f"{n * 1024 / fused / 1e6:7.1f} Gint/s)  unpack + undelta {unf:8.4f} ms ({n * 1024 / unf / 1e6:7.1f} Gint/s)  "
              f"speed-up {unf / fused:.2f}x  results {'identical' if same else 'DIFFER'}", flush=True)
        pk1, b1, o1, t1 = pk[:128 * w // ESZ[ty]], bases[:128 // ESZ[ty]], out[:1024], tmp[:1024]
        f1 = per_call_us(lambda: fl.Delta.undelta_pack(w, pk1, b1, output=o1), 300)

        def unfused1():
            fl.BitPacking.unpack(w, pk1, output=t1)
            fl.Delta.undelta(t1, b1, output=o1)
        u1 = per_call_us(unfused1, 300)
        print(f"    one block, device tier: fused {f1:6.2f} us per call, unpack + undelta {u1:6.2f} us  (speed-up {u1 / f1:.2f}x; launch-bound)", flush=True)
        del pk, bases, out, tmp, want
        torch.cuda.empty_cache()
    for ty in ("u16",):
        T = ESZ[ty] * 8
        n = int(args.gb * 1e9 / (2 * 128 * T))
        src = rnd(n * 128 * T, 1).view(TDT[ty])
        dst = torch.empty_like(src)
        for name, g in (("transpose", fl.Transpose.transpose), ("untranspose", fl.Transpose.untranspose)):
            ms = median(timed(lambda: g(src, output=dst), args.reps, warmup=3))
            s1, d1 = src[:1024], dst[:1024]
            us = per_call_us(lambda: g(s1, output=d1), 300)
            print(f"benches/transpose.rs shape, {name} {ty}: {n} blocks {ms:8.4f} ms ({n * 2 * 128 * T / ms / 1e6:7.1f} GB/s, "
                  f"{n * 1024 / ms / 1e6:7.1f} Gint/s); one block, device tier: {us:6.2f} us per call", flush=True)


def format_mixed_row(name, ty, n, med, nbytes, tail=""):
    return (f"{name:32s} {ty:4s} n={n:>9d} {med:9.4f} ms {nbytes / med / 1e6:8.1f} GB/s {of_peak(nbytes, med):.3f} "
            f"{n * 1024 / med / 1e6:8.1f} Gint/s{tail}")


def lt_decided(w_host, r_host, k):
    """the blocks `x < k` decides from (reference, width) alone -- fl_for_decide.hpp's rule with a = 0, s = k - 1, c = r"""
    r = r_host.astype(object)
    return np.array([int(x) + (1 << int(w)) - 1 <= k - 1 or int(x) >= k for x, w in zip(r, w_host)], dtype=bool)


def case_mixed(args):
    """FoR's and Delta's bodies over device-resident mixed-width columns (fl_<ty>_unfor_pack_widths, ..) next to plain
    unpack_widths / pack_widths of the same column, and an encoder's whole chain: block_min_max -> for_widths ->
    widths_to_offsets -> for_pack_widths (two passes over the values).  Widths seeded-random in 1..T-1, separate tensors.
    unfor_compare_widths rows (selection masks from the FoR-packed column; bytes per block 1 + 8 + sizeof(T) + 128 of metadata and
    mask, plus the 128 * W packed bytes of every UNDECIDED block): an undecided predicate (every block's value range straddles
    the constant), and `x < k` at the 1 % quantile of an ascending column encoded by the library's own chain -- mostly decided from
    the blocks' metadata -- with unfor_pack_widths of that column as its yardstick.  Each row prints its decided share."""
    keep = re.compile(args.rows) if args.rows else None
    wanted = lambda name: not keep or keep.search(name)

    def time_row(c, name, nbytes, f, tail=""):
        """a row of no bytes is run (twice) and not timed"""
        if wanted(name):
            ms = timed(f, args.reps if nbytes else 0)
            if ms:
                print(format_mixed_row(name, c.ty, c.n, median(ms), nbytes, tail), flush=True)

    for c in mixed_columns(args, placement=args.placement, refs="top_clear", bases=True, encode_pair=True):
        ty, T, esz, n = c.ty, c.T, c.esz, c.n
        mm = (torch.empty(n, dtype=TDT[ty], device=dev), torch.empty(n, dtype=TDT[ty], device=dev))
        fl.unfor_pack_widths(c.widths, c.offsets, c.col, c.refs, output=c.un_enc)       # the values every encoder row below reads

        def encoder_chain():
            lo, hi = fl.BitPacking.block_min_max(c.un_enc, output=mm)
            w2 = fl.for_widths(lo, hi)
            o2, _ = fl.widths_to_offsets(ty, w2)
            fl.for_pack_widths(w2, o2, c.un_enc, lo, c.back, check=False)

        two_sided = c.pbytes + n * 128 * T
        rows = (
            ("unpack_widths", two_sided, lambda: fl.unpack_widths(c.widths, c.offsets, c.col, output=c.un, check=False)),
            ("unfor_pack_widths", two_sided, lambda: fl.unfor_pack_widths(c.widths, c.offsets, c.col, c.refs, output=c.un, check=False)),
            ("undelta_pack_widths", two_sided + n * 128, lambda: fl.undelta_pack_widths(c.widths, c.offsets, c.col, c.bases, output=c.un, check=False)),
            ("undelta_pack_untranspose_widths", two_sided + n * 128,
             lambda: fl.undelta_pack_widths(c.widths, c.offsets, c.col, c.bases, output=c.un, check=False, untranspose=True)),
            ("restore", 0, lambda: fl.unfor_pack_widths(c.widths, c.offsets, c.col, c.refs, output=c.un_enc, check=False)),
            ("pack_widths", two_sided, lambda: fl.pack_widths(c.widths, c.offsets, c.un_enc, c.back, check=False)),
            ("for_pack_widths", two_sided, lambda: fl.for_pack_widths(c.widths, c.offsets, c.un_enc, c.refs, c.back, check=False)),
            ("transpose_delta_pack_widths", two_sided + n * 128, lambda: fl.transpose_delta_pack_widths(c.widths, c.offsets, c.un_enc, c.bases_enc, c.back, check=False)),
            ("FoR encoder chain (4 launches)", 2 * n * 128 * T + c.pbytes, encoder_chain),
        )
        for name, nbytes, f in rows:
            time_row(c, name, nbytes, f)
        meta = 1 + 8 + esz + 128
        w_host = c.widths.cpu().numpy()
        mask = torch.empty(n * 32, dtype=torch.int32, device=dev)
        if wanted("unfor_compare_widths undecided"):
            # references k - 1 - (x mod (2^W - 1)): every block's range [r, r + 2^W - 1] holds k - 1 and k, so `x < k` decides none
            k = 1 << (T - 1)
            x = np.random.default_rng(5).integers(0, 1 << 62, size=n, dtype=np.uint64)
            und = np.array([(k - 1 - int(v) % ((1 << int(w)) - 1)) % (1 << T) for v, w in zip(x, w_host)], dtype=np.uint64)
            refs_und = torch.from_numpy(und.astype(NPDT[ty])).to(dev)
            dec = lt_decided(w_host, und, k)
            nbytes = n * meta + int((128 * w_host.astype(np.int64))[~dec].sum())
            time_row(c, "unfor_compare_widths undecided", nbytes,
                     lambda: fl.unfor_compare_widths(c.widths, c.offsets, c.col, refs_und, "<", k, output=mask, check=False),
                     f"  decided {dec.mean():.3f}")
        if wanted("unfor_pack_widths ascending") or wanted("unfor_compare_widths ascending <1%"):
            # an ascending column through the library's own encoder chain
            i = torch.arange(n * 1024, dtype=torch.int64, device=dev)
            asc = i * ((1 << T) - 1) // (n * 1024) if T <= 32 else i * 3          # the type's whole range (u64: a slope of 3)
            k1 = int(asc[len(asc) // 100].item())
            asc_v = asc.to(SIGNED[ty]).view(TDT[ty])
            del asc, i
            lo, hi = fl.BitPacking.block_min_max(asc_v)
            w_asc = fl.for_widths(lo, hi)
            o_asc, t_asc = fl.widths_to_offsets(ty, w_asc)
            pk_asc = torch.empty(max(int(t_asc.item()) // esz, 1), dtype=TDT[ty], device=dev)
            fl.for_pack_widths(w_asc, o_asc, asc_v, lo, pk_asc, check=False)
            del asc_v
            wa, la = w_asc.cpu().numpy(), lo.view(torch.uint8).cpu().numpy().view(NPDT[ty])
            dec = lt_decided(wa, la, k1)
            pb = int(t_asc.item())
            time_row(c, "unfor_pack_widths ascending", pb + n * 128 * T, lambda: fl.unfor_pack_widths(w_asc, o_asc, pk_asc, lo, output=c.un, check=False))
            nbytes = n * meta + int((128 * wa.astype(np.int64))[~dec].sum())
            time_row(c, "unfor_compare_widths ascending <1%", nbytes,
                     lambda: fl.unfor_compare_widths(w_asc, o_asc, pk_asc, lo, "<", k1, output=mask, check=False),
                     f"  decided {dec.mean():.3f}")
            del pk_asc, lo, hi, w_asc, o_asc
        del mm, mask


def format_select_row(name, ty, n, kept, nonempty, nbytes, two_sided, ms, med_pack, med_decided):
    sel = median(ms)
    return (f"unfor_select_widths {name:22s} {ty:4s} kept {kept / (n * 1024):7.4f} non-empty {nonempty:6.4f}  {sel:9.4f} ms (min {min(ms):9.4f})  "
            f"{nbytes / sel / 1e6:8.1f} GB/s {of_peak(nbytes, sel):.3f}  {nbytes / n:7.0f} B/block  "
            f"x{sel / med_pack:.3f} of unfor_pack_widths ({med_pack:.4f} ms, {of_peak(two_sided, med_pack):.3f})  "
            f"x{sel / med_decided:.3f} of compare all decided ({med_decided:.4f} ms)")


def format_mask_offsets_row(ty, n, ms):
    return f"    mask_offsets {ty:4s} {median(ms):9.4f} ms (min {min(ms):.4f})  {n * 136 / median(ms) / 1e6:8.1f} GB/s"


def case_select(args):
    """unfor_select_widths (decode only the rows a selection mask keeps) over the mixed-width column of --cases mixed, at random mask
    densities 0 .. 100 % and one clustered mask (one block in 16 non-empty, 50 % inside it).  Two yardsticks, unchanged kernels, are
    timed in the SAME run on the SAME buffers, round-robin with the row under test: unfor_pack_widths of the column (the select's
    output lies at the start of its output buffer) and unfor_compare_widths with every block decided (`x < 0`: metadata-only traffic,
    a 128-byte mask written per block where select reads one).  Algorithmic bytes per block: packed bytes of the NON-EMPTY blocks
    + 128 (mask) + 8 (out_offsets) + kept * sizeof(T).  mask_offsets (three launches) is timed on a line of its own."""
    reps = max(args.reps, 5)
    for c in mixed_columns(args, placement=args.placement, refs="full"):
        ty, T, esz, n = c.ty, c.T, c.esz, c.n
        cmp_mask = torch.empty(n * 32, dtype=torch.int32, device=dev)
        w_host = c.widths.cpu().numpy().astype(np.int64)
        two_sided = c.pbytes + n * 128 * T
        print(f"# {ty}: n = {n} blocks, packed {c.pbytes / 1e9:.2f} GB, unpacked {n * 128 * T / 1e9:.2f} GB, {reps} launches each, round-robin", flush=True)
        rows = [("0", 0.0, 1), ("1/1024", 1 / 1024, 1), ("1 %", 0.01, 1), ("10 %", 0.1, 1), ("50 %", 0.5, 1), ("100 %", 1.0, 1), ("clustered 1/16 x 50 %", 0.5, 16)]
        for name, density, every in rows:
            mask = random_mask(n, density, 77 + T, every)
            oo, tot = fl.mask_offsets(mask)
            kept = int(tot.item())
            starts = oo.cpu().numpy()
            pop = np.diff(np.concatenate([starts, [kept]]))
            nbytes = int((128 * w_host)[pop > 0].sum()) + n * (128 + 8) + kept * esz
            ms = round_robin({
                "select": lambda: fl.unfor_select_widths(c.widths, c.offsets, c.col, c.refs, mask, out_offsets=oo, total=tot, output=c.un, check=False),
                "unfor_pack_widths": lambda: fl.unfor_pack_widths(c.widths, c.offsets, c.col, c.refs, output=c.un, check=False),
                "compare all decided": lambda: fl.unfor_compare_widths(c.widths, c.offsets, c.col, c.refs, "<", 0, output=cmp_mask, check=False),
                "mask_offsets": lambda: fl.mask_offsets(mask),
            }, reps)
            med = medians(ms)
            print(format_select_row(name, ty, n, kept, float((pop > 0).mean()), nbytes, two_sided, ms["select"], med["unfor_pack_widths"],
                                    med["compare all decided"]), flush=True)
            print(format_mask_offsets_row(ty, n, ms["mask_offsets"]), flush=True)
            if density == 0.0:
                for k in ("select", "compare all decided"):
                    print(f"    spread at density 0: {k:20s} min {min(ms[k]):.4f} median {med[k]:.4f} max {max(ms[k]):.4f} ms", flush=True)
            del mask, oo, tot
        del cmp_mask


def format_aggregate_row(name, ty, n, kept, ms):
    return f"unfor_aggregate_widths {name:10s} {ty:4s} kept {kept / (n * 1024):7.4f}  {show(ms)}  {n / median(ms) / 1e6:8.3f} Gblocks/s"


def format_yardstick_row(name, ty, n, ms, of_ms, of_name="aggregate", pad=24):
    """a comparison row under an aggregate / aggregate_by row: its own figures, then the row under test's time as a multiple of its"""
    return f"    {name:{pad}s} {ty:4s} {show(ms)}  {n / median(ms) / 1e6:8.3f} Gblocks/s  {of_name} x{of_ms / median(ms):.3f} of it"


def case_aggregate(args):
    """unfor_aggregate_widths (count / sum / min / max per block under a selection mask) over the mixed-width column of --cases mixed, at
    random mask densities 0 .. 100 % and with no mask.  Three yardsticks are timed in the SAME run on the SAME buffers, round-robin with
    the row under test: (1) a bare stream of the row's own bytes -- the mean packed bytes per block and, with a mask, 128 bytes in,
    32 bytes out -- through fl_internal_bare_stream; (2) unfor_pack_widths of the column (the same packed reads, plus the
    1024 * sizeof(T) bytes per block the aggregate does not write); (3) the composition the aggregate replaces: unfor_select_widths
    (offsets given) followed by a torch sum of the kept values.  Every figure is the median of `reps` launches with their min .. max
    beside it; the device's unique id heads the table.  aggregate_reduce (two launches) is timed on a line of its own, and once more
    at 10 M blocks."""
    lib = fl.load()
    reps = max(args.reps, 5)
    print(device_header(args.placement), flush=True)
    for c in mixed_columns(args, placement=args.placement, refs="full"):
        ty, T, n, pbytes = c.ty, c.T, c.n, c.pbytes
        slots = torch.empty((n, 4), dtype=torch.int64, device=dev)
        agg_fn = getattr(lib, f"fl_{ty}_unfor_aggregate_widths")
        mean_w2 = int(round(2 * float(c.widths.to(torch.float64).mean().item())))
        s = bare_stream_shape(lib, 3, T, mean_w2)
        assert s is not None
        if c.pair is not None and c.pair.classes:
            s.wn = 31                                  # inside a constructed pair the library launches under the whole-column tile map
        nu = n // s.bpu
        # the shape's unit comes from the ROUNDED mean width: never more than the column holds (the stream reads nu units back to back)
        s.iu = min(s.iu, pbytes // nu // 16 * 16)
        assert 0 < s.iu <= 8192 and s.iu * nu <= pbytes and 128 * s.bpu <= 1024 and s.bpu * nu <= n
        print(f"# {ty}: n = {n} blocks, packed {pbytes / 1e9:.2f} GB ({pbytes / n:.1f} B/block), {reps} launches each, round-robin; bare stream: "
              f"{s.iu} B in (+ {128 * s.bpu} B mask) and {32 * s.bpu} B out per unit of {s.bpu} block(s)", flush=True)
        rows = [("empty", 0.0), ("1/1024", 1 / 1024), ("1 %", 0.01), ("50 %", 0.5), ("100 %", 1.0), ("mask=None", None)]
        for name, density in rows:
            mask = None if density is None else random_mask(n, density, 77 + T)
            variants = {
                # the typed kernel alone, through the C ABI; "aggregate call" is the Python call: that launch plus aggregate_reduce's two
                "aggregate": lambda: agg_fn(c.widths.data_ptr(), c.offsets.data_ptr(), c.col.data_ptr(), pbytes, c.refs.data_ptr(), 1,
                                            mask.data_ptr() if mask is not None else None, n, slots.data_ptr(), None, None),
                "aggregate call": lambda: fl.unfor_aggregate_widths(c.widths, c.offsets, c.col, c.refs, mask, block_aggs=slots, check=False),
                "bare": lambda: lib.fl_internal_bare_stream(c.col.data_ptr(), s.iu, mask.data_ptr() if mask is not None else None,
                                                            128 * s.bpu if mask is not None else 0, slots.data_ptr(), 32 * s.bpu, nu,
                                                            s.nt, s.wv, s.wn, None),
                "unfor_pack_widths": lambda: fl.unfor_pack_widths(c.widths, c.offsets, c.col, c.refs, output=c.un, check=False),
                "aggregate_reduce": lambda: fl.aggregate_reduce(slots),
            }
            if mask is not None:
                oo, tot = fl.mask_offsets(mask)
                kept = int(tot.item())
                variants["select + torch sum"] = lambda: fl.unfor_select_widths(c.widths, c.offsets, c.col, c.refs, mask, out_offsets=oo, total=tot, output=c.un,
                                                                                check=False)[:kept].sum(dtype=torch.int64)
            else:
                kept = n * 1024
                variants["unfor_pack + torch sum"] = lambda: fl.unfor_pack_widths(c.widths, c.offsets, c.col, c.refs, output=c.un, check=False).sum(dtype=torch.int64)
            ms = round_robin(variants, reps)
            print(format_aggregate_row(name, ty, n, kept, ms["aggregate"]), flush=True)
            for k in variants:
                if k != "aggregate":
                    print(format_yardstick_row(k, ty, n, ms[k], median(ms["aggregate"])), flush=True)
            del mask, variants
        del slots
    n = 10_000_000
    slots = rnd(n * 32, 5).view(torch.int64).view(n, 4)
    ms = round_robin({"aggregate_reduce": lambda: fl.aggregate_reduce(slots)}, reps)["aggregate_reduce"]
    print(f"aggregate_reduce {n} blocks  {show(ms)}  {n * 32 / median(ms) / 1e6:8.1f} GB/s", flush=True)


def format_aggregate_by_row(ty, kname, mname, n, ms):
    return f"unfor_aggregate_by_widths {ty:4s} keys {kname:10s} mask {mname:9s}  {show(ms)}  {n / median(ms) / 1e6:8.3f} Gblocks/s"


def case_aggregate_by(args):
    """unfor_aggregate_by_widths (count / sum / min / max per u8 key under a selection mask) over the mixed-width column of --cases mixed
    with a u8 key column beside it: 4 groups uniform (key width 2), 256 groups uniform (key width 8), clustered (every key block
    width 0); mask 100 %, 1 % and none.  Two comparison rows are timed in the SAME run on the SAME buffers, round-robin with the row
    under test: (a) unfor_aggregate_widths of the value column plus unfor_pack_widths of the key column -- the same bytes read, no
    grouping; (b) the composition the call replaces: unfor_pack_widths of both columns, then torch bincount / scatter_add /
    scatter_reduce over the decoded rows (the mask already expanded to a bool tensor, outside the timing).  Every figure is the
    median of `reps` launches with their min .. max beside it; the device's unique id heads the table.  Plain tensors whatever
    --placement says."""
    reps = max(args.reps, 5)
    print(device_header(), flush=True)
    for c in mixed_columns(args, refs="full"):
        ty, T, n = c.ty, c.T, c.n
        kun = torch.empty(n * 1024, dtype=torch.uint8, device=dev)
        slots = torch.empty((n, 4), dtype=torch.int64, device=dev)
        result = torch.empty((256, 4), dtype=torch.int64, device=dev)
        krefs_clustered = rnd((n + 7) // 8 * 8, 3).view(torch.uint8)[:n].contiguous()
        kzero = torch.zeros(1, dtype=torch.uint8, device=dev)
        print(f"# {ty}: n = {n} blocks, packed values {c.pbytes / 1e9:.2f} GB ({c.pbytes / n:.1f} B/block), {reps} launches each, round-robin", flush=True)
        for kname, kwidth, krefs in (("4 groups", 2, kzero), ("256 groups", 8, kzero), ("clustered", 0, krefs_clustered)):
            kwidths = torch.full((n,), kwidth, dtype=torch.uint8, device=dev)
            koffsets, ktotal = fl.widths_to_offsets("u8", kwidths)
            kbytes = int(ktotal.item())
            kcol = rnd(max(kbytes, 16), 4).view(torch.uint8)[:kbytes]
            for mname, density in (("100 %", 1.0), ("1 %", 0.01), ("mask=None", None)):
                # the composition needs the bool tensor too: all n * 1024 bits in ONE draw (not random_mask's chunked one)
                bits = None
                if density is not None:
                    g = torch.Generator(device=dev); g.manual_seed(77 + T)
                    bits = torch.ones(n * 1024, dtype=torch.bool, device=dev) if density >= 1.0 else torch.rand(n * 1024, device=dev, generator=g) < density
                mask = None if bits is None else mask_words(bits)

                def composition():
                    v = fl.unfor_pack_widths(c.widths, c.offsets, c.col, c.refs, output=c.un, check=False).view(SIGNED[ty]).to(torch.int64)
                    k = fl.unfor_pack_widths(kwidths, koffsets, kcol, krefs, output=kun, check=False).to(torch.int64)
                    if T < 64:
                        v &= (1 << T) - 1
                    if bits is not None and density < 1.0:
                        v, k = v[bits], k[bits]
                    count = torch.bincount(k, minlength=256)
                    total_ = torch.zeros(256, dtype=torch.int64, device=dev).scatter_add_(0, k, v)
                    lo = torch.full((256,), (1 << 63) - 1, dtype=torch.int64, device=dev).scatter_reduce_(0, k, v, "amin")
                    hi = torch.full((256,), -(1 << 63), dtype=torch.int64, device=dev).scatter_reduce_(0, k, v, "amax")
                    return count, total_, lo, hi

                def ungrouped():
                    fl.unfor_aggregate_widths(c.widths, c.offsets, c.col, c.refs, mask, block_aggs=slots, check=False)
                    fl.unfor_pack_widths(kwidths, koffsets, kcol, krefs, output=kun, check=False)

                variants = {
                    "aggregate_by": lambda: fl.unfor_aggregate_by_widths(c.widths, c.offsets, c.col, c.refs, kwidths, koffsets, kcol, krefs, mask,
                                                                         result=result, check=False),
                    "(a) aggregate + key unpack": ungrouped,
                    "(b) unpack both + torch": composition,
                }
                ms = round_robin(variants, reps)
                print(format_aggregate_by_row(ty, kname, mname, n, ms["aggregate_by"]), flush=True)
                for k in variants:
                    if k != "aggregate_by":
                        print(format_yardstick_row(k, ty, n, ms[k], median(ms["aggregate_by"]), "aggregate_by", 28), flush=True)
                del bits, mask, variants
            del kwidths, koffsets, kcol
        del kun, slots


def format_compare_range_row(name, ty, n, ms, med_undecided, med_decided):
    return (f"{name:42s} {ty:4s} {show(ms)}  {n / median(ms) / 1e6:8.3f} Gblocks/s  x{median(ms) / med_undecided:.3f} of undecided, "
            f"x{median(ms) / med_decided:.3f} of all decided")


def case_compare_range(args):
    """unfor_compare_range_widths (an interval predicate chained through a mask) over the mixed-width column of --cases mixed, under the
    UNDECIDED predicate of that case (every block's value range straddles the constant, so no block is answered from its metadata and
    whatever is saved is saved by the incoming mask).  Timed in the SAME run on the SAME buffers, round-robin: NEW next to
    unfor_compare_widths; AND with an incoming mask of density 0, a clustered 1 % (one contiguous run of full blocks), a random 10 %
    (every block keeps something) and 100 %; the composition it replaces (unfor_compare_widths, then torch.bitwise_and with the mask so
    far); and unfor_compare_widths with every block decided (`x < 0`: metadata-only traffic).  Every figure is the median of `reps`
    launches with their min .. max beside it; the device's unique id heads the table.  Plain tensors whatever --placement says."""
    reps = max(args.reps, 5)
    print(device_header(args.placement), flush=True)
    for c in mixed_columns(args, refs="full", output=False):
        ty, T, n = c.ty, c.T, c.n
        # `x < k` = [0, k - 1] decides none
        k = 1 << (T - 1)
        refs_und = as_type(undecided_refs(k, rnd(n * 8, 5).view(torch.int64) & ((1 << 62) - 1), c.widths), ty)
        lo, hi = 0, k - 1
        out = torch.empty(n * 32, dtype=torch.int32, device=dev)
        hits = torch.empty(n * 32, dtype=torch.int32, device=dev)
        masks = clustered_and_masks(n, T)
        print(f"# {ty}: n = {n} blocks, packed {c.pbytes / 1e9:.2f} GB ({c.pbytes / n:.1f} B/block), {reps} launches each, round-robin", flush=True)
        variants = {
            "unfor_compare_widths undecided": lambda: fl.unfor_compare_widths(c.widths, c.offsets, c.col, refs_und, "<", k, output=out, check=False),
            "NEW undecided": lambda: fl.unfor_compare_range_widths(c.widths, c.offsets, c.col, refs_und, lo, hi, output=out, check=False),
            "compare all decided": lambda: fl.unfor_compare_widths(c.widths, c.offsets, c.col, c.refs, "<", 0, output=out, check=False),
        }
        for name, m in masks.items():
            variants[name] = lambda m=m: fl.unfor_compare_range_widths(c.widths, c.offsets, c.col, refs_und, lo, hi, mask=m, combine="and", output=out,
                                                                      check=False)
        m10 = masks["AND random 10 %"]
        variants["unfor_compare_widths + torch.bitwise_and"] = lambda: torch.bitwise_and(
            fl.unfor_compare_widths(c.widths, c.offsets, c.col, refs_und, "<", k, output=hits, check=False), m10, out=out)
        ms = round_robin(variants, reps)
        med = medians(ms)
        for kk in variants:
            print(format_compare_range_row(kk, ty, n, ms[kk], med["unfor_compare_widths undecided"], med["compare all decided"]), flush=True)
        del refs_und, out, hits, masks, m10, variants


def format_compare_columns_row(name, ty, n, ms, med_two_compares, med_undecided, med_decided):
    return (f"{name:36s} {ty:4s} {show(ms)}  {n / median(ms) / 1e6:8.3f} Gblock pairs/s  x{median(ms) / med_two_compares:.3f} of "
            f"2 x compare, x{median(ms) / med_undecided:.3f} of NEW undecided, x{median(ms) / med_decided:.3f} of all decided")


def case_compare_columns(args):
    """unfor_compare_columns_widths (a < b between two mixed-width columns, chained through a mask) over the mixed-width column of --cases
    mixed and a second one of the same shape (its own widths, its own packed bytes).  The second column's references sit INSIDE the first
    one's ranges, so no block pair is decided from its metadata and whatever is saved is saved by the incoming mask.  Timed in the SAME
    run on the SAME buffers, round-robin: NEW; AND with an incoming mask of density 0, a clustered 1 % (one contiguous run of full
    blocks), a random 10 % (every block keeps something) and 100 %; an all-decided run (the second column's references pushed just past
    the first one's ranges); yardstick (a) two unfor_compare_widths launches, one per column, each under an undecided constant -- the
    same packed bytes read, two masks written; yardstick (b) the composition the call replaces, unfor_pack_widths of both columns plus
    the torch compare.  Every figure is the median of `reps` launches with their min .. max beside it; the device's unique id heads
    the table.  Plain tensors whatever --placement says."""
    reps = max(args.reps, 5)
    print(device_header(args.placement), flush=True)
    for ty in chosen_types(args):
        # two columns share the --gb budget
        a, b = (mixed_column(ty, args.gb, width_seed=1000 * i, data_seed=10 * i, share=2, output=False) for i in (0, 1))
        T, n = a.T, a.n
        pbytes = a.pbytes + b.pbytes
        # a: references k - 1 - (x mod (2^WA - 1)): every block's range holds k - 1 and k (the undecided constant of yardstick (a));
        # b for yardstick (a): the same construction on its own widths
        k = 1 << (T - 1)
        span_a = (torch.ones(n, dtype=torch.int64, device=dev) << a.widths.to(torch.int64)) - 1
        x = rnd(n * 8, 5).view(torch.int64) & ((1 << 62) - 1)
        y = rnd(n * 8, 6).view(torch.int64) & ((1 << 62) - 1)
        ra64 = undecided_refs(k, x, a.widths)
        ra, rb_own = as_type(ra64, ty), as_type(undecided_refs(k, y, b.widths), ty)
        rb_in = as_type(ra64 + y % (span_a + 1), ty)                    # b starts inside a's range: the ranges overlap, nothing is decided
        ra_dec = torch.zeros(n, dtype=TDT[ty], device=dev)              # a in [0, 2^WA - 1], b from 2^WA on (no wrap: W <= T - 1): a < b everywhere
        rb_dec = as_type(span_a + 1, ty)
        out = torch.empty(n * 32, dtype=torch.int32, device=dev)
        out2 = torch.empty(n * 32, dtype=torch.int32, device=dev)
        masks = clustered_and_masks(n, T)
        una, unb = torch.empty(n * 1024, dtype=TDT[ty], device=dev), torch.empty(n * 1024, dtype=TDT[ty], device=dev)
        hit = torch.empty(n * 1024, dtype=torch.bool, device=dev)
        print(f"# {ty}: n = {n} blocks per column, packed {pbytes / 1e9:.2f} GB in both ({pbytes / n:.1f} B/block pair), {reps} launches each, round-robin", flush=True)

        def columns(ra_, rb_, **kw):
            return fl.unfor_compare_columns_widths(a.widths, a.offsets, a.col, ra_, "<", b.widths, b.offsets, b.col, rb_, output=out, check=False, **kw)

        def two_compares():
            fl.unfor_compare_widths(a.widths, a.offsets, a.col, ra, "<", k, output=out, check=False)
            fl.unfor_compare_widths(b.widths, b.offsets, b.col, rb_own, "<", k, output=out2, check=False)

        def composition():
            fl.unfor_pack_widths(a.widths, a.offsets, a.col, ra, output=una, check=False)
            fl.unfor_pack_widths(b.widths, b.offsets, b.col, rb_in, output=unb, check=False)
            torch.lt(una.view(SIGNED[ty]), unb.view(SIGNED[ty]), out=hit)

        variants = {"2 x unfor_compare_widths undecided": two_compares, "NEW undecided": lambda: columns(ra, rb_in),
                    "NEW all decided": lambda: columns(ra_dec, rb_dec)}
        for name, m in masks.items():
            variants[name] = lambda m=m: columns(ra, rb_in, mask=m, combine="and")
        variants["2 x unfor_pack_widths + torch.lt"] = composition
        ms = round_robin(variants, reps)
        med = medians(ms)
        for kk in variants:
            print(format_compare_columns_row(kk, ty, n, ms[kk], med["2 x unfor_compare_widths undecided"], med["NEW undecided"], med["NEW all decided"]), flush=True)
        del una, unb, hit, out, out2, masks, variants
        release_column(a)
        release_column(b)


def case_single(args):
    """batched unpack_single (bitpacking.rs:132-200; benches/bitpacking.rs:36-65 times one lookup): k lookups into an n-block column
    -- random, sorted, strided (one per block: every lookup a different block) and dense (all 1024 of consecutive blocks);
    uniform-width and mixed-width entry points.  A lookup needs 1-2 words of sizeof(T) bytes (:164-178); the memory system
    moves 32-byte sectors (64-byte requests on gfx950), so a RANDOM lookup costs a sector however small T is."""
    for ty, w in (("u32", 7), ("u64", 17), ("u16", 3), ("u8", 3)):
        esz = ESZ[ty]
        n, k = 1_000_000, 64_000_000
        pk = rnd(n * 128 * w, 1).view(TDT[ty])
        g = torch.Generator(device=dev); g.manual_seed(5)
        idx = torch.randint(0, n * 1024, (k,), dtype=torch.int64, device=dev, generator=g)
        out1 = torch.empty(k, dtype=TDT[ty], device=dev)
        widths = torch.full((n,), w, dtype=torch.uint8, device=dev)
        offsets, _ = fl.widths_to_offsets(ty, widths)
        patterns = (("random", idx), ("sorted", torch.sort(idx).values),
                    ("strided (one per block)", (torch.arange(k, dtype=torch.int64, device=dev) % n) * 1024 + (torch.arange(k, dtype=torch.int64, device=dev) * 7) % 1024),
                    ("dense (whole blocks in order)", torch.arange(k, dtype=torch.int64, device=dev)))
        lib = fl.load()
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        for name, ii in patterns:
            # the raw C ABI: no allocation and no error-flag read-back inside the timed region; the two untimed calls must return 0
            for label, f in (("unpack_single", lambda: getattr(lib, f"fl_{ty}_unpack_single")(w, pk.data_ptr(), n, ii.data_ptr(), k, out1.data_ptr(), err.data_ptr(), None)),
                             ("unpack_single_widths", lambda: getattr(lib, f"fl_{ty}_unpack_single_widths")(widths.data_ptr(), offsets.data_ptr(), pk.data_ptr(), n * 128 * w, n, ii.data_ptr(), k, out1.data_ptr(), err.data_ptr(), None))):
                t = median(timed(f, args.reps, check=True))
                io = k * (8 + esz)                  # the index read and the value written, per lookup
                print(f"{label:21s} {ty:4s} W={w:<2d} {k} lookups, {name:30s} {t:8.3f} ms  {k / t / 1e6:7.2f} G lookups/s  "
                      f"index+result stream {io / t / 1e6:7.1f} GB/s ({of_peak(io, t):.3f} of peak)", flush=True)
        del pk, idx, out1, widths, offsets
        torch.cuda.empty_cache()


ROW_CASES = {"quick": rows_quick, "orig": rows_orig, "consume": rows_consume, "fused": rows_fused, "allwidths": rows_allwidths, "widths": rows_widths}
CASES = {**ROW_CASES, "host": case_host, "small": case_small, "batch": case_batch, "refbench": case_refbench, "mixed": case_mixed,
         "select": case_select, "aggregate": case_aggregate, "aggregate_by": case_aggregate_by, "compare_range": case_compare_range,
         "compare_columns": case_compare_columns, "single": case_single}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=24.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="quick", choices=tuple(CASES))
    ap.add_argument("--wmin", type=int, default=0, help="keep only widths >= this")
    ap.add_argument("--wmax", type=int, default=64, help="keep only widths <= this")
    ap.add_argument("--types", default="", help="keep only these element types of the chosen cases (allwidths with --placement interleaved: one "
                    "process per type -- a constructed pair's address ranges are never re-used within a process, 868 rows exhaust them)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--placement", default="zoned", choices=("zoned", "separate", "interleaved"),
                    help="interleaved (every materialising row; pairs of 8 GiB and more, so --gb 12): the column's buffers from fl_column_pair_alloc(FL_LAYOUT_INTERLEAVED) -- packed sides in one "
                         "class of memory, the other side arranged for the eight XCDs' write positions")
    ap.add_argument("--window-ab", action="store_true", help="every row also under the whole-column tile map and under 2^16-block windows")
    ap.add_argument("--bare", action="store_true", help="pack / unpack / FoR / undelta_pack rows: also a bare stream of the row's bytes on the row's buffers (always on for allwidths)")
    ap.add_argument("--rows", default="", help="--cases mixed: keep only the rows whose name matches this regular expression")
    ap.add_argument("--batch-all", action="store_true", help="--cases batch: every element type and the pack direction too")
    ap.add_argument("--batch-policies", default="", help="--cases batch: comma-separated kernel policies to time next to the default")
    args = ap.parse_args(argv)
    args.bare = args.bare or args.cases == "allwidths"
    if args.cases in ROW_CASES:
        run_rows(ROW_CASES[args.cases](), args)
    else:
        CASES[args.cases](args)


if __name__ == "__main__":
    main()
