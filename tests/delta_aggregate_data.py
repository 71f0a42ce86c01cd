"""What the tests of undelta_aggregate share (numpy and the oracle only; no GPU, no torch): the definition's expected slots, the route a
block takes read off the DEFINITION (not off fl_delta_aggregate_map.hpp), the width-0 block in Python's exact integers, and a numpy
lane-group model of the aggregate that untransposes no value."""
import numpy as np

import bitmodel
from delta_compare_range_data import lane_base
from gpu_support import IDENTITY, expected_blocks
from oracle_lib import tbits

SKIP, IDENTITY_ROUTE, BASES, EACH = 0, 1, 2, 3
FORMS = ("undelta_aggregate", "undelta_aggregate_widths")


def mask_bits(mask_words):
    """[n * 32] int32 words (bit i of word i // 32, LSB first, i = the ORIGINAL row) -> bool[n * 1024]; None stays None (every row)"""
    if mask_words is None:
        return None
    return np.unpackbits(np.ascontiguousarray(mask_words).view(np.uint8), bitorder="little").astype(bool)


def want_slots(vals, mask_words, skipped=()):
    """the definition: uint64[n, 4] = count, wrapping sum, min, max of the kept values of every block; a skipped block: the identity"""
    out = expected_blocks(vals, mask_bits(mask_words))
    for b in skipped:
        out[b] = IDENTITY
    return out


def route_of(ok, mask_block, w):
    """SKIP > IDENTITY > BASES > EACH; mask_block: the block's 32 words, or None (no mask: every row)"""
    if not ok:
        return SKIP
    if mask_block is not None and not np.asarray(mask_block).any():
        return IDENTITY_ROUTE
    return BASES if int(w) == 0 else EACH


def column_routes(widths, mask_words, skipped=()):
    m = None if mask_words is None else np.asarray(mask_words).reshape(-1, 32)
    return [route_of(b not in skipped, None if m is None else m[b], w) for b, w in enumerate(widths)]


def group_popcounts(ty, mask_block):
    """p_l of every FastLanes lane l: the kept rows among the T bits at lane_base(l) of the block's 1024-bit mask"""
    T = tbits(ty)
    bits = np.ones(1024, bool) if mask_block is None else mask_bits(mask_block)
    return [int(bits[lane_base(l):lane_base(l) + T].sum()) for l in range(1024 // T)]


def bases_block(T, bases, p):
    """A width-0 block from the DEFINITION in Python's exact integers: chain l holds p_l kept rows, each equal to base_l"""
    kept = [(int(b) % (1 << T), int(k)) for b, k in zip(bases, p) if k]
    if not kept:
        return [0, 0, (1 << 64) - 1, 0]
    return [sum(k for _, k in kept), sum(b * k for b, k in kept) % (1 << 64), min(b for b, _ in kept), max(b for b, _ in kept)]


def lane_group_model(ty, w, packed, bases, mask_block):
    """One block's slot WITHOUT untransposing a value: every FastLanes lane's chain is summed along its rows (the fields come from
    tests/bitmodel.py's reading of the wire format) and row r of lane l is kept when mask bit lane_base(l) + r is set."""
    T = tbits(ty)
    N = 1 << T
    fields = bitmodel.unpack_bits([int(x) for x in packed], T, w)
    bits = np.ones(1024, bool) if mask_block is None else mask_bits(mask_block)
    used = np.zeros(1024, bool)
    count, total, lo, hi = 0, 0, (1 << 64) - 1, 0
    for l in range(1024 // T):
        run = int(bases[l])
        for r in range(T):
            run = (run + fields[bitmodel.index(r, l)]) % N
            i = lane_base(l) + r
            assert not used[i]
            used[i] = True
            if bits[i]:
                count, total, lo, hi = count + 1, (total + run) % (1 << 64), min(lo, run), max(hi, run)
    assert used.all()                                                       # every mask bit governs exactly one row of one chain
    return np.array([count, total, lo, hi], dtype=np.uint64)


def rows_mask(n, block, r0, r1):
    """[n * 32] int32: rows r0 .. r1 (inclusive) of `block`, nothing else"""
    bits = np.zeros(n * 1024, bool)
    bits[block * 1024 + r0:block * 1024 + r1 + 1] = True
    return np.packbits(bits, bitorder="little").view(np.int32)


def in_full_width_order(ty, mask_words):
    """The mask a FULL-WIDTH packed reading of a buffer in original order has to see: word p = LANES r + l of such a block is its unpacked
    index index(r, l) (macros.rs:20-24), so bit index(r, l) of the result is bit p of `mask_words`."""
    L = 1024 // tbits(ty)
    q = np.array([bitmodel.index(p // L, p % L) for p in range(1024)])
    bits = mask_bits(mask_words).reshape(-1, 1024)
    moved = np.zeros_like(bits)
    moved[:, q] = bits
    return np.packbits(moved.reshape(-1), bitorder="little").view(np.int32)
