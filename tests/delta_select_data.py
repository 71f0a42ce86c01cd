"""What the tests of undelta_select share (numpy and the oracle only; no GPU, no torch): the definition's expected run, the route a block
takes read off the DEFINITION (not off fl_delta_select_map.hpp), and a numpy lane-group model of the select that untransposes no
value: every chain is summed along its rows and row r of FastLanes lane l is written straight to its landing."""
import numpy as np

import bitmodel
from delta_aggregate_data import mask_bits, rows_mask  # noqa: F401 (rows_mask: for the tests)
from delta_compare_range_data import lane_base
from oracle_lib import TYPES, tbits

SKIP, EMPTY, BOUNDS, BASES, EACH = 0, 1, 2, 3, 4
FORMS = ("undelta_select", "undelta_select_widths")


def block_counts(mask_words):
    """kept rows of every block"""
    return mask_bits(mask_words).reshape(-1, 1024).sum(axis=1).astype(np.int64)


def offsets_of(mask_words):
    """(out_offsets, total) as fl_mask_offsets defines them: the exclusive prefix sum of the blocks' popcounts"""
    c = block_counts(mask_words)
    return (np.cumsum(c) - c).astype(np.int64), int(c.sum())


def want_run(vals, mask_words, skipped=()):
    """the definition: vals[bits], in row order -- and, beside it, bool per output slot: False where the slot belongs to a skipped block
    (it must keep what it held)"""
    bits = mask_bits(mask_words)
    written = np.repeat(~np.isin(np.arange(bits.size // 1024), list(skipped)), 1024)[bits]
    return vals[bits], written


def route_of(ok, mask_block, inside, w):
    """SKIP > EMPTY > BOUNDS > BASES > EACH; mask_block: the block's 32 words; inside: the block's run lies inside the output"""
    if not ok:
        return SKIP
    if not np.asarray(mask_block).any():
        return EMPTY
    if not inside:
        return BOUNDS
    return BASES if int(w) == 0 else EACH


def column_routes(widths, mask_words, skipped=(), out_offsets=None, out_len=None):
    m = np.asarray(mask_words).reshape(-1, 32)
    counts = block_counts(mask_words)
    if out_offsets is None:
        out_offsets, out_len = offsets_of(mask_words)
    return [route_of(b not in skipped, m[b], 0 <= int(out_offsets[b]) and int(out_offsets[b]) + int(counts[b]) <= out_len, w)
            for b, w in enumerate(widths)]


def landing_of(bits, p):
    """rank(p): the mask bits of the block below original row p"""
    return int(bits[:p].sum())


def lane_group_model(ty, w, packed, bases, mask_block):
    """One block's run WITHOUT untransposing a value: every FastLanes lane's chain is summed along its rows (the fields come from
    tests/bitmodel.py's reading of the wire format) and row r of lane l, when mask bit lane_base(l) + r is set, goes straight to
    run[popcount(mask bits below lane_base(l) + r)]."""
    T = tbits(ty)
    N = 1 << T
    fields = bitmodel.unpack_bits([int(x) for x in packed], T, w)
    bits = mask_bits(mask_block)
    below = np.concatenate([[0], np.cumsum(bits)])
    count = int(below[-1])
    run = np.zeros(count, dtype=TYPES[ty][0])
    hit = np.zeros(count, dtype=np.int64)
    for l in range(1024 // T):
        x = int(bases[l])
        for r in range(T):
            x = (x + fields[bitmodel.index(r, l)]) % N
            p = lane_base(l) + r
            if bits[p]:
                run[below[p]] = x
                hit[below[p]] += 1
    assert (hit == 1).all()                                                 # every landing in [0, count) is hit exactly once
    return run
