"""What the unfor_aggregate_by_lookup tests share: the numpy model of the definition (over values and keys decoded by the oracle's
unfor_pack; it never reads the kernel's output), the block routes restated in Python integers (tests/test_aggregate_by_lookup_cpu.py
holds them against fastlanes_amd/csrc/fl_aggregate_by_lookup_map.hpp), the column pair in which every route occurs, the group-code
tables, and the raw C ABI call with its own error flag.  torch is imported inside the functions that need it: the numpy half runs
without a GPU."""
import ctypes

import numpy as np

from gpu_support import IDENTITY, mixed_column_host
from lookup_data import ABSENT_SLOT, present_words, route_column, route_masks, window_lo  # noqa: F401 (the tests take them from here)
from oracle_lib import TYPES, tbits
from set_build_data import window_indices

GROUPS = 256
FORMS = ("unfor_aggregate_by_lookup", "unfor_aggregate_by_lookup_widths")
STATS_PREFILL = np.array([1000, (1 << 40) + 7], dtype=np.uint64)
RUN_OF_3 = 2 + 256 * 3 + 65536 * 3               # kernel policy: a wavefront's run is at least 3 blocks
SKIP, NOTHING, MISSING, ONE_GROUP, EACH = range(5)                           # fl_aggregate_by_lookup_map.hpp: AggregateByLookupRoute
ROUTE_NAMES = ("SKIP", "NOTHING", "MISSING", "ONE_GROUP", "EACH")
BAD_KEY_BLOCK, BAD_VALUE_BLOCK = 3, 6            # blocks of route_pair(ty, 11) of non-zero width in the column that is broken


def window_sizes(ty):
    """n_slots = 0, 1, one that the wrapping block straddles, 8192 and 8193 (unfor_lookup's tier boundary: ONE tier here), and 2^T for
    u8 / u16"""
    N = 1 << tbits(ty)
    return sorted({s for s in [0, 1, 45, 8192, 8193] + ([N] if N <= 65536 else []) if s <= N})


def code_table(n_slots, seed):
    """n_slots group codes out of all 256 values; slot 0 (the width-0 key block inside the window) holds 255, slot 2 holds 0: a
    gathered 0 is a valid group, and so is the last one"""
    t = np.random.default_rng(seed).integers(0, 256, size=n_slots, dtype=np.uint64).astype(np.uint8)
    if n_slots > 0:
        t[0] = 255
    if n_slots > 2:
        t[2] = 0
    return t


def route_of(ty, lo, n_slots, key_reference, key_width, mask_empty, ok=True):
    """the route of a block, in Python integers: the block's slots {(c + f) mod 2^T, f < 2^W} meet the window [0, n_slots - 1] iff c
    lies inside it or c + 2^W - 1 passes 2^T"""
    N = 1 << tbits(ty)
    c = (int(key_reference) - int(lo)) % N
    if not ok:
        return SKIP
    if mask_empty:
        return NOTHING
    if n_slots == 0 or not (c <= n_slots - 1 or c + (1 << int(key_width)) - 1 >= N):
        return MISSING
    return ONE_GROUP if int(key_width) == 0 else EACH


def value_widths(ty, n):
    """the value column beside route_column(ty, n): width 0, width T and narrow blocks; n = 3: the width-0 key block inside the window
    meets a width-0 value block (a constant block), n = 11: it meets a W = T block"""
    T = tbits(ty)
    if n == 3:
        return np.array([0, 5, T])
    assert n == 11
    return np.array([5, 0, T, 3, 2, 7, 2, T, 1, 4, 6])


def decode(oracle, ty, blocks, refs):
    return np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])


def route_pair(oracle, ty, n, seed):
    """The host side of the n-block column pair (n = 3 or 11) in which every route occurs: the key column is lookup_data.route_column
    around window_lo(ty), the value column value_widths with random references.  A dict of widths / off / col / refs / decoded values
    for `key` and `val`."""
    T = tbits(ty)
    out = {}
    kw, krefs = route_column(ty, n)
    vrefs = np.random.default_rng(seed + 7).integers(0, 1 << min(T, 63), size=n, dtype=np.uint64).astype(TYPES[ty][0])
    for name, widths, refs, s in (("key", kw, krefs, seed), ("val", value_widths(ty, n), vrefs, seed + 1)):
        w, off, col, blocks = mixed_column_host(ty, widths, s)
        out[name] = dict(widths=w, off=off, col=col, refs=refs, decoded=decode(oracle, ty, blocks, refs))
    return out


def routes_taken(ty, pair, keep, lo, n_slots, present):
    """the names of the routes the key column's blocks take under one (mask, window, bitmap), ONE_GROUP split by its slot's bit"""
    n = pair["key"]["widths"].size
    N = 1 << tbits(ty)
    seen = set()
    for b in range(n):
        empty = keep is not None and not keep[b * 1024:(b + 1) * 1024].any()
        r = route_of(ty, lo, n_slots, pair["key"]["refs"][b], pair["key"]["widths"][b], empty)
        if r == ONE_GROUP:
            c = (int(pair["key"]["refs"][b]) - lo) % N
            bit = present is None or (int(present[c >> 5]) >> (c & 31)) & 1
            seen.add("ONE_GROUP present" if bit else "ONE_GROUP absent")
        else:
            seen.add(ROUTE_NAMES[r])
    return seen


def expected_fused(ty, vals, keys, keep, lo, table, present, prefill_stats=None, without=()):
    """(result uint64[256, 4], stats uint64[2], hit bool per row) of one call over the decoded `vals` and `keys` (the oracle's
    unfor_pack), the rows `keep` keeps (bool per row; None: every row), the window (lo, len(table)), the u8 group codes `table`, the
    bitmap `present` (uint32 words or None).  `without`: blocks that contribute nothing (skipped by the device checks)."""
    kept = np.ones(keys.size, bool) if keep is None else np.asarray(keep).copy()
    for b in without:
        kept[b * 1024:(b + 1) * 1024] = False
    j = window_indices(ty, keys, lo)
    hit = kept & (j < np.uint64(len(table)))
    if present is not None and len(table):
        js = np.where(hit, j, np.uint64(0)).astype(np.int64)
        hit &= ((present[js >> 5] >> (js & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
    g = table[j[hit].astype(np.int64)].astype(np.intp) if len(table) else np.zeros(0, np.intp)
    v = vals[hit].astype(np.uint64)
    out = np.tile(IDENTITY, (GROUPS, 1))
    count, total, low, high = (np.ascontiguousarray(out[:, q]) for q in range(4))
    np.add.at(count, g, np.uint64(1))
    np.add.at(total, g, v)                          # uint64: wraps mod 2^64
    np.minimum.at(low, g, v)
    np.maximum.at(high, g, v)
    stats = np.zeros(2, dtype=np.uint64) if prefill_stats is None else prefill_stats.copy()
    stats += np.array([int(hit.sum()), int((kept & ~hit).sum())], dtype=np.uint64)
    return np.stack([count, total, low, high], axis=1), stats, hit


def upload(pair):
    """the pair's eight leading arguments of the Python mirror, on the device"""
    import torch
    from gpu_support import to_dev
    lead = []
    for name in ("val", "key"):
        c = pair[name]
        lead += [torch.from_numpy(c["widths"]).cuda(), torch.from_numpy(c["off"]).cuda(), to_dev(c["col"]), to_dev(c["refs"])]
    return lead


def raw_fused(fl, ty, lead, n, dmask, lo, n_slots, dtable, dpresent, dresult, dstats):
    """The C ABI call fl_<ty>_unfor_aggregate_by_lookup_widths with its own err_flag on the current stream; lead: upload()'s eight
    tensors (or replacements); dmask / dtable / dpresent / dstats: CUDA tensors or None (NULL).  Returns (status, the flag's value)."""
    import torch
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
    esz = tbits(ty) // 8
    vw, voff, vcol, vrefs, kw, koff, kcol, krefs = lead
    rc = getattr(fl.load(), f"fl_{ty}_unfor_aggregate_by_lookup_widths")(
        vw.data_ptr(), voff.data_ptr(), ptr(vcol), vcol.numel() * esz, vrefs.data_ptr(), 1,
        kw.data_ptr(), koff.data_ptr(), ptr(kcol), kcol.numel() * esz, krefs.data_ptr(), 1,
        ptr(dmask), n, int(lo) % (1 << tbits(ty)), n_slots, ptr(dtable), ptr(dpresent), dresult.data_ptr(), ptr(dstats), err.data_ptr(), stream)
    return rc, int(err.item())
