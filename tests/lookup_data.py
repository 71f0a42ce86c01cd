"""What the unfor_lookup tests share: the numpy model of the definition (built from the oracle's unfor_pack and pack(ty, T_BITS, .); it
never reads the kernel's output), the (key type, payload type) pairs, the tier boundary, the column that holds every route, the raw C
ABI call with its own error flag, and prefilled outputs.  torch is imported inside the functions that need it: the numpy half runs
without a GPU."""
import ctypes

import numpy as np

from oracle_lib import TYPES, tbits

PAIRS = [("u8", "u8"), ("u16", "u16"), ("u16", "u8"), ("u32", "u32"), ("u32", "u8"), ("u64", "u64"), ("u64", "u8")]
LDS_BYTES = 8192                                 # fl_lookup_map.hpp: LOOKUP_LDS_BYTES
STATS_PREFILL = np.array([1000, (1 << 40) + 7], dtype=np.uint64)
RUN_OF_3 = 2 + 256 * 3 + 65536 * 3               # kernel policy: a wavefront's run is at least 3 blocks

# the blocks of route_column
B_W1, B_FULL_WIDTH, B_ZERO_IN, B_WRAP, B_PIVOT, B_ZERO_OUT, B_EMPTY, B_ALL, B_FAR, B_ZERO_ABSENT, B_LAST = range(11)
ABSENT_SLOT = 1                                  # the slot of B_ZERO_ABSENT: its `present` bit is clear


ENTRIES = [(ty, uty, False) for ty, uty in PAIRS] + [("u8", "u8", True)]      # (key, payload, the _u8 name of a u8 key): the C ABI's entries


def entry(ty, uty, widths=True, twin=False):
    """the entry point of a pair; twin: fl_u8_unfor_lookup_u8, the second name of fl_u8_unfor_lookup (every type has one surface)"""
    return f"fl_{ty}_unfor_lookup{'_u8' if uty != ty or twin else ''}{'_widths' if widths else ''}"


def boundary_slots(ty, uty):
    """the largest table of the LDS tier, in slots (a u8 key cannot reach it: its whole domain is in the tier)"""
    return LDS_BYTES // (tbits(uty) // 8)


def window_sizes(ty, uty):
    """n_slots = 0, 1, one that the wrapping block straddles, the LDS / memory boundary, the boundary plus one slot, and 2^T for u8 / u16"""
    N = 1 << tbits(ty)
    sizes = [0, 1, 45, boundary_slots(ty, uty), boundary_slots(ty, uty) + 1] + ([N] if N <= 65536 else [])
    return sorted({s for s in sizes if s <= N})


def window_lo(ty):
    """key_lo near 2^T - 1: a window of more than 40 slots is cyclic"""
    return (1 << tbits(ty)) - 40


def route_column(ty, n):
    """(widths, refs) of an n-block key column (n = 3 or n >= 11) around window_lo(ty) in which every route occurs: a width-1 block, a
    W = T block, a width-0 block on slot 0, a block that wraps past 2^T - 1 and straddles the window's end, one that straddles its
    start, a width-0 block in front of the window, the blocks the masks empty and fill, a block half a domain away, a width-0 block on
    ABSENT_SLOT, and a last block that straddles the start again.  n = 3: the width-0 block on slot 0, the W = T block, the wrapping one."""
    T = tbits(ty)
    N = 1 << T
    lo = window_lo(ty)
    widths = [1, T, 0, 5, 6, 0, 4, 3, 3, 0, 7]
    refs = [lo + 3, 12345 % N, lo, lo + 20, lo - 30, lo - 5, lo + 1, lo + 2, lo + N // 2, lo + ABSENT_SLOT, lo - 60]
    if n == 3:
        pick = [B_ZERO_IN, B_FULL_WIDTH, B_WRAP]
        widths, refs = [widths[i] for i in pick], [refs[i] for i in pick]
    else:
        assert n >= 11
        rs = np.random.default_rng(3000 + T + n)
        extra = n - 11
        widths = widths[:-1] + [int(w) for w in rs.integers(0, min(T, 9) + 1, size=extra)] + widths[-1:]
        refs = refs[:-1] + [lo - 100 + int(x) for x in rs.integers(0, 300, size=extra)] + refs[-1:]
    return np.array(widths), np.array([r % N for r in refs], dtype=np.uint64).astype(TYPES[ty][0])


def route_masks(n, seed):
    """name -> bool[n * 1024] or None: no mask, a random one with the blocks B_EMPTY and B_ALL emptied and filled, the empty mask"""
    bits = np.random.default_rng(seed).random(n * 1024) < 0.5
    if n > B_ALL:
        bits[B_EMPTY * 1024:(B_EMPTY + 1) * 1024] = False
        bits[B_ALL * 1024:(B_ALL + 1) * 1024] = True
    return {"no mask": None, "random": bits, "empty": np.zeros(n * 1024, bool)}


def table_of(uty, n_slots, seed):
    """n_slots distinct-looking values of the payload type, none equal to 0 or all-ones (the two `missing` values of the tests)"""
    U = tbits(uty)
    t = np.random.default_rng(seed).integers(1, (1 << U) - 1, size=n_slots, dtype=np.uint64, endpoint=False) if U < 64 else \
        np.random.default_rng(seed).integers(1, (1 << 63) - 1, size=n_slots, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return t.astype(TYPES[uty][0])


def present_words(n_slots, seed, clear=()):
    """a bitmap of the window at 3/4 density with the bits `clear` cleared; every bit at a position >= n_slots of the last word is SET
    (stray bits that must be ignored)"""
    bits = np.random.default_rng(seed).random(n_slots) < 0.75
    for j in clear:
        if j < n_slots:
            bits[j] = False
    words = np.packbits(np.concatenate([bits, np.ones(-n_slots % 32, bool)]), bitorder="little").view(np.uint32).copy()
    return words


def pack_full_width(oracle, uty, v):
    """pack::<8 * sizeof(U)>(v) per block: a permutation of v; for u8 the identity -- asserted here"""
    out = np.concatenate([oracle.pack(uty, tbits(uty), blk) for blk in v.reshape(-1, 1024)]) if v.size else v.copy()
    if uty == "u8":
        assert np.array_equal(out, v), "pack(u8, 8, v) == v"
    return out


def expected_lookup(oracle, ty, uty, keys, keep, lo, table, present, missing, prefill_stats=None):
    """(out in full-width packed order, hit words int32[n * 32], stats uint64[2], v in row order, h bool) of one call over the decoded
    `keys` (the oracle's unfor_pack), the rows `keep` keeps (bool per row; None: every row), the window (lo, len(table)), the bitmap
    `present` (uint32 words or None) and `missing`"""
    T = tbits(ty)
    with np.errstate(over="ignore"):
        j = keys.astype(np.uint64) - np.uint64(int(lo) % (1 << T))
    if T < 64:
        j &= np.uint64((1 << T) - 1)
    kept = np.ones(keys.size, bool) if keep is None else keep
    hit = kept & (j < np.uint64(len(table)))
    js = np.where(hit, j, np.uint64(0)).astype(np.int64)
    if present is not None and len(table):
        hit &= ((present[js >> 5] >> (js & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
    miss_value = np.array(int(missing) & ((1 << tbits(uty)) - 1), dtype=np.uint64).astype(TYPES[uty][0])
    v = np.where(hit, table[np.where(hit, js, 0)] if len(table) else miss_value, miss_value).astype(TYPES[uty][0])
    stats = np.zeros(2, dtype=np.uint64) if prefill_stats is None else prefill_stats.copy()
    stats += np.array([int(hit.sum()), int((kept & ~hit).sum())], dtype=np.uint64)
    return pack_full_width(oracle, uty, v), np.packbits(hit, bitorder="little").view(np.int32), stats, v, hit


def raw_lookup(fl, ty, uty, dw, doff, dcol, drefs, n, dmask, lo, n_slots, dtable, dpresent, missing, dout, dhit, dstats, ref_stride=1, twin=False):
    """The C ABI call fl_<ty>_unfor_lookup[_u8]_widths with its own err_flag on the current stream; dmask / dtable / dpresent / dhit /
    dstats: CUDA tensors or None (NULL).  Returns (status, the flag's value)."""
    import torch
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
    rc = getattr(fl.load(), entry(ty, uty, True, twin))(
        dw.data_ptr(), doff.data_ptr(), ptr(dcol), dcol.numel() * (tbits(ty) // 8), drefs.data_ptr(), ref_stride, ptr(dmask), n,
        int(lo) % (1 << tbits(ty)), n_slots, ptr(dtable), ptr(dpresent), int(missing) & ((1 << tbits(uty)) - 1), dout.data_ptr(), ptr(dhit),
        ptr(dstats), err.data_ptr(), stream)
    return rc, int(err.item())
