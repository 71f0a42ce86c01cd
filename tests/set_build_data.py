"""What the unfor_set_build tests share: the expected side (numpy over already-decoded values; it never reads the kernel's bitmap), the
prefilled bitmap and counters a call must OR / add into, the raw C ABI call with its own error flag, and the library's own encoder for
columns given as values.  torch is imported inside the functions that need it: the numpy half runs without a GPU."""
import ctypes

import numpy as np

from oracle_lib import tbits

STATS_PREFILL = np.array([1000, (1 << 40) + 7], dtype=np.uint64)


def window_indices(ty, vals, lo):
    """j = (v - lo) mod 2^T of every value, as uint64"""
    T = tbits(ty)
    with np.errstate(over="ignore"):
        j = vals.astype(np.uint64) - np.uint64(int(lo) % (1 << T))
    return j & np.uint64((1 << T) - 1) if T < 64 else j


def expected_build(ty, vals, keep, lo, bits, prefill_words=None, prefill_stats=None):
    """(words uint32[ceil(bits / 32)], stats uint64[2]) after one call: words = prefill | bits(j[j < bits]), stats = prefill + (count
    inside, count outside), over the rows `keep` (bool per value; None: every row) keeps"""
    j = window_indices(ty, vals if keep is None else vals[keep], lo)
    inside = j < np.uint64(bits)
    words = np.zeros((bits + 31) // 32, dtype=np.uint32) if prefill_words is None else prefill_words.copy()
    ji = np.unique(j[inside])
    np.bitwise_or.at(words, (ji >> np.uint64(5)).astype(np.int64), np.uint32(1) << (ji & np.uint64(31)).astype(np.uint32))
    stats = np.zeros(2, dtype=np.uint64) if prefill_stats is None else prefill_stats.copy()
    stats += np.array([int(inside.sum()), int(inside.size - inside.sum())], dtype=np.uint64)
    return words, stats


def prefill_words(bits, rng):
    """a sparse random bitmap of the window's words; the last word's bits at positions >= bits are ALL set (garbage that must survive)"""
    nw = (bits + 31) // 32
    words = (rng.integers(0, 1 << 32, size=nw, dtype=np.uint64) & rng.integers(0, 1 << 32, size=nw, dtype=np.uint64)
             & rng.integers(0, 1 << 32, size=nw, dtype=np.uint64)).astype(np.uint32)
    if bits % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (bits % 32)) & 0xFFFFFFFF)
    return words


def raw_build(fl, ty, dw, doff, dcol, drefs, n, dmask, lo, bits, dwords, dstats, ref_stride=1):
    """The C ABI call fl_<ty>_unfor_set_build_widths with its own err_flag on the current stream; dmask / dwords / dstats: CUDA tensors
    or None (NULL).  Returns (status, the flag's value)."""
    import torch
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = getattr(fl.load(), f"fl_{ty}_unfor_set_build_widths")(
        dw.data_ptr(), doff.data_ptr(), ptr(dcol) if dcol.numel() else None, dcol.numel() * (tbits(ty) // 8), drefs.data_ptr(), ref_stride, ptr(dmask), n,
        int(lo) % (1 << tbits(ty)), bits, ptr(dwords), ptr(dstats), err.data_ptr(), stream)
    return rc, int(err.item())


def words_of(t):
    return t.cpu().numpy().view(np.uint32)


def stats_of(t):
    return t.cpu().numpy().view(np.uint64)


def encode(fl, ty, vals):
    """values -> (widths, offsets, packed, references) on the device through the library's own encoder"""
    import torch
    from gpu_support import TDT, to_dev
    dv = to_dev(vals)
    mins, maxs = fl.BitPacking.block_min_max(dv)
    dw = fl.for_widths(mins, maxs)
    doff, dtotal = fl.widths_to_offsets(ty, dw)
    dpk = torch.zeros(max(int(dtotal.item()) // (tbits(ty) // 8), 1), dtype=getattr(torch, TDT[ty]), device="cuda:0")
    fl.for_pack_widths(dw, doff, dv, mins, dpk)
    return dw, doff, dpk, mins
