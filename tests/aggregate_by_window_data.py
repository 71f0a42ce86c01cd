"""What the unfor_aggregate_by_window tests share: the expected side (numpy over already-decoded values and keys: np.add.at /
np.minimum.at / np.maximum.at on uint64 over prefilled arrays; it never reads the kernel's output), the prefilled arrays and counters a
call must accumulate into, and the raw C ABI call with its own error flag.  torch is imported inside the functions that need it: the
numpy half runs without a GPU."""
import ctypes

import numpy as np

from oracle_lib import tbits
from set_build_data import STATS_PREFILL, window_indices  # noqa: F401 (STATS_PREFILL: re-exported)

WHAT = ("count", "sum", "min", "max")
U64_MAX = np.uint64(2 ** 64 - 1)
LDS_GROUPS = 256                                 # fastlanes_amd/csrc/fl_aggregate_by_window_map.hpp: AGGREGATE_BY_WINDOW_LDS_GROUPS


def identities(n_groups):
    """the four arrays of a fresh table: 0 / 0 / 2^64 - 1 / 0"""
    z = np.zeros(n_groups, dtype=np.uint64)
    return [z.copy(), z.copy(), np.full(n_groups, U64_MAX, dtype=np.uint64), z.copy()]


def prefill_arrays(n_groups, rng):
    """random counts and sums; mins and maxs half identities, half random values of every magnitude (so that min and max against an
    earlier call's entry are checked in both directions)"""
    def any_magnitude():
        return rng.integers(0, 1 << 63, size=n_groups, dtype=np.uint64) >> rng.integers(0, 63, size=n_groups).astype(np.uint64)
    fresh = rng.random(n_groups) < 0.5
    return [rng.integers(0, 1 << 40, size=n_groups, dtype=np.uint64), rng.integers(0, 1 << 63, size=n_groups, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
            np.where(fresh, U64_MAX, any_magnitude()), np.where(fresh, np.uint64(0), any_magnitude())]


def expected_table(ty, vals, keys, keep, lo, n_groups, prefill=None, prefill_stats=None):
    """([counts, sums, mins, maxs] uint64[n_groups], stats uint64[2]) after one call over the rows `keep` (bool per row; None: every
    row) keeps: slot j = (key - lo) mod 2^T < n_groups receives the row's value, zero-extended; sums wrap mod 2^64"""
    if keep is not None:
        vals, keys = vals[keep], keys[keep]
    j = window_indices(ty, keys, lo)
    inside = j < np.uint64(n_groups)
    at, v = j[inside].astype(np.int64), vals[inside].astype(np.uint64)
    arrays = identities(n_groups) if prefill is None else [a.copy() for a in prefill]
    with np.errstate(over="ignore"):
        np.add.at(arrays[0], at, np.uint64(1))
        np.add.at(arrays[1], at, v)
    np.minimum.at(arrays[2], at, v)
    np.maximum.at(arrays[3], at, v)
    stats = np.zeros(2, dtype=np.uint64) if prefill_stats is None else prefill_stats.copy()
    stats += np.array([int(inside.sum()), int(inside.size - inside.sum())], dtype=np.uint64)
    return arrays, stats


def raw_window(fl, ty, val, key, n, dmask, lo, n_groups, darrays, dstats, ref_stride=1, key_ref_stride=1):
    """The C ABI call fl_<ty>_unfor_aggregate_by_window_widths with its own err_flag on the current stream.  val / key: (widths,
    offsets, packed, references) CUDA tensors, `packed` None or empty: NULL with packed_bytes 0; dmask / darrays[i] / dstats: CUDA
    tensors or None (NULL).  Returns (status, the flag's value)."""
    import torch
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
    esz = tbits(ty) // 8

    def column(c, stride):
        dw, doff, dcol, drefs = c
        return (dw.data_ptr(), doff.data_ptr(), ptr(dcol), dcol.numel() * esz if dcol is not None else 0, drefs.data_ptr(), stride)

    rc = getattr(fl.load(), f"fl_{ty}_unfor_aggregate_by_window_widths")(
        *column(val, ref_stride), *column(key, key_ref_stride), ptr(dmask), n, int(lo) % (1 << tbits(ty)), n_groups,
        *(ptr(t) for t in darrays), ptr(dstats), err.data_ptr(), stream)
    return rc, int(err.item())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def table_arrays(table):
    """a GroupTable's four arrays as numpy uint64 (None stays None)"""
    return [None if t is None else u64(t) for t in (table.counts, table.sums, table.mins, table.maxs)]
