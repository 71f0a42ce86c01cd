"""GPU: the three mask producers -- unpack_compare, unfor_compare, unfor_compare_widths -- on boundary-dense columns
(tests/boundary_data.py): every (row, lane) of a block holds k - 1, k and k + 1, next to 0, 2^W - 1 and k in the neighbouring rows and
lanes.  None of these kernels extracts a field and compares it ([field | junk] <= [k | ones], a borrow-free SWAR subtract in the
packed domain, (f + c) mod 2^T <= s at a runtime width), so an off-by-one, a wrong junk fill or a borrow from a neighbour changes a
verdict only where field == k or k + 1 -- which uniform random data reaches in row 0 and, beyond W ~ 12, nowhere else.

Every type, every W in 0..T, all six ops; the expected mask is numpy's comparison of the constructed values themselves (the columns
are packed by the oracle, whose pack is cross-checked against the bit model in test_boundary_data_cpu.py; nothing is unpacked on the
host).  Bit-exact.  The coverage conditions are asserted before any launch."""
import numpy as np
import pytest

import boundary_data as bd
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import POLICIES as FOR_POLICIES  # the five of test_gpu_for_compare.py::test_policies_streams_and_empty_columns
from gpu_support import TYS, to_dev, want_mask

pytestmark = pytest.mark.gpu

OPS = ["==", "!=", "<", "<=", ">", ">="]
UNPACK_POLICIES = [0, 1, 2]
ONE_BLOCK_WIDTHS = (0, 7, 17)          # and W = T: the widths test_unpack_compare_u32_u64_every_width runs at one block too


def first_difference(got, want, T):
    """(block, row, lane) of the first differing mask bit, for the assertion message."""
    d = np.unpackbits((got ^ want).view(np.uint8), bitorder="little")
    i = int(np.flatnonzero(d)[0])
    blk, idx = divmod(i, 1024)
    L = 1024 // T
    for r in range(T):
        base = bd.FL_ORDER[r // 8] * 16 + (r % 8) * 128          # bitmodel.index(r, 0)
        if base <= idx < base + L:
            return blk, r, idx - base
    raise AssertionError(idx)


def check(got_tensor, want, T, *what):
    got = got_tensor.cpu().numpy().view(np.int32)
    if not np.array_equal(got, want):
        blk, row, lane = first_difference(got, want, T)
        raise AssertionError(f"{what}: {int(np.unpackbits((got ^ want).view(np.uint8)).sum())} verdicts differ, the first in block {blk}, row {row}, lane {lane}")


@pytest.fixture
def column(oracle):
    """column(ty, W, kf) -> (field values in index order as np.uint64, packed column): coverage asserted first, each column built
    once and kept until the test releases it (column.clear(): the uniform-width tests do after each W) or ends."""
    built = {}

    def get(ty, W, kf):
        key = (ty, W, kf)
        if key not in built:
            T = tbits(ty)
            F = bd.fields(T, W, kf, bd.seed_of(T, W))
            bd.check_coverage(F, W, kf)
            v = bd.in_index_order(F)
            built[key] = (v, bd.pack_column(oracle, ty, W, v))
        return built[key]
    get.clear = built.clear
    yield get
    built.clear()


def seeded(T, W, salt):
    return int.from_bytes(np.random.default_rng(88000 + 1000 * salt + 100 * T + W).bytes(8), "little") & ((1 << T) - 1)


@pytest.mark.parametrize("ty", TYS)
def test_unpack_compare_at_the_boundaries(fl, column, kernel_policy, ty):
    """unpack_compare: constants 0, 1, a mid value, 2^W - 2, 2^W - 1 in the field domain, each on a column built around it, and
    beyond the field (2^W, M) on the column built around 2^W - 1; kernel policies 0 / 1 / 2; 29 blocks, and one block at
    W in {0, 7, 17, T} (the column's first sweep block alone: a launch of a single, partly filled wavefront -- only this entry point
    has a uniform one-block form that the older tests single out)."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    M = (1 << T) - 1
    for W in range(T + 1):
        m = (1 << W) - 1
        pl = packed_len(ty, W)
        for kf in bd.constants(W, bd.seed_of(T, W)):
            v, pk = column(ty, W, kf)
            vals = v.astype(dt)
            dpk = to_dev(pk)
            ks = [kf] + (sorted({m + 1, M}) if (W < T and kf == m) else [])
            for n in ((vals.size // 1024, 1) if W in ONE_BLOCK_WIDTHS + (T,) else (vals.size // 1024,)):
                want = {(op, k): want_mask(vals[:n * 1024], op, k) for op in OPS for k in ks}
                for policy in UNPACK_POLICIES:
                    kernel_policy(policy)
                    for (op, k), w in want.items():
                        check(fl.BitPacking.unpack_compare(W, dpk[:n * pl], op, k, n_blocks=n), w, T, ty, "unpack_compare", f"W={W}", op, f"k={k}",
                              f"policy={policy}", f"n={n}")
        column.clear()


def for_reference(T, W, kf):
    """The broadcast reference of (T, W): seeded for even W; for odd W one with r + 2^W - 1 > M (the values wrap inside the block)."""
    M = (1 << T) - 1
    return seeded(T, W, 1) if W % 2 == 0 else (M - ((1 << W) - 1) // 2) & M


@pytest.mark.parametrize("ty", TYS)
def test_unfor_compare_at_the_boundaries(fl, column, kernel_policy, ty):
    """FoR.unfor_compare, uniform width.  One pass with a broadcast reference r (stride 0): K = (kf + r) mod 2^T on the column built
    around kf.  One pass with per-block references over the five columns back to back: K in {0, a seeded value, M} and
    r_b = (K - kf_b) mod 2^T, so K - r_b is the constant each block was built around -- and r_b + 2^W - 1 > M for most blocks at
    K = 0.  The five policies of test_policies_streams_and_empty_columns."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    M = (1 << T) - 1
    u = np.uint64
    for W in range(T + 1):
        kfs = bd.constants(W, bd.seed_of(T, W))
        calls = []                       # (packed, reference argument, n_blocks, op, K, want, label)
        for kf in kfs:
            v, pk = column(ty, W, kf)
            r = for_reference(T, W, kf)
            vals = ((v + u(r)) & u(M)).astype(dt)
            K = (kf + r) & M
            dpk = to_dev(pk)
            calls += [(dpk, r, v.size // 1024, op, K, want_mask(vals, op, K), f"broadcast r={r} kf={kf}") for op in OPS]
        v_all = np.concatenate([column(ty, W, kf)[0] for kf in kfs])
        dpk_all = to_dev(np.concatenate([column(ty, W, kf)[1] for kf in kfs]))
        nb = column(ty, W, kfs[0])[0].size // 1024
        kf_b = np.repeat(np.array(kfs, dtype=np.uint64), nb)
        for K in sorted({0, seeded(T, W, 2), M}):
            r_b = (u(K) - kf_b) & u(M)
            vals = ((v_all + np.repeat(r_b, 1024)) & u(M)).astype(dt)
            drefs = to_dev(r_b.astype(dt))
            calls += [(dpk_all, drefs, kf_b.size, op, K, want_mask(vals, op, K), "per-block references") for op in OPS]
        for policy in FOR_POLICIES:
            kernel_policy(policy)
            for dpk, ref, n, op, K, want, label in calls:
                check(fl.FoR.unfor_compare(W, dpk, ref, op, K, n_blocks=n), want, T, ty, "unfor_compare", f"W={W}", op, f"K={K}", label,
                      f"policy={policy}")
        column.clear()


@pytest.mark.parametrize("ty", TYS)
def test_unfor_compare_widths_at_the_boundaries(fl, column, kernel_policy, ty):
    """unfor_compare_widths over ONE column that holds every width's boundary blocks back to back (every W in 0..T, the five
    constants each): per-block references r_b = (K - kf_b) mod 2^T for K in {0, a seeded value, M}, and one broadcast reference
    with K - r in {0, 1, 2} (the boundary of every block wide enough to hold it; the narrower ones are decided by their metadata)."""
    import torch
    T = tbits(ty)
    dt = TYPES[ty][0]
    esz = T // 8
    M = (1 << T) - 1
    u = np.uint64
    vs, pks, widths, kf_b = [], [], [], []
    for W in range(T + 1):
        for kf in bd.constants(W, bd.seed_of(T, W)):
            v, pk = column(ty, W, kf)
            vs.append(v)
            pks.append(pk)
            widths += [W] * (v.size // 1024)
            kf_b += [kf] * (v.size // 1024)
    v_all, col = np.concatenate(vs), np.concatenate(pks)
    widths = np.array(widths, dtype=np.uint8)
    kf_b = np.array(kf_b, dtype=np.uint64)
    n = widths.size
    off = np.concatenate([[0], np.cumsum(widths.astype(np.int64) * 128)])
    assert off[-1] == col.size * esz
    dw, doff, dcol = torch.from_numpy(widths).cuda(), torch.from_numpy(off[:-1].copy()).cuda(), to_dev(col)
    calls = []
    for K in sorted({0, seeded(T, 0, 3), M}):
        r_b = (u(K) - kf_b) & u(M)
        vals = ((v_all + np.repeat(r_b, 1024)) & u(M)).astype(dt)
        drefs = to_dev(r_b.astype(dt))
        calls += [(drefs, op, K, want_mask(vals, op, K), "per-block references") for op in OPS]
    r = seeded(T, 0, 4)
    vals = ((v_all + u(r)) & u(M)).astype(dt)
    dref = to_dev(np.array([r], dtype=dt))
    for d in (0, 1, 2):
        K = (r + d) & M
        calls += [(dref, op, K, want_mask(vals, op, K), f"broadcast r={r}") for op in OPS]
    for policy in FOR_POLICIES:
        kernel_policy(policy)
        for ref, op, K, want, label in calls:
            got = fl.unfor_compare_widths(dw, doff, dcol, ref, op, K)
            g = got.cpu().numpy().view(np.int32)
            if not np.array_equal(g, want):
                blk, row, lane = first_difference(g, want, T)
                raise AssertionError(f"{ty} unfor_compare_widths {op} K={K} {label} policy={policy}: first differing verdict in block {blk} "
                                     f"(W={int(widths[blk])}, kf={int(kf_b[blk])}), row {row}, lane {lane}")
