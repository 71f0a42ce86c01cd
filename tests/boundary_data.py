"""Boundary-dense columns for the compare kernels (unpack_compare, unfor_compare, unfor_compare_widths).

The compare kernels decide at `field == k`, and uniform random data (datagen.values) almost never gets there beyond W ~ 12.  The
columns made here hold nothing but a handful of candidate field values around one field-domain constant kf,

    kf - 1, kf, kf + 1, 0, 2^W - 1, kf with its top field bit flipped, ~kf, one seeded value      (all mod 2^W)

placed so that (check_coverage, asserted on the CPU for every (T, W, kf) the GPU tests use):
 1. every (row, lane) position of a block holds each of kf - 1, kf, kf + 1 in at least one block;
 2. for every row r and every ordered pair (a, b), a in {kf - 1, kf, kf + 1}, b in {0, 2^W - 1, kf}: some lane of some block holds a
    in row r and b in row r + 1, and some holds a in row r and b in row r - 1 (rows are neighbours in a lane's bit stream: the
    in-place u8 / u16 classes share one subtraction between them, a u32 / u64 field's junk is its lower neighbour);
 3. the same pairs in adjacent lanes (l, l + 1) of every row, both ways round (u8 / u16 hold 4 / 2 lanes per 32-bit SWAR word).

Fields are kept as np.uint64 in (block, row, lane) coordinates; `in_index_order` gives the 1024 values of each block in the unpacked
index order (bitmodel.index), which is what the oracle packs and what the expected masks are computed from -- nothing here unpacks."""
import numpy as np

from bitmodel import FL_ORDER

N_SWEEP = 8
N_RANDOM = 3


def seed_of(T, W):
    """The seed of (T, W)'s columns: the CPU coverage test and the GPU tests build the same arrays."""
    return 77000 + 100 * T + W


def candidates(W, kf, seed):
    """The eight candidate fields around kf (python ints, mod 2^W; duplicates at tiny W)."""
    m = (1 << W) - 1
    rnd = int.from_bytes(np.random.default_rng(seed).bytes(8), "little")
    top = 1 << (W - 1) if W else 0
    return [x & m for x in (kf - 1, kf, kf + 1, 0, m, kf ^ top, ~kf, rnd)]


def pairs(W, kf):
    """The ordered pairs (a, b) of conditions 2 and 3."""
    m = (1 << W) - 1
    return [(a & m, b & m) for a in (kf - 1, kf, kf + 1) for b in (0, m, kf)]


def constants(W, seed):
    """Field-domain constants: 0, 1, a seeded mid value, 2^W - 2, 2^W - 1 (mod 2^W, deduplicated, ascending)."""
    m = (1 << W) - 1
    mid = int.from_bytes(np.random.default_rng(seed).bytes(8), "little") & m
    if W >= 3:
        mid = min(max(mid, 2), m - 3)
    return sorted({x & m for x in (0, 1, mid, m - 1, m)})


def fields(T, W, kf, seed):
    """[n_blocks, T rows, 1024 / T lanes] np.uint64 fields: 8 sweep blocks, 18 checkerboard blocks, 3 blocks of seeded picks."""
    L = 1024 // T
    C = np.array(candidates(W, kf, seed), dtype=np.uint64)
    n = len(C)
    r = np.arange(T)[:, None]
    l = np.arange(L)[None, :]
    blocks = [C[(r * (l % n) + b) % n] for b in range(N_SWEEP)]
    even = (l % 2 == 0) & (r >= 0)
    for a, b in pairs(W, kf):
        blocks.append(np.where(even, np.uint64(a), np.uint64(b)))
        blocks.append(np.where(even, np.uint64(b), np.uint64(a)))
    rng = np.random.default_rng(seed + 1)
    blocks += [C[rng.integers(0, n, size=(T, L))] for _ in range(N_RANDOM)]
    return np.stack(blocks)


def in_index_order(F):
    """[n_blocks, T, L] fields -> [n_blocks * 1024] values in the unpacked index order (macros.rs:20-24: bitmodel.index)."""
    nb, T, L = F.shape
    r = np.arange(T)[:, None]
    l = np.arange(L)[None, :]
    idx = np.array(FL_ORDER)[r // 8] * 16 + (r % 8) * 128 + l
    out = np.empty((nb, 1024), dtype=np.uint64)
    out[:, idx.ravel()] = F.reshape(nb, T * L)
    return out.ravel()


def check_coverage(F, W, kf):
    """Conditions 1-3 of the module docstring on a [n_blocks, T, L] field array; raises AssertionError naming the first gap."""
    m = (1 << W) - 1
    assert int(F.max()) <= m, "a field wider than W"
    for a in {(kf - 1) & m, kf & m, (kf + 1) & m}:
        assert (F == np.uint64(a)).any(axis=0).all(), ("condition 1", W, kf, a)
    for a, b in pairs(W, kf):
        A, B = F == np.uint64(a), F == np.uint64(b)
        assert (A[:, :-1, :] & B[:, 1:, :]).any(axis=(0, 2)).all(), ("condition 2, row below", W, kf, a, b)
        assert (A[:, 1:, :] & B[:, :-1, :]).any(axis=(0, 2)).all(), ("condition 2, row above", W, kf, a, b)
        assert (A[:, :, :-1] & B[:, :, 1:]).any(axis=0).all(), ("condition 3, lane l + 1", W, kf, a, b)
        assert (A[:, :, 1:] & B[:, :, :-1]).any(axis=0).all(), ("condition 3, lane l - 1", W, kf, a, b)
    # 0 and 2^W - 1 are present in every block of the sweep: the column really spans the field range its width declares
    if W:
        assert (F[:N_SWEEP] == 0).any(axis=(1, 2)).all() and (F[:N_SWEEP] == np.uint64(m)).any(axis=(1, 2)).all()


def pack_column(oracle, ty, W, values):
    """oracle.pack per block over values in index order (np.uint64) -> the packed column in the element type."""
    from oracle_lib import TYPES, packed_len
    dt = TYPES[ty][0]
    v = values.astype(dt)
    n = v.size // 1024
    pl = packed_len(ty, W)
    out = np.zeros(n * pl, dtype=dt)
    for b in range(n):
        out[b * pl:(b + 1) * pl] = oracle.pack(ty, W, v[b * 1024:(b + 1) * 1024])
    return out
