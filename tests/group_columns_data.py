"""What the unfor_aggregate_by_columns tests share (tests/test_group_columns_data_cpu.py, tests/test_gpu_aggregate_by_columns.py): the
three-column cases -- two mixed-width value columns of one type and a u8 key column, every block packed bytes plus the oracle's
unfor_pack of them (the decode is what the expected values come from) -- and the numpy reference: both values zero-extended, the
operation mod 2^64 (`expr`), reduced per key with group_data.expected_groups.  numpy only: no GPU is needed to import or use this
module."""
import numpy as np

from datagen import values
from gpu_support import mixed_column_host, uniform_widths
from group_data import KEY_KINDS, expected_groups, key_blocks, key_column
from oracle_lib import TYPES, tbits

OPS = ["*", "+", "-"]
MIXED_BLOCKS = {"u8": 43, "u16": 67, "u32": 83, "u64": 163}            # T + 1 widths and a tail; none a multiple of 4
PAIR_CLASSES = {(a, b) for a in (0, 1, 2) for b in (0, 1, 2)}           # (wa, wb), each 0: width 0, 1: 0 < w < T, 2: width T


def expr(op, va, vb):
    """the definition: zero-extend, then the operation mod 2^64"""
    x, y = np.asarray(va).astype(np.uint64), np.asarray(vb).astype(np.uint64)
    with np.errstate(over="ignore"):
        return x * y if op == "*" else x + y if op == "+" else x - y


def width_class(w, T):
    return 0 if w == 0 else 2 if w == T else 1


def pair_classes(wa, wb, T):
    return {(width_class(int(a), T), width_class(int(b), T)) for a, b in zip(wa, wb)}


def value_column(oracle, ty, widths, seed, refs):
    """a mixed-width value column: (widths uint8, byte offsets int64, packed column, references, the oracle's decode of every block)"""
    w, off, col, blocks = mixed_column_host(ty, widths, seed)
    vals = np.concatenate([oracle.unfor_pack(ty, bw, pk, refs[b]) for b, (bw, pk) in enumerate(blocks)]) if len(blocks) else np.zeros(0, TYPES[ty][0])
    return w, off, col, refs, vals


def mixed_widths(ty, n, rng):
    """column a with the widths 0..T and a tail, column b with T..0 and another tail: every pair class of PAIR_CLASSES occurs"""
    T = tbits(ty)
    assert n >= T + 1 + 6
    tail_a, tail_b = rng.integers(0, T + 1, size=n - (T + 1)), rng.integers(0, T + 1, size=n - (T + 1))
    tail_a[:6], tail_b[:6] = (0, T, 0, 3, T, 3), (0, T, 2, 0, 3, T)
    return np.concatenate([np.arange(T + 1), tail_a]), np.concatenate([np.arange(T, -1, -1), tail_b])


def mixed_case(oracle, ty, seed, n=None, broadcast=False):
    """THE mixed-width case of `ty`: MIXED_BLOCKS[ty] blocks, the widths of mixed_widths, key blocks cycling through every
    distribution of KEY_KINDS, random (wrapping) per-block references -- or, `broadcast`, one reference per column.
    Returns (a, b, key, kinds): a and b as value_column gives them, key as group_data.key_column does, kinds[b] the key block's
    distribution."""
    T = tbits(ty)
    n = MIXED_BLOCKS[ty] if n is None else n
    rng = np.random.default_rng(seed)
    wa, wb = mixed_widths(ty, n, rng)
    ra, rb = values(ty, n, seed + 1), values(ty, n, seed + 2)
    kinds = [KEY_KINDS[(b + b // 7) % len(KEY_KINDS)] for b in range(n)]
    kblocks = [key_blocks(oracle, kind, 1, rng)[0] for kind in kinds]
    if broadcast:
        ra, rb = np.full(n, ra[3], dtype=ra.dtype), np.full(n, rb[5], dtype=rb.dtype)
        kblocks = [(w, kblocks[2][1], pk) for w, _, pk in kblocks]
    a = value_column(oracle, ty, wa, seed + 3, ra)
    b = value_column(oracle, ty, wb, seed + 4, rb)
    return a, b, key_column(oracle, kblocks), kinds


def routed_case(oracle, ty, n, seed):
    """n blocks whose routes alternate: block b % 5 == 0 keeps nothing (SKIP), key width 0 on b % 3 == 1 (ONE_KEY), the others are
    decoded; the value widths cycle so that every route meets a width-0 and a packed block on either side.  Returns (a, b, key,
    bits, routes) with routes[b] in 0 (SKIP), 1 (ONE_KEY), 2 (DECODE)."""
    rng = np.random.default_rng(seed)
    cyc = uniform_widths(ty)
    wa = np.array([cyc[(b + b // 5) % 5] for b in range(n)], dtype=np.int64)
    wb = np.array([cyc[(2 * b + b // 7) % 5] for b in range(n)], dtype=np.int64)
    wa[13] = wb[13] = 0                                                     # a ONE_KEY block that keeps rows: the constant route
    a = value_column(oracle, ty, wa, seed + 1, values(ty, n, seed + 2))
    b = value_column(oracle, ty, wb, seed + 3, values(ty, n, seed + 4))
    decoded = ("wrapping", "uniform", "two", "permutation")
    kinds = ["clustered" if blk % 3 == 1 else decoded[blk % len(decoded)] for blk in range(n)]
    key = key_column(oracle, [key_blocks(oracle, kind, 1, rng)[0] for kind in kinds])
    bits = rng.random(n * 1024) < 0.3
    bits.reshape(n, 1024)[::5] = False
    kept = bits.reshape(n, 1024).any(axis=1)
    routes = [0 if not kept[blk] else 1 if key[0][blk] == 0 else 2 for blk in range(n)]
    return a, b, key, bits, routes


def expected(op, a, b, key, bits, without=()):
    """uint64[256, 4] of the case under `op` and the mask's bits (None: every row)"""
    return expected_groups(expr(op, a[4], b[4]), key[4], bits, without=without)


def kept_rows(bits, size):
    return np.ones(size, bool) if bits is None else bits


def wrapped_products(va, vb):
    x, y = va.astype(np.uint64), vb.astype(np.uint64)
    return (x != 0) & (expr("*", va, vb) // np.where(x == 0, np.uint64(1), x) != y)


def blocks_of_group(keys, bits, g):
    """the blocks that hold a kept row of key g"""
    hit = (np.asarray(keys).reshape(-1, 1024) == g) & kept_rows(bits, np.asarray(keys).size).reshape(-1, 1024)
    return np.flatnonzero(hit.any(axis=1))
